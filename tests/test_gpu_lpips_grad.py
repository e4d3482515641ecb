"""The picture gradients of LPIPS on the HIP path (masic_amd/lpips.py, masic_amd/csrc/lpips_bwd.hip) against float64 torch.autograd
through the restatement of tests/test_gpu_lpips.py on the CPU.

Ruler for a gradient, per picture: max |g - g64| / max |g64| (`_pic_err`).  Where a gate is "4 x floor", floor is the error of the SAME
restatement differentiated in float32 on the CPU under that ruler -- another summation order of the same float32 arithmetic.

Measured on an MI355X and its host: end to end, distorted group: floor 1.2e-5, HIP 4.2e-6 .. 2.0e-5; near group:
floor 1.5e-4, HIP 1.7e-4 .. 2.4e-4 (set by the cancellation in u - v, not by the kernels).  Distance backward alone: floors
7.4e-8 .. 3.8e-7, HIP 4.6e-8 .. 2.1e-7 (at most 1.3 x the case's floor).  First layer: 6.5e-7 .. 9.5e-7 of the largest gradient."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_lpips import CHNS, DEV, GROUPS, SCALE, _model, _model_sd, _pair, ref_distance, ref_lpips, ref_scaling
from tests.util import RTOL, assert_close

pytestmark = pytest.mark.gpu


def _ops():
    import lpips  # noqa: F401
    from masic_amd import ops
    return ops


def _pic_err(g, ref):
    """The ruler: per picture max |g - ref| / max |ref|; the largest over the pictures.  inf if g is not finite."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == ref.shape, (tuple(g.shape), tuple(ref.shape))
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    scale = ref.abs().flatten(1).max(1).values
    assert bool((scale > 0).all())
    return float(((g - ref).abs().flatten(1).max(1).values / scale).max())


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. first layer
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 31, 31), (1, 3, 67, 93), (2, 3, 64, 96), (1, 3, 75, 280), (1, 3, 34, 38)])
def test_first_layer_input_gradient_vs_float64_autograd(shape, normalize):
    """Float64 autograd of the pre-ReLU conv2d(ref_scaling(x)) under a random output gradient (the layer is linear in x: the gradient
    does not depend on the picture).  One-sided launches for either side and the interleaved launch that splits into both tensors.
    34 x 38: the last row and column lie under no window and must come out exactly 0."""
    ops = _ops()
    N, _, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 7)
    w = torch.randn(64, 3, 11, 11, generator=g) * 0.05
    Ho, Wo = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    gy = torch.randn(2 * N, 64, Ho, Wo, generator=g)
    x = torch.rand(2 * N, 3, H, W, generator=g).double().requires_grad_(True)
    F.conv2d(ref_scaling(x, normalize), w.double(), None, stride=4, padding=2).backward(gy.double())
    ref = x.grad
    packed = ops.pack_lpips_conv1_bwd_weight(w.to(DEV))
    scale = torch.tensor(SCALE).view(1, 3, 1, 1).to(DEV)
    both = ops.lpips_conv1_bwd(gy.to(DEV), packed, scale, H, W, normalize, 3)
    only0 = ops.lpips_conv1_bwd(gy[0::2].contiguous().to(DEV), packed, scale, H, W, normalize, 1)
    only1 = ops.lpips_conv1_bwd(gy[1::2].contiguous().to(DEV), packed, scale, H, W, normalize, 2)
    assert only0[1] is None and only1[0] is None
    errs = []
    for name, got, want in (("both, in0", both[0], ref[0::2]), ("both, in1", both[1], ref[1::2]), ("in0 alone", only0[0], ref[0::2]),
                            ("in1 alone", only1[1], ref[1::2])):
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, H, W)
        errs.append(assert_close(got, want, f"first-layer input gradient, {name}"))
        if shape == (1, 3, 34, 38):
            got = got.cpu()
            assert bool((want[:, :, -1] == 0).all()) and bool((want[:, :, :, -1] == 0).all())
            assert bool((got[:, :, -1] == 0).all()) and bool((got[:, :, :, -1] == 0).all()), name
    assert _bits_equal(both[0], only0[0]) and _bits_equal(both[1], only1[1])
    print(f"lpips first-layer input gradient {shape} normalize={normalize}: relative error {max(errs):.2e}")


# ---------------------------------------------------------------- 2. max-pool backward
@pytest.mark.parametrize("hw", [(7, 7), (16, 22), (8, 9), (15, 15)])
def test_pool_backward_bit_equal_to_max_pool2d(hw):
    """Small-integer inputs: most windows hold ties.  The forward input is picked out of a 2N batch by image stride and offset."""
    ops = _ops()
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1] + 1)
    N, C = 2, 5
    x = torch.randint(0, 3, (2 * N, C) + hw, generator=g).float()
    Ho, Wo = (hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1
    ties = 0
    for side in (0, 1):
        gy = torch.randn(N, C, Ho, Wo, generator=g)
        xs = x[side::2].clone().requires_grad_(True)
        y = F.max_pool2d(xs, 3, 2)
        y.backward(gy)
        win = F.unfold(xs.detach().reshape(N * C, 1, *hw), 3, stride=2)
        ties += int(((win == win.max(1, keepdim=True).values).sum(1) > 1).sum())
        got = ops.maxpool3s2_bwd(x.to(DEV), gy.to(DEV), 2, side).cpu()
        assert _bits_equal(got, xs.grad), (hw, side)
    assert ties > N * C * Ho * Wo, "badly chosen input: ties in fewer than half of the windows"
    gy = torch.randn(2 * N, C, Ho, Wo, generator=g)
    xs = x.clone().requires_grad_(True)
    F.max_pool2d(xs, 3, 2).backward(gy)
    assert _bits_equal(ops.maxpool3s2_bwd(x.to(DEV), gy.to(DEV)).cpu(), xs.grad)


# ---------------------------------------------------------------- 3. distance backward
def _dist_reference(p0, p1, lin, G, gin0, gin1, dtype):
    """Autograd of sum_n G_n ref_distance(relu(p0), relu(p1))[n] + <gin, relu(p)> with respect to the pre-activations: (g_dist + g_in) [p > 0]."""
    a, b = p0.detach().to(dtype).clone().requires_grad_(True), p1.detach().to(dtype).clone().requires_grad_(True)
    fa, fb = F.relu(a), F.relu(b)
    loss = (G.to(dtype) * ref_distance(fa, fb, lin.to(dtype)).reshape(-1)).sum() + (gin0.to(dtype) * fa).sum() + (gin1.to(dtype) * fb).sum()
    loss.backward()
    return a.grad, b.grad


def _dist_hip(ops, f, lin, gout, t, gin0, gin1):
    """The kernel's three forms: (in0 side alone, in1 side alone, both interleaved -> split)."""
    N = f.shape[0] // 2
    gin = torch.empty_like(f)
    gin[0::2], gin[1::2] = gin0, gin1
    fd, ld, gd = f.to(DEV), lin.to(DEV), gout.to(DEV)
    a = ops.lpips_dist_bwd(fd, ld, gd, t, 1, g_in=gin0.contiguous().to(DEV))
    b = ops.lpips_dist_bwd(fd, ld, gd, t, 2, g_in=gin1.contiguous().to(DEV))
    buf = gin.to(DEV)
    ab = ops.lpips_dist_bwd(fd, ld, gd, t, 3, g_in=buf, out=buf)            # in place
    assert ab.data_ptr() == buf.data_ptr() and tuple(a.shape) == (N,) + tuple(f.shape[1:])
    return a.cpu(), b.cpu(), ab.cpu()


@pytest.mark.parametrize("hw", [(1, 1), (3, 3), (7, 7), (15, 15)])
@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_distance_backward_vs_float64_autograd(C, hw):
    """Post-ReLU-like taps (about half the entries zero) of four comparisons, a random incoming gradient and random upstream gradients of
    the value and of the tap's per-layer value.  15 x 15 spans four 64-pixel chunks.  Gate: 4 x the float32 restatement's error."""
    ops = _ops()
    N, t = 4, CHNS.index(C)
    g = torch.Generator().manual_seed(C * 10 + hw[0])
    p0, p1 = torch.randn(N, C, *hw, generator=g), torch.randn(N, C, *hw, generator=g)
    lin = torch.rand(1, C, 1, 1, generator=g)
    gout = torch.randn(6, N, generator=g)
    gin0, gin1 = torch.randn(N, C, *hw, generator=g) * 0.01, torch.randn(N, C, *hw, generator=g) * 0.01
    G = gout[0] + gout[1 + t]
    r0, r1 = _dist_reference(p0, p1, lin, G, gin0, gin1, torch.float64)
    s0, s1 = _dist_reference(p0, p1, lin, G, gin0, gin1, torch.float32)
    assert bool(torch.isfinite(r0).all()) and bool(torch.isfinite(r1).all())
    floor = max(_pic_err(s0, r0), _pic_err(s1, r1))
    gate = 4 * floor
    f = torch.empty(2 * N, C, *hw)
    f[0::2], f[1::2] = F.relu(p0), F.relu(p1)
    a, b, ab = _dist_hip(ops, f, lin, gout, t, gin0, gin1)
    err = max(_pic_err(a, r0), _pic_err(b, r1), _pic_err(ab[0::2], r0), _pic_err(ab[1::2], r1))
    print(f"lpips distance backward C={C} {hw}: float32 restatement floor {floor:.2e}, gate {gate:.2e}, HIP {err:.2e}")
    assert _bits_equal(ab[0::2], a) and _bits_equal(ab[1::2], b)
    assert gate <= RTOL, f"badly chosen case: 4 x floor = {gate:.2e} exceeds RTOL"
    assert err <= gate, f"C={C} {hw}: relative error {err:.2e} against the gate {gate:.2e} (floor {floor:.2e})"


def test_distance_backward_at_all_zero_pixels():
    """Pixel (0, 1) of comparison 0 is all-zero in the first picture only, pixel (1, 1) in both.  lpips's autograd gives NaN at such a
    pixel (0 / 0 in sqrt's backward); the kernel defines the norm's derivative as 0 there.  What the kernel writes is masked by
    [f > 0], so the all-zero picture's own gradient at the pixel is 0 under the convention's closed form 2 G lin_c d_c / (HW 1e-10) as
    well; the OTHER picture's gradient at the one-sided pixel is the closed form with u = 0, which is checked here in float64."""
    ops = _ops()
    N, C, hw, t = 2, 64, (3, 3), 0
    g = torch.Generator().manual_seed(77)
    p0, p1 = torch.randn(N, C, *hw, generator=g), torch.randn(N, C, *hw, generator=g)
    p0[0, :, 0, 1] = -1.0
    p0[0, :, 1, 1] = -1.0
    p1[0, :, 1, 1] = -1.0
    lin = torch.rand(1, C, 1, 1, generator=g)
    gout = torch.randn(6, N, generator=g)
    gin0, gin1 = torch.randn(N, C, *hw, generator=g) * 0.01, torch.randn(N, C, *hw, generator=g) * 0.01
    G = (gout[0] + gout[1 + t]).double()
    f = torch.empty(2 * N, C, *hw)
    f[0::2], f[1::2] = F.relu(p0), F.relu(p1)
    a, b, ab = _dist_hip(ops, f, lin, gout, t, gin0, gin1)
    assert all(bool(torch.isfinite(v).all()) for v in (a, b, ab))
    assert _bits_equal(ab[0::2], a) and _bits_equal(ab[1::2], b)
    # both zero: exactly 0 on both sides; one-sided: the zero picture's gradient is masked to exactly 0
    assert bool((a[0, :, 1, 1] == 0).all()) and bool((b[0, :, 1, 1] == 0).all()) and bool((a[0, :, 0, 1] == 0).all())
    # the other picture at the one-sided pixel: -(2 G / HW) (lin d / nb - b sum(lin d b) / (nb^2 sqrt(sum b^2))) with d = 0 - v
    bb, l64 = f[1, :, 0, 1].double(), lin.double().reshape(-1)
    sb = torch.sqrt((bb ** 2).sum())
    nb = sb + 1e-10
    d = -bb / nb
    want = -(2 * G[0] / 9) * (l64 * d / nb - bb * (l64 * d * bb).sum() / (nb ** 2 * sb))
    want = (want + gin1[0, :, 0, 1].double()) * (bb > 0)
    assert float((b[0, :, 0, 1].double() - want).abs().max()) <= RTOL * float(want.abs().max())
    # every other pixel: autograd (the NaN of a zero pixel stays in that pixel)
    r0, r1 = _dist_reference(p0, p1, lin, G, gin0, gin1, torch.float64)
    keep = torch.ones(N, 1, *hw, dtype=torch.bool)
    keep[0, :, 0, 1] = keep[0, :, 1, 1] = False
    for got, ref in ((a, r0), (b, r1)):
        ref = torch.where(keep, ref, torch.zeros_like(ref))
        assert bool(torch.isfinite(ref).all())
        assert _pic_err(torch.where(keep, got.double(), torch.zeros_like(ref)), ref) <= RTOL


# ---------------------------------------------------------------- 4. end to end
def _coefficients(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, generator=g) + 0.5, torch.rand(5, N, generator=g) + 0.5


def _loss(val, res, c, d):
    """sum_n c_n val[n] + sum_t sum_n d_tn res_t[n]: every upstream gradient G differs."""
    out = (c.to(val) * val.reshape(-1)).sum()
    for t, r in enumerate(res):
        out = out + (d[t].to(r) * r.reshape(-1)).sum()
    return out


def _ref_grads(y, x, normalize, c, d, dtype):
    yy, xx = y.detach().to(dtype).clone().requires_grad_(True), x.detach().to(dtype).clone().requires_grad_(True)
    val, res = ref_lpips(yy, xx, _model_sd(), normalize)
    _loss(val, res, c, d).backward()
    return yy.grad, xx.grad


def _hip_grads(net, y, x, normalize, c, d, need0, need1):
    yy, xx = y.to(DEV).requires_grad_(need0), x.to(DEV).requires_grad_(need1)
    val, res = net(yy, xx, retPerLayer=True, normalize=normalize)
    _loss(val, res, c.to(DEV), d.to(DEV)).backward()
    return yy.grad, xx.grad


@functools.lru_cache(maxsize=None)
def _grad_group(name):
    """Per case and normalize value: (y, x, normalize, c, d, float64 gradients); and the group's float32 floor."""
    cases, floor = [], 0.0
    for shape, sigma, seed in GROUPS[name]:
        y, x = _pair(shape, sigma, seed)
        c, d = _coefficients(shape[0], seed + 100)
        for normalize in (False, True):
            ref = _ref_grads(y, x, normalize, c, d, torch.float64)
            assert all(bool(torch.isfinite(r).all()) for r in ref), "the float64 reference gradient is not finite (an all-zero feature pixel?)"
            low = _ref_grads(y, x, normalize, c, d, torch.float32)
            floor = max(floor, _pic_err(low[0], ref[0]), _pic_err(low[1], ref[1]))
            cases.append((y, x, normalize, c, d, ref))
    return cases, floor


@pytest.mark.parametrize("name", ["distorted", "near"])
def test_end_to_end_gradients_vs_float64_restatement(name):
    cases, floor = _grad_group(name)
    gate = 4 * floor
    print(f"lpips gradients {name}: float32 restatement floor {floor:.2e}, gate {gate:.2e}")
    if name == "distorted":
        assert gate <= RTOL, f"badly chosen cases: 4 x floor = {gate:.2e} exceeds RTOL"
    net = _model()
    errs = []
    for y, x, normalize, c, d, (ry, rx) in cases:
        gy, none = _hip_grads(net, y, x, normalize, c, d, True, False)
        assert none is None and gy.dtype == torch.float32 and gy.shape == y.shape
        none, gx = _hip_grads(net, y, x, normalize, c, d, False, True)
        assert none is None and gx.dtype == torch.float32 and gx.shape == x.shape
        by, bx = _hip_grads(net, y, x, normalize, c, d, True, True)
        e = [_pic_err(gy, ry), _pic_err(gx, rx), _pic_err(by, ry), _pic_err(bx, rx)]
        errs.append(max(e))
        print(f"lpips gradients {name} {tuple(y.shape)} normalize={normalize}: in0 alone {e[0]:.2e}, in1 alone {e[1]:.2e}, "
              f"both {e[2]:.2e} {e[3]:.2e}")
    assert max(errs) <= gate, f"{name}: relative errors {['%.2e' % e for e in errs]} against the gate {gate:.2e} (floor {floor:.2e})"


# ---------------------------------------------------------------- 5. identical pictures
def test_identical_pictures_give_exactly_zero_gradients():
    net = _model()
    y, _ = _pair((1, 3, 64, 96), 0.05, 31)
    c, d = _coefficients(1, 131)
    ry, rx = _ref_grads(y, y.clone(), False, c, d, torch.float64)
    assert torch.equal(ry, torch.zeros_like(ry)) and torch.equal(rx, torch.zeros_like(rx))
    gy, gx = _hip_grads(net, y, y.clone(), False, c, d, True, True)
    assert torch.equal(gy.cpu(), torch.zeros(y.shape)) and torch.equal(gx.cpu(), torch.zeros(y.shape))


# ---------------------------------------------------------------- 6. reproducible, batch-invariant
def test_gradients_reproducible_and_batch_invariant():
    net = _model()
    y, x = _pair((3, 3, 64, 96), 0.05, 32)
    c, d = _coefficients(3, 132)
    gy, gx = _hip_grads(net, y, x, False, c, d, True, True)
    again = _hip_grads(net, y, x, False, c, d, True, True)
    assert _bits_equal(gy, again[0]) and _bits_equal(gx, again[1])
    for n in range(3):
        ay, ax = _hip_grads(net, y[n:n + 1].contiguous(), x[n:n + 1].contiguous(), False, c[n:n + 1], d[:, n:n + 1], True, True)
        assert _bits_equal(ay[0], gy[n]) and _bits_equal(ax[0], gx[n]), f"picture {n}: alone and in the batch differ"
    # the one-sided chains (N images) against the two-sided one (2N interleaved): every layer's input gradient gives an image the
    # arithmetic of a one-image launch, so the bits agree
    assert _bits_equal(_hip_grads(net, y, x, False, c, d, False, True)[1], gx)
    assert _bits_equal(_hip_grads(net, y, x, False, c, d, True, False)[0], gy)


def test_per_unit_input_gradient_launches_equal_the_batched_launch():
    """Forcing every plan signature to differ makes layers 2-5 (forward, per pair) and their input gradients (per image) run split; the
    gradients keep the default call's bits."""
    from masic_amd import lpips as L
    net = _model()
    y, x = _pair((3, 3, 64, 96), 0.05, 33)
    c, d = _coefficients(3, 133)
    want = _hip_grads(net, y, x, False, c, d, True, True)
    want1 = _hip_grads(net, y, x, False, c, d, False, True)
    orig, seen = L._hip.conv_plan_signature, []

    def forced(desc):
        seen.append((desc.transposed, desc.B))
        return ("per unit", desc.B)

    L._hip.conv_plan_signature = forced
    try:
        split = _hip_grads(net, y, x, False, c, d, True, True)
        split1 = _hip_grads(net, y, x, False, c, d, False, True)
    finally:
        L._hip.conv_plan_signature = orig
    assert (1, 6) in seen and (1, 3) in seen and (1, 1) in seen
    assert _bits_equal(split[0], want[0]) and _bits_equal(split[1], want[1]) and _bits_equal(split1[1], want1[1])


# ---------------------------------------------------------------- 7. capture
def test_forward_and_backward_capturable_into_one_graph():
    net = _model()
    y1, x1 = _pair((2, 3, 64, 96), 0.05, 34)
    y2, x2 = _pair((2, 3, 64, 96), 0.05, 35)
    y1, x1, y2, x2 = (t.to(DEV) for t in (y1, x1, y2, x2))

    def eager(y, x):
        xx = x.clone().requires_grad_(True)
        val = net(y, xx)
        return val.detach(), torch.autograd.grad(val.sum(), xx)[0]

    sy, sx = y1.clone(), x1.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(net(sy, sx).sum(), sx)      # weight packs and allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        val = net(sy, sx)
        grad, = torch.autograd.grad(val.sum(), sx)
    g.replay()
    torch.cuda.synchronize()
    v1, g1 = eager(y1, x1)
    assert torch.equal(val.detach(), v1) and _bits_equal(grad, g1)
    with torch.no_grad():
        sy.copy_(y2)
        sx.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    v2, g2 = eager(y2, x2)
    assert torch.equal(val.detach(), v2) and _bits_equal(grad, g2) and not _bits_equal(g2, g1)


# ---------------------------------------------------------------- 8. interface
def test_loss_interface():
    import lpips
    m = _model()
    x, xh = _pair((2, 3, 40, 48), 0.05, 36)
    x, xh = x.to(DEV), xh.to(DEV).requires_grad_(True)
    loss = m(xh, x).mean()
    with torch.no_grad():
        assert torch.equal(loss.detach(), m(xh, x).mean())                 # the forward's bits with and without grad
    loss.backward()
    assert xh.grad is not None and xh.grad.dtype == torch.float32 and xh.grad.shape == xh.shape and x.grad is None
    assert bool(torch.isfinite(xh.grad).all()) and float(xh.grad.abs().max()) > 0
    # a non-contiguous x_hat: the gradient has its shape and the values of the contiguous call
    wide = torch.zeros(2, 3, 40, 96, device=DEV)
    wide[..., ::2] = xh.detach()
    nc = wide[..., ::2].requires_grad_(True)
    assert not nc.is_contiguous()
    m(nc, x).mean().backward()
    assert nc.grad.shape == nc.shape and torch.equal(nc.grad, xh.grad)
    # in0 is in1: both paths are summed (each is exactly 0 for identical pictures); x against itself plus another use
    t = xh.detach().clone().requires_grad_(True)
    (m(t, t).sum() + m(t, x).mean()).backward()
    assert torch.equal(t.grad, xh.grad)
    # what still raises
    flipped = lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False).to(DEV)
    flipped.lin0.model[1].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        flipped(xh, x)
    with torch.no_grad():
        flipped(xh, x)
    tr = lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False).to(DEV).train()
    with pytest.raises(NotImplementedError):
        tr(xh, x)
    with pytest.raises(NotImplementedError):
        m.features(xh, x)
    t = xh.detach().clone().requires_grad_(True)
    g1, = torch.autograd.grad(m(t, x).sum(), t, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


# ---------------------------------------------------------------- 9. a loss that moves
STEP = 2.0          # the value is ~9e-3 and its gradient ~4e-4 per pixel: ten such steps lower the float64 value by ~15 %, monotonically


def test_gradient_descent_lowers_the_value():
    """Ten steps of x_hat <- x_hat - STEP * d LPIPS / d x_hat from the distorted pair.  Precondition: under that step the float64
    restatement on the CPU descends monotonically."""
    net = _model()
    y, x0 = _pair((1, 3, 64, 96), 0.05, 37)
    sd = _model_sd()
    xr, ref_vals = x0.double(), []
    for _ in range(10):
        xr = xr.detach().requires_grad_(True)
        v = ref_lpips(y.double(), xr, sd)[0].sum()
        ref_vals.append(float(v.detach()))
        xr = xr - STEP * torch.autograd.grad(v, xr)[0]
    assert all(b < a for a, b in zip(ref_vals, ref_vals[1:])), f"badly chosen step: the float64 restatement gives {ref_vals}"
    yd, xh, vals = y.to(DEV), x0.to(DEV), []
    for _ in range(10):
        xh = xh.detach().requires_grad_(True)
        v = net(yd, xh).sum()
        vals.append(float(v.detach()))
        xh = xh - STEP * torch.autograd.grad(v, xh)[0]
    print(f"lpips descent: {vals[0]:.6f} -> {vals[-1]:.6f} (float64 restatement {ref_vals[0]:.6f} -> {ref_vals[-1]:.6f})")
    assert vals[-1] < vals[0]
