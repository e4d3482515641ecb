"""LPIPS on the AlexNet trunk on the HIP path (masic_amd/lpips.py, masic_amd/csrc/lpips.hip) against a restatement of lpips 0.1.4.

The restatement below (`ref_*`) is the published op sequence in plain torch ops on the CPU, in the dtype of its inputs (float64 for the
reference, float32 for the error floor): x <- 2x - 1 if normalize; (x - shift) / scale; AlexNet's `features` with a tap after each of
the five ReLUs; per tap f / (sqrt(sum_c f^2) + 1e-10), sum_c lin_c (f0 - f1)^2 as a 1x1 convolution, the spatial mean; the sum of the
taps.  tests/test_cpu_lpips.py checks it against closed forms and torch's own modules.  No trained weights exist in this repository:
every model here is `LPIPS(pnet_rand=True, pretrained=False)` with seeded weights.

End-to-end gate: relative error against the float64 restatement, at most 4 x floor, where floor is the largest relative error of
the SAME restatement evaluated in float32 on the CPU over the group's cases (another accumulation order of the same float32
arithmetic, K up to 3456, lands a few times away from one order's error); the gate may not exceed tests/util.py::RTOL.  The ruler
(`_relerr`) is the value itself: |val - ref| / ref, and the five per-tap values in the same unit.
Measured on an MI355X and its host: floor 8.7e-7, HIP 1.8e-7 .. 9.4e-7 for the distorted group; floor 2.2e-5
(8.7e-6 .. 1.1e-5 on another CPU), HIP 1.1e-5 and 3.4e-5 for the near-identical one."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import RTOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHNS = (64, 192, 384, 256, 256)
# torchvision's alexnet.features: index -> (stride, padding) of the convolutions; MaxPool2d(3, 2) at 2 and 5; taps after 1, 4, 7, 9, 11
CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
CONV_GEOM = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))
POOL_BEFORE = (False, True, True, False, False)


# ---------------------------------------------------------------- restatement (CPU, dtype of the inputs)
def ref_scaling(x, normalize=False):
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def ref_conv1(x, w, b, normalize=False):
    return F.relu(F.conv2d(ref_scaling(x, normalize), w, b, stride=4, padding=2))


def ref_features(x, sd, normalize=False):
    """The five taps of one picture batch; sd: the LPIPS state dict (any dtype, converted to x's)."""
    taps, h = [], ref_scaling(x, normalize)
    for key, (stride, pad), pool in zip(CONV_KEYS, CONV_GEOM, POOL_BEFORE):
        if pool:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, sd[key + ".weight"].to(x.dtype), sd[key + ".bias"].to(x.dtype), stride=stride, padding=pad))
        taps.append(h)
    return taps


def ref_normalize(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def ref_distance(f0, f1, lin):
    """[N,1,1,1]: the spatial mean of the 1x1 `lin` convolution (no bias) of the squared difference of the normalised features."""
    d = (ref_normalize(f0) - ref_normalize(f1)) ** 2
    return F.conv2d(d, lin.to(d.dtype).view(1, -1, 1, 1)).mean([2, 3], keepdim=True)


def ref_lpips(in0, in1, sd, normalize=False):
    """(val [N,1,1,1], [five [N,1,1,1]])"""
    t0, t1 = ref_features(in0, sd, normalize), ref_features(in1, sd, normalize)
    res = [ref_distance(a, b, sd[f"lin{i}.model.1.weight"]) for i, (a, b) in enumerate(zip(t0, t1))]
    val = res[0]
    for r in res[1:]:
        val = val + r
    return val, res


# ---------------------------------------------------------------- fixtures shared by the tests
def _ops():
    from masic_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _model_sd(seed=5):
    """Seeded float32 state dict: torch's default initialisation for the trunk, non-negative random lin weights."""
    import lpips
    torch.manual_seed(seed)
    m = lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for i, c in enumerate(CHNS):
        w = torch.rand(1, c, 1, 1, generator=g)
        sd[f"lin{i}.model.1.weight"] = w
        sd[f"lins.{i}.model.1.weight"] = w.clone()
    return sd


@functools.lru_cache(maxsize=None)
def _model():
    import lpips
    m = lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False)
    m.load_state_dict(_model_sd())
    return m.to(DEV)


def _pair(shape, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g)
    x = (y + sigma * torch.randn(shape, generator=g)).clamp(0, 1)
    return y, x


GROUPS = {
    "distorted": [((2, 3, 64, 96), 0.05, 11), ((1, 3, 67, 93), 0.05, 12), ((2, 3, 31, 31), 0.05, 13)],
    "near": [((1, 3, 35, 131), 0.002, 14)],
}


def _relerr(got, ref):
    """The ruler of the end-to-end gate, per picture: |val - ref| / ref, and for the five per-tap values |r_t - ref_t| / ref -- the
    taps in units of the value they add up to (the convention of tests/util.py::rel_err: a tensor's error is scaled by its largest
    magnitude).  A tap's own magnitude would be the wrong ruler: on a 1 x 1 map the last tap is 256 terms and a thousandth of the
    value.  Returns (largest of all six, error of val alone)."""
    val, res = got
    rval, rres = ref
    r = rval.double().reshape(-1)
    assert bool((r > 0).all())
    errs = []
    for g, t in zip([val] + list(res), [rval] + list(rres)):
        g = g.detach().double().cpu().reshape(-1)
        assert bool(torch.isfinite(g).all())
        errs.append(float(((g - t.double().reshape(-1)).abs() / r).max()))
    return max(errs), errs[0]


@functools.lru_cache(maxsize=None)
def _group(name):
    """Per case and normalize value: (y, x, normalize, float64 reference); and the group's float32 floor."""
    sd = _model_sd()
    cases, floor = [], 0.0
    for shape, sigma, seed in GROUPS[name]:
        y, x = _pair(shape, sigma, seed)
        for normalize in (False, True):
            ref = ref_lpips(y.double(), x.double(), sd, normalize)
            floor = max(floor, _relerr(ref_lpips(y, x, sd, normalize), ref)[0])
            cases.append((y, x, normalize, ref))
    return cases, floor


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 31, 31), (1, 3, 67, 93), (2, 3, 64, 96), (1, 3, 75, 280)])
def test_first_layer_vs_conv2d_float64(shape, normalize):
    import lpips  # noqa: F401
    ops = _ops()
    g = torch.Generator().manual_seed(sum(shape))
    in0, in1 = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    w = torch.randn(64, 3, 11, 11, generator=g) * 0.05
    b = torch.randn(64, generator=g) * 0.1
    shift, scale = torch.tensor(SHIFT).view(1, 3, 1, 1), torch.tensor(SCALE).view(1, 3, 1, 1)
    y = ops.lpips_conv1(in0.to(DEV), in1.to(DEV), ops.pack_lpips_conv1_weight(w.to(DEV)), b.to(DEV), shift.to(DEV), scale.to(DEV), normalize)
    r0, r1 = (ref_conv1(t.double(), w.double(), b.double(), normalize) for t in (in0, in1))
    assert tuple(y.shape) == (2 * shape[0], 64, (shape[2] - 7) // 4 + 1, (shape[3] - 7) // 4 + 1)
    e0, e1 = assert_close(y[0::2], r0, "first layer, in0"), assert_close(y[1::2], r1, "first layer, in1")
    print(f"lpips first layer {shape} normalize={normalize}: relative error {max(e0, e1):.2e}")


@pytest.mark.parametrize("hw", [(7, 7), (16, 22), (8, 9)])
def test_pool_bit_equal_to_max_pool2d(hw):
    import lpips  # noqa: F401
    ops = _ops()
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randint(-2, 3, (2, 5) + hw, generator=g).float()
    x[x == 0] = torch.where(torch.rand(int((x == 0).sum()), generator=g) < 0.5, -0.0, 0.0)      # ties between -0 and +0
    u = torch.rand(x.shape, generator=g)
    x[u < 0.04] = float("nan")
    x[(u >= 0.04) & (u < 0.08)] = float("inf")
    x[(u >= 0.08) & (u < 0.16)] = float("-inf")
    x[1, 4] = float("-inf")                                                                     # a plane of -inf only
    x[0, 0] = torch.randn(hw, generator=g)
    want = F.max_pool2d(x, 3, 2)
    got = ops.maxpool3s2(x.to(DEV)).cpu()
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_distance_kernel_vs_restatement(rot):
    import lpips  # noqa: F401
    ops = _ops()
    maps = [(1, 1), (3, 5), (16, 22)]
    N = 2
    g = torch.Generator().manual_seed(40 + rot)
    feats, lins = [], []
    for t, C in enumerate((64, 192, 384, 256, 256)):
        h, w = maps[(t + rot) % 3]
        f = F.relu(torch.randn(2 * N, C, h, w, generator=g))
        if h * w > 1:
            f[0, :, 0, 1] = 0            # all-zero in the first picture only
            f[1, :, 1, 2] = 0            # ... in the second only
            f[2:4, :, 2, 0] = 0          # ... in both (comparison 1)
        else:
            f[2 + (t & 1)] = 0           # one picture of comparison 1 is all zero
            if t == 3:
                f[2:4] = 0               # both are
        feats.append(f)
        lins.append(torch.rand(1, C, 1, 1, generator=g))
    out = ops.lpips_distance([f.to(DEV) for f in feats], [w.to(DEV) for w in lins]).cpu()
    assert tuple(out.shape) == (6, N) and bool(torch.isfinite(out).all())
    total = torch.zeros(N, dtype=torch.float64)
    for t, (f, w) in enumerate(zip(feats, lins)):
        ref = ref_distance(f[0::2].double(), f[1::2].double(), w.double()).reshape(N)
        total += ref
        for n in range(N):
            assert abs(float(out[1 + t, n]) - float(ref[n])) <= RTOL * float(ref[n]), (t, n, float(out[1 + t, n]), float(ref[n]))
    for n in range(N):
        assert abs(float(out[0, n]) - float(total[n])) <= RTOL * float(total[n])


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["distorted", "near"])
def test_end_to_end_vs_float64_restatement(name):
    cases, floor = _group(name)
    gate = 4 * floor
    print(f"lpips {name}: float32 restatement floor {floor:.2e}, gate {gate:.2e}")
    assert gate <= RTOL, f"badly chosen cases: 4 x floor = {gate:.2e} exceeds RTOL"
    net = _model()
    errs = []
    for y, x, normalize, ref in cases:
        with torch.no_grad():
            val, res = net.forward(y.to(DEV), x.to(DEV), retPerLayer=True, normalize=normalize)
            alone = net.forward(y.to(DEV), x.to(DEV), normalize=normalize)
        assert val.dtype == torch.float32 and tuple(val.shape) == (y.shape[0], 1, 1, 1) and len(res) == 5
        assert all(tuple(r.shape) == (y.shape[0], 1, 1, 1) for r in res) and torch.equal(alone, val)
        e, e_val = _relerr((val, res), ref)
        errs.append(e)
        print(f"lpips {name} {tuple(y.shape)} normalize={normalize}: value {float(ref[0].flatten()[0]):.6f}, relative error {e:.2e} "
              f"(of val alone {e_val:.2e})")
    assert max(errs) <= gate, f"{name}: relative errors {['%.2e' % e for e in errs]} against the gate {gate:.2e} (floor {floor:.2e})"


# ---------------------------------------------------------------- properties
def test_identical_pictures_give_exactly_zero():
    net = _model()
    y, _ = _pair((2, 3, 67, 93), 0.05, 21)
    with torch.no_grad():
        val, res = net(y.to(DEV), y.clone().to(DEV), retPerLayer=True)
    assert torch.equal(val.cpu(), torch.zeros(2, 1, 1, 1))
    assert all(torch.equal(r.cpu(), torch.zeros(2, 1, 1, 1)) for r in res)


def test_reproducible_and_batch_invariant():
    net = _model()
    y, x = _pair((3, 3, 64, 96), 0.05, 22)
    y, x = y.to(DEV), x.to(DEV)
    with torch.no_grad():
        val, res = net(y, x, retPerLayer=True)
        again, res2 = net(y, x, retPerLayer=True)
        assert torch.equal(val, again) and all(torch.equal(a, b) for a, b in zip(res, res2))
        for i in range(3):
            vi, ri = net(y[i:i + 1].contiguous(), x[i:i + 1].contiguous(), retPerLayer=True)
            assert torch.equal(vi[0], val[i]), f"picture {i}: {float(vi[0])} alone, {float(val[i])} in the batch"
            assert all(torch.equal(a[0], b[i]) for a, b in zip(ri, res))


@pytest.mark.parametrize("shape", [(3, 3, 64, 96), (8, 3, 512, 512)])
def test_per_pair_launches_equal_the_batched_launch(shape):
    """Layers 2-5 run as one launch for the 2N images when its plan sums in the order of the two-image plan, else once per picture pair.
    Forcing the per-pair form gives the bits of the default call: at 3 x 64 x 96 the two plans are the same; at 8 x 512 x 512 the batched
    plan has other tiles than the two-image plan but the same K chunk (GPU against GPU, no CPU reference at that size)."""
    import ctypes
    from masic_amd import lpips as L
    net = _model()
    y, x = _pair(shape, 0.05, 23)
    y, x = y.to(DEV), x.to(DEV)
    with torch.no_grad():
        val, res = net(y, x, retPerLayer=True)
        orig = L._hip.conv_plan_signature
        plans = set()

        def forced(d):
            buf = ctypes.create_string_buffer(512)
            L._hip.lib.masic_conv_plan_name(ctypes.byref(d), 0, buf, 512)
            plans.add((d.Cin, d.B, buf.value.decode().split("|")[0].strip(), orig(d)))
            return ("per pair", d.B)

        L._hip.conv_plan_signature = forced
        try:
            split, sres = net(y, x, retPerLayer=True)
        finally:
            L._hip.conv_plan_signature = orig
    for cin in (64, 192, 384, 256):
        print(f"lpips {shape} layer with {cin} input channels:", sorted(p[1:] for p in plans if p[0] == cin))
    assert len(plans) == 8 and torch.equal(val, split) and all(torch.equal(a, b) for a, b in zip(res, sres))


def test_forward_is_capturable_into_a_graph():
    net = _model()
    y1, x1 = _pair((2, 3, 64, 96), 0.05, 24)
    y2, x2 = _pair((2, 3, 64, 96), 0.05, 25)
    y1, x1, y2, x2 = (t.to(DEV) for t in (y1, x1, y2, x2))
    sy, sx = y1.clone(), x1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        net(sy, sx)                                    # weight packs and allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = net(sy, sx)
    g.replay()
    with torch.no_grad():
        assert torch.equal(out, net(y1, x1))
        sy.copy_(y2)
        sx.copy_(x2)
        g.replay()
        torch.cuda.synchronize()
        eager = net(y2, x2)
        assert torch.equal(out, eager)
        assert not torch.equal(eager, net(y1, x1))


def test_evaluator_lines_give_a_python_float():
    """coremasic/mywork/test2_real.py:105-112 restated: LPIPS of both views, each `.mean().item()`, averaged."""
    loss_fn = _model()
    t1, xh1 = _pair((1, 3, 64, 96), 0.05, 26)
    t2, xh2 = _pair((1, 3, 64, 96), 0.05, 27)
    with torch.no_grad():
        lp1 = loss_fn.forward(t1.to(DEV), xh1.to(DEV)).mean().item()
        lp2 = loss_fn.forward(t2.to(DEV), xh2.to(DEV)).mean().item()
    lp = (lp1 + lp2) / 2
    assert isinstance(lp, float) and 0.0 < lp < 10.0
