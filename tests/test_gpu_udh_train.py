"""GPU tests (-m gpu) of the UDH homography net's training stage (udh/udh/model.py -> masic_amd/udh_train.py on
masic_amd/csrc/udh_train.hip): each new kernel against float64 torch, the whole step against the reference's recorded step
(tests/golden/udh_train.npz), reproducibility, the reference's training loop, and the hand-over to the codec-side net.

Bound for every comparison with the reference or float64 torch: error over the tensor's peak (tests/util.assert_close) within
max(1e-4, 2 x float32 floor): 1e-4 is the project's float32-path contract, the floor is the reference's own float32-against-float64
deviation (from the fixture, or measured in the test where the test says so).  Measured on an MI355X: DESIGN.md section 8.4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import udh_train_ref as TR
from tests import udh_weights as UW
from tests.udh_train_cases import CASES, case_inputs, check_step, load_udh_model
from tests.util import assert_close, load_npz, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
_CACHE = {}


def _ops():
    from masic_amd import ops
    return ops


def _M():
    if "M" not in _CACHE:
        _CACHE["M"] = load_udh_model()
    return _CACHE["M"]


def _net(p, train):
    net = _M().Net(patch_size=p).to(DEV)
    UW.fill(net, UW.WEIGHT_SEED)
    return net.train(train)


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


@pytest.fixture(scope="module")
def fx():
    return load_npz("udh_train.npz")


def _step(fx, index, net=None):
    """One forward + loss + backward of fixture case `index` on the GPU: (loss, delta, {name: grad})."""
    p, B, _, mode = CASES[index]
    a, b, img, pb, corners, masks = case_inputs(fx, index)
    a, b, img, pb, corners = _dev(a, b, img, pb, corners)
    masks = None if masks is None else _dev(*masks)
    net = net if net is not None else _net(p, mode == "train")
    net.zero_grad(set_to_none=True)
    delta = net(a, b, dropout_masks=masks)
    loss = _M().photometric_loss(delta, img, pb, corners)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), delta.detach(), {n: q.grad for n, q in net.named_parameters()}


# ---- 1. pool + ReLU backward
@pytest.mark.parametrize("shape", [(5, 6, 10), (1, 2, 2)])
def test_maxpool2_relu_bwd_equals_torch(shape):
    ops = _ops()
    rs = np.random.default_rng(2)
    planes, H, W = shape
    z = rs.standard_normal((1, planes, H, W)).astype(np.float32)
    z[0, 0, 0:2, 0:2] = 0.0                            # an all-zero window
    z[0, 0, 0:2, 2:4] = -1.5 if W > 2 else 0.0         # an all-negative one
    if W > 4:
        z[0, 0, 0:2, 4:6] = [[0.25, 0.75], [0.75, 0.75]]   # equal maxima: the first in scan order takes the gradient
        z[0, 1, 2:4, 0:2] = 0.5                            # four equal positive values
    z = torch.from_numpy(z)
    gy = torch.from_numpy(rs.standard_normal((1, planes, H // 2, W // 2)).astype(np.float32))
    zr = z.clone().requires_grad_(True)
    F.max_pool2d(F.relu(zr), 2, 2).backward(gy)
    got = ops.maxpool2_relu_bwd(z.to(DEV), gy.to(DEV))
    assert torch.equal(got.cpu(), zr.grad)
    assert torch.equal(ops.maxpool2_relu_bwd(F.relu(z).to(DEV), gy.to(DEV)).cpu(), zr.grad)      # given the layer's output after its ReLU
    assert torch.equal(ops.maxpool2_relu_bwd(z.to(DEV), gy.to(DEV)), got)


# ---- 2. first-layer weight gradient
@pytest.mark.parametrize("cout", [32, 64])
def test_udh_conv1_wgrad_against_float64(cout):
    ops = _ops()
    rs = np.random.default_rng(3)
    a, b = (torch.from_numpy(rs.standard_normal((3, 1, 37, 29), dtype=np.float32)) for _ in range(2))
    dy = torch.from_numpy(rs.standard_normal((3, cout, 37, 29), dtype=np.float32))
    w = torch.zeros(cout, 2, 3, 3, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (F.conv2d(torch.cat((a, b), 1).double(), w, bias, padding=1) * dy.double()).sum().backward()
    dw, db = ops.udh_conv1_wgrad(*_dev(a, b, dy))
    print(f"udh_conv1_wgrad Cout {cout}: dW {rel_err(dw, w.grad):.2e}, db {rel_err(db, bias.grad):.2e}")
    assert_close(dw, w.grad, "dW")
    assert_close(db, bias.grad, "db")
    dw2, db2 = ops.udh_conv1_wgrad(*_dev(a, b, dy))
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ---- 3. the two linear layers, training forward and backward
@pytest.mark.parametrize("B", [1, 11, 24, 52, 64])
def test_linear_training_forward_and_backward_against_float64(B):
    """B = 11 crosses the 8-row group and K = 1536 is three chunks.  The streaming kernel holds up to four row groups (32 rows) in
    registers and takes one further pass per 32 rows that adds to gW1: B = 24 is three groups in one pass, B = 52 a second pass of
    three groups, B = 64 one of four."""
    ops = _ops()
    K, N, M = 1536, 256, 8
    rs = np.random.default_rng(40 + B)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s, dtype=np.float32))  # noqa: E731
    x, w1, b1, w2, b2, gout = f(B, K), f(N, K) / 16, f(N) / 4, f(M, N) / 8, f(M), f(B, M)
    m1 = torch.from_numpy((rs.random((B, K)) >= 0.5).astype(np.uint8))
    m2 = torch.from_numpy((rs.random((B, N)) >= 0.5).astype(np.uint8))
    xr, w1r, b1r, w2r, b2r = (t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2))
    hidden = F.relu(F.linear(xr * (2.0 * m1.double()), w1r, b1r))
    out = F.linear(hidden * (2.0 * m2.double()), w2r, b2r)
    out.backward(gout.double())
    xd, hid, got = ops.udh_fc_train(*_dev(x, w1, b1, w2, b2, m1, m2))
    res = ops.udh_fc_bwd(gout.to(DEV), xd, hid, w1.to(DEV), w2.to(DEV), m1.to(DEV), m2.to(DEV))
    pairs = {"hidden": (hid, hidden), "out": (got, out), "gw1": (res[0], w1r.grad), "gb1": (res[1], b1r.grad), "gw2": (res[2], w2r.grad),
             "gb2": (res[3], b2r.grad), "gx": (res[4], xr.grad)}
    print(f"udh linear train B {B}: " + ", ".join(f"{k} {rel_err(g, r):.2e}" for k, (g, r) in pairs.items()))
    for k, (g, r) in pairs.items():
        assert_close(g, r, k)
    res2 = ops.udh_fc_bwd(gout.to(DEV), xd, hid, w1.to(DEV), w2.to(DEV), m1.to(DEV), m2.to(DEV))
    assert all(torch.equal(u, v) for u, v in zip(res, res2))
    # without masks the forward is the inference pair of kernels
    xd0, hid0, out0 = ops.udh_fc_train(*_dev(x, w1, b1, w2, b2))
    assert torch.equal(out0, ops.udh_fc(*_dev(x, w1, b1, w2, b2)))
    assert_close(ops.udh_fc_bwd(gout.to(DEV), xd0, hid0, w1.to(DEV), w2.to(DEV))[4],
                 torch.autograd.functional.vjp(lambda t: F.linear(F.relu(F.linear(t, w1.double(), b1.double())), w2.double(), b2.double()),
                                               x.double(), gout.double())[1], "gx without masks")


# ---- 4. the sampling matrix and its adjoint
def test_photo_matrix_and_adjoint_against_float64_autograd():
    ops = _ops()
    rs = np.random.default_rng(8)
    _, _, corners = TR.loss_inputs([11, 12, 13, 14, 15], (40, 48), (32, 32), 0.0)
    corners = corners + 100.0                          # away from the origin: the loss shifts them to their first corner
    corners[4] = torch.tensor([[100.0, 100.0], [110.0, 100.0], [120.0, 100.0], [100.0, 131.0]])    # three collinear corners
    delta = torch.from_numpy(rs.uniform(-6, 6, (5, 4, 2)).astype(np.float32))
    delta[4] = 0.0
    g_s = torch.from_numpy(rs.standard_normal((5, 3, 3)).astype(np.float32))
    dr = delta[:4].double().requires_grad_(True)
    S_ref = TR.photo_matrix(dr, corners[:4].double(), (40, 48), (32, 32))
    S_ref.backward(g_s[:4].double())
    S = ops.udh_photo_matrix(corners.to(DEV), delta.to(DEV), (40, 48), (32, 32))
    gd = ops.udh_photo_matrix_bwd(corners.to(DEV), delta.to(DEV), g_s.reshape(5, 9).to(DEV), (40, 48), (32, 32))
    print(f"udh photo matrix: S {rel_err(S[:4], S_ref):.2e}, adjoint {rel_err(gd[:4], dr.grad):.2e}")
    assert_close(S[:4], S_ref, "S")
    assert_close(gd[:4], dr.grad, "g_delta")
    assert bool(torch.isnan(S[4]).all()) and bool(torch.isnan(gd[4]).all())
    assert bool(torch.isfinite(S[:4]).all()) and bool(torch.isfinite(gd[:4]).all())
    # rows do not depend on their neighbours, and two runs agree to the bit
    assert torch.equal(ops.udh_photo_matrix(corners[:4].to(DEV), delta[:4].to(DEV), (40, 48), (32, 32)), S[:4])
    assert torch.equal(ops.udh_photo_matrix_bwd(corners.to(DEV), delta.to(DEV), g_s.reshape(5, 9).to(DEV), (40, 48), (32, 32))[:4], gd[:4])
    # slots are added: two half-weight slots give the one-slot result
    two = torch.stack((0.5 * g_s.reshape(5, 9), 0.5 * g_s.reshape(5, 9)), dim=1).contiguous()
    assert_close(ops.udh_photo_matrix_bwd(corners.to(DEV), delta.to(DEV), two.to(DEV), (40, 48), (32, 32))[:4], dr.grad, "two slots")


# ---- 5. the loss and its backward
@pytest.mark.parametrize("img_hw,out_hw", [((40, 48), (32, 32)), ((33, 50), (24, 40))])
def test_photometric_loss_forward_and_backward_against_float64(img_hw, out_hw):
    ops = _ops()
    M = _M()
    B, rho = 3, 5.0
    delta = torch.from_numpy(np.random.default_rng(img_hw[0]).uniform(-rho, rho, (B, 4, 2)).astype(np.float32))
    seeds = TR.find_pair_seeds(delta, img_hw, out_hw, rho, first=7000, align_corners=(True, False))
    img, pb, corners = TR.loss_inputs(seeds, img_hw, out_hw, rho)
    before = ops.get_warp_align_corners()
    try:
        for ac in (True, False):
            ops.set_warp_align_corners(ac)
            coord, diff, outside = TR.margins(delta, img, pb, corners, ac)
            assert coord > TR.MARGIN_COORD and diff >= TR.MARGIN_DIFF
            dr = delta.double().requires_grad_(True)
            ref = TR.photometric_loss(dr, img.double(), pb.double(), corners.double(), align_corners=ac)
            (3.0 * ref).backward()
            dg = delta.to(DEV).requires_grad_(True)
            loss = M.photometric_loss(dg, *_dev(img, pb, corners))
            assert loss.dim() == 0 and loss.requires_grad
            (3.0 * loss).backward()
            print(f"udh photometric loss img {img_hw} out {out_hw} align_corners {ac}: outside {outside:.3f}, loss {rel_err(loss, ref):.2e}, "
                  f"g_delta {rel_err(dg.grad, dr.grad):.2e}")
            assert_close(loss, ref, "loss")
            assert_close(dg.grad, dr.grad, "g_delta")
            dg2 = delta.to(DEV).requires_grad_(True)
            loss2 = M.photometric_loss(dg2, *_dev(img, pb, corners))
            (3.0 * loss2).backward()
            assert torch.equal(loss2, loss) and torch.equal(dg2.grad, dg.grad)
    finally:
        ops.set_warp_align_corners(before)


def test_photometric_loss_sign_of_zero_is_zero():
    """patch_b equal to the warp itself: every diff is exactly zero, so is the gradient (torch.sign(0) = 0)."""
    ops = _ops()
    delta = torch.zeros(2, 4, 2)
    img, _, corners = TR.loss_inputs([3, 4], (40, 48), (32, 32), 3.0)
    S = ops.udh_photo_matrix(corners.to(DEV), delta.to(DEV), (40, 48), (32, 32))
    pb = ops.warp_perspective(img.to(DEV), S, (32, 32))
    dg = delta.to(DEV).requires_grad_(True)
    loss = _M().photometric_loss(dg, img.to(DEV), pb, corners.to(DEV))
    loss.backward()
    assert float(loss) == 0.0 and float(dg.grad.abs().max()) == 0.0


# ---- 6. the whole step against the reference
@pytest.mark.parametrize("index", range(len(CASES)))
def test_step_parity_with_the_reference(fx, index):
    loss, delta, grads = _step(fx, index)
    assert loss.dim() == 0
    check_step(fx, index, loss, delta, grads, "udh training step on HIP")


# ---- 7. reproducibility
def test_step_is_bit_reproducible_in_deterministic_mode(fx):
    from masic_amd import determinism
    with determinism.deterministic():
        l1, d1, g1 = _step(fx, 1)
        g1 = {n: g.clone() for n, g in g1.items()}
        l2, d2, g2 = _step(fx, 1)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


# ---- 8. the reference's loop
def _training_loop(model_net, loss_fn, batch, masks_kw, steps=3):
    """udh/udh/train.py: configure_optimizers + training_step, three times."""
    class HomographyModel:
        def __init__(self):
            self.model = model_net

        def training_step(self, batch, batch_idx):
            img_a, img_b, patch_a, patch_b, corners, gt = batch
            delta = self.model(patch_a, patch_b)
            loss = loss_fn(delta, img_a, patch_b, corners)
            logs = {"loss": loss}
            return {"loss": loss, "log": logs}

    wrapper = HomographyModel()
    forward = model_net.forward
    model_net.forward = lambda a, b: forward(a, b, **masks_kw)         # the fixed masks; the caller's lines stay verbatim
    opt = torch.optim.Adam(model_net.parameters(), lr=1e-4, foreach=False, fused=False)
    losses = []
    try:
        for i in range(steps):
            opt.zero_grad()
            out = wrapper.training_step(batch, i)
            out["loss"].backward()
            opt.step()
            losses.append(float(out["loss"]))
        model_net.eval()
        with torch.no_grad():
            delta = forward(batch[2], batch[3])
    finally:
        del model_net.forward
    return torch.tensor(losses, dtype=torch.float64), delta.detach().cpu()


def test_three_adam_steps_of_the_reference_loop():
    p, B, img_hw, rho = 32, 4, (40, 48), 6.0
    a = UW.patches(77, B, p)[0]
    rs = np.random.default_rng(78)
    img, pb, corners = TR.loss_inputs([21, 22, 23, 24], img_hw, (p, p), rho)
    patch_b = torch.from_numpy(rs.standard_normal((B, 1, p, p), dtype=np.float32))
    m1 = torch.from_numpy((rs.random((B, 128 * 16)) >= 0.5).astype(np.uint8))
    m2 = torch.from_numpy((rs.random((B, 1024)) >= 0.5).astype(np.uint8))
    batch = (img, None, a, patch_b, corners, None)

    def ref_loop(dtype):
        net = TR.Net(p)
        UW.fill(net, UW.WEIGHT_SEED)
        net = net.to(dtype)
        cast = tuple(None if t is None else t.to(dtype) for t in batch)
        return _training_loop(net, TR.photometric_loss, cast, {"masks": (m1, m2)})

    l32, d32 = ref_loop(torch.float32)
    l64, d64 = ref_loop(torch.float64)
    floor_l, floor_d = rel_err(l32, l64), rel_err(d32, d64)
    net = _net(p, True)
    lg, dg = _training_loop(net, _M().photometric_loss, _dev(*batch), {"dropout_masks": _dev(m1, m2)})
    el, ed = rel_err(lg, l32), rel_err(dg, d32)
    print(f"udh reference loop: losses {lg.tolist()}, error {el:.2e} (floor {floor_l:.2e}), final delta error {ed:.2e} (floor {floor_d:.2e})")
    assert float(lg[0]) != float(lg[-1])
    assert_close(lg, l32, "losses", rtol=max(1e-4, 2 * floor_l))
    assert_close(dg, d32, "final delta", rtol=max(1e-4, 2 * floor_d))
    _CACHE["trained"] = net


# ---- 9. hand-over to the codec-side net
def test_trained_state_dict_loads_into_the_codec_side_net():
    import model as codec_model
    p, B = 32, 4
    net = _CACHE.get("trained")
    if net is None:
        net = _net(p, False)
    net.eval()
    a, b = _dev(*UW.patches(79, B, p))
    with torch.no_grad():
        mine = net(a, b)
    assert mine.grad_fn is None
    codec = codec_model.Net(patch_size=p).to(DEV).eval()
    codec.load_state_dict(net.state_dict())
    theirs = codec(a, b)
    assert torch.equal(mine, theirs)
    corners = TR.loss_inputs([31, 32, 33, 34], (40, 48), (p, p), 0.0)[2].to(DEV)
    h = codec.h_matrix(a, b, corners, (64, 96), (40, 48))
    assert tuple(h.shape) == (B, 3, 3) and bool(torch.isfinite(h).all())
    assert torch.equal(net.get_h(a, b, corners), codec.get_h(a, b, corners))


# ---- 10. training mode without given masks
def test_training_mode_draws_its_own_masks():
    p, B = 32, 2
    net = _net(p, True)
    a, b = _dev(*UW.patches(80, B, p))
    img, pb, corners = _dev(*TR.loss_inputs([41, 42], (40, 48), (p, p), 6.0))
    d1, d2 = net(a, b), net(a, b)
    assert d1.grad_fn is not None and not torch.equal(d1, d2)
    loss = _M().photometric_loss(d1, img, pb, corners)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in net.parameters())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        d3 = net(a, b)
    torch.cuda.synchronize()
    assert d3.grad_fn is None and not d3.requires_grad
    assert torch.cuda.memory_allocated() - before <= d3.numel() * 4 + 512      # nothing but the output survives the call
    # the node saves the parameters: an in-place update between forward and backward is refused, not silently mixed in
    d4 = net(a, b)
    with torch.no_grad():
        net.fc[5].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        d4.sum().backward()
    net.eval()
    with torch.no_grad():
        assert torch.equal(net(a, b), net(a, b))
