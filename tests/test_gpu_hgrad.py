"""Gradients with respect to h_matrix: the warp differentiated in its 3 x 3 matrix (masic_amd/csrc/warp_bwd_matrix.hip), the adjoints of
the two homography chains, and HSIC.forward differentiable in h_matrix.  References: float64 torch autograd over the CPU oracle.

Comparisons are made only on ADMITTED cases (tests/hgrad_cases.py: the oracle's float32 and float64 gradients agree to 1e-4; off the
cell boundaries of the bilinear sample); tests/test_cpu_hgrad.py asserts that every named case is admitted, and the tests here assert it
again before they compare, so nothing is skipped silently."""
import functools

import pytest
import torch

from oracle import hsic_oracle as O
from tests import hgrad_cases as HC
from tests import udh_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = 2e-4          # what tests/test_gpu_backward.py holds the parameter gradients of the same training step to
FACTOR = 4.0         # x e32: covers last-bit differences of minv_norm / the sampling coordinates between the two float32 chains


def _matrix_grad(case, M=None, src=None, g_dst=None):
    """(d loss / d M [B,3,3], the slots [B,slots,9]) of one case on the HIP kernels: sampling matrix as the forward makes it, the warp's
    matrix gradient, the chain's adjoint."""
    from masic_amd import homography, ops
    M = (case.M if M is None else M).to(DEV)
    src = case.src if src is None else src
    g_dst = (case.g_dst if g_dst is None else g_dst).to(DEV)
    B = M.shape[0]
    prev = ops.get_warp_align_corners()
    ops.set_warp_align_corners(case.align_corners)
    try:
        minv, _ = homography.warp_matrices(M, case.src_hw, case.dst_hw)
        if case.ones:
            part = ops.warp_perspective_bwd_matrix(None, minv, g_dst, ones_like=(B,) + case.src_hw)
        else:
            part = ops.warp_perspective_bwd_matrix(src.to(DEV), minv, g_dst)
        g = ops.warp_matrix_bwd(M, case.src_hw, case.dst_hw, g_fwd=part)
    finally:
        ops.set_warp_align_corners(prev)
    return g, part


@pytest.mark.parametrize("case", HC.operator_cases(), ids=lambda c: c.name)
def test_warp_matrix_gradient_vs_float64_oracle(case):
    e32, g64 = case.admission()
    assert e32 <= HC.ADMIT, (case.name, e32)
    g, part = _matrix_grad(case)
    assert part.dtype == torch.float64 and tuple(part.shape[::2]) == (case.M.shape[0], 9)
    err = HC.rel(g, g64)
    print(f"{case.name}: error {err:.2e}, oracle float32 vs float64 e32 {e32:.2e}, ratio {err / e32:.2f}")
    assert err <= FACTOR * e32, (case.name, err, e32)


@pytest.mark.parametrize("case", HC.ones_cases(), ids=lambda c: c.name)
def test_ones_source_matrix_gradient(case):
    e32, g64 = case.admission()
    g, part = _matrix_grad(case)
    if case.kind == "magnify1.5":
        # every sample lies inside the source: the warped mask is 1 whatever the matrix, and each tap difference is exactly 0
        assert float(g64.abs().max()) == 0.0
        assert float(part.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
        return
    assert e32 <= HC.ADMIT, (case.name, e32)
    err = HC.rel(g, g64)
    print(f"{case.name}: error {err:.2e}, e32 {e32:.2e}, ratio {err / e32:.2f}")
    assert err <= FACTOR * e32, (case.name, err, e32)


def test_reproducible_and_batch_invariant():
    kinds = ["rotate12", "projective", "translate"]
    case = HC.Case("mixed", "rotate12", 3, 5, (48, 64), (32, 40), seed=400)
    M = HC.matrices(kinds, case.src_hw)
    g0, p0 = _matrix_grad(case, M=M)
    g1, p1 = _matrix_grad(case, M=M)
    assert torch.equal(p0, p1) and torch.equal(g0, g1), "two calls on the same inputs must give the same bits"
    assert p0.shape[1] > 1, "more than one workgroup per item"
    for n in range(3):
        gn, pn = _matrix_grad(case, M=M[n:n + 1], src=case.src[n:n + 1], g_dst=case.g_dst[n:n + 1])
        assert torch.equal(pn[0], p0[n]) and torch.equal(gn[0], g0[n]), f"item {n} alone differs from item {n} of the batch"


@pytest.mark.parametrize("case", HC.rejected_cases(), ids=lambda c: c.name)
def test_rejected_kinds_are_finite_and_reproducible(case):
    """Samples on cell boundaries: the derivative taken is the forward's own cell's, a valid one-sided one; nothing to compare it with."""
    g0, p0 = _matrix_grad(case)
    g1, p1 = _matrix_grad(case)
    assert bool(torch.isfinite(g0).all()) and bool(torch.isfinite(p0).all())
    assert torch.equal(p0, p1) and torch.equal(g0, g1)


def test_warp_nodes_return_the_slot_sums():
    """WarpFn / WarpOnesFn hand autograd the sum of the slots (a fixed order, float64), rounded once to float32; WarpFn keeps its source gradient."""
    from masic_amd import autograd as A, homography, ops
    case = HC.Case("nodes", "projective", 2, 3, (48, 64), (32, 40), seed=500)
    M = case.M.to(DEV)
    minv, _ = homography.warp_matrices(M, case.src_hw, case.dst_hw)
    src, g_dst = case.src.to(DEV), case.g_dst.to(DEV)
    part = ops.warp_perspective_bwd_matrix(src, minv, g_dst)
    m = minv.clone().requires_grad_(True)
    s = src.clone().requires_grad_(True)
    A.WarpFn.apply(s, m, case.dst_hw).backward(g_dst)
    assert torch.equal(m.grad, part.sum(1).float().view(2, 3, 3)) or HC.rel(m.grad, part.sum(1).view(2, 3, 3)) <= 2.0 ** -23
    assert torch.equal(s.grad, ops.warp_perspective_bwd(g_dst, minv, tuple(src.shape)))
    m2 = minv.clone().requires_grad_(True)
    A.WarpFn.apply(src, m2, case.dst_hw).backward(g_dst)          # the source does not require grad: the matrix gradient alone
    assert torch.equal(m2.grad, m.grad)
    m3 = minv.clone().requires_grad_(True)
    g1 = g_dst[:, :1].contiguous()
    A.WarpOnesFn.apply(m3, (2,) + case.src_hw, case.dst_hw).backward(g1)
    p1 = ops.warp_perspective_bwd_matrix(None, minv, g1, ones_like=(2,) + case.src_hw)
    assert HC.rel(m3.grad, p1.sum(1).view(2, 3, 3)) <= 2.0 ** -23
    ones = torch.ones((2, 1) + case.src_hw, device=DEV)
    p2 = ops.warp_perspective_bwd_matrix(ones, minv, g1)
    assert torch.equal(p1, p2), "the all-ones source is the C = 1 source of ones"


# ---------------------------------------------------------------------------------------------- the two chains' adjoints
def _h_adjust(h, a, b):
    """newtrain_codec_real.py:49-59, out of place"""
    rows = torch.tensor([a, b, 1.0], dtype=h.dtype).view(1, 3, 1)
    cols = torch.tensor([1.0 / a, 1.0 / b, 1.0], dtype=h.dtype).view(1, 1, 3)
    return h * rows * cols


def test_warp_matrix_bwd_vs_float64_autograd():
    """Both sides take the float32 inputs exactly and work in float64; the only difference is the float32 store: 1e-6 of the largest entry."""
    from masic_amd import ops
    B, src_hw, dst_hw = 3, (48, 64), (32, 40)
    M = HC.matrices(["rotate12", "projective", "translate"], src_hw)
    gen = torch.Generator().manual_seed(5)
    slots_f = torch.randn((B, 130, 9), generator=gen).double()          # more slots than a wave has lanes
    slots_i = torch.randn((B, 2, 9), generator=gen).double()

    def ref(use_f, use_i):
        m = M.double().clone().requires_grad_(True)
        loss = 0.0
        if use_f:
            loss = loss + (R.sampling_matrix(m, src_hw, dst_hw) * slots_f.sum(1).view(B, 3, 3)).sum()
        if use_i:
            loss = loss + (R.sampling_matrix(torch.inverse(m), src_hw, dst_hw) * slots_i.sum(1).view(B, 3, 3)).sum()
        loss.backward()
        return m.grad

    Md = M.to(DEV)
    for use_f, use_i in ((True, False), (False, True), (True, True)):
        want = ref(use_f, use_i)
        got = ops.warp_matrix_bwd(Md, src_hw, dst_hw, slots_f.to(DEV) if use_f else None, slots_i.to(DEV) if use_i else None)
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print(f"warp_matrix_bwd forward {use_f} inverse {use_i}: max error {err:.2e} of the largest entry")
        assert err <= 1e-6, (use_f, use_i, err)
        # float32 [B,3,3] gradients, as autograd hands them over: the same adjoint on the same values
        f32 = [t.sum(1).float().view(B, 3, 3).contiguous().to(DEV) if u else None for t, u in ((slots_f, use_f), (slots_i, use_i))]
        want32 = ops.warp_matrix_bwd(Md, src_hw, dst_hw, None if f32[0] is None else f32[0].double(), None if f32[1] is None else f32[1].double())
        assert torch.equal(ops.warp_matrix_bwd(Md, src_hw, dst_hw, f32[0], f32[1]), want32)


def test_homography_from_corners_bwd_vs_float64_autograd():
    from masic_amd import ops
    B = 3
    ori_hw, patch_hw = (96, 160), (128, 128)
    gen = torch.Generator().manual_seed(9)
    base = torch.tensor([[32.0, 24.0], [159.0, 24.0], [159.0, 151.0], [32.0, 151.0]])
    corners = (base.unsqueeze(0) + torch.randint(-8, 9, (B, 1, 2), generator=gen).float()).contiguous()
    delta = (torch.rand((B, 4, 2), generator=gen) * 12.0 - 6.0).contiguous()
    g_h = torch.randn((B, 3, 3), generator=gen)
    a, b = ori_hw[0] / patch_hw[0], ori_hw[1] / patch_hw[1]
    q = (corners + delta).double()                               # corners_hat is formed in float32
    d = torch.zeros_like(q, requires_grad=True)
    h = _h_adjust(torch.inverse(R.get_perspective_transform(corners.double(), q + d)), a, b)
    (h * g_h.double()).sum().backward()
    fwd = ops.homography_from_corners(corners.to(DEV), delta.to(DEV), ori_hw, patch_hw)
    assert float((fwd.cpu().double() - h.detach()).abs().max() / h.detach().abs().max()) <= 1e-6
    got = ops.homography_from_corners_bwd(corners.to(DEV), delta.to(DEV), g_h.to(DEV), ori_hw, patch_hw)
    err = float((got.cpu().double() - d.grad).abs().max() / d.grad.abs().max())
    print(f"homography_from_corners_bwd: max error {err:.2e} of the largest entry")
    assert tuple(got.shape) == (B, 4, 2) and err <= 1e-6, err


# ---------------------------------------------------------------------------------------------- model level
NMK = (16, 24, 3)
LMBDA = 0.01


@functools.lru_cache(maxsize=None)
def _small_setup():
    import MASIC
    from masic_amd import synth
    N, M, K = NMK
    sd0 = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=31)
    x1, x2, _ = synth.synth_inputs(2, 64, 64, seed=31)
    noise = synth.synth_noise(2, N, M, 64, 64, seed=40)
    return sd0, x1, x2, HC.model_h_matrices((64, 64)), noise


@functools.lru_cache(maxsize=None)
def _oracle_h_grad():
    """(e32, d loss / d h_matrix in float64) of the training-mode step over oracle.hsic_oracle.hsic_forward"""
    sd0, x1, x2, hm, noise = _small_setup()

    def grad(dt):
        sd = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        for cp in ("context_prediction1.weight", "context_prediction2.weight"):
            sd[cp] = O.masked_weight(sd[cp])
        h = hm.to(dt).clone().requires_grad_(True)
        out = O.hsic_forward(sd, x1.to(dt), x2.to(dt), h, K=NMK[2], training=True, noise={k: v.to(dt) for k, v in noise.items()})
        O.rd_loss(out, x1.to(dt), x2.to(dt), LMBDA)["loss"].backward()
        return h.grad.detach()

    g64 = grad(torch.float64)
    return HC.rel(grad(torch.float32), g64), g64


def _small_net():
    import MASIC
    net = MASIC.HSIC(*NMK)
    net.load_state_dict(_small_setup()[0])
    return net.to(DEV).train()


def _small_step(net, hm, streams=None):
    """one training-mode forward + rate_distortion + backward with the oracle's noise; returns (loss, output dict)"""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd.loss import rate_distortion
    _, x1, x2, _, noise = _small_setup()
    queue = [noise[k].to(DEV) for k in O.NOISE_KEYS]
    orig, prev = EntropyModel._get_noise_cached, MASIC._TRAIN_STREAMS
    EntropyModel._get_noise_cached = lambda self, x: queue.pop(0).reshape(x.shape).contiguous()
    if streams is not None:
        MASIC._TRAIN_STREAMS = streams
    try:
        for _, p in net.named_parameters():          # (HSIC.parameters() leaves out the entropy bottlenecks')
            p.grad = None
        x1, x2 = x1.to(DEV), x2.to(DEV)
        out = net(x1, x2, hm)
        loss = rate_distortion(out, x1, x2, LMBDA)["loss"]
        loss.backward()
        torch.cuda.synchronize()
    finally:
        EntropyModel._get_noise_cached = orig
        MASIC._TRAIN_STREAMS = prev
    return loss.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


def test_model_h_matrix_gradient_vs_float64_oracle():
    """HSIC(16,24,3), B=2, 64 x 64, .train(), float32 operands, the oracle's noise, loss = rate_distortion: h_matrix.grad against float64
    autograd over the CPU oracle, bound 4 x max(e32, GTOL).  On the parent commit h_matrix.grad is None.
    The parameter gradients of that run (side streams on) equal, bit for bit, those of a run with h_matrix detached on one stream; both
    runs are made in the deterministic mode (masic_amd/determinism.py), the mode in which a step's bits are defined at all -- by
    default the large weight gradients are float-atomic sums whose last bits depend on timing."""
    from masic_amd import determinism
    e32, g64 = _oracle_h_grad()
    print(f"model level: oracle float32 vs float64 h_matrix gradient e32 {e32:.2e}")
    assert e32 <= HC.ADMIT, e32
    hm = _small_setup()[3]
    net = _small_net()
    with determinism.deterministic():
        h = hm.to(DEV).requires_grad_(True)
        loss_h, grads_h = _small_step(net, h, streams=True)
        assert h.grad is not None, "h_matrix.requires_grad must yield h_matrix.grad"
        loss_d, grads_d = _small_step(net, hm.to(DEV), streams=False)
    err = HC.rel(h.grad, g64)
    print(f"model level: h_matrix.grad error {err:.2e} (bound {FACTOR * max(e32, GTOL):.1e})")
    assert tuple(h.grad.shape) == (2, 3, 3) and h.grad.dtype == torch.float32
    assert err <= FACTOR * max(e32, GTOL), (err, e32)
    assert torch.equal(loss_h, loss_d)
    assert grads_h.keys() == grads_d.keys() and len(grads_h) > 100
    differing = [n for n in grads_h if not torch.equal(grads_h[n], grads_d[n])]
    assert not differing, differing


def test_model_h_matrix_gradient_bf16_operands():
    """HSIC(128,192,5), 2 x 128 x 128, the bf16-operand training step (fused transform nodes, device sampling-matrix kernel, side streams):
    h_matrix.grad against the float32-mode gradient on the same weights, inputs and noise.  Bounds set the way
    test_training_step_bf16_mode_against_float32 sets its own, what is measured plus margin: measured relative error 2.0e-3 and cosine
    1.00000 (18 numbers, every one a sum over all pixels of the four warps, so the operand roundings average out further than in a weight
    gradient) -> relative error <= 1e-2, that test's own bound on the median parameter gradient and 5 x the measured value; and cosine
    >= 0.9999, which is what a relative error of 1e-2 leaves of it (1 - 1e-4 / 2).  A contribution to h_matrix.grad that is dropped or mis-scaled by more than
    1 % of the whole gradient fails the first."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn, synth
    from masic_amd.loss import rate_distortion
    N, M, K = 128, 192, 5
    hm = HC.model_h_matrices((128, 128))

    def run(prec):
        mnn.set_precision(prec)
        try:
            net = MASIC.HSIC(N, M, K)
            net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=7))
            net = net.to(DEV).train()
            x1, x2, _ = (t.to(DEV) for t in synth.synth_inputs(2, 128, 128, seed=7))
            h = hm.to(DEV).requires_grad_(True)
            g = torch.Generator(device=DEV)
            g.manual_seed(7)
            orig = EntropyModel._get_noise_cached
            EntropyModel._get_noise_cached = lambda self, x: torch.rand(x.shape, device=x.device, generator=g) - 0.5
            try:
                out = net(x1, x2, h)
            finally:
                EntropyModel._get_noise_cached = orig
            rate_distortion(out, x1, x2, LMBDA)["loss"].backward()
            torch.cuda.synchronize()
            return h.grad.detach().double().cpu().flatten()
        finally:
            mnn.set_precision("f32")

    gf, gb = run("f32"), run("bf16")
    assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gb).all())
    cos = float((gf @ gb) / (gf.norm() * gb.norm()))
    err = float((gf - gb).norm() / gf.norm())
    print(f"bf16-operand step, h_matrix.grad vs float32 mode: cosine {cos:.5f}, relative error {err:.2e}")
    assert err <= 1e-2, err
    assert cos >= 0.9999, cos


def test_delta_to_loss_end_to_end():
    """delta.requires_grad -> h_matrix_from_corners -> HSIC -> loss.backward(): delta.grad is homography_from_corners_bwd(h_matrix.grad)."""
    from masic_amd import homography, ops
    ori_hw, patch_hw = (64, 64), (128, 128)
    corners = torch.tensor([[32.0, 32.0], [159.0, 32.0], [159.0, 159.0], [32.0, 159.0]]).repeat(2, 1, 1).to(DEV)
    delta = torch.tensor([[[1.3, -0.7], [-2.1, 0.4], [0.9, 1.6], [-0.5, -1.2]], [[-3.2, 0.8], [-2.6, 1.1], [-3.4, 0.3], [-2.9, 1.5]]]).to(DEV).requires_grad_(True)
    h = homography.h_matrix_from_corners(corners, delta, ori_hw, patch_hw)
    assert h.requires_grad and torch.equal(h.detach(), ops.homography_from_corners(corners, delta.detach(), ori_hw, patch_hw))
    h.retain_grad()
    _small_step(_small_net(), h)
    assert h.grad is not None and delta.grad is not None and bool(torch.isfinite(delta.grad).all()) and float(delta.grad.abs().max()) > 0.0
    assert torch.equal(delta.grad, ops.homography_from_corners_bwd(corners, delta.detach(), h.grad, ori_hw, patch_hw))


def test_detached_h_matrix_never_reaches_the_new_ops(monkeypatch):
    from masic_amd import ops

    def refuse(*a, **k):
        raise AssertionError("a matrix-gradient op was called for an h_matrix that does not require grad")
    for name in ("warp_perspective_bwd_matrix", "warp_matrix_bwd", "homography_from_corners_bwd"):
        monkeypatch.setattr(ops, name, refuse)
    hm = _small_setup()[3].to(DEV)
    loss, grads = _small_step(_small_net(), hm)
    assert hm.grad is None and bool(torch.isfinite(loss)) and len(grads) > 100


def test_unsupported_h_matrix_gradients_raise():
    import MASIC
    from masic_amd.graph import GraphedTrainStep
    _, x1, x2, hm, _ = _small_setup()
    x1, x2 = x1.to(DEV), x2.to(DEV)
    h = hm.to(DEV).requires_grad_(True)
    net = _small_net()
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(net, x1, x2, h, LMBDA)
    net.eval()
    with pytest.raises(NotImplementedError):
        net(x1, x2, h)
    with torch.no_grad():
        net(x1, x2, h)                                   # nothing to differentiate: as before
    en = MASIC.Independent_EN().to(DEV)
    with pytest.raises(NotImplementedError):
        en(x1, x2, h)
    en(x1, x2, h.detach())


def test_graphed_train_step_call_refuses_h_matrix_gradient():
    """A GraphedTrainStep captured with a detached h_matrix refuses a gradient-requiring one when called, and still replays afterwards."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn, synth
    from masic_amd.graph import GraphedTrainStep
    N, M, K, B, H, W = 16, 32, 3, 2, 64, 64
    x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=60))
    noise = synth.synth_noise(B, N, M, H, W, seed=70)
    slots = [noise[k].to(DEV) for k in O.NOISE_KEYS]
    state = {"i": 0}

    def static_noise(self, x):
        t = slots[state["i"] % len(slots)]
        state["i"] += 1
        return t.reshape(x.shape)

    orig, prev = EntropyModel._get_noise_cached, MASIC._TRAIN_STREAMS
    EntropyModel._get_noise_cached = static_noise
    MASIC._TRAIN_STREAMS = False
    mnn.set_precision("bf16")
    try:
        net = MASIC.HSIC(N, M, K)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=55))
        step = GraphedTrainStep(net.to(DEV).train(), x1, x2, hm, LMBDA, warmup=1)
        with pytest.raises(NotImplementedError):
            step(x1, x2, hm.clone().requires_grad_(True))
        crit, _ = step(x1, x2, hm)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(crit["loss"]))
    finally:
        EntropyModel._get_noise_cached = orig
        MASIC._TRAIN_STREAMS = prev
        mnn.set_precision("f32")
