"""GPU tests (-m gpu) of the deterministic mode (masic_amd/determinism.py): every weight-gradient family and the warp backward's
fallback against float64 references, bitwise repeatability (alone, and on a side stream while another stream is busy), and whole
training steps that must agree to the bit: two runs, side streams against one stream, a captured graph against the eager step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hsic_oracle as O
from tests.util import assert_close, golden_state_dict, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = 2e-4          # tests/test_gpu_backward.py


def _rand(*shape, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(size=shape) * scale).astype(np.float32))


def _bf(t):
    return t.bfloat16().float()


def _repeatable(fn, what):
    """ten calls give the same bits; a call on a side stream while the current stream runs a large convolution gives them too"""
    first = fn()
    torch.cuda.synchronize()
    for _ in range(9):
        assert torch.equal(fn(), first), what + ": two calls differ"
    big_x = torch.randn(8, 128, 128, 128, device=DEV)
    big_w = torch.randn(128, 128, 5, 5, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        F.conv2d(big_x, big_w, padding=2)       # keeps the current stream busy
    with torch.cuda.stream(side):
        got = fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(got, first), what + ": a call on a side stream under load differs"
    return first


def _wgrad_ref(x, dy, k, s, tr):
    """float64 autograd weight gradient of Conv2d / ConvTranspose2d (padding k // 2, output_padding s - 1)"""
    B, Cin = x.shape[:2]
    Cout = dy.shape[1]
    w = torch.zeros((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    y = (F.conv_transpose2d(x.double(), w, stride=s, padding=k // 2, output_padding=s - 1) if tr
         else F.conv2d(x.double(), w, stride=s, padding=k // 2))
    y.backward(dy.double())
    return w.grad


from tests.test_gpu_backward import CONV_BWD_CASES, WGRAD_BF16_CASES     # noqa: E402  (the shapes of the default kernel's tests)

NCHW_CASES = [("f32",) + c for c in CONV_BWD_CASES if not c[9]] + [("bf16",) + c for c in WGRAD_BF16_CASES if not c[9]] + [
    # more than one split in deterministic mode for every kernel family (the query is >= 2 x |dW| * 4 bytes: checked below)
    ("bf16", "k5s2_wide", 8, 192, 64, 64, 192, 5, 2, False, False, 0),
    ("bf16", "gemm1x1_deep", 8, 320, 32, 32, 192, 1, 1, False, False, 0),
]


@pytest.mark.parametrize("case", NCHW_CASES, ids=[c[0] + "-" + c[1] for c in NCHW_CASES])
def test_conv2d_wgrad_det(case):
    """masic_conv2d_wgrad_det against float64 autograd (float32 operands: GTOL as test_conv_backward; bf16 operands: on the rounded
    operands at the bf16 test's 2e-5 of the peak), ten calls bitwise equal, a side-stream call under load bitwise equal."""
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16, PREC_F32
    from masic_amd.determinism import deterministic
    prec, name, B, Cin, H, W, Cout, k, s, tr, masked, act = case
    d = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=tr, prec=PREC_BF16 if prec == "bf16" else PREC_F32)
    x = _rand(B, Cin, H, W, seed=11, scale=2.0)
    dy = _rand(B, Cout, d.Ho, d.Wo, seed=12)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    nbytes = ops._desc_query("masic_conv2d_wgrad_det_workspace_bytes", d)
    wb = Cin * Cout * k * k * 4
    assert nbytes > 0 and nbytes % wb == 0 and nbytes <= max(64 << 20, 8 * wb), (nbytes, wb)
    if name in ("k5s2_wide", "gemm1x1_deep"):
        assert nbytes >= 2 * wb, "this case must run more than one split"
    xd, dyd = x.to(DEV), dy.to(DEV)
    with deterministic():
        got = _repeatable(lambda: ops.conv2d_wgrad(xd, dyd, d, wshape), name)
        if prec == "bf16" and ops.conv2d_wgrad_b16_supported(d):     # the bf16-input kernel: same operand values, same bits
            assert torch.equal(ops.conv2d_wgrad(xd.bfloat16(), dyd.bfloat16(), d, wshape), got), name + ": bf16 NCHW operands"
    if prec == "bf16":
        want = _wgrad_ref(_bf(x), _bf(dy), k, s, tr)
        assert float((got.cpu().double() - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-6, name
    else:
        assert_close(got, _wgrad_ref(x, dy, k, s, tr), name + ":dw", GTOL)
    # the default path afterwards is still the default (no state left behind by the deterministic call)
    dflt = ops.conv2d_wgrad(xd, dyd, d, wshape)
    assert float((dflt - got).abs().max()) <= 1e-4 * float(got.abs().max()) + 1e-6


K3_CASES = [(3, 2, 32, 32, 16, 64), (3, 1, 64, 96, 24, 40), (3, 2, 96, 64, 9, 70), (3, 1, 96, 96, 64, 64), (3, 1, 128, 32, 8, 32),
            (5, 2, 192, 384, 16, 24), (5, 1, 32, 96, 7, 9), (5, 8, 192, 128, 32, 32), (5, 1, 64, 32, 20, 70), (5, 3, 288, 384, 8, 8),
            (3, 8, 96, 96, 128, 128)]         # Independent_EN's layer shape: many splits


@pytest.mark.parametrize("KS,B,Cin,Cout,H,W", K3_CASES)
def test_conv_wgrad_f16k_det(KS, B, Cin, Cout, H, W):
    """masic_conv{3x3,5x5}_wgrad_f16k_det against float64 on the bf16-rounded operands (the F16K tests' 1e-5), repeatable to the bit."""
    from masic_amd import ops
    from masic_amd.determinism import deterministic
    g = torch.Generator().manual_seed(H * W + Cin)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    q = f"masic_conv{KS}x{KS}_wgrad_f16k_det_workspace_bytes"
    nbytes = ops._int_query(q, B, Cin, Cout, H, W)
    wb = KS * KS * Cin * Cout * 4
    assert nbytes % wb == 0 and wb <= nbytes <= max(64 << 20, wb)
    if (KS, B, H) in ((3, 8, 128), (5, 8, 32)):
        assert nbytes >= 2 * wb
    fn = ops.conv3x3_wgrad_f16k if KS == 3 else ops.conv5x5_wgrad_f16k
    x16, g16 = ops.nchw_to_f16k(x.to(DEV)), ops.nchw_to_f16k(dy.to(DEV))
    with deterministic():
        got = _repeatable(lambda: fn(x16, g16, B, Cin, Cout, H, W), f"wgrad{KS}_f16k")
    w = torch.zeros((Cout, Cin, KS, KS), dtype=torch.float64, requires_grad=True)
    F.conv2d(_bf(x).double(), w, padding=KS // 2).backward(_bf(dy).double())
    assert_close(got, w.grad, f"conv{KS}x{KS}_wgrad_f16k_det {Cin}->{Cout}", 1e-5)


GEMM1_CASES = [(2, 1152, 768, 16, 24), (3, 96, 160, 7, 9), (1, 768, 960, 32, 32), (2, 32, 48, 5, 3), (8, 384, 256, 32, 32)]


@pytest.mark.parametrize("B,Cout,Cin,H,W", GEMM1_CASES)
def test_gemm_wgrad_f16k_det(B, Cout, Cin, H, W):
    """masic_gemm_wgrad_bias_f16k_det, both orientations and both bias modes, against float64 on the bf16-rounded operands (2e-5 of the
    peak, as the default kernel's test), repeatable to the bit, bias sums included."""
    from masic_amd import ops
    from masic_amd.determinism import deterministic
    x = _rand(B, Cin, H, W, seed=1, scale=1.5)
    dy = _rand(B, Cout, H, W, seed=2)
    q = lambda t: t.bfloat16().double()
    want = torch.einsum("bohw,bchw->oc", q(dy), q(x))
    bsum = q(dy).sum(dim=(0, 2, 3))
    for bias_of, CA, CQ in ((0, Cout, Cin), (1, Cout, Cin), (2, Cin, Cout)):
        nbytes = ops._int_query("masic_gemm_wgrad_bias_f16k_det_workspace_bytes", bias_of, B, CA, CQ, H * W)
        assert nbytes % (CA * CQ * 4) == 0 and nbytes >= CA * CQ * 4
    if B == 8:
        assert ops._int_query("masic_gemm_wgrad_bias_f16k_det_workspace_bytes", 0, B, Cout, Cin, H * W) >= 2 * Cout * Cin * 4
    x16, g16 = ops.nchw_to_f16k(x.to(DEV)), ops.nchw_to_f16k(dy.to(DEV))
    with deterministic():
        got = _repeatable(lambda: ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W), "gemm_wgrad_f16k")
        b1 = _repeatable(lambda: torch.cat([t.reshape(-1) for t in ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W, bias_of=1)]), "bias_of=1")
        b2 = _repeatable(lambda: torch.cat([t.reshape(-1) for t in ops.gemm_wgrad_f16k(x16, g16, B, Cin, Cout, H * W, bias_of=2)]), "bias_of=2")
    peak = float(want.abs().max())
    assert float((got.cpu().double() - want).abs().max()) <= 2e-5 * peak
    n = Cout * Cin
    assert torch.equal(b1[:n].view(Cout, Cin), got), "bias_of=1: the same weight gradient"
    assert float((b2[:n].view(Cin, Cout).cpu().double() - want.t()).abs().max()) <= 2e-5 * peak
    for db in (b1[n:], b2[n:]):
        assert float((db.cpu().double() - bsum).abs().max()) <= 2e-5 * float(q(dy).abs().sum(dim=(0, 2, 3)).max())


def test_det_digests_are_the_recorded():
    """Every deterministic weight gradient of the three case lists above has the bits recorded in tests/golden/wgrad_det_digest.json
    (tests/golden/make_wgrad_det_digest.py: written before the host side became a plan and a table) -- same kernels, same grids, same
    split counts, same order of the sums."""
    import importlib.util
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_wgrad_det_digest", os.path.join(here, "golden", "make_wgrad_det_digest.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(here, "golden", "wgrad_det_digest.json")) as f:
        want = json.load(f)
    got = gen.digests(NCHW_CASES, K3_CASES, GEMM1_CASES, DEV)
    assert got.keys() == want.keys() and len(got) >= len(NCHW_CASES) + len(K3_CASES) + 3 * len(GEMM1_CASES)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} digests differ: {bad[:8]}"


def _warp_case(kind, B=2, H=48, W=64):
    """the homographies of tests/test_gpu_backward.py::test_warp_backward_gather_form_is_the_adjoint"""
    from masic_amd import synth
    x, _, hm = synth.synth_inputs(B, H, W, seed=14)
    x = torch.cat([x, x[:, :2] * 0.5], 1)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    if kind == "strong_magnify":
        hm = torch.tensor([[4.0, 0.0, cx - 4.0 * cx], [0.0, 4.0, cy - 4.0 * cy], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    elif kind == "horizon":
        hm = torch.eye(3).repeat(B, 1, 1)
        hm[:, 2, 0] = -1.0 / 40.0
    elif kind == "rotation":
        import math
        t = math.radians(12)
        a, b_, c, d = math.cos(t), -math.sin(t), math.sin(t), math.cos(t)
        hm = torch.tensor([[a, b_, cx - a * cx - b_ * cy], [c, d, cy - c * cx - d * cy], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    return x, hm


@pytest.mark.parametrize("kind", ["strong_magnify", "horizon", "synthetic", "rotation"])
def test_warp_backward_det(kind):
    """The two flag-raising homographies take the deterministic store-and-sum fallback: flag raised, the oracle's adjoint (off the
    horizon, as the default test) and the scatter form's values (2e-5), two calls bitwise equal.  On the gather path both modes give the
    same bits."""
    from masic_amd import ops
    from masic_amd.determinism import deterministic
    from masic_amd.homography import warp_matrices
    B, C, H, W = 2, 5, 48, 64
    x, hm = _warp_case(kind)
    xr = x.clone().requires_grad_(True)
    yr = O.warp_perspective(xr, hm, (H, W))
    go = _rand(*yr.shape, seed=15)
    yr.backward(go)
    m, _ = warp_matrices(hm.to(DEV), (H, W), (H, W))
    g = go.to(DEV).contiguous()
    with deterministic():
        got, flag = ops.warp_perspective_bwd(g, m, (B, C, H, W), want_flag=True)
        again, _ = ops.warp_perspective_bwd(g, m, (B, C, H, W), want_flag=True)
    dflt, dflag = ops.warp_perspective_bwd(g, m, (B, C, H, W), want_flag=True)
    fell_back = bool(int(flag.item()))
    assert fell_back == (kind in ("strong_magnify", "horizon")) and fell_back == bool(int(dflag.item())), kind
    assert torch.equal(got, again), kind + ": two calls differ"
    if not fell_back:
        assert torch.equal(got, dflt), kind + ": the gather path must not depend on the mode"
    ref = ops.zeros((B, C, H, W), torch.float32, DEV)
    ops.check(ops.lib.masic_warp_perspective_bwd(ops._p(g), ops._p(m), ops._p(ref), B, C, H, W, H, W, ops._stream()), "warp_perspective_bwd")
    assert_close(got, ref.cpu(), "warp det vs scatter", 2e-5)
    if kind != "horizon":
        assert_close(got, xr.grad, "warp det vs oracle autograd", GTOL)


# ------------------------------------------------------------------------------------------------ whole training steps
def _hsic_setup(N, M, K, B, H, W, nsteps=3):
    import MASIC
    from masic_amd import synth
    sd0 = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=55)
    batches = [tuple(t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=60 + i)) for i in range(nsteps)]
    noises = [synth.synth_noise(B, N, M, H, W, seed=70 + i) for i in range(nsteps)]
    return sd0, batches, noises


class _StaticNoise:
    """the seven noise draws of a step from static buffers refilled before each step (as the graphed-step test does)"""

    def __init__(self, noises):
        self.noises = noises
        self.slots = [noises[0][k].to(DEV).clone() for k in O.NOISE_KEYS]
        self.i = 0

    def __call__(self, model, x):
        t = self.slots[self.i % len(self.slots)]
        self.i += 1
        return t.reshape(x.shape)

    def load(self, it):
        self.i = 0
        for s, k in zip(self.slots, O.NOISE_KEYS):
            s.copy_(self.noises[it][k].to(DEV))


def _run_eager(sd0, batches, noise, N, M, K, streams):
    """three eager train_steps with the graph's optimizer flavour; returns (losses, grads after each step, final parameters)"""
    import MASIC
    from masic_amd import train
    prev, MASIC._TRAIN_STREAMS = MASIC._TRAIN_STREAMS, streams
    try:
        net = MASIC.HSIC(N, M, K)
        net.load_state_dict(sd0)
        net = net.to(DEV).train()
        opt = torch.optim.Adam(list(net.parameters()), lr=1e-4, capturable=True, fused=True)
        aopt = torch.optim.Adam(list(net.aux_parameters()), lr=1e-3, capturable=True, fused=True)
        losses, grads = [], []
        for it in range(len(batches)):
            noise.load(it)
            crit, aux = train.train_step(net, opt, aopt, *batches[it], 0.01)
            losses.append(torch.stack([crit["loss"].detach().reshape(()), aux.detach().reshape(())]).cpu())
            grads.append({n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        return losses, grads, {n: p.detach().clone() for n, p in net.named_parameters()}
    finally:
        MASIC._TRAIN_STREAMS = prev


def _assert_same_run(a, b, what):
    la, ga, pa = a
    lb, gb, pb = b
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), f"{what}: losses of step {i} differ ({x.tolist()} vs {y.tolist()})"
    for i, (x, y) in enumerate(zip(ga, gb)):
        assert x.keys() == y.keys(), what
        bad = [n for n in x if not torch.equal(x[n], y[n])]
        assert not bad, f"{what}: gradients of step {i} differ: {bad[:5]} ({len(bad)} tensors)"
    bad = [n for n in pa if not torch.equal(pa[n], pb[n])]
    assert not bad, f"{what}: parameters after the steps differ: {bad[:5]} ({len(bad)} tensors)"


def test_hsic_training_steps_are_bitwise_reproducible():
    """HSIC(128,192,5), bf16 operands, B=2 at 256 x 256, fixed noise, deterministic mode: two fresh three-step runs with the side streams
    (MASIC._TRAIN_STREAMS, the default), the one-stream run, and a GraphedTrainStep captured in deterministic mode -- every loss, every
    gradient and every parameter torch.equal, no tolerance."""
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn
    from masic_amd.determinism import deterministic
    from masic_amd.graph import GraphedTrainStep
    import MASIC
    N, M, K, B, H, W = 128, 192, 5, 2, 256, 256
    sd0, batches, noises = _hsic_setup(N, M, K, B, H, W)
    noise = _StaticNoise(noises)
    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = lambda self, x: noise(self, x)
    mnn.set_precision("bf16")
    try:
        with deterministic():
            assert MASIC._TRAIN_STREAMS, "the default schedule uses the side streams"
            r1 = _run_eager(sd0, batches, noise, N, M, K, streams=True)
            r2 = _run_eager(sd0, batches, noise, N, M, K, streams=True)
            _assert_same_run(r1, r2, "two side-stream runs")
            r0 = _run_eager(sd0, batches, noise, N, M, K, streams=False)
            _assert_same_run(r1, r0, "side streams vs one stream")
            net = MASIC.HSIC(N, M, K)
            net.load_state_dict(sd0)
            net = net.to(DEV).train()
            noise.load(0)
            step = GraphedTrainStep(net, *batches[0], 0.01)
            losses, grads = [], []
            for it in range(len(batches)):
                noise.load(it)
                crit, aux = step(*batches[it])
                losses.append(torch.stack([crit["loss"].detach().reshape(()), aux.detach().reshape(())]).cpu())
                grads.append({n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
            torch.cuda.synchronize()
            rg = (losses, grads, {n: p.detach().clone() for n, p in net.named_parameters()})
            _assert_same_run(r0, rg, "graph replay vs eager")
    finally:
        EntropyModel._get_noise_cached = orig
        mnn.set_precision("f32")


def test_graphed_train_step_refuses_another_mode():
    """A GraphedTrainStep replays the kernels of its capture: replaying it under the other mode raises, in both directions."""
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn
    from masic_amd.determinism import deterministic
    from masic_amd.graph import GraphedTrainStep
    import MASIC
    N, M, K, B, H, W = 16, 32, 3, 1, 64, 64
    sd0, batches, noises = _hsic_setup(N, M, K, B, H, W, nsteps=1)
    noise = _StaticNoise(noises)
    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = lambda self, x: noise(self, x)
    mnn.set_precision("bf16")
    try:
        for captured_det in (True, False):
            net = MASIC.HSIC(N, M, K)
            net.load_state_dict(sd0)
            net = net.to(DEV).train()
            with deterministic(captured_det):
                step = GraphedTrainStep(net, *batches[0], 0.01, warmup=1)
                step(*batches[0])
            with deterministic(not captured_det):
                with pytest.raises(RuntimeError, match="deterministic"):
                    step(*batches[0])
            if not captured_det:          # torch's switch counts as well
                torch.use_deterministic_algorithms(True, warn_only=True)
                try:
                    with pytest.raises(RuntimeError, match="deterministic"):
                        step(*batches[0])
                finally:
                    torch.use_deterministic_algorithms(False)
    finally:
        EntropyModel._get_noise_cached = orig
        mnn.set_precision("f32")


def test_training_step_gradients_vs_reference_golden_det():
    """tests/golden/hsic_tiny.npz in deterministic mode: every parameter gradient of the reference's training step at GTOL."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd.determinism import deterministic
    from masic_amd.loss import rate_distortion
    fx = load_npz("hsic_tiny.npz")
    N, M, K = (int(v) for v in fx["NMK"])
    sd = golden_state_dict(fx, MASIC.HSIC(N, M, K).state_dict())
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x1, x2, H = (torch.from_numpy(fx[k]).to(DEV) for k in ("x1", "x2", "h_matrix"))
    queue = [torch.from_numpy(fx["train/noise_" + k]).to(DEV) for k in O.NOISE_KEYS]
    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = lambda self, x: queue.pop(0).reshape(x.shape).contiguous()
    try:
        with deterministic():
            out = net(x1, x2, H)
            crit = rate_distortion(out, x1, x2, float(fx["lmbda"]))
            crit["loss"].backward()
    finally:
        EntropyModel._get_noise_cached = orig
    grads = dict(net.named_parameters())
    n = 0
    for key in fx:
        if key.startswith("train/grad/"):
            name = key[len("train/grad/"):]
            assert_close(grads[name].grad, torch.from_numpy(fx[key]), "det:" + name, GTOL)
            n += 1
    assert n == 164


def _cqe_step(det):
    """one CQE training step (newtrain_cqe_real.py:128-174) on hsic_tiny's HSIC and cqe_train's Independent_EN: (loss, gradients, params)"""
    import MASIC
    from masic_amd import synth
    from masic_amd.determinism import deterministic
    from masic_amd.train import cqe_train_step
    fx = load_npz("cqe_train.npz")
    tiny = load_npz("hsic_tiny.npz")
    N, M, K = (int(v) for v in tiny["NMK"])
    hsic = MASIC.HSIC(N, M, K)
    hsic.load_state_dict(golden_state_dict(tiny, hsic.state_dict()))
    hsic = hsic.to(DEV).eval()
    net2 = MASIC.Independent_EN()
    net2.load_state_dict(synth.synth_state_dict(net2.state_dict(), seed=int(fx["seed_en"])))
    net2 = net2.to(DEV).train()
    x1, x2, hm = (torch.from_numpy(tiny[k]).to(DEV) for k in ("x1", "x2", "h_matrix"))
    opt = torch.optim.Adam(net2.parameters(), lr=1e-4)
    grads = {}
    hooks = [p.register_post_accumulate_grad_hook(lambda p, n=n: grads.__setitem__(n, p.grad.detach().clone())) for n, p in net2.named_parameters()]
    with deterministic(det):
        crit, _ = cqe_train_step(hsic, net2, opt, x1, x2, hm, float(fx["lmbda"]))
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    return fx, float(crit["loss"].detach()), grads, {n: p.detach().clone() for n, p in net2.named_parameters()}


def test_cqe_training_step_det_vs_golden_and_bitwise():
    """The CQE step in deterministic mode: Independent_EN's 86 gradients against cqe_train.npz at the CQE test's tolerance rule
    (max(1e-4, 2 x the reference's float32 floor)), and two runs bitwise equal."""
    from tests.test_gpu_cqe import _check_grad
    fx, l1, g1, p1 = _cqe_step(True)
    _, l2, g2, p2 = _cqe_step(True)
    worst = [0.0, ""]
    for name in p1:
        _check_grad(fx, "chain/grad/" + name, g1.get(name), worst, "chain/f32_floor/" + name)
    assert len(g1) == 86 and worst[0] <= 1.0, worst
    assert l1 == l2
    assert g1.keys() == g2.keys() and all(torch.equal(g1[n], g2[n]) for n in g1), "two CQE steps give different gradients"
    assert all(torch.equal(p1[n], p2[n]) for n in p1), "two CQE steps give different parameters"
