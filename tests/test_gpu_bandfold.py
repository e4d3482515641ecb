"""The band-aware entropy model on the GPU: the fold / unfold kernels (masic_amd/csrc/band_fold.hip) bit for bit against numpy, the banded
context node against CPU autograd of the per-band convolution, and HSIC.band_rows through every place that evaluates a context model
outside the coder -- the oracle with its context models applied band by band, band independence, no change at 0, one training step, the
latent refinement and the captured graphs."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import hsic_oracle as O
from tests import bandfold_ref as BR
from tests import bands_ref as R
from tests.test_gpu_backward import GTOL, assert_close
from tests.util import assert_symbols, tie_zone

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1234.5
SENTINEL16 = 0x7B7B                     # a bf16 pattern no result below holds
N, M, K, SEED, H, W = 32, 48, 3, 360, 128, 192            # the model tests: a latent of 8 x 12; the seed: tests/test_cpu_bandfold.py
MODEL_S = [3, 4]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", BR.CASES + BR.PAST_CAP_CASES, ids=str)
def test_fold_bit_exact_over_a_nan_destination(case):
    from masic_amd import _lib, bandfold
    B, C, h, w, S = case
    x = BR.rand((B, C, h, w), seed=21)
    want = BR.fold(x, S)
    got = bandfold.fold(_dev(x), S)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(_bits(got), want.view(np.uint32))
    # every element is written, the padding rows of a short last band as +0.0: no memset beside the kernel
    dst = torch.full(want.shape, float("nan"), dtype=torch.float32, device=DEV)
    assert _lib.lib.masic_bandfold_fold(_p(_dev(x)), _p(dst), B, C, h, w, S, _stream()) == 0
    assert np.array_equal(_bits(dst), want.view(np.uint32))


@pytest.mark.parametrize("case", BR.CASES + BR.PAST_CAP_CASES, ids=str)
def test_unfold_bit_exact_float32_and_f16k(case):
    from masic_amd import bandfold
    from masic_amd.f16k import F16K
    B, C, h, w, S = case
    xb = BR.rand((B * BR.n_bands(h, S), C, S, w), seed=22)            # values in the padding rows too: they are dropped
    want = BR.unfold(xb, B, h, S)
    got = bandfold.unfold(_dev(xb), B, h, S)
    assert np.array_equal(_bits(got), want.view(np.uint32))
    assert np.array_equal(_bits(bandfold.unfold(bandfold.fold(got, S), B, h, S)), want.view(np.uint32))       # unfold(fold(x)) == x
    # a whole F16K of ceil16(C) channels: the records of the C channels, zeros up to the end of the last 16-byte half record, the rest kept
    ctot = (C + 15) // 16 * 16
    dst = F16K.wrap(torch.full((B * ctot * h * w,), SENTINEL16, dtype=torch.int16, device=DEV), B, C, h, w)
    assert bandfold.unfold(_dev(xb), B, h, S, out=dst) is dst
    rec = BR.f16k_records(BR.bf16_bits(want), ctot)
    kept = np.zeros((B, ctot), dtype=bool)
    kept[:, (C + 7) // 8 * 8:] = True
    rec = np.where(np.ascontiguousarray(kept.reshape(B, ctot // 16, 1, 16)), np.uint16(SENTINEL16), rec)
    assert np.array_equal(dst.buf.cpu().numpy().view(np.uint16).reshape(rec.shape), rec)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("case", [(2, 32, 8, 12, 3), (2, 32, 5, 7, 2)], ids=str)
def test_unfold_into_a_channel_slice(case, gated):
    """channels [32, 64) of an 80-channel float32 buffer and of an 80-channel F16K, with and without the gate from channel 1 of a
    3-channel gate tensor; the channels outside the slice keep their sentinel"""
    from masic_amd import bandfold
    from masic_amd.f16k import F16K
    B, C, h, w, S = case
    xb = BR.rand((B * BR.n_bands(h, S), C, S, w), seed=23)
    gate = BR.rand((B, 3, h, w), seed=24, scale=1.0) if gated else None
    want = BR.gated(BR.unfold(xb, B, h, S), gate, 1)
    gd = None if gate is None else _dev(gate)
    buf = torch.full((B, 80, h, w), SENTINEL, dtype=torch.float32, device=DEV)
    assert bandfold.unfold(_dev(xb), B, h, S, out=buf, out_coff=32, gate=gd, gate_c=1) is buf
    ref = np.full((B, 80, h, w), SENTINEL, dtype=np.float32)
    ref[:, 32:64] = want
    assert np.array_equal(_bits(buf), ref.view(np.uint32))
    whole = F16K.wrap(torch.full((B * 80 * h * w,), SENTINEL16, dtype=torch.int16, device=DEV), B, 80, h, w)
    bandfold.unfold(_dev(xb), B, h, S, out=whole.channels(32, 32), gate=gd, gate_c=1)
    bits = np.full((B, 80, h, w), SENTINEL16, dtype=np.uint16)
    bits[:, 32:64] = BR.bf16_bits(want)                       # ONE rounding, after the float32 gate product
    assert np.array_equal(whole.buf.cpu().numpy().view(np.uint16).reshape(B, 5, h * w, 16), BR.f16k_records(bits, 80))
    # the rounding is the one ops.nchw_to_f16k_view applies
    other = F16K.wrap(torch.full((B * 80 * h * w,), SENTINEL16, dtype=torch.int16, device=DEV), B, 80, h, w)
    other.channels(32, 32).fill_from_nchw(_dev(BR.unfold(xb, B, h, S)), gate=gd, gate_c=1)
    assert torch.equal(other.buf, whole.buf)


def test_bad_arguments_return_err_arg():
    from masic_amd import _lib
    lib = _lib.lib
    t = torch.zeros(4096, dtype=torch.float32, device=DEV)
    good = dict(B=1, C=2, h=4, w=4, S=2)
    for key, bad in (("S", 0), ("S", -1), ("B", 0), ("C", 0), ("h", 0), ("w", -3)):
        a = dict(good, **{key: bad})
        shape = (a["B"], a["C"], a["h"], a["w"], a["S"])
        assert lib.masic_bandfold_fold(_p(t), _p(t), *shape, _stream()) == _lib.ERR_ARG, (key, bad)
        assert b"bandfold_fold" in lib.masic_last_error()
        assert lib.masic_bandfold_unfold(_p(t), _p(t), *shape, 2, 0, None, 0, 0, _stream()) == _lib.ERR_ARG, (key, bad)
        assert lib.masic_bandfold_unfold_f16k(_p(t), _p(t), *shape, 16, 0, None, 0, 0, _stream()) == _lib.ERR_ARG, (key, bad)
    shape = tuple(good[k] for k in ("B", "C", "h", "w", "S"))
    assert lib.masic_bandfold_fold(None, _p(t), *shape, _stream()) == _lib.ERR_ARG
    assert lib.masic_bandfold_unfold(_p(t), None, *shape, 2, 0, None, 0, 0, _stream()) == _lib.ERR_ARG
    # a slice outside its buffer, a gate channel outside the gate: refused too (MASIC_ERR_SHAPE), nothing launched
    assert lib.masic_bandfold_unfold(_p(t), _p(t), *shape, 2, 1, None, 0, 0, _stream()) == _lib.ERR_SHAPE
    assert lib.masic_bandfold_unfold_f16k(_p(t), _p(t), *shape, 16, 8, None, 0, 0, _stream()) == _lib.ERR_SHAPE
    assert lib.masic_bandfold_unfold(_p(t), _p(t), *shape, 2, 0, _p(t), 3, 3, _stream()) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert not t.any()


def test_kernels_are_capturable_and_reproducible():
    from masic_amd import bandfold
    from masic_amd.f16k import F16K
    B, C, h, w, S = 2, 32, 16, 24, 5
    x = _dev(BR.rand((B, C, h, w), seed=25))
    gate = _dev(BR.rand((B, 3, h, w), seed=26, scale=1.0))
    out16 = F16K.empty(B, C, h, w, DEV)
    eager = bandfold.fold(x, S)
    eager32 = bandfold.unfold(eager, B, h, S, gate=gate, gate_c=2)
    eager16 = bandfold.unfold(eager, B, h, S, out=out16, gate=gate, gate_c=2).buf.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bandfold.fold(x, S)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f = bandfold.fold(x, S)
        u = bandfold.unfold(f, B, h, S, gate=gate, gate_c=2)
        bandfold.unfold(f, B, h, S, out=out16, gate=gate, gate_c=2)
    for _ in range(2):
        f.fill_(float("nan"))
        u.fill_(float("nan"))
        out16.buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(f, eager) and _same(u, eager32) and torch.equal(out16.buf, eager16)


# ------------------------------------------------------------------------------------------------------------------ the node
NODE = (2, 32, 7, 12, 64)               # tests/test_gpu_backward.py's masked5 geometry, reduced


def _masked5():
    from compressai.layers import MaskedConv2d
    from tests.test_gpu_backward import _rand
    B, Cin, h, w, Cout = NODE
    mod = MaskedConv2d(Cin, Cout, kernel_size=5, padding=2, stride=1)
    wt = _rand(*mod.weight.shape, seed=2, scale=(2.0 / (Cin * 25)) ** 0.5)
    b = _rand(Cout, seed=3, scale=0.1)
    with torch.no_grad():
        mod.weight.copy_(wt)
        mod.bias.copy_(b)
    return mod.to(DEV), wt, b, _rand(B, Cin, h, w, seed=1, scale=2.0), _rand(B, Cout, h, w, seed=4)


def _node_reference(wt, b, x, go, S):
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = BR.banded_conv_reference(xr, O.masked_weight(wr), br, S)
    yr.backward(go)
    return yr.detach(), xr.grad, wr.grad, br.grad


@pytest.mark.parametrize("S", [1, 3, 7])
def test_banded_context_node_float32(S):
    from masic_amd import autograd as A
    mod, wt, b, x, go = _masked5()
    yr, dxr, dwr, dbr = _node_reference(wt, b, x, go, S)
    xd = x.to(DEV).requires_grad_(True)
    y = A.banded_context(mod, xd, S)
    assert_close(y, yr, f"S={S}:fwd")
    y.backward(go.to(DEV))
    assert_close(xd.grad, dxr, f"S={S}:dx", GTOL)
    assert_close(mod.weight.grad, dwr, f"S={S}:dw", GTOL)
    assert_close(mod.bias.grad, dbr, f"S={S}:db", GTOL)
    if S == 7:                          # one band: not folded at all -- A.conv itself, bit for bit
        x2 = x.to(DEV).requires_grad_(True)
        y2 = A.conv(mod, x2)
        y2.backward(go.to(DEV))
        assert _same(y, y2) and _same(xd.grad, x2.grad)


@pytest.mark.parametrize("S", [1, 3, 7])
def test_banded_context_node_bf16_mode(S):
    """against float32 autograd at bf16 operand noise: 2e-2 of each tensor's peak, the rule of
    tests/test_gpu_backward.py::test_conv_backward_bf16_mode"""
    from masic_amd import autograd as A
    from masic_amd import nn as mnn
    mod, wt, b, x, go = _masked5()
    ref = _node_reference(wt, b, x, go, S)
    mnn.set_precision("bf16")
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = A.banded_context(mod, xd, S)
        y.backward(go.to(DEV))
        got = (y, xd.grad, mod.weight.grad.clone(), mod.bias.grad.clone())
        if S == 7:                      # (a second backward through the same module: its parameter gradients accumulate)
            x2 = x.to(DEV).requires_grad_(True)
            y2 = A.conv(mod, x2)
            y2.backward(go.to(DEV))
            assert _same(y, y2) and _same(xd.grad, x2.grad)
    finally:
        mnn.set_precision("f32")
    for nm, have, want in zip(("y", "dx", "dw", "db"), got, ref):
        peak = float(want.abs().max())
        err = float((have.detach().cpu() - want).abs().max())
        print(f"S={S} {nm}: error {err:.3e} of peak {peak:.3e}")
        assert err <= 2e-2 * peak, (S, nm, err, peak)


def test_banded_context_refuses_a_destination_under_autograd():
    from masic_amd import autograd as A
    mod, _, _, x, _ = _masked5()
    out = torch.zeros((2, 80, 7, 12), device=DEV)
    with pytest.raises(RuntimeError, match="inference-only fusion"):
        A.banded_context(mod, x.to(DEV).requires_grad_(True), 3, call=mod.run, out=out, out_coff=8)


# ------------------------------------------------------------------------------------------------------------------ the model
def _inputs():
    from masic_amd import synth
    return tuple(t.to(DEV) for t in synth.synth_inputs(1, H, W, seed=SEED))


def _assert_outputs_same(a, b, keys=("x1_hat", "x2_hat", "y1_hat", "z1_hat", "x1_mask_R", "x1_mask_L")):
    for k in keys:
        if k in a or k in b:
            assert _same(a[k], b[k]), k
    for k in a["likelihoods"]:
        assert _same(a["likelihoods"][k], b["likelihoods"][k]), k


def _from_latents_operands(net, x1, x2, hm):
    from masic_amd import ops
    from masic_amd.homography import warp_matrices
    m_fwd, m_back = warp_matrices(hm, (H, W), (H, W), want_inverse=True)
    gates = net.mask2weights_unit(ops.warp_perspective(None, m_fwd, (H, W), ones_like=(x1.shape[0], H, W))).contiguous()
    return [t.contiguous() for t in net.latents(x1, x2, hm)], m_fwd, m_back, gates


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("S", MODEL_S)
def test_context_bands_equals_the_torch_chain_it_replaces(S, prec):
    """HSIC._context_bands on the two kernels against the pad / view / permute / multiply / fill_from_nchw chain around the same
    convolution (tests/bandfold_ref.py), bit for bit, into each kind of destination"""
    from masic_amd import nn as mnn
    from masic_amd.f16k import F16K
    try:
        net = R.hsic(N, M, K, SEED, prec)
        y = _dev(BR.rand((2, M, 8, 12), seed=31))
        gates = _dev(BR.rand((2, 3, 8, 12), seed=32, scale=1.0))
        ctx = net.context_prediction2
        with torch.no_grad():
            for gate in (None, gates):
                want = BR.context_bands_torch_chain(net, ctx, y, None, 0, gate, 1, S)
                assert _same(net._context(ctx, y, None, gate=gate, gate_c=1, band_rows=S), want)
                a, b = (torch.full((2, 5 * M, 8, 12), SENTINEL, device=DEV) for _ in range(2))
                BR.context_bands_torch_chain(net, ctx, y, a, 2 * M, gate, 1, S)
                net._context(ctx, y, b, 2 * M, gate=gate, gate_c=1, band_rows=S)
                assert _same(a, b)
                a, b = (F16K.wrap(torch.full((2 * 5 * M * 96,), SENTINEL16, dtype=torch.int16, device=DEV), 2, 5 * M, 8, 12) for _ in range(2))
                BR.context_bands_torch_chain(net, ctx, y, a.channels(2 * M, 2 * M), 0, gate, 1, S)
                net._context(ctx, y, b.channels(2 * M, 2 * M), gate=gate, gate_c=1, band_rows=S)
                assert torch.equal(a.buf, b.buf)
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("S", MODEL_S)
def test_eval_forward_against_the_oracle_with_banded_context_models(S):
    """(a) tolerance and tie-zone rule of tests/test_gpu_hsic.py's float32 forward against the oracle: symbols bit-exact outside the tie
    zone |frac - 1/2| < 1e-4, flips inside it at most max(1, 1e-4 of the symbols); latent pixels whose y1_warp lies in the zone left out
    of the y2 likelihood, no more of them than flips are allowed there; everything else at 1e-4.  The seed's zone is empty on the
    oracle (tests/test_cpu_bandfold.py), so here nothing is excluded."""
    import MASIC
    from masic_amd import nn as mnn, synth
    try:
        net = R.hsic(N, M, K, SEED, "f32")
        sd = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=SEED)
        x1, x2, hm = synth.synth_inputs(1, H, W, seed=SEED)
        with torch.no_grad():
            with BR.oracle_with_bands(O, S):
                ref = O.hsic_forward(sd, x1, x2, hm, K=K, keep=True)
            plain = O.hsic_forward(sd, x1, x2, hm, K=K)
            aux = ref["_aux"]
            assert not torch.equal(ref["likelihoods"]["y1"], plain["likelihoods"]["y1"])          # the bands are in the reference
            assert not torch.equal(ref["likelihoods"]["y2"], plain["likelihoods"]["y2"])
            x1d, x2d, hmd = x1.to(DEV), x2.to(DEV), hm.to(DEV)
            net.band_rows = S
            out = net(x1d, x2d, hmd)
            sym = net.symbol_streams(x1d, x2d, hmd)
        osym = O.symbols(aux, sd)
        flips = zone = 0
        for k in ("y1", "y2", "z1", "z2"):
            v = aux[k] if k[0] == "y" else aux[k] - sd[f"entropy_bottleneck{k[1]}.quantiles"][:, 0, 1].view(1, -1, 1, 1)
            flips += assert_symbols(sym[k], osym[k], v, k)
            zone += int(tie_zone(v).sum())
        total = sum(v.numel() for v in osym.values())
        tied = tie_zone(aux["y1_warp"]).any(1, keepdim=True)
        print(f"S={S}: {total} symbols, {zone} in the tie zone, {flips} flipped; {int(tied.sum())} of {tied.numel()} latent pixels left out")
        assert flips <= zone and flips <= max(1, int(1e-4 * total))
        assert int(tied.sum()) <= int(1e-4 * tied.numel())
        assert flips == 0 and int(tied.sum()) == 0
        for k in ("x1_hat", "x2_hat", "y1_hat", "z1_hat", "x1_mask_R", "x1_mask_L"):
            assert_close(out[k], ref[k], f"S={S}:{k}")
        for k in ("y1", "y2", "z1", "z2"):
            assert_close(out["likelihoods"][k], ref["likelihoods"][k], f"S={S}:lik_{k}")
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("S", MODEL_S)
def test_bands_do_not_see_across_their_top_edge(S, prec):
    """(b) through _eval_from_latents with z fixed: + 1.0 on y1 in the last row of band 0 leaves y1's likelihoods of every later band
    bit-equal with band_rows = S and changes them with band_rows = 0.  Fails on a model that ignores the attribute."""
    from masic_amd import nn as mnn
    try:
        net = R.hsic(N, M, K, SEED, prec)
        x1, x2, hm = _inputs()
        with torch.no_grad():
            (y1, y2, z1, z2), m_fwd, _, gates = _from_latents_operands(net, x1, x2, hm)
            moved = y1.clone()
            moved[:, :, S - 1] += 1.0

            def lik(y):
                return net._eval_from_latents(y, y2, z1, z2, m_fwd, gates)["likelihoods"]["y1"]

            net.band_rows = S
            a, b = lik(y1), lik(moved)
            assert not _same(a[:, :, :S], b[:, :, :S])
            assert _same(a[:, :, S:], b[:, :, S:])
            net.band_rows = 0
            a0, b0 = lik(y1), lik(moved)
            assert not _same(a0[:, :, S:S + 2], b0[:, :, S:S + 2])
            assert _same(a0[:, :, S + 2:], b0[:, :, S + 2:])            # the mask reaches two rows up
            assert not _same(a, a0)
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_band_rows_0_and_one_band_change_nothing(prec, monkeypatch):
    """(c) band_rows 0 and 8 (>= h) against a model whose attribute was never set: eval forward, the no-grad training-mode forward and
    one training-graph forward + backward under fixed noise seeds, bit-equal outputs, and neither kernel launched"""
    from masic_amd import bandfold, nn as mnn
    from masic_amd.loss import rate_distortion
    try:
        never = R.hsic(N, M, K, SEED, prec)
        net = R.hsic(N, M, K, SEED, prec)
        x1, x2, hm = _inputs()

        def runs(model):
            model.eval()
            with torch.no_grad():
                ev = model(x1, x2, hm)
            model.train()
            torch.manual_seed(77)
            with torch.no_grad():
                tr = model(x1, x2, hm)
            torch.manual_seed(78)
            model.zero_grad()
            gr = model(x1, x2, hm)
            crit = rate_distortion(gr, x1, x2, 0.01)
            crit["loss"].backward()
            torch.cuda.synchronize()
            return ev, tr, gr, crit["loss"].detach().clone(), model.context_prediction1.weight.grad.clone()

        want = runs(never)
        assert "_band_rows" in never.__dict__ and never.band_rows == 0

        def refuse(*a, **k):
            raise AssertionError("band_rows = 0 / one band must not launch the fold kernels")
        monkeypatch.setattr(bandfold, "fold", refuse)
        monkeypatch.setattr(bandfold, "unfold", refuse)
        for value in (0, 8, 255):
            net.band_rows = value
            got = runs(net)
            for a, b in zip(got[:3], want[:3]):
                _assert_outputs_same(a, b)
            assert abs(float(got[3]) - float(want[3])) <= 1e-6 * abs(float(want[3]))
            assert float((got[4] - want[4]).abs().max()) <= 1e-3 * float(want[4].abs().max())      # (float atomics: not bit-equal run to run)
    finally:
        mnn.set_precision("f32")


def test_one_training_step_with_bands_bf16():
    """(d) one train_step in training mode at S = 3 with bf16 operands beside the same step at S = 0"""
    from masic_amd import nn as mnn, train
    try:
        x1, x2, hm = _inputs()
        got = {}
        for S in (0, 3):
            net = R.hsic(N, M, K, SEED, "bf16").train()
            net.band_rows = S
            opt, aopt = train.make_optimizers(net)
            torch.manual_seed(79)
            crit, _ = train.train_step(net, opt, aopt, x1, x2, hm, 0.01)
            torch.cuda.synchronize()
            got[S] = (float(crit["loss"].detach()), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
        (l0, g0), (l3, g3) = got[0], got[3]
        assert np.isfinite(l3) and np.isfinite(l0) and l3 != l0
        assert set(g3) >= set(g0) and len(g0) > 100
        for n in g0:
            assert bool(torch.isfinite(g3[n]).all()), n
        for n in ("context_prediction1.weight", "context_prediction2.weight"):
            assert not torch.equal(g3[n], g0[n]) and float((g3[n] - g0[n]).abs().max()) > 1e-3 * float(g0[n].abs().max()), n
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("S", MODEL_S)
def test_refinement_descends_and_checks_the_banded_objective(S):
    """(e) refine_latents with the attribute set: cost_start is the banded objective of _eval_from_latents bit for bit (and not the
    unbanded one), cost_best <= cost_start, and under budget_rel = 1.0 the kept bits stay within the banded target"""
    from masic_amd import bands, metrics, nn as mnn
    from masic_amd.refine import RefineConfig, refine_latents
    lmbda = 0.01
    try:
        net = R.hsic(N, M, K, SEED, "f32")
        x1, x2, hm = _inputs()

        def objective(lat):
            with torch.no_grad():
                _, m_fwd, _, gates = _from_latents_operands(net, x1, x2, hm)
                out = net._eval_from_latents(*lat, m_fwd, gates)
                L = out["likelihoods"]
                rows = metrics.pair_rd(out["x1_hat"].contiguous(), x1, out["x2_hat"].contiguous(), x2, [L[k].contiguous() for k in ("y1", "y2", "z1", "z2")])
                return metrics.pair_objective(rows, lmbda, H * W, 3 * H * W), rows[:, 2:].sum(dim=1) * (-1.0 / math.log(2.0))

        with bands.model_band_rows(net, S):
            start = refine_latents(net, x1, x2, hm, lmbda, RefineConfig(steps=0))
            banded, banded_bits = objective(start[:4])
            r = refine_latents(net, x1, x2, hm, lmbda, RefineConfig(steps=4, check_every=2))
            rb = refine_latents(net, x1, x2, hm, lmbda, RefineConfig(steps=4, check_every=2, budget_rel=1.0))
        unbanded, _ = objective(start[:4])
        assert net.band_rows == 0
        assert torch.equal(r.cost_start, banded) and torch.equal(start.cost_start, banded)
        assert not torch.equal(banded, unbanded)
        assert bool((r.cost_best <= r.cost_start).all())
        assert bool((rb.bits_best <= rb.target_bits).all())
        assert torch.equal(rb.bits_start, banded_bits) and torch.equal(rb.target_bits, banded_bits)
        print(f"S={S}: cost {float(r.cost_start[0]):.6f} -> {float(r.cost_best[0]):.6f} (unbanded start {float(unbanded[0]):.6f}); "
              f"budget: bits {float(rb.bits_start[0]):.1f} -> {float(rb.bits_best[0]):.1f} of {float(rb.target_bits[0]):.1f}")
    finally:
        mnn.set_precision("f32")


def test_evaluate_and_refuse_fp8():
    """fp8 operands: the folded path is refused, not answered with the unbanded estimate; band_rows 0 and one band still run"""
    from masic_amd import nn as mnn
    try:
        net = R.hsic(N, M, K, SEED, "f32")
        mnn.set_precision("fp8")
        assert net._model_bands(8) == 0
        net.band_rows = 8
        assert net._model_bands(8) == 0
        net.band_rows = 3
        with pytest.raises(NotImplementedError, match="fp8"):
            net._model_bands(8)
        x1, x2, hm = _inputs()
        with pytest.raises(NotImplementedError, match="fp8"), torch.no_grad():
            net(x1, x2, hm)
    finally:
        mnn.set_precision("f32")


def test_graphed_forward_follows_on_stale_when_band_rows_changes():
    """(f) GraphedHSIC treats a change of band_rows as it treats stale weights"""
    from masic_amd import nn as mnn
    from masic_amd.graph import GraphedHSIC
    try:
        net = R.hsic(N, M, K, SEED, "bf16")
        x1, x2, hm = _inputs()
        with torch.no_grad():
            plain = net(x1, x2, hm)
            net.band_rows = 3
            banded = net(x1, x2, hm)
            net.band_rows = 0
            assert not _same(plain["likelihoods"]["y1"], banded["likelihoods"]["y1"])
            strict = GraphedHSIC(net, x1, x2, hm, on_stale="raise")
            lenient = GraphedHSIC(net, x1, x2, hm)
            _assert_outputs_same(strict(x1, x2, hm), plain)
            net.band_rows = 3
            with pytest.raises(RuntimeError, match="band_rows"):
                strict(x1, x2, hm)
            rep = lenient(x1, x2, hm)                      # recaptured under band_rows = 3
            torch.cuda.synchronize()
            _assert_outputs_same(rep, banded)
            net.band_rows = 0
            rep = strict(x1, x2, hm)                       # its capture is valid again
            torch.cuda.synchronize()
            _assert_outputs_same(rep, plain)
    finally:
        mnn.set_precision("f32")


def test_graphed_train_step_raises_when_band_rows_changes():
    """(f) GraphedTrainStep replays the context models of its capture: a call under another band_rows raises"""
    from masic_amd import nn as mnn
    from masic_amd.graph import GraphedTrainStep
    try:
        net = R.hsic(N, M, K, SEED, "bf16").train()
        net.band_rows = 3
        x1, x2, hm = _inputs()
        step = GraphedTrainStep(net, x1, x2, hm, 0.01, warmup=2)
        crit, _ = step(x1, x2, hm)
        torch.cuda.synchronize()
        assert np.isfinite(float(crit["loss"]))
        net.band_rows = 0
        with pytest.raises(RuntimeError, match="captured with band_rows = 3"):
            step(x1, x2, hm)
        net.band_rows = 3
        crit, _ = step(x1, x2, hm)
        torch.cuda.synchronize()
        assert np.isfinite(float(crit["loss"]))
    finally:
        mnn.set_precision("f32")
