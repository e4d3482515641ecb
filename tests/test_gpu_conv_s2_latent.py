"""conv_s2_latent_f16k (masic_amd/csrc/conv_s2_latent.hip, masic_amd/latent.py): the 128 -> 192 5x5 stride-2 latent layer with the
multi-output epilogue on the kernel of its own.

The yardstick is the kernel it stands for: masic_conv_f16k_multi_fwd (ops.conv2d_f16k_multi) on the same packed operands, compared with
torch.equal on the raw float32 / bf16 buffers -- the contraction order and the epilogue are the same, so the match is exact and needs no
tolerance.  `launch` is called directly: `preferred` is not consulted.  The shapes (B, Hi, Wi) are the smallest at which each mechanism
can go wrong (a tile is 4 x 32 output pixels):
    (1, 5, 7)      one partial tile; a picture smaller than the patch; Ho = 3, Wo = 4
    (2, 33, 130)   Ho = 17, Wo = 65: five tile rows, three tile columns, the last of each a single row / column; odd height and even
                   width, so the bottom and right padding differ
    (8, 16, 64)    two full tiles per image; the image-per-XCD block map with the grid rounded up to 8
    (9, 16, 64)    the plain block map
    (8, 32, 128)   eight tiles per image on the XCD map; halos shared across tile borders in both directions
The data is tests/test_gpu_latent_layouts._operator_data's: exact ties, sums in (-0.5, 0) that round to -0, |v| > 256.  The references are
computed once per shape and kept, and the allocator's free blocks of the output sizes are overwritten before every launch, so no output
buffer of the kernel under test is a freed buffer that already holds the answer.

One case is also held to the float64 reference of tests/f16k_ref.py under the check tests/test_gpu_f16k_rows.py applies to its multi rows
(_check_multi: y32 at that test's gate, the other three layouts as functions of y32, bit for bit).
"""
import functools
import types

import pytest
import torch

from tests import f16k_ref as R
from tests.test_gpu_f16k_rows import _check_multi
from tests.test_gpu_latent_layouts import _operator_data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 192
SHAPES = [(1, 5, 7), (2, 33, 130), (8, 16, 64), (9, 16, 64), (8, 32, 128)]
SUBSETS = [("y32", "round32", "round16", "abs16"), ("gated",), ("y32", "abs16")]
NAME = "conv_s2_latent_f16k"
PREFILL = 0x1234


def _case(B, H, W):
    return R.case_of((B, 128, H, W, M, 5, 2, 0, 0), flags=R.F16K_MULTI)


@functools.lru_cache(maxsize=None)
def _operands(shape, bias=True):
    """x16, packed weights, bias, the gates and conv_f16k_multi's outputs for every subset (computed once per shape, never written)"""
    from masic_amd import ops
    B, H, W = shape
    x, w, b = _operator_data(B, H, W, seed=5300 + sum(shape))
    if not bias:
        b = None
    d = R.desc_of(_case(*shape))
    assert ops.conv_f16k_multi_supported(d)
    x16, wp = ops.nchw_to_f16k(x), ops.pack_conv_f16k_weight(w, d)
    gates = torch.rand((B, 3, d.Ho, d.Wo), generator=torch.Generator().manual_seed(7))
    gates[:, 2].view(B, -1)[:, 0::5] = 0.0
    gates[:, 2].view(B, -1)[:, 1::5] = 1.0
    gates = gates.to(DEV)
    ref = {}
    for subset in SUBSETS:
        if subset == ("gated",):
            cat = torch.full((B * 5 * M * d.Ho * d.Wo,), PREFILL, dtype=torch.int16, device=DEV)
            ops.conv2d_f16k_multi(x16, wp, b, d, want=("round16",), round16=cat, round16_ctot=5 * M, round16_coff=4 * M, gate=gates, gate_c=2)
            ref[subset] = {"round16": cat}
        else:
            ref[subset] = ops.conv2d_f16k_multi(x16, wp, b, d, want=subset)
    torch.cuda.synchronize()
    if bias:                                               # the data must hold the cases the stores can get wrong
        y, r = ref[SUBSETS[0]]["y32"], ref[SUBSETS[0]]["round32"]
        assert int(((y - torch.floor(y)) == 0.5).sum()) > 10, "no exact ties"
        assert int(((r == 0) & torch.signbit(r)).sum()) > 0, "no -0"
        assert int((y.abs() > 256).sum()) > 0, "no |v| > 256"
    return x16, wp, b, gates, ref


def _poison(B, Ho, Wo):
    """`launch` takes its output buffers from the allocator, which hands out what earlier launches freed: overwrite the free blocks of
    those sizes first, so that an element the kernel leaves out shows as NaN / the prefill and not as an earlier launch's value"""
    junk = [torch.full((B, M, Ho, Wo), float("nan"), device=DEV) for _ in range(3)]
    junk += [torch.full((B * M * Ho * Wo,), PREFILL, dtype=torch.int16, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    del junk


def _launch(shape, subset, x16, wp, b, gates):
    from masic_amd import latent
    B, H, W = shape
    _poison(B, *latent.out_hw(H, W))
    if subset == ("gated",):
        Ho, Wo = latent.out_hw(H, W)
        cat = torch.full((B * 5 * M * Ho * Wo,), PREFILL, dtype=torch.int16, device=DEV)
        out = latent.launch(x16, wp, b, B, H, W, want=("round16",), round16=cat, round16_ctot=5 * M, round16_coff=4 * M, gate=gates, gate_c=2)
        assert set(out) == {"round16"} and out["round16"] is cat
        return out
    out = latent.launch(x16, wp, b, B, H, W, want=subset)
    assert set(out) == set(subset)
    return out


def _assert_same(shape, subset, out, ref):
    for k, want in ref.items():
        got = out[k]
        assert got.shape == want.shape and got.dtype == want.dtype, (shape, subset, k)
        diff = int((R.bits(got) != R.bits(want)).sum())
        print(f"conv_s2_latent | {shape} | {'+'.join(subset)} | {k} | {diff} of {want.numel()} values differ")
        assert torch.equal(R.bits(got), R.bits(want)), f"{shape} {subset} {k}: {diff} of {want.numel()} values differ from conv_f16k_multi's"


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bits_of_conv_f16k_multi(shape, subset):
    """all four layouts; round16 alone, gated, into channels 4M .. 5M of a 5M buffer whose other channels must come back untouched;
    y32 + abs16"""
    x16, wp, b, gates, ref = _operands(shape)
    out = _launch(shape, subset, x16, wp, b, gates)
    torch.cuda.synchronize()
    _assert_same(shape, subset, out, ref[subset])


def test_no_bias():
    shape = (2, 33, 130)
    x16, wp, b, gates, ref = _operands(shape, bias=False)
    assert b is None
    for subset in SUBSETS[:2]:
        out = _launch(shape, subset, x16, wp, None, gates)
        torch.cuda.synchronize()
        _assert_same(shape, subset, out, ref[subset])


def test_vs_float64():
    from masic_amd import latent, ops
    shape = (2, 33, 130)
    B, H, W = shape
    c = _case(*shape)
    x, w, bias = R.inputs(c, 5300 + sum(shape))
    ref = R.conv64(c, x, w, bias)
    wp = ops.pack_conv_f16k_weight(w.to(DEV), R.desc_of(c))
    out = latent.launch(R.to_f16k(x).to(DEV), wp, bias.to(DEV), B, H, W)
    torch.cuda.synchronize()
    _check_multi(types.SimpleNamespace(case=c, id=f"conv_s2_latent {shape}", kernel=NAME), out, ref, None, False)


def test_kernel_name():
    from masic_amd import latent
    for shape in ((8, 64, 64), (8, 32, 32), (1, 64, 64), (1, 5, 7)):
        assert latent.kernel_name(*shape) == NAME
    with pytest.raises(RuntimeError):
        latent.kernel_name(0, 8, 8)


def _encoder():
    import MASIC
    from masic_amd import synth
    net = MASIC.HSIC(128, M, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31))
    return net.encoder1.to(DEV).eval()


def test_module_and_refusals():
    """g_a_conv4 of a synthetic-weight encoder: run() returns the dict of run_f16k_multi with the same bits; every form the kernel does
    not run is refused, at the module level (the form) and by the library (the shape and the arguments)"""
    import MASIC
    from masic_amd import _lib, latent
    from masic_amd.f16k import F16K
    enc = _encoder()
    cv = enc.g_a_conv4
    B, H, W = 1, 16, 64
    x = R.inputs(R.case_of((B, 128, H, W, 128, 5, 2, 0, 0)), 5307)[0]
    x16 = F16K.wrap(R.to_f16k(x).to(DEV), B, 128, H, W)
    assert latent.supported(cv, B, H, W) and latent.supported(cv, 8, 64, 64)
    with torch.no_grad():
        want = cv.run_f16k_multi(x16, latent.WANT)
        got = latent.run(cv, x16, latent.WANT)
    torch.cuda.synchronize()
    assert set(got) == set(want) == set(latent.WANT)
    for k in ("y32", "round32"):
        assert torch.equal(R.bits(got[k]), R.bits(want[k])), k
    for k in ("round16", "abs16"):
        g, w_ = got[k], want[k]
        assert (g.B, g.C, g.H, g.W, g.ctot, g.coff) == (w_.B, w_.C, w_.H, w_.W, w_.ctot, w_.coff) == (B, M, 8, 32, M, 0), k
        assert torch.equal(g.buf, w_.buf), k

    dec = MASIC.Decoder1(128, M).to(DEV)
    assert not latent.supported(dec.g_s_conv1, B, H, W)                                 # transposed (192 -> 128)
    assert not latent.supported(enc.g_a_conv3, B, H, W)                                 # 128 -> 128
    assert not latent.supported(MASIC.conv(128, M, kernel_size=3, stride=1).to(DEV), B, H, W)     # another geometry
    assert not latent.supported(MASIC.conv(128, M, kernel_size=5, stride=1).to(DEV), B, H, W)
    assert not latent.supported(MASIC.conv(160, M).to(DEV), B, H, W)                    # other input channels
    assert not latent.supported(cv, B, H, W, in_ctot=160, in_coff=16)                   # a channel view of the input
    assert not latent.supported(cv, B, H, W, prec=_lib.PREC_FP8)                        # fp8 operands
    assert not latent.supported(cv, B, H, W, prec=_lib.PREC_F32)                        # float32
    masked = types.SimpleNamespace(transposed_conv=False, masked_conv=True, in_channels=128, out_channels=M, _geometry=lambda: (5, 5, 2, 2))
    assert not latent.supported(masked, B, H, W)                                        # a masked convolution
    assert _lib.lib.masic_latent_s2_f16k_supported(1, 5, 7) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 2048, 2048)):
        assert _lib.lib.masic_latent_s2_f16k_supported(*bad) == 0, bad
        assert _lib.lib.masic_latent_s2_f16k_preferred(*bad) == 0, bad
    x5, wp, b, gates, _ = _operands((1, 5, 7))
    with pytest.raises(RuntimeError):
        latent.launch(x5, wp[:-1], b, 1, 5, 7)
    with pytest.raises(RuntimeError):
        latent.launch(x5, wp, b, 1, 5, 8)
    with pytest.raises(RuntimeError):
        latent.launch(x5, wp, b[:-1].contiguous(), 1, 5, 7)
    with pytest.raises(ValueError):
        latent.launch(x5, wp, b, 1, 5, 7, want=())
    with pytest.raises(ValueError):
        latent.launch(x5, wp, b, 1, 5, 7, want=("y16",))
    cat = torch.full((1 * 5 * M * 3 * 4,), PREFILL, dtype=torch.int16, device=DEV)
    with pytest.raises(RuntimeError, match="16-aligned channel view"):                  # the view does not hold 192 channels
        latent.launch(x5, wp, b, 1, 5, 7, want=("round16",), round16=cat, round16_ctot=5 * M, round16_coff=4 * M + 16)
    with pytest.raises(RuntimeError, match="gate"):                                     # a gate without round16; a gate channel out of range
        latent.launch(x5, wp, b, 1, 5, 7, want=("y32",), gate=gates, gate_c=2)
    with pytest.raises(RuntimeError, match="gate"):
        latent.launch(x5, wp, b, 1, 5, 7, want=("round16",), gate=gates, gate_c=3)
    with pytest.raises(RuntimeError):                                                   # a channel view of the input
        latent.run(cv, F16K(torch.empty(1 * 160 * 5 * 7, dtype=torch.int16, device=DEV), 1, 128, 5, 7, 160, 16), latent.WANT)
    torch.cuda.synchronize()
    assert bool((cat == PREFILL).all())


def _smallest_preferred():
    """the smallest picture (B = 8, H x 16) whose latent layer (input 8 x 128 x H/8 x 2: H / 64 tiles per image) `preferred` takes"""
    from masic_amd import latent
    for H in range(64, 2048 + 1, 64):
        if latent.preferred(None, 8, H // 8, 2):
            return H
    return None


def test_preferred_rule():
    """a threshold on the workgroup count: 0 at B = 2, 64 x 128 pictures (two workgroups), 1 at the benchmark shape (64), monotonic"""
    from masic_amd import latent
    assert not latent.preferred(None, 2, 8, 16)
    assert latent.preferred(None, 8, 64, 64)
    H = _smallest_preferred()
    assert H is not None and H // 64 * 8 >= 8
    assert latent.preferred(None, 8, 2 * H // 8, 2) and not latent.preferred(None, 8, (H - 64) // 8, 2)


def test_encoder_takes_either_path():
    """Encoder1.latent_layouts at the smallest shape `preferred` takes: g_a_conv4 runs on the new kernel, and with it refused on
    conv_f16k_multi as before -- the same tensors bit for bit both ways.  At B = 2, 64 x 128 the forward stays on conv_f16k_multi."""
    from masic_amd import latent
    from masic_amd import nn as mnn
    from masic_amd.f16k import F16K
    enc = _encoder()
    H = _smallest_preferred()
    assert H is not None
    B, W = 8, 16
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    h, w = latent.out_hw(H // 8, W // 8)
    gates = torch.rand((B, 3, h, w), generator=torch.Generator().manual_seed(6)).to(DEV)
    calls = []
    run = latent.run

    def layouts():
        cat = F16K.wrap(torch.full((B * 5 * M * h * w,), PREFILL, dtype=torch.int16, device=DEV), B, 5 * M, h, w)
        return dict(want=latent.WANT, round16=cat.channels(4 * M, M), gate=gates, gate_c=2)

    mnn.set_precision("bf16")
    try:
        with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
            mp.setattr(latent, "run", lambda *a, **k: calls.append((a[1].B, a[1].H, a[1].W)) or run(*a, **k))
            new = enc.latent_layouts(x, **layouts())
            assert calls == [(B, H // 8, W // 8)]
            mp.setattr(latent, "preferred", lambda *a, **k: False)
            old = enc.latent_layouts(x, **layouts())
            assert len(calls) == 1
            mp.undo()
            mp.setattr(latent, "run", lambda *a, **k: calls.append("small") or run(*a, **k))
            small = enc.latent_layouts(torch.rand(2, 3, 64, 128, generator=torch.Generator().manual_seed(5)).to(DEV), want=("y32",))
            assert len(calls) == 1 and tuple(small["y32"].shape) == (2, M, 4, 8)
    finally:
        mnn.set_precision("f32")
    torch.cuda.synchronize()
    assert new is not None and old is not None and set(new) == set(old) == set(latent.WANT)
    assert tuple(new["y32"].shape) == (B, M, h, w) and bool(torch.isfinite(new["y32"]).all())
    for k in ("y32", "round32"):
        assert torch.equal(R.bits(new[k]), R.bits(old[k])), k
    for k in ("round16", "abs16"):
        assert (new[k].ctot, new[k].coff) == (old[k].ctot, old[k].coff)
        assert torch.equal(new[k].buf, old[k].buf), k
