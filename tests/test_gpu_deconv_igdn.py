"""deconv_igdn_f16k (masic_amd/csrc/deconv_igdn.hip, masic_amd/deconv.py): the 128 -> 128 transposed 5x5 stride-2 convolution with fused
one-product inverse GDN on the kernel of its own.

The yardstick is the kernel it stands for: masic_conv_f16k_gdn_fwd (ops.conv2d_f16k, gdn = inverse, one product) on the same packed
operands, compared on the raw bf16 records -- the contraction order and the epilogue are the same, so the match is exact and needs no
tolerance.  Every shape runs on both tiles (16 x 32 and 8 x 32 input pixels) and on the one the library picks, with one, two and four
workgroups per tile (all four output phases in one workgroup, two, one):
    (1, 8, 8)     one partial tile
    (2, 20, 36)   two 16 x 32 tiles along each axis (3 x 2 of 8 x 32), the last ones partial
    (8, 16, 32)   the image-per-XCD block map
    (9, 16, 32)   the plain block map
    (8, 32, 32)   two tiles per image on the 16 x 32 tile, the grid rounded up to the 8 XCDs
and the kernel choice is checked at the two shapes of the benchmark.  Operands come from tests/f16k_ref.py and the GDN parameters from
the row test's generator.

One case is also held to the float64 reference of tests/f16k_ref.py under the gates tests/test_gpu_f16k_rows.py applies to the
one-product GDN of conv_f16k<2, 2, 2, 5, 1, true, 4, 2, false> where the output is F16K: 2^-8 of the peak for the rounding to bf16
plus f16k_ref.one_product_bound(q) on the operands as drawn, and 2^-8 + 2^-9 on the operands times the power of two at which q <= 0.45.
"""
import functools

import pytest
import torch

from tests import f16k_ref as R
from tests import layer_kernel_cases as L
from tests.layer_kernel_cases import DEV, one_product as _one_product
from tests.test_gpu_f16k_rows import _gdn_params
from tests.util import rel_err

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 8), (2, 20, 36), (8, 16, 32), (9, 16, 32), (8, 32, 32)]
SEED = 4100


def _case(B, H, W):
    return R.case_of((B, 128, H, W, 128, 5, 2, 1, 0), flags=R.F16K_GDN)


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """x16, packed weights, bias, packed GDN on the device and the output of the existing kernel (computed once per shape, never written)"""
    return L.operands(_case(*shape), SEED + sum(shape), SEED, True)


NAMES = {1: "deconv_igdn_f16k<8, 2, 5>", 2: "deconv_igdn_f16k<8, 1, 5>"}


@pytest.mark.parametrize("split", [0, 1, 2, 4])
@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bits_of_conv_f16k(shape, tile, split):
    from masic_amd import deconv
    B, H, W = shape
    x16, wp, bias, gp, want = _operands(shape)
    out = torch.full((B * 128 * 4 * H * W,), R.PREFILL_BITS, dtype=torch.int16, device=DEV)
    got = deconv.deconv_igdn_f16k(x16, wp, bias, gp, B, H, W, out16=out, tile=tile, split=split)
    assert got is out
    name = deconv.kernel_name(B, H, W, tile, split)
    print(f"deconv_igdn | {shape} | tile {tile} split {split} | {name}")
    assert name == NAMES[tile or 2]           # (all five are small: fewer than 256 workgroups on the 16 x 32 tile)
    diff = int((got.cpu() != want).sum())
    assert diff == 0, f"{shape} tile {tile} split {split}: {diff} of {want.numel()} bf16 values differ from conv_f16k's"


def test_tile_choice():
    """the 16 x 32 tile where it makes at least one workgroup per CU with one phase each -- both layers of the benchmark -- else 8 x 32"""
    from masic_amd import deconv
    assert deconv.kernel_name(8, 128, 128) == NAMES[1]
    assert deconv.kernel_name(8, 64, 64) == NAMES[1]
    assert deconv.kernel_name(8, 64, 64, split=1) == NAMES[2]
    assert deconv.kernel_name(8, 32, 32) == NAMES[2]
    assert deconv.kernel_name(1, 8, 8, tile=1) == NAMES[1]


def test_no_bias():
    from masic_amd import deconv, ops
    shape = (1, 8, 8)
    x16, wp, _, gp, _ = _operands(shape)
    with _one_product():
        want = ops.conv2d_f16k(x16, wp, None, R.desc_of(_case(*shape)), gdn=(gp, True))
    assert torch.equal(deconv.deconv_igdn_f16k(x16, wp, None, gp, *shape), want)


def test_vs_float64():
    from masic_amd import deconv, ops
    shape = (2, 20, 36)
    B, H, W = shape
    c = _case(*shape)
    x, w, bias = R.inputs(c, SEED + sum(shape))
    beta, gamma = _gdn_params(SEED)
    _, wp, _, gp, _ = _operands(shape)
    ref = R.conv64(c, x, w, bias)
    s = R.one_product_scale(ref, beta, gamma, True)
    for sc in (1.0, s):
        q = R.one_product_share(sc * ref, beta, gamma, True)
        assert sc == 1.0 or q <= 0.45
        gate = 2.0 ** -8 + (R.one_product_bound(q) if sc == 1.0 else 2.0 ** -9)
        y16 = deconv.deconv_igdn_f16k(R.to_f16k(x * sc).to(DEV), wp, (bias * sc).to(DEV), gp, B, H, W)
        e = rel_err(R.from_f16k(y16, B, 128, 2 * H, 2 * W).float(), R.gdn64(sc * ref, beta, gamma, True))
        print(f"deconv_igdn | {shape} | operands times {sc:g} | share {q:.2f} | gate {gate:.3e} | error {e:.3e}")
        assert e <= gate, f"operands times {sc:g}: {e:.3e} > {gate:.3e}"


def _decoder():
    import MASIC
    from masic_amd import synth
    dec = MASIC.Decoder1(128, 192)
    dec.load_state_dict(synth.synth_state_dict(dec.state_dict(), seed=31))
    return dec.to(DEV).eval()


def test_refusals():
    """every form the kernel does not run is refused, at the module level (the form) and by the library (the shape)"""
    import MASIC
    from masic_amd import _lib, deconv, ops
    dec = _decoder()
    cv, gdn = dec.g_s_conv2, dec.g_s_gdn2
    assert deconv.supported(cv, gdn, 1, 8, 8) and deconv.supported(dec.g_s_conv3, dec.g_s_gdn3, 8, 128, 128)
    assert not deconv.supported(dec.g_s_conv1, dec.g_s_gdn1, 1, 8, 8)                 # 192 -> 128
    assert not deconv.supported(dec.g_s_conv4, None, 1, 8, 8)                         # 128 -> 3, no GDN
    assert not deconv.supported(cv, MASIC.GDN(128).to(DEV), 1, 8, 8)                  # a forward GDN
    assert not deconv.supported(cv, gdn, 1, 8, 8, products=3)                         # the three-product contraction
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_FUSED_GDN_PRODUCTS", 3)
        assert not deconv.supported(cv, gdn, 1, 8, 8)
    assert not deconv.supported(cv, gdn, 1, 8, 8, out_ctot=160, out_coff=16)          # a channel view of the output
    assert not deconv.supported(cv, gdn, 1, 8, 8, in_ctot=160, in_coff=16)            # ... of the input
    assert not deconv.supported(cv, gdn, 1, 8, 8, prec=_lib.PREC_FP8)                 # fp8 operands
    assert not deconv.supported(cv, gdn, 1, 8, 8, y_pre=torch.empty(1, dtype=torch.int16, device=DEV))   # the pre-GDN output of a training step
    assert _lib.lib.masic_deconv_igdn_f16k_supported(1, 8, 8) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 2048, 2048)):
        assert _lib.lib.masic_deconv_igdn_f16k_supported(*bad) == 0, bad
    x16, wp, bias, gp, _ = _operands((1, 8, 8))
    with pytest.raises(RuntimeError):
        deconv.deconv_igdn_f16k(x16, wp[:-1], bias, gp, 1, 8, 8)
    with pytest.raises(RuntimeError):
        deconv.deconv_igdn_f16k(x16, wp, bias, gp, 1, 8, 16)


def test_decoder_takes_either_path():
    """Decoder1.reconstruct at 1 x 3 x 64 x 64: g_s_conv2 and g_s_conv3 run on the new kernel, and with it refused on conv_f16k as before --
    the same bits both ways"""
    from masic_amd import deconv
    from masic_amd import nn as mnn
    dec = _decoder()
    y_hat = torch.round(4.0 * torch.randn(1, 192, 4, 4, generator=torch.Generator().manual_seed(5))).to(DEV)
    calls = []
    run = deconv.run
    mnn.set_precision("bf16")
    try:
        with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
            mp.setattr(deconv, "run", lambda *a, **k: calls.append((a[2].B, a[2].H, a[2].W)) or run(*a, **k))
            new = dec.reconstruct(y_hat)
            assert calls == [(1, 8, 8), (1, 16, 16)]
            mp.setattr(deconv, "supported", lambda *a, **k: False)
            old = dec.reconstruct(y_hat)
            assert len(calls) == 2
    finally:
        mnn.set_precision("f32")
    assert tuple(new.shape) == (1, 3, 64, 64) and bool(torch.isfinite(new).all())
    assert torch.equal(R.bits(new), R.bits(old))


def test_graph_replay():
    """two back-to-back launches (8 x 8 -> 16 x 16 -> 32 x 32; the first with all four phases per workgroup) captured in a graph replay to
    the eager bits, also on new input"""
    from masic_amd import deconv
    x16, wp, bias, gp, _ = _operands((1, 8, 8))

    def chain(x):
        return deconv.deconv_igdn_f16k(deconv.deconv_igdn_f16k(x, wp, bias, gp, 1, 8, 8, split=1), wp, bias, gp, 1, 16, 16)

    x2 = R.to_f16k(R.inputs(_case(1, 8, 8), SEED + 1)[0]).to(DEV)
    want1, want2 = chain(x16).clone(), chain(x2).clone()
    sx = x16.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(sx)                                      # the LDS opt-in and the allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = chain(sx)
    g.replay()
    assert torch.equal(out, want1)
    sx.copy_(x2)
    g.replay()
    assert torch.equal(out, want2)
