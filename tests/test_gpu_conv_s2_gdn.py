"""conv_s2_gdn_f16k (masic_amd/csrc/conv_s2_gdn.hip, masic_amd/conv_s2.py): the 128 -> 128 5x5 stride-2 convolution with fused one-product
forward GDN on the kernel of its own.

The yardstick is the kernel it stands for: masic_conv_f16k_gdn_fwd (ops.conv2d_f16k, gdn = forward, one product) on the same packed
operands, compared on the raw bf16 records -- the contraction order and the epilogue are the same, so the match is exact and needs no
tolerance.  The shapes (B, Hi, Wi) are the smallest at which each mechanism can go wrong:
    (1, 5, 7)      one partial tile; a picture smaller than the patch; Ho = 3, Wo = 4
    (2, 33, 130)   Ho = 17, Wo = 65: three tile rows and columns, the last a single row / column; odd height and even width, so the
                   bottom and right padding differ
    (8, 16, 64)    exactly one full tile per image; the image-per-XCD block map with the grid rounded up to 8
    (9, 16, 64)    the plain block map
    (8, 32, 128)   four tiles per image on the XCD map; halos shared across tile borders in both directions
and the kernel's name is checked at the two shapes of the benchmark.  Operands come from tests/f16k_ref.py and the GDN parameters from
the row test's generator; every output buffer is prefilled.

One case is also held to the float64 reference of tests/f16k_ref.py under the gates tests/test_gpu_f16k_rows.py (the gdn_dual form)
applies to the one-product GDN of conv_f16k where the output is F16K: the rounding to bf16 plus f16k_ref.one_product_bound(q) on the
operands as drawn, and the rounding plus half of it on the operands times the power of two at which q <= 0.45.
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
SHAPES = [(1, 5, 7), (2, 33, 130), (8, 16, 64), (9, 16, 64), (8, 32, 128)]
SEED = 5200
NAME = "conv_s2_gdn_f16k"
BF16_ROUNDING = 2.0 ** -8                             # tests/test_gpu_f16k_rows.py: an F16K output against float64


def _case(B, H, W):
    return R.case_of((B, 128, H, W, 128, 5, 2, 0, 0), flags=R.F16K_GDN)


def _prefilled(shape):
    return L.prefilled(_case(*shape))


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """x16, packed weights, bias, packed GDN on the device and the output of the existing kernel (computed once per shape, never written)"""
    return L.operands(_case(*shape), SEED + sum(shape), SEED, False, out16=_prefilled(shape))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bits_of_conv_f16k(shape):
    from masic_amd import conv_s2
    B, H, W = shape
    x16, wp, bias, gp, want = _operands(shape)
    out = _prefilled(shape)
    got = conv_s2.conv_s2_gdn_f16k(x16, wp, bias, gp, B, H, W, out16=out)
    assert got is out
    assert conv_s2.kernel_name(B, H, W) == NAME
    diff = int((got.cpu() != want).sum())
    print(f"conv_s2_gdn | {shape} | {NAME} | {diff} of {want.numel()} bf16 values differ")
    assert diff == 0, f"{shape}: {diff} of {want.numel()} bf16 values differ from conv_f16k's"


def test_kernel_name():
    from masic_amd import conv_s2
    assert conv_s2.kernel_name(8, 256, 256) == NAME
    assert conv_s2.kernel_name(8, 128, 128) == NAME


def test_no_bias():
    from masic_amd import conv_s2, ops
    shape = (1, 5, 7)
    x16, wp, _, gp, _ = _operands(shape)
    with _one_product():
        want = ops.conv2d_f16k(x16, wp, None, R.desc_of(_case(*shape)), gdn=(gp, False), out16=_prefilled(shape))
    assert torch.equal(conv_s2.conv_s2_gdn_f16k(x16, wp, None, gp, *shape, out16=_prefilled(shape)), want)


def test_vs_float64():
    from masic_amd import conv_s2
    shape = (2, 33, 130)
    B, H, W = shape
    c = _case(*shape)
    Ho, Wo = R.out_hw(c)
    x, w, bias = R.inputs(c, SEED + sum(shape))
    beta, gamma = _gdn_params(SEED)
    _, wp, _, gp, _ = _operands(shape)
    ref = R.conv64(c, x, w, bias)
    s = R.one_product_scale(ref, beta, gamma, False)
    for sc in (1.0, s):
        q = R.one_product_share(sc * ref, beta, gamma, False)
        assert sc == 1.0 or q <= 0.45
        gate = BF16_ROUNDING + (R.one_product_bound(q) if sc == 1.0 else BF16_ROUNDING / 2)
        y16 = conv_s2.conv_s2_gdn_f16k(R.to_f16k(x * sc).to(DEV), wp, (bias * sc).to(DEV), gp, B, H, W, out16=_prefilled(shape))
        e = rel_err(R.from_f16k(y16, B, 128, Ho, Wo).float(), R.gdn64(sc * ref, beta, gamma, False))
        print(f"conv_s2_gdn | {shape} | operands times {sc:g} | share {q:.2f} | gate {gate:.3e} | error {e:.3e}")
        assert e <= gate, f"operands times {sc:g}: {e:.3e} > {gate:.3e}"


def _encoder():
    import MASIC
    from masic_amd import synth
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31))
    return net.encoder1.to(DEV).eval()


def test_module_and_refusals():
    """g_a_conv2 / g_a_gdn2 of a synthetic-weight encoder: run() stores the bits of run_f16k(gdn=...); every form the kernel does not run is
    refused, at the module level (the form) and by the library (the shape)"""
    import MASIC
    from masic_amd import _lib, conv_s2, ops
    from masic_amd.f16k import F16K
    enc = _encoder()
    cv, gdn = enc.g_a_conv2, enc.g_a_gdn2
    B, H, W = 1, 32, 64
    x = R.inputs(_case(B, H, W), SEED + 7)[0]
    x16 = F16K.wrap(R.to_f16k(x).to(DEV), B, 128, H, W)
    assert conv_s2.supported(cv, gdn, B, H, W) and conv_s2.supported(enc.g_a_conv3, enc.g_a_gdn3, 8, 128, 128)
    with torch.no_grad(), _one_product():
        got, want = conv_s2.run(cv, gdn, x16), cv.run_f16k(x16, gdn=gdn)
    assert (got.B, got.C, got.H, got.W, got.ctot, got.coff) == (want.B, want.C, want.H, want.W, want.ctot, want.coff) == (B, 128, 16, 32, 128, 0)
    assert torch.equal(got.buf, want.buf)

    dec = MASIC.Decoder1(128, 192).to(DEV)
    assert not conv_s2.supported(dec.g_s_conv2, gdn, B, H, W)                           # transposed
    assert not conv_s2.supported(enc.g_a_conv4, gdn, B, H, W)                           # 128 -> 192
    assert not conv_s2.supported(MASIC.conv(128, 128, kernel_size=3, stride=1).to(DEV), gdn, B, H, W)    # another geometry
    assert not conv_s2.supported(MASIC.conv(128, 128, kernel_size=5, stride=1).to(DEV), gdn, B, H, W)
    assert not conv_s2.supported(cv, None, B, H, W)                                     # no GDN
    assert not conv_s2.supported(cv, dec.g_s_gdn2, B, H, W)                             # an inverse GDN
    assert not conv_s2.supported(cv, gdn, B, H, W, products=3)                          # the three-product contraction
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_FUSED_GDN_PRODUCTS", 3)
        assert not conv_s2.supported(cv, gdn, B, H, W)
    assert not conv_s2.supported(cv, gdn, B, H, W, out_ctot=160, out_coff=16)           # a channel view of the output
    assert not conv_s2.supported(cv, gdn, B, H, W, in_ctot=160, in_coff=16)             # ... of the input
    assert not conv_s2.supported(cv, gdn, B, H, W, prec=_lib.PREC_FP8)                  # fp8 operands
    assert not conv_s2.supported(cv, gdn, B, H, W, prec=_lib.PREC_F32)                  # float32
    assert not conv_s2.supported(cv, gdn, B, H, W, y_pre=torch.empty(1, dtype=torch.int16, device=DEV))   # the pre-GDN output of a training step
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(1, 5, 7) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 4096, 4096)):
        assert _lib.lib.masic_conv_s2_gdn_f16k_supported(*bad) == 0, bad
    x16, wp, bias, gp, _ = _operands((1, 5, 7))
    with pytest.raises(RuntimeError):
        conv_s2.conv_s2_gdn_f16k(x16, wp[:-1], bias, gp, 1, 5, 7)
    with pytest.raises(RuntimeError):
        conv_s2.conv_s2_gdn_f16k(x16, wp, bias, gp, 1, 5, 8)
    with pytest.raises(RuntimeError):
        conv_s2.run(cv, gdn, F16K(torch.empty(1 * 160 * 5 * 7, dtype=torch.int16, device=DEV), 1, 128, 5, 7, 160, 16))


def test_encoder_takes_either_path():
    """Encoder1.latent at 1 x 3 x 64 x 128 with bf16 operands: g_a_conv2 and g_a_conv3 run on the new kernel, and with it refused on
    conv_f16k as before -- the same bits both ways"""
    from masic_amd import conv_s2
    from masic_amd import nn as mnn
    enc = _encoder()
    x = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = []
    run = conv_s2.run
    mnn.set_precision("bf16")
    try:
        with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
            mp.setattr(conv_s2, "run", lambda *a, **k: calls.append((a[2].B, a[2].H, a[2].W)) or run(*a, **k))
            new = enc.latent(x)
            assert calls == [(1, 32, 64), (1, 16, 32)]
            mp.setattr(conv_s2, "supported", lambda *a, **k: False)
            old = enc.latent(x)
            assert len(calls) == 2
    finally:
        mnn.set_precision("f32")
    assert tuple(new.shape) == (1, 192, 4, 8) and bool(torch.isfinite(new).all())
    assert torch.equal(R.bits(new), R.bits(old))
