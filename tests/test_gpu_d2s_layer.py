"""d2s_layer_f16k (masic_amd/csrc/d2s_layer.hip, masic_amd/d2s_layer.py): the 128 -> C <= 8 last layer of the synthesis transforms on the
kernel of its own.

Bit equality.  The yardstick is the kernel it stands for: masic_conv_f16k_d2s_fwd (ops.conv2d_f16k_d2s) on the same packed operands,
compared with torch.equal on the whole output view -- the contraction order and the epilogue are the same, so the match is exact and
needs no tolerance.  That holds only where conv_f16k runs the layer on its 16-channel-chunk row (asserted by name first), which by
choose_f16k needs ceil(Wi / 32) ceil(Hi / 32) B >= 512.  `launch` is called directly: `preferred` is not consulted.  (B, Hi, Wi); a
tile is 16 x 32 pixels:
    (57, 65, 65)   513 tiles of conv_f16k; here 5 x 3 tiles per image, interior tiles with halos on all sides, a single last row and
                   a single last column, the plain block map, 62 MB of input
    (88, 33, 65)   528 tiles of conv_f16k; here 3 x 3 tiles per image, the image-per-XCD map (11 images per XCD), single-row and
                   single-column edge tiles
Each runs three ways: C = 3 into channels 1 .. 3 of a 5-channel buffer, C = 8 (every padded row live) into channels 1 .. 8 of 10, and
C = 3 with the grid capped (200 workgroups for 855 tiles: 5 or 4 tiles each; 64 for 99 tiles per XCD: 13 or 12 each).  The output
buffers are prefilled with a sentinel that must survive outside the view, and the allocator's free blocks of the output sizes are
overwritten before every launch.  The operands are real-valued (bf16 x and w, float32 bias), so a changed sum order would show.

Float64.  Small shapes on which conv_f16k would take another row and another stream, so the stream is packed for a descriptor that takes
the row: (1, 5, 7) a picture smaller than a tile; (2, 33, 70) ragged in both directions, tiles of two images; (9, 16, 64).  Each with
the launcher's own grid and with one workgroup that walks every tile across the images.  The check is the one
tests/test_gpu_f16k_rows.py makes for the depth-to-space form -- whole-number operands drawn by its _ints through f16k_ref.d2s_weight
(the bias and the weights of rows >= 4C are zero), every partial sum exact in float32, the output view equal to the float64 transposed
convolution with the prefill outside -- and, on real operands, tests.util.assert_close at the 2e-5 that file holds the row itself to.

Whole model.  HSIC's eval forward at the smallest square pictures (B = 8) for which `preferred` is true, with the layer forced onto
either kernel: x1_hat and x2_hat equal bit for bit.
"""
import functools

import pytest
import torch

from tests import f16k_ref as R
from tests.test_gpu_f16k_rows import _ints
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "d2s_layer_f16k"
SENTINEL = -777.25
BIG = [(57, 65, 65), (88, 33, 65)]
CAP = {(57, 65, 65): 200, (88, 33, 65): 64}
WAYS = [("C3 view", 3, 0), ("C8", 8, 0), ("C3 capped", 3, 1)]
SMALL = [(1, 5, 7), (2, 33, 70), (9, 16, 64)]


def _row_desc():
    """a descriptor of the layer that takes the 16-channel-chunk row: its pack is the stream the kernel reads at every shape"""
    from masic_amd import d2s_layer
    assert d2s_layer.takes_row(512, 32, 32)
    return d2s_layer.conv_desc(512, 32, 32)


@functools.lru_cache(maxsize=None)
def _big_operands(shape, C):
    """x16, packed weights, bias and conv_f16k's output view (computed once per shape and C, never written)"""
    from masic_amd import d2s_layer, ops
    B, H, W = shape
    assert d2s_layer.takes_row(B, H, W), "conv_f16k does not run this shape on the 16-channel-chunk row"
    g = torch.Generator(device=DEV).manual_seed(7100 + sum(shape) + C)
    x16 = ops.nchw_to_f16k(2.0 * torch.randn((B, 128, H, W), device=DEV, generator=g))
    gc = torch.Generator().manual_seed(7100 + C)
    wt = (torch.randn((128, C, 5, 5), generator=gc) * (128 * 9) ** -0.5).bfloat16().float()
    w, b = R.d2s_weight(wt, torch.randn(C, generator=gc))
    d = d2s_layer.conv_desc(B, H, W)
    wp, b = ops.pack_conv_f16k_weight(w.to(DEV), d), b.to(DEV)
    ref = torch.full((B, C + 2, 2 * H, 2 * W), SENTINEL, device=DEV)
    ops.conv2d_f16k_d2s(x16, wp, b, d, C, out=ref, out_coff=1)
    torch.cuda.synchronize()
    assert bool((ref[:, 0] == SENTINEL).all()) and bool((ref[:, C + 1] == SENTINEL).all()) and bool(torch.isfinite(ref).all())
    return x16, wp, b, ref


def _poison(shape):
    """overwrite the allocator's free blocks of the output's size, so that an element the kernel leaves out shows as NaN and not as an
    earlier launch's value"""
    junk = [torch.full(shape, float("nan"), device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("way", WAYS, ids=[w[0] for w in WAYS])
@pytest.mark.parametrize("shape", BIG, ids=["x".join(map(str, s)) for s in BIG])
def test_bits_of_conv_f16k(shape, way):
    from masic_amd import d2s_layer
    _, C, capped = way
    B, H, W = shape
    assert d2s_layer.takes_row(B, H, W) and d2s_layer.ROW == "conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false>"
    x16, wp, b, ref = _big_operands(shape, C)
    _poison(tuple(ref.shape))
    out = torch.full(tuple(ref.shape), SENTINEL, device=DEV)
    got = d2s_layer.launch(x16, wp, b, B, H, W, C, out=out, out_coff=1, max_wgs=CAP[shape] if capped else 0)
    torch.cuda.synchronize()
    assert got is out
    diff = int((R.bits(out) != R.bits(ref)).sum())
    print(f"d2s_layer | {shape} | {way[0]} | {diff} of {ref.numel()} values differ")
    assert torch.equal(R.bits(out), R.bits(ref)), f"{shape} {way[0]}: {diff} of {ref.numel()} values differ from conv_f16k's"


@pytest.mark.parametrize("max_wgs", [0, 1])
@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_vs_float64(shape, max_wgs):
    from masic_amd import d2s_layer, ops
    B, H, W = shape
    c = R.case_of((B, 128, H, W, 32, 3, 1, 0, 0), flags=R.F16K_NOSPLIT)
    g = torch.Generator().manual_seed(7200 + sum(shape))
    d = _row_desc()

    def run(x, w, bias):
        out = torch.full((B, 5, 2 * H, 2 * W), R.PREFILL, device=DEV)
        _poison(tuple(out.shape))
        d2s_layer.launch(R.to_f16k(x).to(DEV), ops.pack_conv_f16k_weight(w.to(DEV), d), bias.to(DEV), B, H, W, 3, out=out, out_coff=1, max_wgs=max_wgs)
        torch.cuda.synchronize()
        return out.cpu()

    # whole numbers: every partial sum is a float32 integer, the result is the float64 transposed convolution exactly
    x = R.inputs(c, 7200 + sum(shape), integers=True)[0]
    wt, bt = _ints(g, (128, 3, 5, 5), 4), _ints(g, (3,), 20)
    w, bias = R.d2s_weight(wt, bt)
    assert R.exact_bound(c, x, w, bias) < 2 ** 24
    ref = torch.nn.functional.conv_transpose2d(x.double(), wt.double(), bt.double(), stride=2, padding=2, output_padding=1)
    assert torch.equal(run(x, w, bias).double(), R.in_view(ref, 5, 1)), f"{shape} max_wgs {max_wgs}: whole numbers"

    # real operands: the gate of the row
    x = R.inputs(c, 7700 + sum(shape))[0]
    wt = (torch.randn((128, 3, 5, 5), generator=g) * (128 * 9) ** -0.5).bfloat16().float()
    bt = torch.randn(3, generator=g)
    w, bias = R.d2s_weight(wt, bt)
    ref = torch.nn.functional.conv_transpose2d(x.double(), wt.double(), bt.double(), stride=2, padding=2, output_padding=1)
    out = run(x, w, bias)
    assert bool((out[:, 0] == R.PREFILL).all()) and bool((out[:, 4] == R.PREFILL).all()), "prefill"
    e = assert_close(out[:, 1:4], ref, f"{shape} max_wgs {max_wgs}", 2e-5)
    print(f"d2s_layer | {shape} | max_wgs {max_wgs} | real operands | gate 2.0e-05 | error {e:.3e}")


def test_no_bias_and_refusals():
    from masic_amd import d2s_layer
    shape = (57, 65, 65)
    B, H, W = shape
    x16, wp, b, ref = _big_operands(shape, 3)
    out = d2s_layer.launch(x16, wp, None, B, H, W, 3)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, 3, 2 * H, 2 * W)
    # the bias is the accumulators' start: without it the sums differ, by about the bias
    assert float((out - ref[:, 1:4]).abs().max()) <= float(b.abs().max()) * 1.01 + 1e-3
    assert d2s_layer.kernel_name(B, H, W) == d2s_layer.kernel_name(1, 5, 7) == NAME
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp[:-1], b, B, H, W, 3)
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp, b, B, H, W + 1, 3)
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp, b[:-1].contiguous(), B, H, W, 3)
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp, b, B, H, W, 9)
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp, b, B, H, W, 3, out=torch.empty((B, 5, 2 * H, 2 * W), device=DEV), out_coff=3)
    with pytest.raises(RuntimeError):
        d2s_layer.launch(x16, wp, b, B, H, W, 3, max_wgs=-1)
    torch.cuda.synchronize()


def _smallest_preferred():
    """the smallest square pictures (B = 8, side a multiple of 64) whose last synthesis layer `preferred` takes"""
    from masic_amd import d2s_layer
    for S in range(64, 1024 + 1, 64):
        if d2s_layer.preferred(None, 8, S // 2, S // 2):
            return S
    return None


def test_model_takes_either_path():
    """HSIC eval forward, bf16 operands: g_s_conv4 of both decoders on the new kernel, and with it refused on conv_f16k as before"""
    import MASIC
    from masic_amd import d2s_layer, synth
    from masic_amd import nn as mnn
    S = _smallest_preferred()
    if S is None:
        assert not d2s_layer.preferred(None, 8, 256, 256)         # the rule takes no shape: nothing to compare
        return
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=33))
    net = net.to(DEV).eval()
    x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(8, S, S, seed=33))
    calls = []
    run = d2s_layer.run
    mnn.set_precision("bf16")
    try:
        with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
            mp.setattr(d2s_layer, "run", lambda *a, **k: calls.append((a[1].B, a[1].H, a[1].W)) or run(*a, **k))
            new = net(x1, x2, hm)
            n_new = len(calls)
            mp.setattr(d2s_layer, "preferred", lambda *a, **k: False)
            old = net(x1, x2, hm)
    finally:
        mnn.set_precision("f32")
    torch.cuda.synchronize()
    assert n_new >= 2 and len(calls) == n_new and set(calls) == {(8, S // 2, S // 2)}
    for k in ("x1_hat", "x2_hat"):
        assert bool(torch.isfinite(new[k]).all())
        assert torch.equal(R.bits(new[k]), R.bits(old[k])), k
