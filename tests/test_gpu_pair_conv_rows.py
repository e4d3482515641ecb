"""GPU tests (-m gpu) of conv5s1_pair_rows, the four-pixels-per-lane kernel behind ops.conv5s1_pair for W % 4 == 0 and
16-byte aligned tensors (encoder2.pre_conv + pre_gdn, decoder2.after_gdn + cat + after_conv).  It must produce the bits of
conv5s1_small<4>, so every comparison is torch.equal and the reference is that kernel, reached without a switch:
  * without a GDN, through the generic ops.conv2d on the concatenated sources;
  * with a GDN, through ops.conv5s1_pair at width W + 1 (not a multiple of 4: the dispatch falls back) on inputs with an
    all-zero last column, cropped to W columns: zero padding and a zero column go through the same FMAs, gdn3(0) = 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2
# (H, W): exactly one 64x16 tile; one partial tile in both directions; three tiles wide with a ragged last one and three
# tall with one row in the last; image smaller than the halo; second tile 4 columns wide
SHAPES = [(16, 64), (37, 52), (33, 132), (5, 4), (20, 68)]


def _rand(*shape, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(size=shape) * scale).astype(np.float32)).to(DEV)


def _layer(H, W, transposed):
    from masic_amd import ops
    w = _rand(*((6, 3, 5, 5) if transposed else (3, 6, 5, 5)), seed=3, scale=0.1)
    bias = _rand(3, seed=4, scale=0.1)
    desc = ops.make_conv_desc(B, 6, H, W, 3, 5, 5, 1, 2, transposed=transposed)
    return ops.pack_conv_weight(w, desc), bias, desc


def _gdn(inverse):
    from masic_amd import synth
    rs = np.random.RandomState(5)
    return synth.synth_tensor("g.beta", (3,), rs).to(DEV), synth.synth_tensor("g.gamma", (3, 3), rs).to(DEV), inverse


def _zero_col(x):
    """x with one all-zero column appended (a fresh, aligned tensor of width W + 1)."""
    return torch.cat((x, torch.zeros_like(x[..., :1])), -1).contiguous()


def _pair(xa, xb, packed, bias, where, transposed):
    from masic_amd import ops
    g = _gdn(transposed)
    return ops.conv5s1_pair(xa, xb, packed, bias, gdn_in=g if where == "in" else None, gdn_out=g if where == "out" else None)


@pytest.mark.parametrize("transposed", [False, True], ids=["conv", "deconv"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_rows_equals_generic_path(H, W, transposed):
    from masic_amd import ops
    xa, xb = _rand(B, 3, H, W, seed=1), _rand(B, 3, H, W, seed=2)
    packed, bias, desc = _layer(H, W, transposed)
    ref = ops.conv2d(torch.cat((xa, xb), 1), packed, bias, desc)          # conv5s1_small<4>
    assert torch.equal(_pair(xa, xb, packed, bias, "none", transposed), ref)
    assert torch.equal(ops.conv5s1_pair(xa, xb, packed, None), ops.conv2d(torch.cat((xa, xb), 1), packed, None, desc))


@pytest.mark.parametrize("where", ["in", "out"])
@pytest.mark.parametrize("transposed", [False, True], ids=["conv", "deconv"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_rows_with_gdn_equals_old_kernel_cropped(H, W, transposed, where):
    xa, xb = _rand(B, 3, H, W, seed=1), _rand(B, 3, H, W, seed=2)
    packed, bias, _ = _layer(H, W, transposed)
    ref = _pair(_zero_col(xa), _zero_col(xb), packed, bias, where, transposed)[..., :W]      # W + 1: conv5s1_small<4>
    assert torch.equal(_pair(xa, xb, packed, bias, where, transposed), ref)


@pytest.mark.parametrize("where", ["none", "in", "out"])
def test_crop_yardstick_is_exact_on_the_old_kernel(where):
    """The yardstick of the GDN test, checked where both sides are conv5s1_small<4>: W and W + 1 are no multiples of 4."""
    H, W = 37, 53
    xa, xb = _rand(B, 3, H, W, seed=1), _rand(B, 3, H, W, seed=2)
    packed, bias, _ = _layer(H, W, True)
    ref = _pair(_zero_col(xa), _zero_col(xb), packed, bias, where, True)[..., :W]
    assert torch.equal(_pair(xa, xb, packed, bias, where, True), ref)


def test_fallback_width_equals_generic_path():
    from masic_amd import ops
    H, W = 37, 53
    xa, xb = _rand(B, 3, H, W, seed=1), _rand(B, 3, H, W, seed=2)
    packed, bias, desc = _layer(H, W, False)
    assert torch.equal(ops.conv5s1_pair(xa, xb, packed, bias), ops.conv2d(torch.cat((xa, xb), 1), packed, bias, desc))


@pytest.mark.parametrize("off_a,off_b", [(1, 0), (0, 2), (3, 1)])
def test_offset_views_take_the_fallback(off_a, off_b):
    """Contiguous views whose storage offset is no multiple of 16 bytes (off floats into an aligned buffer)."""
    from masic_amd import ops
    H, W = 37, 52
    n = B * 3 * H * W

    def view(seed, off):
        buf = torch.zeros(n + 4, device=DEV)
        v = buf[off:off + n].view(B, 3, H, W)
        v.copy_(_rand(B, 3, H, W, seed=seed))
        assert v.data_ptr() % 16 == 4 * off
        return v

    xa, xb = view(1, off_a), view(2, off_b)
    packed, bias, desc = _layer(H, W, True)
    ref = ops.conv2d(torch.cat((xa, xb), 1), packed, bias, desc)
    assert torch.equal(ops.conv5s1_pair(xa, xb, packed, bias), ref)
    assert torch.equal(ops.conv5s1_pair(xa.clone(), xb.clone(), packed, bias), ref)          # aligned copies: the new kernel
