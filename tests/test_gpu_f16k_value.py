"""The F16K value type (masic_amd/f16k.py) on the device: conversions through a value and through a channel view, and a convolution
that writes into a view -- bit for bit what the whole-tensor forms give, with every other channel of the wider buffer untouched."""
import pytest
import torch

from masic_amd import ops
from masic_amd.f16k import F16K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bf(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("in_op,ref", [(ops.INOP_NONE, lambda x: x), (ops.INOP_ABS, torch.abs), (ops.INOP_ROUND, torch.round)])
def test_round_trip_at_channels_that_are_no_multiple_of_16(in_op, ref):
    x = 3.0 * torch.randn(2, 40, 3, 5, generator=torch.Generator().manual_seed(40))
    v = F16K.from_nchw(x.to(DEV), in_op=in_op)
    assert v.shape == (2, 40, 3, 5) and v.ctot == 48 and v.whole
    got = v.to_nchw().cpu()
    assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(_bf(ref(x))))
    assert torch.equal(v.to_nchw(bf16=True).cpu().float(), got)               # the bf16 NCHW form holds the same values


def test_fill_through_a_view_leaves_the_other_channels_alone():
    B, H, W = 2, 4, 8
    parent = F16K.from_nchw(torch.full((B, 64, H, W), 7.0, device=DEV))
    x32 = torch.randn(B, 32, H, W, generator=torch.Generator().manual_seed(41))
    view = parent.channels(16, 32)
    assert view.fill_from_nchw(x32.to(DEV)) is view
    got = ops.f16k_to_nchw(parent.buf, B, 64, H, W).cpu()
    assert torch.equal(_bits(got[:, :16]), _bits(torch.full((B, 16, H, W), 7.0)))
    assert torch.equal(_bits(got[:, 48:]), _bits(torch.full((B, 16, H, W), 7.0)))
    assert torch.equal(_bits(got[:, 16:48]), _bits(_bf(x32)))
    assert torch.equal(_bits(view.to_nchw().cpu()), _bits(_bf(x32)))          # ... and the view reads back its own channels
    with pytest.raises(ValueError):
        view.fill_from_nchw(torch.zeros(B, 16, H, W, device=DEV))


def test_run_f16k_into_a_view_gives_the_whole_tensor_bits():
    from masic_amd import nn as mnn
    B, C, H, W = 1, 32, 16, 32
    conv = mnn.Conv2d(C, C, 3, padding=1).to(DEV)
    x = F16K.from_nchw(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(42)).to(DEV))
    assert conv.f16k_supported(B, H, W)
    with torch.no_grad():
        whole = conv.run_f16k(x, act=ops.ACT_LEAKY)
        assert whole.shape == (B, C, H, W) and whole.whole
        wide = F16K.from_nchw(torch.full((B, 96, H, W), 7.0, device=DEV))
        view = wide.channels(32, 32)
        assert conv.run_f16k(x, act=ops.ACT_LEAKY, out=view) is view
    torch.cuda.synchronize()
    want = torch.full((B, 96 // 16, H * W, 16), 7.0).bfloat16().view(torch.int16)
    want[:, 2:4] = whole.buf.cpu().view(B, 2, H * W, 16)                      # the whole-tensor result copied into blocks 2, 3
    assert torch.equal(wide.buf.cpu().view(B, 6, H * W, 16), want)
    with pytest.raises(RuntimeError):
        conv.run_f16k(x, out=wide.channels(32, 48))                           # not this layer's output
