"""The F16K value type (masic_amd/f16k.py) on CPU int16 tensors: what wrap refuses, how channel views compose, and that a view names the
channel range a hand-built slice of the decoded parent gives."""
import pytest
import torch

from masic_amd import ops
from masic_amd.f16k import F16K


def _buf(B, ctot, H, W):
    return torch.zeros(B * ctot * H * W, dtype=torch.int16)


def test_wrap_rejects_what_no_kernel_takes():
    B, H, W = 2, 3, 5
    ok = F16K.wrap(_buf(B, 48, H, W), B, 40, H, W)
    assert (ok.ctot, ok.coff, ok.shape, ok.whole) == (48, 0, (B, 40, H, W), True)
    with pytest.raises(TypeError):
        F16K.wrap(_buf(B, 48, H, W).to(torch.int32), B, 40, H, W)            # dtype
    with pytest.raises(ValueError):
        F16K.wrap(_buf(B, 48, H, W)[:-1], B, 40, H, W)                       # numel
    with pytest.raises(ValueError):
        F16K.wrap(torch.zeros(B * 40 * H * W, dtype=torch.int16), B, 40, H, W, ctot=40)      # ctot % 16
    with pytest.raises(ValueError):
        F16K.wrap(_buf(B, 48, H, W), B, 16, H, W, ctot=48, coff=8)           # coff % 16
    with pytest.raises(ValueError):
        F16K.wrap(_buf(B, 48, H, W), B, 40, H, W, ctot=48, coff=16)          # coff + C > ctot


@pytest.mark.parametrize("C", [3, 16, 40, 192])
def test_empty_rounds_the_channels_up_to_16(C):
    t = F16K.empty(2, C, 3, 5, "cpu")
    want = (C + 15) // 16 * 16
    assert t.ctot == want and t.coff == 0 and t.whole and t.shape == (2, C, 3, 5)
    assert t.buf.dtype == torch.int16 and t.buf.numel() == 2 * want * 3 * 5


def test_channel_views_share_storage_and_compose():
    B, H, W = 2, 2, 3
    p = F16K.wrap(_buf(B, 96, H, W), B, 96, H, W)
    v = p.channels(32, 48)
    assert v.buf.data_ptr() == p.buf.data_ptr() and v.buf is p.buf
    assert (v.coff, v.C, v.ctot, v.shape) == (32, 48, 96, (B, 48, H, W))
    w = v.channels(16, 32)
    assert w.coff == v.coff + 16 and w.C == 32 and w.ctot == 96 and w.buf is p.buf
    assert p.whole and not v.whole and not w.whole and not p.channels(0, 48).whole
    assert p.channels(0, 96).whole                                  # the full range is the unsliced value again
    for coff, C in ((8, 16), (0, 0), (-16, 16), (32, 32), (48, 16)):         # misaligned, empty, negative, past the view's end
        with pytest.raises(ValueError):
            v.channels(coff, C)
    p.buf[5] = 7
    assert int(v.buf[5]) == 7


def test_view_names_the_channels_a_hand_built_slice_gives():
    """Parent [2][3 blocks][H*W = 6][16] filled with distinct small integers (every one exact in bf16): the torch-op checker decodes
    the parent, and the view's (coff, C) select the same channels as slicing the blocked buffer by hand."""
    B, H, W, ctot = 2, 2, 3, 48
    vals = torch.arange(B * ctot * H * W, dtype=torch.float32) % 251 - 125            # |v| <= 125: exact in bf16
    buf = vals.bfloat16().view(torch.int16)
    p = F16K.wrap(buf, B, ctot, H, W)
    full = ops.f16k_to_nchw(p.buf, B, ctot, H, W)
    blocks = vals.view(B, ctot // 16, H * W, 16)
    for coff, C in ((0, 48), (16, 32), (16, 16), (32, 5), (0, 17)):
        v = p.channels(coff, C)
        got = full[:, v.coff:v.coff + v.C]
        assert tuple(got.shape) == v.shape
        for c in range(C):
            ch = coff + c
            want = blocks[:, ch // 16, :, ch % 16].reshape(B, H, W)
            assert torch.equal(got[:, c], want), (coff, C, c)
