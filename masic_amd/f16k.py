"""F16K activations as one value: the flat buffer, its shape and the channel view it stands for (DESIGN.md "The F16K value").

F16K is the bf16 activation layout of every reduced-precision path, [B][ctot/16][H*W][16] in a flat int16 tensor (include/masic_hip.h).
The buffer carries no shape; `F16K` carries it: `C` logical channels starting at channel `coff` of a buffer of `ctot` channels at
B x H x W.  Raw buffers, descriptors and integers below masic_amd/ops.py (the ctypes boundary), `F16K` above it.  `F8K` is the fp8
sibling: [B][ceil32(C)/32][H*W][32] in a uint8 tensor holding fp8(x / scale).
"""
import torch

from . import ops


def _ceil(c, blk):
    return (c + blk - 1) // blk * blk


class F16K:
    __slots__ = ("buf", "B", "C", "H", "W", "ctot", "coff")

    def __init__(self, buf, B, C, H, W, ctot, coff):
        """Unchecked (what a kernel wrapper just allocated); everything else goes through wrap / empty / from_nchw / channels."""
        self.buf, self.B, self.C, self.H, self.W, self.ctot, self.coff = buf, B, C, H, W, ctot, coff

    @classmethod
    def wrap(cls, buf, B, C, H, W, ctot=None, coff=0):
        """Channels [coff, coff + C) of the existing buffer `buf` of `ctot` (default ceil16(C)) channels; any device."""
        ctot = _ceil(C, 16) if ctot is None else ctot
        if not torch.is_tensor(buf) or buf.dtype != torch.int16:
            raise TypeError("F16K: the buffer must be an int16 tensor")
        if ctot % 16 or coff % 16:
            raise ValueError(f"F16K: ctot {ctot} and coff {coff} must be multiples of 16")
        if C < 1 or coff < 0 or coff + C > ctot:
            raise ValueError(f"F16K: channels [{coff}, {coff + C}) do not lie in a buffer of {ctot}")
        if buf.numel() != B * ctot * H * W:
            raise ValueError(f"F16K: a buffer of {buf.numel()} elements does not hold [{B}, {ctot}, {H}, {W}]")
        return cls(buf, B, C, H, W, ctot, coff)

    @classmethod
    def empty(cls, B, C, H, W, device):
        """An uninitialised whole buffer of ceil16(C) channels."""
        ctot = _ceil(C, 16)
        return cls(torch.empty(B * ctot * H * W, dtype=torch.int16, device=device), B, C, H, W, ctot, 0)

    @classmethod
    def from_nchw(cls, x, in_op=ops.INOP_NONE, C=None, coff=0):
        """bf16(in_op(x[:, coff:coff + C])) of a float32 NCHW tensor (ops.nchw_to_f16k); in_op: |x| / round(x) on the way."""
        B, ctot, H, W = x.shape
        C = ctot if C is None else C
        return cls(ops.nchw_to_f16k(x, C=C, coff=coff, in_op=in_op), B, C, H, W, _ceil(C, 16), 0)

    @property
    def shape(self):
        return (self.B, self.C, self.H, self.W)

    @property
    def whole(self):
        return self.coff == 0 and self.ctot == _ceil(self.C, 16)

    def channels(self, coff, C):
        """The view of channels [coff, coff + C) of this one, on the same buffer."""
        if coff % 16 or C < 1 or coff < 0 or coff + C > self.C:
            raise ValueError(f"F16K: channels [{coff}, {coff + C}) are misaligned or outside {self!r}")
        return F16K(self.buf, self.B, C, self.H, self.W, self.ctot, self.coff + coff)

    def to_nchw(self, bf16=False):
        """float32 (bf16: exact bf16) NCHW copy of the view (ops.f16k_to_nchw_dev)."""
        return ops.f16k_to_nchw_dev(self.buf, self.B, self.C, self.H, self.W, src_ctot=self.ctot, src_coff=self.coff, bf16=bf16)

    def fill_from_nchw(self, x, in_op=ops.INOP_NONE, gate=None, gate_c=0):
        """view = bf16(in_op(x) * gate[:, gate_c]) for a float32 NCHW x of the view's shape (ops.nchw_to_f16k_view)."""
        if tuple(x.shape) != self.shape:
            raise ValueError(f"F16K: a tensor of {tuple(x.shape)} does not fill {self!r}")
        ops.nchw_to_f16k_view(x, self.buf, self.ctot, self.coff, in_op=in_op, gate=gate, gate_c=gate_c)
        return self

    def fill_gated(self, src, gate=None, gate_c=0, minv=None):
        """view = (warp(src, minv) if minv is not None else src) * gate[:, gate_c] for a whole F16K src of the view's shape (ops.f16k_gate)."""
        if not src.whole or src.shape != self.shape:
            raise ValueError(f"F16K: {src!r} does not fill {self!r}")
        ops.f16k_gate(src.buf, self.B, self.C, self.H, self.W, self.buf, self.ctot, self.coff, gate=gate, gate_c=gate_c, minv=minv)
        return self

    def record_stream(self, stream):
        self.buf.record_stream(stream)

    def __repr__(self):
        return f"F16K([{self.B}, {self.C}, {self.H}, {self.W}], channels {self.coff}.. of {self.ctot})"


class F8K:
    """fp8(x / scale) records of 32 channels (whole tensors only: no kernel takes a channel view of one)."""
    __slots__ = ("buf", "B", "C", "H", "W", "scale")

    def __init__(self, buf, B, C, H, W, scale):
        self.buf, self.B, self.C, self.H, self.W, self.scale = buf, B, C, H, W, scale

    @classmethod
    def wrap(cls, buf, B, C, H, W, scale):
        if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.numel() != B * _ceil(C, 32) * H * W:
            raise ValueError(f"F8K: the buffer must be a uint8 tensor holding [{B}, {_ceil(C, 32)}, {H}, {W}]")
        if not scale > 0:
            raise ValueError("F8K: the scale must be positive")
        return cls(buf, B, C, H, W, scale)

    @property
    def shape(self):
        return (self.B, self.C, self.H, self.W)
