"""The Python side of a kernel that owns one fixed 128 -> 128 5x5 stride-2 layer with a fused one-product (I)GDN beside conv_f16k
(DESIGN.md section 4.1): masic_amd/deconv.py and masic_amd/conv_s2.py each declare one LayerKernel and bind their public names from it.

A LayerKernel states what differs between such layers -- its side header and C entry points (masic_<stem>_supported / _fwd /
_kernel_name), the direction of the convolution and of the GDN, the size of the packed weight stream, the output size, and the extra
integer arguments of its launcher -- and holds what does not: the operand checks, the KernelTimer hook, `supported` with its list of
refusals, and `run`.  Operands are conv_f16k's (the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k`): no
pack and no cache of its own.  No CPU path.
"""
import ctypes
import os

import torch

from . import _lib, ops
from .f16k import F16K
from .ops import _p, _stream

CHANNELS = 128


class LayerKernel:
    def __init__(self, header, prefix, stem, *, transposed, inverse, packed_bytes, out_hw, extras=()):
        """header, prefix: the side header and the prefix of its names (_lib.bind_header); stem: masic_<stem>_supported(B, Hi, Wi),
        masic_<stem>_fwd(x, w, bias, gdn, y, B, Hi, Wi, *extras, stream), masic_<stem>_kernel_name(B, Hi, Wi, *extras, buf, n);
        out_hw(Hi, Wi) -> (Ho, Wo); extras: ((name, allowed values), ...) of the launcher's extra integer arguments, each 0 by default."""
        self.header_path = os.path.join(os.path.dirname(_lib.HEADER_PATH), header)
        self.signatures = _lib.bind_header(self.header_path, prefix)
        self.stem, self.transposed, self.inverse, self.packed_bytes, self.out_hw, self.extras = stem, transposed, inverse, packed_bytes, out_hw, extras
        self.layer = f"128 -> 128 {'transposed ' if transposed else ''}5x5 stride-2 layer"
        self._supported, self._fwd, self._name = (getattr(_lib.lib, f"masic_{stem}_{f}") for f in ("supported", "fwd", "kernel_name"))

    def _extra(self, args, kw):
        """the extra integers in the launcher's order, from positional and keyword arguments"""
        names = [name for name, _ in self.extras]
        given = dict(zip(names, args), **kw)
        if len(args) > len(names) or set(given) - set(names):
            raise TypeError(f"masic_amd.{self.stem}: the extra arguments are {names}, got {list(args)} and {sorted(kw)}")
        return tuple(given.get(name, 0) for name in names)

    def kernel_name(self, B, Hi, Wi, *args, **kw):
        """The symbol of the kernel the launcher starts for the shape (and the extra arguments), as rocprofv3 prints it."""
        buf = ctypes.create_string_buffer(96)
        _lib.check(self._name(B, Hi, Wi, *self._extra(args, kw), buf, 96), f"{self.stem}_kernel_name")
        return buf.value.decode()

    def launch(self, x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None, **kw):
        """(I)GDN(conv(x) + bias) of the fixed layer: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of
        ops.pack_conv_f16k_weight for the layer, `gdn_packed` ops.pack_gdn_f16k's image; returns the F16K buffer [B][8][Ho*Wo][16]
        (`out16` if given).  The extra arguments (0: chosen from the shape) change the launch, not the bits."""
        who = f"masic_amd.{self.stem}"
        if x16.dtype != torch.int16 or not x16.is_cuda or x16.numel() != B * CHANNELS * Hi * Wi:
            raise RuntimeError(f"{who}: input must be an F16K int16 CUDA buffer of [{B},{CHANNELS},{Hi},{Wi}]")
        if packed.dtype != torch.int16 or packed.numel() * 2 != self.packed_bytes or packed.device != x16.device:
            raise RuntimeError(f"{who}: `packed` is not the slab stream of a {self.layer}")
        if gdn_packed.numel() * gdn_packed.element_size() != ops._int_query("masic_gdn_f16k_packed_bytes") or gdn_packed.device != x16.device:
            raise RuntimeError(f"{who}: `gdn_packed` is not a packed 128-channel GDN")
        if bias is not None:
            ops._dev(bias, "bias")
            if bias.numel() != CHANNELS or bias.device != x16.device:
                raise RuntimeError(f"{who}: bias must hold 128 values on the input's device")
        extra = self._extra((), kw)
        if any(v not in allowed for v, (_, allowed) in zip(extra, self.extras)):
            raise ValueError(f"{who}: " + ", ".join(f"{name} must be one of {allowed}" for name, allowed in self.extras))
        if not self._supported(B, Hi, Wi):
            raise RuntimeError(f"{who}: shape [{B},{CHANNELS},{Hi},{Wi}] is not supported")
        Ho, Wo = self.out_hw(Hi, Wi)
        n_out = B * CHANNELS * Ho * Wo
        if out16 is None:
            out16 = torch.empty(n_out, dtype=torch.int16, device=x16.device)
        elif out16.dtype != torch.int16 or out16.numel() != n_out or out16.device != x16.device or not out16.is_contiguous():
            raise RuntimeError(f"{who}: out16 does not match the output")
        timed = None
        if ops._timer is not None:
            desc = ops.make_conv_desc(B, CHANNELS, Hi, Wi, CHANNELS, 5, 5, 2, 2, transposed=self.transposed, prec=_lib.PREC_BF16)
            timed = ops._timer_open(desc, lambda d, buf, n: self._name(B, Hi, Wi, *extra, buf, n))
        _lib.check(self._fwd(_p(x16), _p(packed), _p(bias), _p(gdn_packed), _p(out16), B, Hi, Wi, *extra, _stream()), f"{self.stem}_fwd")
        if timed is not None:
            ops._timer_close(timed)
        return out16

    def supported(self, cv, gdn, B, Hi, Wi, out_ctot=None, out_coff=0, in_ctot=None, in_coff=0, y_pre=None, prec=_lib.PREC_BF16, products=None):
        """True where run(cv, gdn, x) stands for cv.run_f16k(x, gdn=gdn) on a whole F16K x of [B, 128, Hi, Wi]: the layer's (transposed)
        5x5 stride-2 convolution, padding 2 (output_padding 1), unmasked, followed by a 128-channel GDN of the layer's direction in its
        one-product form, bf16 operands.  The keyword arguments name what the caller would ask of conv_f16k besides: a channel view of
        the input or the output, a second pre-GDN output, fp8 operands, the three-product contraction -- each of them is refused."""
        if gdn is None or getattr(cv, "transposed_conv", None) is not self.transposed or getattr(cv, "masked_conv", True):
            return False
        if cv.in_channels != CHANNELS or cv.out_channels != CHANNELS:
            return False
        if cv._geometry() != (5, 5, 2, 2) or bool(gdn.inverse) is not self.inverse or gdn.beta.numel() != CHANNELS:
            return False
        if prec != _lib.PREC_BF16 or y_pre is not None or (ops._gdn_flags(self.inverse, products) & 2):
            return False
        if out_coff != 0 or out_ctot not in (None, CHANNELS) or in_coff != 0 or in_ctot not in (None, CHANNELS):
            return False
        return bool(self._supported(B, Hi, Wi)) and cv.f16k_supported(B, Hi, Wi)

    def run(self, cv, gdn, x):
        """The F16K of cv.run_f16k(x, gdn=gdn) where supported(cv, gdn, x.B, x.H, x.W); the packs are the ones that call uses."""
        from .nn import packed_gdn_f16k
        if not x.whole or x.C != CHANNELS:
            raise RuntimeError(f"masic_amd.{self.stem}: run takes whole 128-channel tensors, not {x!r}")
        desc = cv._desc_f16k(x.B, x.H, x.W, out_ctot=CHANNELS)
        bias = None if cv.bias is None else cv.bias.detach()
        y16 = self.launch(x.buf, cv.packed_f16k_weight(desc), bias, packed_gdn_f16k(gdn), x.B, x.H, x.W)
        return F16K(y16, x.B, CHANNELS, desc.Ho, desc.Wo, CHANNELS, 0)
