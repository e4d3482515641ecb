"""The Python side of a kernel that owns one fixed 5x5 stride-2 layer on a whole 128-channel bf16 F16K input beside conv_f16k (DESIGN.md
section 4.1): masic_amd/deconv.py, conv_s2.py, latent.py and d2s_layer.py each declare one LayerKernel and bind their public names from it.

A LayerKernel states what differs between such layers -- its side header and C entry points (masic_<stem>_supported / _fwd /
_kernel_name, _preferred where the header has one), the direction of the convolution, the output widths, the packed weight stream and the
bias it takes, the extra integer arguments of its kernel_name -- and holds what does not: the operand checks every launcher makes first,
the KernelTimer hook, the refusals common to every `supported`, and `preferred`.  GdnLayerKernel adds what the two 128 -> 128 layers with
a fused one-product (I)GDN share: the packed-GDN operand, `out16`, the refusals of the GDN's other forms, and `run`.  Operands are
conv_f16k's (the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k`): no pack and no cache of its own.  No
CPU path.
"""
import ctypes

import torch

from . import _lib, ops
from .f16k import F16K
from .ops import _p, _stream

IN_CHANNELS = CHANNELS = 128


class LayerKernel:
    def __init__(self, header, prefix, stem, *, transposed, out_channels, layer, packed_bytes, bias_len, who=None, extras=(), desc=None,
                 cv_supported="f16k_supported"):
        """header, prefix: the side header and the prefix of its names (_lib.bind_header); stem: masic_<stem>_supported(B, Hi, Wi),
        masic_<stem>_preferred(B, Hi, Wi) if declared, masic_<stem>_fwd(..., stream), masic_<stem>_kernel_name(B, Hi, Wi, *extras, buf, n);
        out_channels: the widths `supported` takes; layer: what `packed` (packed_bytes) is the slab stream of, for the message; who: the
        name the messages begin with; extras: ((name, allowed values), ...) of the extra integer arguments, each 0 by default;
        desc(B, Hi, Wi): the descriptor a KernelTimer accounts the launch under (default: the layer's own, out_channels[0] wide);
        cv_supported: the method of the convolution module that answers for conv_f16k's side of the shape."""
        self.header_path = _lib.header_path(header)
        self.signatures = _lib.bind_header(header, prefix)
        self.stem, self.transposed, self.out_channels, self.layer, self.packed_bytes, self.bias_len = stem, transposed, out_channels, layer, packed_bytes, bias_len
        self.who, self.extras, self.cv_supported = f"masic_amd.{who or stem}", extras, cv_supported
        self.desc = desc or (lambda B, Hi, Wi: ops.make_conv_desc(B, IN_CHANNELS, Hi, Wi, out_channels[0], 5, 5, 2, 2, transposed=transposed,
                                                                  prec=_lib.PREC_BF16))
        self._supported, self._fwd, self._name = (getattr(_lib.lib, f"masic_{stem}_{f}") for f in ("supported", "fwd", "kernel_name"))
        self._preferred = getattr(_lib.lib, f"masic_{stem}_preferred") if f"masic_{stem}_preferred" in self.signatures else None

    def _extra(self, args, kw):
        """the extra integers in the launcher's order, from positional and keyword arguments"""
        if not (self.extras or args or kw):
            return ()
        names = [name for name, _ in self.extras]
        given = dict(zip(names, args), **kw)
        if len(args) > len(names) or set(given) - set(names):
            raise TypeError(f"{self.who}: the extra arguments are {names}, got {list(args)} and {sorted(kw)}")
        return tuple(given.get(name, 0) for name in names)

    def kernel_name(self, B, Hi, Wi, *args, **kw):
        """The symbol of the kernel the launcher starts for the shape (and the extra arguments), as rocprofv3 prints it."""
        buf = ctypes.create_string_buffer(96)
        _lib.check(self._name(B, Hi, Wi, *self._extra(args, kw), buf, 96), f"{self.stem}_kernel_name")
        return buf.value.decode()

    def check(self, x16, packed, bias, B, Hi, Wi):
        """what every launcher checks first: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the layer's slab stream, the bias, the shape"""
        if x16.dtype != torch.int16 or not x16.is_cuda or x16.numel() != B * IN_CHANNELS * Hi * Wi:
            raise RuntimeError(f"{self.who}: input must be an F16K int16 CUDA buffer of [{B},{IN_CHANNELS},{Hi},{Wi}]")
        if packed.dtype != torch.int16 or packed.numel() * 2 != self.packed_bytes or packed.device != x16.device:
            raise RuntimeError(f"{self.who}: `packed` is not the slab stream of {self.layer}")
        if bias is not None:
            ops._dev(bias, "bias")
            if bias.numel() != self.bias_len or bias.device != x16.device:
                raise RuntimeError(f"{self.who}: bias must hold {self.bias_len} values on the input's device")
        if not self._supported(B, Hi, Wi):
            raise RuntimeError(f"{self.who}: shape [{B},{IN_CHANNELS},{Hi},{Wi}] is not supported")

    def fwd(self, B, Hi, Wi, extra, *args):
        """masic_<stem>_fwd(*args, stream) inside the installed KernelTimer's bracket, if there is one"""
        timed = None
        if ops._timer is not None:
            timed = ops._timer_open(self.desc(B, Hi, Wi), lambda d, buf, n: self._name(B, Hi, Wi, *extra, buf, n))
        _lib.check(self._fwd(*args, _stream()), f"{self.stem}_fwd")
        if timed is not None:
            ops._timer_close(timed)

    def supported(self, cv, B, Hi, Wi, in_ctot=None, in_coff=0, prec=_lib.PREC_BF16):
        """True where the kernel stands for conv_f16k on the module cv and a whole F16K x of [B, 128, Hi, Wi]: the layer's (transposed)
        5x5 stride-2 convolution, padding 2 (output_padding 1), unmasked, of one of the layer's widths, bf16 operands, at a shape both
        take.  The keyword arguments name what the caller would ask of conv_f16k besides: a channel view of the input, other operands
        -- each of them is refused."""
        if getattr(cv, "transposed_conv", None) is not self.transposed or getattr(cv, "masked_conv", True):
            return False
        if cv.in_channels != IN_CHANNELS or cv.out_channels not in self.out_channels or cv._geometry() != (5, 5, 2, 2):
            return False
        if prec != _lib.PREC_BF16 or in_coff != 0 or in_ctot not in (None, IN_CHANNELS):
            return False
        return bool(self._supported(B, Hi, Wi)) and getattr(cv, self.cv_supported)(B, Hi, Wi)

    def preferred(self, cv, B, Hi, Wi):
        """True where the eval forward takes this kernel for the shape instead of conv_f16k (masic_<stem>_preferred; True without one)."""
        return self._preferred is None or bool(self._preferred(B, Hi, Wi))


class GdnLayerKernel(LayerKernel):
    def __init__(self, header, prefix, stem, *, transposed, inverse, packed_bytes, out_hw, extras=()):
        """a 128 -> 128 layer with a fused GDN of direction `inverse`: masic_<stem>_fwd(x, w, bias, gdn, y, B, Hi, Wi, *extras, stream);
        out_hw(Hi, Wi) -> (Ho, Wo)"""
        super().__init__(header, prefix, stem, transposed=transposed, out_channels=(CHANNELS,), packed_bytes=packed_bytes, bias_len=CHANNELS,
                         layer=f"a 128 -> 128 {'transposed ' if transposed else ''}5x5 stride-2 layer", extras=extras)
        self.inverse, self.out_hw = inverse, out_hw

    def launch(self, x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None, **kw):
        """(I)GDN(conv(x) + bias) of the fixed layer: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of
        ops.pack_conv_f16k_weight for the layer, `gdn_packed` ops.pack_gdn_f16k's image; returns the F16K buffer [B][8][Ho*Wo][16]
        (`out16` if given).  The extra arguments (0: chosen from the shape) change the launch, not the bits."""
        self.check(x16, packed, bias, B, Hi, Wi)
        if gdn_packed.numel() * gdn_packed.element_size() != ops._int_query("masic_gdn_f16k_packed_bytes") or gdn_packed.device != x16.device:
            raise RuntimeError(f"{self.who}: `gdn_packed` is not a packed 128-channel GDN")
        extra = self._extra((), kw)
        if any(v not in allowed for v, (_, allowed) in zip(extra, self.extras)):
            raise ValueError(f"{self.who}: " + ", ".join(f"{name} must be one of {allowed}" for name, allowed in self.extras))
        Ho, Wo = self.out_hw(Hi, Wi)
        n_out = B * CHANNELS * Ho * Wo
        if out16 is None:
            out16 = torch.empty(n_out, dtype=torch.int16, device=x16.device)
        elif out16.dtype != torch.int16 or out16.numel() != n_out or out16.device != x16.device or not out16.is_contiguous():
            raise RuntimeError(f"{self.who}: out16 does not match the output")
        self.fwd(B, Hi, Wi, extra, _p(x16), _p(packed), _p(bias), _p(gdn_packed), _p(out16), B, Hi, Wi, *extra)
        return out16

    def supported(self, cv, gdn, B, Hi, Wi, out_ctot=None, out_coff=0, in_ctot=None, in_coff=0, y_pre=None, prec=_lib.PREC_BF16, products=None):
        """True where run(cv, gdn, x) stands for cv.run_f16k(x, gdn=gdn): LayerKernel.supported, followed by a 128-channel GDN of the
        layer's direction in its one-product form.  Refused besides: a channel view of the output, a second pre-GDN output, the
        three-product contraction."""
        if gdn is None or bool(gdn.inverse) is not self.inverse or gdn.beta.numel() != CHANNELS:
            return False
        if y_pre is not None or (products or ops._FUSED_GDN_PRODUCTS) == 3 or out_coff != 0 or out_ctot not in (None, CHANNELS):
            return False
        return LayerKernel.supported(self, cv, B, Hi, Wi, in_ctot, in_coff, prec)

    def run(self, cv, gdn, x):
        """The F16K of cv.run_f16k(x, gdn=gdn) where supported(cv, gdn, x.B, x.H, x.W); the packs are the ones that call uses."""
        from .nn import packed_gdn_f16k
        if not x.whole or x.C != CHANNELS:
            raise RuntimeError(f"{self.who}: run takes whole 128-channel tensors, not {x!r}")
        desc = cv._desc_f16k(x.B, x.H, x.W, out_ctot=CHANNELS)
        bias = None if cv.bias is None else cv.bias.detach()
        y16 = self.launch(x.buf, cv.packed_f16k_weight(desc), bias, packed_gdn_f16k(gdn), x.B, x.H, x.W)
        return F16K(y16, x.B, CHANNELS, desc.Ho, desc.Wo, CHANNELS, 0)
