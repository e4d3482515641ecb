"""The 128 -> 128 5x5 stride-2 convolution with fused forward GDN of the analysis transforms (g_a_conv2 / g_a_conv3) on a kernel of its
own (masic_amd/csrc/conv_s2_gdn.hip).

    if conv_s2.supported(cv, gdn, B, Hi, Wi):
        y = conv_s2.run(cv, gdn, x)        # x, y F16K values; the bits of cv.run_f16k(x, gdn=gdn)

Operands are conv_f16k's: the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k` -- no pack and no cache of
its own.  The form is fixed (bf16 F16K in and out without a channel view, one-product forward GDN); `supported` answers False for
everything else and the caller keeps conv_f16k for it.

The entry points are declared in include/masic_conv_s2.h, a header of libmasic_hip.so beside include/masic_hip.h, whose declarations and
what masic_amd._lib derives from them are a pinned ABI (tests/golden/abi.json).  The header is parsed by _lib.parse_header and bound on
_lib.lib here.  No CPU path.
"""
import ctypes
import os

import torch

from . import _lib, ops
from .f16k import F16K
from .ops import _p, _stream

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "masic_conv_s2.h")
CHANNELS = 128
PACKED_BYTES = 8 * 5 * 20480                      # the layer's slab stream: 8 chunks x 5 steps of 5 taps x 4 KiB


def _bind():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"masic_amd.conv_s2: {HEADER_PATH} is missing: the binding is derived from it.  There is no CPU fallback for "
                          "the HIP path.")
    with open(HEADER_PATH) as f:
        signatures, constants, structs = _lib.parse_header(f.read(), header="masic_conv_s2.h")
    if constants or structs:
        raise ValueError("masic_conv_s2.h: declares constants or structs; it holds prototypes only")
    for name, (res, args) in signatures.items():
        if not name.startswith("masic_conv_s2_") or name in _lib.SIGNATURES:
            raise ValueError(f"masic_conv_s2.h: {name} is not a masic_conv_s2_* entry point of its own")
        fn = getattr(_lib.lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return signatures


SIGNATURES = _bind()          # name -> (restype, argtypes) of every prototype of masic_conv_s2.h


def out_hw(Hi, Wi):
    return (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1


def kernel_name(B, Hi, Wi):
    """The symbol of the kernel conv_s2_gdn_f16k launches for the shape, as rocprofv3 prints it."""
    buf = ctypes.create_string_buffer(96)
    _lib.check(_lib.lib.masic_conv_s2_gdn_f16k_kernel_name(B, Hi, Wi, buf, 96), "conv_s2_gdn_f16k_kernel_name")
    return buf.value.decode()


def conv_s2_gdn_f16k(x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None):
    """GDN(conv(x) + bias) of the fixed 128 -> 128 layer: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of
    ops.pack_conv_f16k_weight for the layer, `gdn_packed` ops.pack_gdn_f16k's image; returns the F16K buffer [B][8][Ho*Wo][16]
    (`out16` if given)."""
    if x16.dtype != torch.int16 or not x16.is_cuda or x16.numel() != B * CHANNELS * Hi * Wi:
        raise RuntimeError(f"masic_amd.conv_s2_gdn_f16k: input must be an F16K int16 CUDA buffer of [{B},{CHANNELS},{Hi},{Wi}]")
    if packed.dtype != torch.int16 or packed.numel() * 2 != PACKED_BYTES or packed.device != x16.device:
        raise RuntimeError("masic_amd.conv_s2_gdn_f16k: `packed` is not the slab stream of a 128 -> 128 5x5 stride-2 layer")
    if gdn_packed.numel() * gdn_packed.element_size() != ops._int_query("masic_gdn_f16k_packed_bytes") or gdn_packed.device != x16.device:
        raise RuntimeError("masic_amd.conv_s2_gdn_f16k: `gdn_packed` is not a packed 128-channel GDN")
    if bias is not None:
        ops._dev(bias, "bias")
        if bias.numel() != CHANNELS or bias.device != x16.device:
            raise RuntimeError("masic_amd.conv_s2_gdn_f16k: bias must hold 128 values on the input's device")
    if not _lib.lib.masic_conv_s2_gdn_f16k_supported(B, Hi, Wi):
        raise RuntimeError(f"masic_amd.conv_s2_gdn_f16k: shape [{B},{CHANNELS},{Hi},{Wi}] is not supported")
    Ho, Wo = out_hw(Hi, Wi)
    n_out = B * CHANNELS * Ho * Wo
    if out16 is None:
        out16 = torch.empty(n_out, dtype=torch.int16, device=x16.device)
    elif out16.dtype != torch.int16 or out16.numel() != n_out or out16.device != x16.device or not out16.is_contiguous():
        raise RuntimeError("masic_amd.conv_s2_gdn_f16k: out16 does not match the output")
    timed = None
    if ops._timer is not None:
        desc = ops.make_conv_desc(B, CHANNELS, Hi, Wi, CHANNELS, 5, 5, 2, 2, prec=_lib.PREC_BF16)
        timed = ops._timer_open(desc, lambda d, buf, n: _lib.lib.masic_conv_s2_gdn_f16k_kernel_name(B, Hi, Wi, buf, n))
    _lib.check(_lib.lib.masic_conv_s2_gdn_f16k_fwd(_p(x16), _p(packed), _p(bias), _p(gdn_packed), _p(out16), B, Hi, Wi, _stream()),
               "conv_s2_gdn_f16k_fwd")
    if timed is not None:
        ops._timer_close(timed)
    return out16


def supported(cv, gdn, B, Hi, Wi, out_ctot=None, out_coff=0, in_ctot=None, in_coff=0, y_pre=None, prec=_lib.PREC_BF16, products=None):
    """True where run(cv, gdn, x) stands for cv.run_f16k(x, gdn=gdn) on a whole F16K x of [B, 128, Hi, Wi]: a Conv2d(128, 128, 5,
    stride 2, padding 2) followed by a 128-channel forward GDN in its one-product form, bf16 operands.
    The keyword arguments name what the caller would ask of conv_f16k besides: a channel view of the input or the output, a second
    pre-GDN output, fp8 operands, the three-product contraction -- each of them is refused."""
    if gdn is None or getattr(cv, "transposed_conv", True) or getattr(cv, "masked_conv", True):
        return False
    if cv.in_channels != CHANNELS or cv.out_channels != CHANNELS:
        return False
    if cv._geometry() != (5, 5, 2, 2) or gdn.inverse or gdn.beta.numel() != CHANNELS:
        return False
    if prec != _lib.PREC_BF16 or y_pre is not None or (ops._gdn_flags(False, products) & 2):
        return False
    if out_coff != 0 or out_ctot not in (None, CHANNELS) or in_coff != 0 or in_ctot not in (None, CHANNELS):
        return False
    return bool(_lib.lib.masic_conv_s2_gdn_f16k_supported(B, Hi, Wi)) and cv.f16k_supported(B, Hi, Wi)


def run(cv, gdn, x):
    """The F16K of cv.run_f16k(x, gdn=gdn) where supported(cv, gdn, x.B, x.H, x.W); the packs are the ones that call uses."""
    from .nn import packed_gdn_f16k
    if not x.whole or x.C != CHANNELS:
        raise RuntimeError(f"masic_amd.conv_s2.run: the kernel takes whole 128-channel tensors, not {x!r}")
    desc = cv._desc_f16k(x.B, x.H, x.W, out_ctot=CHANNELS)
    bias = None if cv.bias is None else cv.bias.detach()
    y16 = conv_s2_gdn_f16k(x.buf, cv.packed_f16k_weight(desc), bias, packed_gdn_f16k(gdn), x.B, x.H, x.W)
    return F16K(y16, x.B, CHANNELS, desc.Ho, desc.Wo, CHANNELS, 0)
