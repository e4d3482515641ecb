"""The 128 -> 128 transposed 5x5 stride-2 convolution with fused inverse GDN of the synthesis transforms (g_s_conv2 / g_s_conv3) on a
kernel of its own (masic_amd/csrc/deconv_igdn.hip).

    if deconv.supported(cv, gdn, B, Hi, Wi):
        y = deconv.run(cv, gdn, x)        # x, y F16K values; the bits of cv.run_f16k(x, gdn=gdn)

Operands are conv_f16k's: the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k` -- no pack and no cache of
its own.  The form is fixed (bf16 F16K in and out without a channel view, one-product inverse GDN); `supported` answers False for
everything else and the caller keeps conv_f16k for it.

The entry points are declared in include/masic_deconv.h, a header of libmasic_hip.so beside include/masic_hip.h, whose declarations and
what masic_amd._lib derives from them are a pinned ABI (tests/golden/abi.json).  The header is parsed by _lib.parse_header and bound on
_lib.lib here.  No CPU path.
"""
import ctypes
import os

import torch

from . import _lib, ops
from .f16k import F16K
from .ops import _p, _stream

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "masic_deconv.h")
CHANNELS = 128
PACKED_BYTES = 4 * (5 + 3 + 3 + 2) * 16384        # the layer's slab stream: 4 chunks x (5 + 3 + 3 + 2) steps of 2 taps x 2 blocks x 4 KiB
TILES = (0, 1, 2)                                 # 0: chosen from the shape, 1: 16 x 32 input pixels per workgroup, 2: 8 x 32
SPLITS = (0, 1, 2, 4)                             # workgroups per tile: 4 = one output phase each (what 0 chooses), 1 = all four phases


def _bind():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"masic_amd.deconv: {HEADER_PATH} is missing: the binding is derived from it.  There is no CPU fallback for "
                          "the HIP path.")
    with open(HEADER_PATH) as f:
        signatures, constants, structs = _lib.parse_header(f.read(), header="masic_deconv.h")
    if constants or structs:
        raise ValueError("masic_deconv.h: declares constants or structs; it holds prototypes only")
    for name, (res, args) in signatures.items():
        if not name.startswith("masic_deconv_") or name in _lib.SIGNATURES:
            raise ValueError(f"masic_deconv.h: {name} is not a masic_deconv_* entry point of its own")
        fn = getattr(_lib.lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return signatures


SIGNATURES = _bind()          # name -> (restype, argtypes) of every prototype of masic_deconv.h


def kernel_name(B, Hi, Wi, tile=0, split=0):
    """The symbol of the kernel deconv_igdn_f16k launches for the shape, as rocprofv3 prints it."""
    buf = ctypes.create_string_buffer(96)
    _lib.check(_lib.lib.masic_deconv_igdn_f16k_kernel_name(B, Hi, Wi, tile, split, buf, 96), "deconv_igdn_f16k_kernel_name")
    return buf.value.decode()


def deconv_igdn_f16k(x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None, tile=0, split=0):
    """IGDN(conv_transpose(x) + bias) of the fixed 128 -> 128 layer: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of
    ops.pack_conv_f16k_weight for the layer, `gdn_packed` ops.pack_gdn_f16k's image; returns the F16K buffer [B][8][4*Hi*Wi][16]
    (`out16` if given).  tile, split: the workgroup's tile and the workgroups per tile (0: chosen from the shape); same bits for all."""
    if x16.dtype != torch.int16 or not x16.is_cuda or x16.numel() != B * CHANNELS * Hi * Wi:
        raise RuntimeError(f"masic_amd.deconv_igdn_f16k: input must be an F16K int16 CUDA buffer of [{B},{CHANNELS},{Hi},{Wi}]")
    if packed.dtype != torch.int16 or packed.numel() * 2 != PACKED_BYTES or packed.device != x16.device:
        raise RuntimeError("masic_amd.deconv_igdn_f16k: `packed` is not the slab stream of a 128 -> 128 transposed 5x5 stride-2 layer")
    if gdn_packed.numel() * gdn_packed.element_size() != ops._int_query("masic_gdn_f16k_packed_bytes") or gdn_packed.device != x16.device:
        raise RuntimeError("masic_amd.deconv_igdn_f16k: `gdn_packed` is not a packed 128-channel GDN")
    if bias is not None:
        ops._dev(bias, "bias")
        if bias.numel() != CHANNELS or bias.device != x16.device:
            raise RuntimeError("masic_amd.deconv_igdn_f16k: bias must hold 128 values on the input's device")
    if tile not in TILES or split not in SPLITS:
        raise ValueError(f"masic_amd.deconv_igdn_f16k: tile must be one of {TILES}, split one of {SPLITS}")
    if not _lib.lib.masic_deconv_igdn_f16k_supported(B, Hi, Wi):
        raise RuntimeError(f"masic_amd.deconv_igdn_f16k: shape [{B},{CHANNELS},{Hi},{Wi}] is not supported")
    n_out = B * CHANNELS * 4 * Hi * Wi
    if out16 is None:
        out16 = torch.empty(n_out, dtype=torch.int16, device=x16.device)
    elif out16.dtype != torch.int16 or out16.numel() != n_out or out16.device != x16.device or not out16.is_contiguous():
        raise RuntimeError("masic_amd.deconv_igdn_f16k: out16 does not match the output")
    timed = None
    if ops._timer is not None:
        desc = ops.make_conv_desc(B, CHANNELS, Hi, Wi, CHANNELS, 5, 5, 2, 2, transposed=True, prec=_lib.PREC_BF16)
        timed = ops._timer_open(desc, lambda d, buf, n: _lib.lib.masic_deconv_igdn_f16k_kernel_name(B, Hi, Wi, tile, split, buf, n))
    _lib.check(_lib.lib.masic_deconv_igdn_f16k_fwd(_p(x16), _p(packed), _p(bias), _p(gdn_packed), _p(out16), B, Hi, Wi, tile, split, _stream()),
               "deconv_igdn_f16k_fwd")
    if timed is not None:
        ops._timer_close(timed)
    return out16


def supported(cv, gdn, B, Hi, Wi, out_ctot=None, out_coff=0, in_ctot=None, in_coff=0, y_pre=None, prec=_lib.PREC_BF16, products=None):
    """True where run(cv, gdn, x) stands for cv.run_f16k(x, gdn=gdn) on a whole F16K x of [B, 128, Hi, Wi]: a ConvTranspose2d(128, 128,
    5, stride 2, padding 2, output_padding 1) followed by a 128-channel inverse GDN in its one-product form, bf16 operands.
    The keyword arguments name what the caller would ask of conv_f16k besides: a channel view of the input or the output, a second
    pre-GDN output, fp8 operands, the three-product contraction -- each of them is refused."""
    if gdn is None or not getattr(cv, "transposed_conv", False) or cv.in_channels != CHANNELS or cv.out_channels != CHANNELS:
        return False
    if cv._geometry() != (5, 5, 2, 2) or not gdn.inverse or gdn.beta.numel() != CHANNELS:
        return False
    if prec != _lib.PREC_BF16 or y_pre is not None or (ops._gdn_flags(True, products) & 2):
        return False
    if out_coff != 0 or out_ctot not in (None, CHANNELS) or in_coff != 0 or in_ctot not in (None, CHANNELS):
        return False
    return bool(_lib.lib.masic_deconv_igdn_f16k_supported(B, Hi, Wi)) and cv.f16k_supported(B, Hi, Wi)


def run(cv, gdn, x):
    """The F16K of cv.run_f16k(x, gdn=gdn) where supported(cv, gdn, x.B, x.H, x.W); the packs are the ones that call uses."""
    from .nn import packed_gdn_f16k
    if not x.whole or x.C != CHANNELS:
        raise RuntimeError(f"masic_amd.deconv.run: the kernel takes whole 128-channel tensors, not {x!r}")
    desc = cv._desc_f16k(x.B, x.H, x.W, out_ctot=CHANNELS)
    bias = None if cv.bias is None else cv.bias.detach()
    y16 = deconv_igdn_f16k(x.buf, cv.packed_f16k_weight(desc), bias, packed_gdn_f16k(gdn), x.B, x.H, x.W)
    return F16K(y16, x.B, CHANNELS, desc.Ho, desc.Wo, CHANNELS, 0)
