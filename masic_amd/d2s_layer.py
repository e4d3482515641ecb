"""The 128 -> C (C <= 8) 5x5 stride-2 transposed last layer of the synthesis transforms (g_s_conv4) on a kernel of its own
(masic_amd/csrc/d2s_layer.hip).

    if d2s_layer.supported(cv, B, Hi, Wi) and d2s_layer.preferred(cv, B, Hi, Wi):
        y = d2s_layer.run(cv, x, out=..., out_coff=...)       # the tensor and the bits of cv.run_f16k_d2s(x, out, out_coff)

Operands are conv_f16k's: the slab stream and the 32-entry bias `cv.packed_d2s` packs and caches for run_f16k_d2s -- no pack and no
cache of its own.  The form is fixed (a whole 128-channel bf16 F16K input, the equivalent 3x3 convolution to 32 padded rows, the
depth-to-space store); `supported` answers False for everything else -- and for the shapes whose stream conv_f16k packs in another
order (its 32-channel-chunk row) -- and the caller keeps run_f16k_d2s for it.  `preferred` is the library's rule for the eval forward
(profiles/d2s_layer_ab.txt); the bits do not depend on it.

The entry points are declared in include/masic_d2s.h, a side header of libmasic_hip.so bound by _lib.bind_header; the launcher's first
checks, the KernelTimer hook, the common part of `supported`, and `preferred` are layer_kernel.LayerKernel's.  No CPU path.
"""
import ctypes
import functools

import torch

from . import _lib, ops
from .f16k import F16K
from .layer_kernel import IN_CHANNELS, LayerKernel
from .ops import _p

MAX_OUT_CHANNELS = 8
PACKED_BYTES = 8 * 5 * 2 * 4096                   # the layer's slab stream: 8 chunks of 16 channels x 5 steps of 2 taps x 4 KiB
ROW = "conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false>"     # the conv_f16k row whose stream and sum order the kernel shares


def conv_desc(B, Hi, Wi):
    """The descriptor of the equivalent stride-1 3x3 convolution to 32 rows: run_f16k_d2s's."""
    return ops.make_conv_desc(B, IN_CHANNELS, Hi, Wi, 32, 3, 3, 1, 1, prec=_lib.PREC_BF16)


_KERNEL = LayerKernel("masic_d2s.h", "masic_d2s_", "d2s_layer_f16k", who="d2s_layer", transposed=True, out_channels=range(1, MAX_OUT_CHANNELS + 1),
                      layer="the 128 -> 32 3x3 layer", packed_bytes=PACKED_BYTES, bias_len=32, desc=conv_desc, cv_supported="d2s_supported")
HEADER_PATH, SIGNATURES = _KERNEL.header_path, _KERNEL.signatures          # name -> (restype, argtypes) of every prototype of masic_d2s.h
kernel_name = _KERNEL.kernel_name                 # (B, Hi, Wi)
preferred = _KERNEL.preferred                     # (cv, B, Hi, Wi): masic_d2s_layer_f16k_preferred
_WHO = _KERNEL.who


@functools.lru_cache(maxsize=256)
def takes_row(B, Hi, Wi):
    """True where conv_f16k runs the depth-to-space form of the shape on ROW (masic_conv_f16k_kernel_name)."""
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib.masic_conv_f16k_kernel_name(ctypes.byref(conv_desc(B, Hi, Wi)), _lib.F16K_NOSPLIT, buf, 96)
    return rc == 0 and buf.value.decode() == ROW


def launch(x16, packed, bias, B, Hi, Wi, C, out=None, out_coff=0, max_wgs=0):
    """The layer with the arguments, the tensor and -- where conv_f16k runs the shape on ROW -- the bits of ops.conv2d_f16k_d2s: x16 an
    F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of ops.pack_conv_f16k_weight for a descriptor that takes ROW, bias the 32
    values of ops.deconv_s2_as_conv_weight or None.  Returns float32 NCHW [B, C, 2Hi, 2Wi], or `out` written at channels out_coff ..;
    max_wgs > 0 caps the grid (tests)."""
    _KERNEL.check(x16, packed, bias, B, Hi, Wi)
    if not 0 < C <= MAX_OUT_CHANNELS:
        raise RuntimeError(f"{_WHO}: 1 to {MAX_OUT_CHANNELS} output channels, not {C}")
    if out is None:
        out_coff = 0
        out = torch.empty((B, C, 2 * Hi, 2 * Wi), dtype=torch.float32, device=x16.device)
    else:
        ops._dev(out, "output")
        if (out.dim() != 4 or (out.shape[0], out.shape[2], out.shape[3]) != (B, 2 * Hi, 2 * Wi) or out.device != x16.device
                or not 0 <= out_coff <= out.shape[1] - C):
            raise RuntimeError(f"{_WHO}: `out` is not a float32 [{B}, >= {out_coff + C}, {2 * Hi}, {2 * Wi}] tensor on the input's device")
    _KERNEL.fwd(B, Hi, Wi, (), _p(x16), _p(packed), _p(bias), _p(out), C, out.shape[1], out_coff, B, Hi, Wi, max_wgs)
    return out


def supported(cv, B, Hi, Wi, in_ctot=None, in_coff=0, prec=_lib.PREC_BF16):
    """True where run(cv, x, ...) stands for cv.run_f16k_d2s(x, ...) on a whole F16K x of [B, 128, Hi, Wi]: ConvTranspose2d(128, C <= 8,
    5, stride 2, padding 2), bf16 operands (LayerKernel.supported), and a shape at which conv_f16k runs the layer on ROW, so that the
    cached stream is in this kernel's order."""
    return _KERNEL.supported(cv, B, Hi, Wi, in_ctot, in_coff, prec) and takes_row(B, Hi, Wi)


def run(cv, x, out=None, out_coff=0):
    """cv.run_f16k_d2s(x, out, out_coff) where supported(cv, x.B, x.H, x.W): float32 NCHW [B, C, 2Hi, 2Wi], or `out` written at
    channels out_coff ..; the pack is the one that call uses."""
    if not isinstance(x, F16K) or not x.whole or x.C != IN_CHANNELS or not supported(cv, x.B, x.H, x.W):
        raise RuntimeError(f"{_WHO}: run takes whole 128-channel tensors and the 128 -> C <= 8 5x5 stride-2 transposed layer at the shapes of "
                           f"{ROW}, not {x!r} on {cv!r}")
    _, wp, bc = cv.packed_d2s(x.B, x.H, x.W)
    return launch(x.buf, wp, bc, x.B, x.H, x.W, cv.out_channels, out=out, out_coff=out_coff)
