"""The 128 -> 192 5x5 stride-2 latent layer of the analysis transforms (g_a_conv4) on a kernel of its own
(masic_amd/csrc/conv_s2_latent.hip).

    if latent.supported(cv, B, Hi, Wi) and latent.preferred(cv, B, Hi, Wi):
        lay = latent.run(cv, x, want, round16=..., gate=..., gate_c=...)     # the dict and the bits of cv.run_f16k_multi(x, want, ...)

Operands are conv_f16k's: the weight stream of `cv.packed_f16k_weight` -- no pack and no cache of its own.  The form is fixed (a whole
128-channel bf16 F16K input, 192 output channels, no activation, the outputs of conv_f16k_multi); `supported` answers False for everything
else and the caller keeps conv_f16k_multi for it.  `preferred` is the library's rule for the eval forward: a threshold on the launch's
workgroup count (profiles/conv_s2_latent_ab.txt); the bits do not depend on it.

The entry points are declared in include/masic_latent.h, a side header of libmasic_hip.so bound by _lib.bind_header; the launcher's
first checks, the KernelTimer hook, `supported` and `preferred` are layer_kernel.LayerKernel's.  No CPU path.
"""
import torch

from . import ops
from .f16k import F16K
from .layer_kernel import IN_CHANNELS, LayerKernel
from .ops import _p

OUT_CHANNELS = 192
PACKED_BYTES = 2 * 8 * 5 * 20480                  # the layer's slab stream: 2 co-blocks x 8 chunks x 5 steps of 5 taps x 4 KiB
WANT = ("y32", "round32", "round16", "abs16")

_KERNEL = LayerKernel("masic_latent.h", "masic_latent_", "latent_s2_f16k", who="latent", transposed=False, out_channels=(OUT_CHANNELS,),
                      layer="a 128 -> 192 5x5 stride-2 layer", packed_bytes=PACKED_BYTES, bias_len=OUT_CHANNELS,
                      cv_supported="f16k_multi_supported")
HEADER_PATH, SIGNATURES = _KERNEL.header_path, _KERNEL.signatures          # name -> (restype, argtypes) of every prototype of masic_latent.h
kernel_name = _KERNEL.kernel_name                 # (B, Hi, Wi)
supported = _KERNEL.supported                     # (cv, B, Hi, Wi, in_ctot=None, in_coff=0, prec=PREC_BF16): where run stands for cv.run_f16k_multi
preferred = _KERNEL.preferred                     # (cv, B, Hi, Wi): masic_latent_s2_f16k_preferred
_WHO = _KERNEL.who


def out_hw(Hi, Wi):
    return (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1


def launch(x16, packed, bias, B, Hi, Wi, want=WANT, round16=None, round16_ctot=0, round16_coff=0, gate=None, gate_c=0):
    """v = conv(x) + bias of the fixed layer written once in the layouts named by `want`, with the arguments, the dict of raw tensors and
    the bits of ops.conv2d_f16k_multi: x16 an F16K buffer [B][8][Hi*Wi][16], `packed` the slab stream of ops.pack_conv_f16k_weight for
    the layer."""
    _KERNEL.check(x16, packed, bias, B, Hi, Wi)
    if not want or set(want) - set(WANT):
        raise ValueError(f"{_WHO}: want names some of {WANT}, got {want!r}")
    C, (Ho, Wo), dev = OUT_CHANNELS, out_hw(Hi, Wi), x16.device
    out = {}
    if "y32" in want:
        out["y32"] = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev)
    if "round32" in want:
        out["round32"] = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev)
    if "round16" in want:
        if round16 is None:
            round16_ctot, round16_coff = C, 0
            round16 = torch.empty(B * C * Ho * Wo, dtype=torch.int16, device=dev)
        elif (round16.dtype != torch.int16 or round16.numel() != B * round16_ctot * Ho * Wo or round16.device != dev
              or not round16.is_contiguous()):
            raise RuntimeError(f"{_WHO}: round16 is not an F16K buffer of round16_ctot channels at the output size")
        out["round16"] = round16
    if "abs16" in want:
        out["abs16"] = torch.empty(B * C * Ho * Wo, dtype=torch.int16, device=dev)
    gate_ctot = 0
    if gate is not None:
        ops._dev(gate, "gate")
        if gate.shape[0] != B or tuple(gate.shape[2:]) != (Ho, Wo) or gate.device != dev:
            raise RuntimeError(f"{_WHO}: gate does not match the output")
        gate_ctot = gate.shape[1]
    _KERNEL.fwd(B, Hi, Wi, (), _p(x16), _p(packed), _p(bias), _p(out.get("y32")), _p(out.get("round32")), _p(out.get("round16")),
                _p(out.get("abs16")), _p(gate), B, Hi, Wi, round16_ctot, round16_coff, gate_ctot, gate_c)
    return out


def run(cv, x, want, round16=None, gate=None, gate_c=0):
    """The dict of cv.run_f16k_multi(x, want, round16, gate, gate_c) where supported(cv, x.B, x.H, x.W): float32 NCHW tensors under
    'y32' / 'round32', F16K values under 'round16' (`round16` itself when given) / 'abs16'; the pack is the one that call uses."""
    if not isinstance(x, F16K) or not x.whole or x.C != IN_CHANNELS or not supported(cv, x.B, x.H, x.W):
        raise RuntimeError(f"{_WHO}: run takes whole 128-channel tensors and the 128 -> 192 5x5 stride-2 layer, not {x!r} on {cv!r}")
    desc = cv._desc_of(x, nchw=True)
    r = (None, 0, 0) if round16 is None else (round16.buf, round16.ctot, round16.coff)
    if round16 is not None and round16.shape != (x.B, OUT_CHANNELS, desc.Ho, desc.Wo):
        raise RuntimeError(f"{_WHO}: {round16!r} is not the output of this layer on {x!r}")
    lay = launch(x.buf, cv.packed_f16k_weight(desc), cv._bias(), x.B, x.H, x.W, want=want, round16=r[0], round16_ctot=r[1], round16_coff=r[2],
                 gate=gate, gate_c=gate_c)
    for k in ("round16", "abs16"):
        if k in lay:
            lay[k] = round16 if (k == "round16" and round16 is not None) else F16K.wrap(lay[k], x.B, OUT_CHANNELS, desc.Ho, desc.Wo)
    return lay
