"""The row bands of a latent as a batch of images, and back: masic_amd/csrc/band_fold.hip (DESIGN.md section 8.1 "Row bands in the model").

    fold(x, S)                                  float32 [B, C, h, w] -> [B T, C, S, w], T = ceil(h / S); missing rows of a short last band +0.0
    unfold(xb, B, h, S, out=, out_coff=, gate=, gate_c=)
                                                the inverse map, padding rows dropped, optionally * gate[:, gate_c]: a fresh float32 tensor,
                                                channels [out_coff, ..) of a float32 NCHW `out`, or an F16K view `out`

One launch each, no allocation below this file, capturable.  Fold and the ungated float32 unfold are each other's adjoint
(autograd.BandFoldFn / BandUnfoldFn).  The entry points are declared in include/masic_bandfold.h, a side header of libmasic_hip.so bound
by _lib.bind_header.  No CPU path.
"""
import torch

from . import _lib
from .ops import _p, _stream

HEADER_PATH = _lib.header_path("masic_bandfold.h")

SIGNATURES = _lib.bind_header(HEADER_PATH, "masic_bandfold_")       # name -> (restype, argtypes) of every prototype of masic_bandfold.h


def _f32(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise ValueError(f"masic_amd.bandfold: {what} must be a contiguous float32 [B, C, h, w] device tensor")
    return t


def bands_of(h, S):
    """T = ceil(h / S)"""
    return -(-int(h) // int(S))


def max_blocks():
    """The grid cap of the float32 kernels, in workgroups of 256 lanes."""
    return int(_lib.lib.masic_bandfold_max_blocks())


def fold(x, S):
    """[B, C, h, w] -> [B T, C, S, w] (masic_bandfold_fold)."""
    B, C, h, w = _f32(x, "x").shape
    S = int(S)
    if S < 1:
        raise ValueError(f"masic_amd.bandfold.fold: band_rows = {S} must be at least 1")
    out = torch.empty((B * bands_of(h, S), C, S, w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.masic_bandfold_fold(_p(x), _p(out), B, C, h, w, S, _stream()), "bandfold_fold")
    return out


def unfold(xb, B, h, S, out=None, out_coff=0, gate=None, gate_c=0):
    """[B T, C, S, w] -> [B, C, h, w] (masic_bandfold_unfold / _unfold_f16k).  out: None (a fresh float32 tensor, returned), a float32
    NCHW buffer written at channels [out_coff, out_coff + C), or an F16K view of C channels; returns `out` then."""
    from .f16k import F16K
    BT, C, S_, w = _f32(xb, "xb").shape
    B, h, S = int(B), int(h), int(S)
    if S < 1 or S_ != S or h < 1 or BT != B * bands_of(h, S):
        raise ValueError(f"masic_amd.bandfold.unfold: {tuple(xb.shape)} is not [B T, C, S, w] of B = {B}, h = {h}, band_rows = {S}")
    gate_ctot = 0
    if gate is not None:
        gb, _, gh, gw = _f32(gate, "gate").shape
        if (gb, gh, gw) != (B, h, w) or gate.device != xb.device:
            raise ValueError(f"masic_amd.bandfold.unfold: a gate of {tuple(gate.shape)} does not match [{B}, *, {h}, {w}]")
        gate_ctot = gate.shape[1]
    if isinstance(out, F16K):
        if out.shape != (B, C, h, w) or out.buf.device != xb.device:
            raise ValueError(f"masic_amd.bandfold.unfold: {out!r} does not take [{B}, {C}, {h}, {w}]")
        _lib.check(_lib.lib.masic_bandfold_unfold_f16k(_p(xb), _p(out.buf), B, C, h, w, S, out.ctot, out.coff, _p(gate), gate_ctot, int(gate_c),
                                                       _stream()), "bandfold_unfold_f16k")
        return out
    if out is None:
        out, out_coff = torch.empty((B, C, h, w), dtype=torch.float32, device=xb.device), 0
    elif (_f32(out, "out").shape[0],) + tuple(out.shape[2:]) != (B, h, w) or out.device != xb.device:
        raise ValueError(f"masic_amd.bandfold.unfold: a destination of {tuple(out.shape)} does not match [{B}, *, {h}, {w}]")
    _lib.check(_lib.lib.masic_bandfold_unfold(_p(xb), _p(out), B, C, h, w, S, out.shape[1], int(out_coff), _p(gate), gate_ctot, int(gate_c),
                                              _stream()), "bandfold_unfold")
    return out
