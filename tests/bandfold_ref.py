"""What the tests of the band-aware entropy model share (tests/test_cpu_bandfold.py, tests/test_gpu_bandfold.py): numpy references of
the fold / unfold kernels (masic_amd/csrc/band_fold.hip) with the float32 gate product and the one rounding to bf16 of the F16K
destination, the per-band reference of the banded masked convolution, the chain of torch operations HSIC._context_bands was before the
kernels, and the oracle's forward with its two context models applied band by band.  Nothing here needs a GPU."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import bands_ref as R

# (B, C, h, w, S) of the kernel tests
CASES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 2), (2, 16, 8, 12, 3), (1, 19, 4, 4, 4), (2, 32, 16, 24, 5), (2, 16, 6, 5, 1)]
# more lanes than the capped grid holds (1024 workgroups of 256 lanes), on the 16-byte and on the single-float path
PAST_CAP_CASES = [(4, 96, 56, 52, 8), (2, 64, 45, 47, 7)]
GRID_CAP_LANES = 1024 * 256


def rand(shape, seed, scale=3.0):
    return (np.random.RandomState(seed).standard_normal(size=shape) * scale).astype(np.float32)


def n_bands(h, S):
    return -(-h // S)


def fold(x, S):
    """[B, C, h, w] -> [B T, C, S, w]; the rows a short last band lacks are +0.0"""
    B, C, h, w = x.shape
    T = n_bands(h, S)
    out = np.zeros((B * T, C, S, w), dtype=x.dtype)
    for b in range(B):
        for t in range(T):
            rows = min(S, h - t * S)
            out[b * T + t, :, :rows] = x[b, :, t * S:t * S + rows]
    return out


def unfold(xb, B, h, S):
    """[B T, C, S, w] -> [B, C, h, w]: the inverse index map, padding rows dropped"""
    BT, C, S_, w = xb.shape
    T = n_bands(h, S)
    assert S_ == S and BT == B * T
    out = np.empty((B, C, h, w), dtype=xb.dtype)
    for b in range(B):
        for t in range(T):
            rows = min(S, h - t * S)
            out[b, :, t * S:t * S + rows] = xb[b * T + t, :, :rows]
    return out


def gated(x, gate, gate_c):
    """x * gate[:, gate_c] as one float32 multiplication (gate None: x)"""
    return x if gate is None else (x.astype(np.float32) * gate[:, gate_c:gate_c + 1].astype(np.float32)).astype(np.float32)


def bf16_bits(x):
    """float32 -> the 16 bits of bf16(x), round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def f16k_records(bits, ctot):
    """uint16 [B, C, h, w] (C <= ctot) -> uint16 [B, ctot / 16, h w, 16]: the F16K records of the channels, the missing ones zero"""
    B, C, h, w = bits.shape
    full = np.zeros((B, ctot, h * w), dtype=np.uint16)
    full[:, :C] = bits.reshape(B, C, h * w)
    return np.ascontiguousarray(full.reshape(B, ctot // 16, 16, h * w).transpose(0, 1, 3, 2))


def banded_conv_reference(x, weff, bias, S):
    """The banded masked convolution on the CPU, differentiable: F.conv2d (5x5, padding 2) of every band of x as an image of its own,
    concatenated along the rows.  weff: the masked weight (oracle.hsic_oracle.masked_weight)."""
    return torch.cat([F.conv2d(x[:, :, r0:r1], weff, bias, padding=2) for r0, r1 in R.bands(x.shape[2], S)], dim=2)


def context_bands_torch_chain(net, ctx, y, out, out_coff, gate, gate_c, S):
    """HSIC._context_bands as it was before the fold / unfold kernels: pad / view / permute / contiguous around the same call of
    net._context, the gate as a torch product, fill_from_nchw or a slice assignment for the destination."""
    from masic_amd.f16k import F16K
    B, M, h, w = y.shape
    T = -(-h // S)
    yb = F.pad(y, (0, 0, 0, T * S - h)).view(B, M, T, S, w).permute(0, 2, 1, 3, 4).reshape(B * T, M, S, w).contiguous()
    cb = net._context(ctx, yb, None)
    C = cb.shape[1]
    c = cb.view(B, T, C, S, w).permute(0, 2, 1, 3, 4).reshape(B, C, T * S, w)[:, :, :h]
    if gate is not None:
        c = c * gate[:, gate_c:gate_c + 1]
    if isinstance(out, F16K):
        return out.fill_from_nchw(c.contiguous())
    if out is None:
        return c.contiguous()
    out[:, out_coff:out_coff + C] = c
    return out


class _BandedFunctional:
    """torch.nn.functional for the oracle, with conv2d applied band by band when its weight is one the oracle's masked_weight made: the
    oracle's two context models, each band an image of its own."""

    def __init__(self, S, masked):
        self._S, self._masked = S, masked

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, weight, *args, **kwargs):
        if not any(weight is m for m in self._masked):
            return F.conv2d(x, weight, *args, **kwargs)
        return torch.cat([F.conv2d(x[:, :, r0:r1], weight, *args, **kwargs) for r0, r1 in R.bands(x.shape[2], self._S)], dim=2)


@contextlib.contextmanager
def oracle_with_bands(O, S):
    """Inside: oracle.hsic_oracle's forward evaluates its two context models on bands of S rows (the module's files stay as they are:
    its names `F` and `masked_weight` are wrapped here and put back)."""
    masked = []
    orig_mw, orig_F = O.masked_weight, O.F

    def masked_weight(w):
        m = orig_mw(w)
        masked.append(m)
        return m

    O.masked_weight, O.F = masked_weight, _BandedFunctional(S, masked)
    try:
        yield
    finally:
        O.masked_weight, O.F = orig_mw, orig_F
