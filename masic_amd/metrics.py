"""Per-pair reductions of the test-split evaluation (masic_amd/csrc/metrics.hip).

    metrics.pair_rd(x1_hat, x1, x2_hat, x2, liks)   float64 [B,6]: per image, sum (x1_hat - x1)^2, sum (x2_hat - x2)^2 and
                                                    sum log of up to four likelihood tensors (0 for the absent ones)
    metrics.u8_sse(a, b)                            int64 [P]: per picture, the exact sum of squared byte differences

ops.sse / ops.sum_log / loss.rate_distortion return one value per batch; an evaluation averages per-pair values.  Row b of pair_rd is,
bit for bit, what ops.sse / ops.sum_log return for image b's slice alone, so a batched evaluation has the numbers of one pair at a time
by construction.  Both calls are two launches on torch's current stream, without atomics and without a wait for the device.

The entry points are declared in include/masic_metrics.h, a side header of libmasic_hip.so bound by _lib.bind_header.  No CPU path.
"""
import ctypes
import math

import torch

from . import _lib

HEADER_PATH = _lib.header_path("masic_metrics.h")
MAX_LIKS = 4
MAX_IMAGES = 65535                # the image is a grid dimension of the kernels

SIGNATURES = _lib.bind_header(HEADER_PATH, "masic_metrics_")          # name -> (restype, argtypes) of every prototype of masic_metrics.h


def _dev(t, name, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"masic_amd.metrics: {name} must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"masic_amd.metrics: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"masic_amd.metrics: {name} must be contiguous")
    return t


def pair_rd(x1_hat, x1, x2_hat, x2, liks=()):
    """float64 [B,6] device tensor (masic_metrics_pair_rd).  The pictures: contiguous float32 [B, ...] of one shape; liks: up to four
    contiguous float32 [B, ...] tensors.  Row b, columns 0 / 1: ops.sse of image b's slices; columns 2 + k: ops.sum_log of liks[k][b];
    the columns of absent likelihood tensors hold 0."""
    from . import ops
    liks = list(liks)
    for name, t in (("x1_hat", x1_hat), ("x1", x1), ("x2_hat", x2_hat), ("x2", x2), *((f"liks[{k}]", l) for k, l in enumerate(liks))):
        _dev(t, name, torch.float32)
    if not (x1_hat.shape == x1.shape == x2_hat.shape == x2.shape) or x1.dim() < 1:
        raise RuntimeError("masic_amd.metrics.pair_rd: the four pictures must have one shape [B, ...]")
    if len(liks) > MAX_LIKS:
        raise RuntimeError(f"masic_amd.metrics.pair_rd: at most {MAX_LIKS} likelihood tensors, got {len(liks)}")
    B = int(x1.shape[0])
    if not 1 <= B <= MAX_IMAGES:
        raise RuntimeError(f"masic_amd.metrics.pair_rd: B = {B} outside 1 .. {MAX_IMAGES}")
    for k, l in enumerate(liks):
        if l.dim() < 1 or l.shape[0] != B:
            raise RuntimeError(f"masic_amd.metrics.pair_rd: liks[{k}] is {tuple(l.shape)}, the pictures hold {B} images")
    dev = x1.device
    out = torch.empty((B, 6), dtype=torch.float64, device=dev)
    ws = ops._cached_ws("metrics_pair_rd", dev, _lib.lib.masic_metrics_pair_rd_workspace_bytes(B))
    n = max(len(liks), 1)
    arr = (ctypes.c_void_p * n)(*[l.data_ptr() for l in liks])
    cnt = (ctypes.c_size_t * n)(*[l.numel() // B for l in liks])
    _lib.check(_lib.lib.masic_metrics_pair_rd(ops._p(x1_hat), ops._p(x1), ops._p(x2_hat), ops._p(x2), x1.numel() // B, arr, cnt, len(liks),
                                              B, ops._p(out), ops._p(ws), ops._stream()), "metrics_pair_rd")
    return out


def pair_objective(rows, lmbda, hw, n_pic):
    """float64 [B]: J_b = bits_b / hw + lmbda 255^2 (MSE1_b + MSE2_b) from pair_rd's rows -- bits_b = -sum of the four log columns
    / ln 2, MSE_b = squared error / n_pic (n_pic = 3 hw for RGB pictures).  The rate-distortion objective of ONE pair: nothing is
    averaged over the batch.  A few float64 torch operations on [B]-sized tensors, on the device."""
    bits = rows[:, 2:].sum(dim=1) * (-1.0 / math.log(2.0))
    return bits / float(hw) + (float(lmbda) * 255.0 ** 2 / float(n_pic)) * (rows[:, 0] + rows[:, 1])


def u8_sse(a, b):
    """int64 [P] device tensor (masic_metrics_u8_sse): sum (a[p] - b[p])^2 over the bytes of picture p.  a, b: contiguous uint8
    [P, ...] of one shape (a single picture [H,W,3] is passed as pic[None]).  Exact; a picture of 2^49 bytes would be needed to pass
    int64."""
    from . import ops
    _dev(a, "a", torch.uint8); _dev(b, "b", torch.uint8)
    if a.shape != b.shape or a.dim() < 2:
        raise RuntimeError(f"masic_amd.metrics.u8_sse: a is {tuple(a.shape)}, b is {tuple(b.shape)}: two stacks [P, ...] of one shape")
    P = int(a.shape[0])
    if not 1 <= P <= MAX_IMAGES or a.numel() == 0:
        raise RuntimeError(f"masic_amd.metrics.u8_sse: {P} pictures of {a.numel() // max(P, 1)} bytes: 1 .. {MAX_IMAGES} non-empty pictures")
    out = torch.empty(P, dtype=torch.int64, device=a.device)
    ws = ops._cached_ws("metrics_u8_sse", a.device, _lib.lib.masic_metrics_u8_sse_workspace_bytes(P))
    _lib.check(_lib.lib.masic_metrics_u8_sse(ops._p(a), ops._p(b), a.numel() // P, P, ops._p(out), ops._p(ws), ops._stream()), "metrics_u8_sse")
    return out
