"""TEST INFRASTRUCTURE of tests/test_cpu_hgrad.py and tests/test_gpu_hgrad.py: the named homographies, the sources, and the CPU
oracle's gradient with respect to the warp matrix (torch autograd through oracle.hsic_oracle.warp_perspective) in float32 and float64.

The bilinear sample is piecewise smooth in the sampling coordinate: on a cell boundary (an integer coordinate) its derivative is
one-sided, and two correct evaluations whose coordinates differ in the last bit may stand on different sides.  A comparison of matrix
gradients therefore means something only where the oracle agrees with itself -- the ADMISSION RULE:

    e32 = |g_float32 - g_float64| / |g_float64|   (Frobenius norms over the [B,3,3] gradient)   <=   ADMIT = 1e-4.

Identity and a 0.6 x minification about the centre put samples exactly on integer coordinates and are rejected (e32 of order 1);
the four ADMITTED kinds below pass with e32 between 1e-7 and 1e-5 at 48 x 64.
"""
import math

import numpy as np
import torch

from oracle import hsic_oracle as O

ADMIT = 1e-4
ADMITTED = ("rotate12", "magnify1.5", "projective", "translate")
REJECTED = ("identity", "minify0.6")


def _about_centre(a, hw):
    """pixel-space [[a, c], [0 0 1]] acting about the picture centre"""
    cx, cy = (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0
    t = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1]], dtype=np.float64)
    ti = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]], dtype=np.float64)
    m = np.eye(3)
    m[:2, :2] = a
    return t @ m @ ti


def matrix(kind, hw):
    """float32 [3,3] homography (destination <- source, pixel space) of a source of hw = (H, W)."""
    if kind == "rotate12":
        c, s = math.cos(math.radians(12.0)), math.sin(math.radians(12.0))
        m = _about_centre(np.array([[c, -s], [s, c]]), hw)
    elif kind == "magnify1.5":
        m = _about_centre(1.5 * np.eye(2), hw)
    elif kind == "minify0.6":
        m = _about_centre(0.6 * np.eye(2), hw)
    elif kind == "projective":
        m = np.array([[1.02, 0.03, -4.3], [-0.02, 0.97, 2.6], [1.5e-4, -8e-5, 1.0]])
    elif kind == "translate":
        m = np.array([[1.0, 0.0, -7.37], [0.0, 1.0, 1.61], [0.0, 0.0, 1.0]])
    elif kind == "identity":
        m = np.eye(3)
    else:
        raise KeyError(kind)
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))


def matrices(kinds, hw):
    return torch.stack([matrix(k, hw) for k in kinds])


def sources(B, C, hw, seed):
    """float32 [B,C,H,W]: even items smooth (three plane waves per channel), odd items white noise."""
    rng = np.random.default_rng(seed)
    H, W = hw
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, C, H, W))
    for b in range(B):
        for c in range(C):
            if b % 2:
                out[b, c] = rng.standard_normal((H, W))
            else:
                img = np.zeros((H, W))
                for _ in range(3):
                    fx, fy = rng.uniform(0.05, 0.4, 2)
                    img += rng.uniform(0.3, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 6.28))
                out[b, c] = img
    return torch.from_numpy(out.astype(np.float32))


def incoming(B, C, hw, seed):
    """float32 [B,C,h,w] gradient arriving at the warp's output"""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, C) + tuple(hw)).astype(np.float32))


def oracle_grad(src, M, g_dst, dtype, align_corners=True):
    """d <warp(src, M), g_dst> / d M by torch autograd through the oracle warp, computed in `dtype` from the float32 inputs."""
    m = M.detach().to(dtype).clone().requires_grad_(True)
    out = O.warp_perspective(src.to(dtype), m, tuple(g_dst.shape[-2:]), align_corners=align_corners)
    (out * g_dst.to(dtype)).sum().backward()
    return m.grad.detach()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def admission(src, M, g_dst, align_corners=True):
    """(e32, g_float64) of one case"""
    g64 = oracle_grad(src, M, g_dst, torch.float64, align_corners)
    g32 = oracle_grad(src, M, g_dst, torch.float32, align_corners)
    return rel(g32, g64), g64


class Case:
    """One operator-level case: sources, matrices, incoming gradient; the oracle's answer is computed once and shared."""

    def __init__(self, name, kind, B, C, src_hw, dst_hw, align_corners=True, ones=False, seed=0):
        self.name, self.kind, self.align_corners, self.ones = name, kind, align_corners, ones
        self.src_hw, self.dst_hw = tuple(src_hw), tuple(dst_hw)
        self.src = torch.ones((B, 1) + self.src_hw) if ones else sources(B, C, self.src_hw, seed)
        self.M = matrices([kind] * B, self.src_hw)
        self.g_dst = incoming(B, 1 if ones else C, self.dst_hw, seed + 1)
        self._adm = None

    def admission(self):
        if self._adm is None:
            self._adm = admission(self.src, self.M, self.g_dst, self.align_corners)
        return self._adm


def operator_cases():
    """Issue list: the four admitted matrices at B=2, C=5, 48 x 64 -> 48 x 64 and -> 32 x 40; B=3, C=1, 17 x 23 (a ragged last
    workgroup); one case with align_corners=False."""
    cases = []
    for i, kind in enumerate(ADMITTED):
        cases.append(Case(f"{kind}-same", kind, 2, 5, (48, 64), (48, 64), seed=100 + 10 * i))
        cases.append(Case(f"{kind}-smaller", kind, 2, 5, (48, 64), (32, 40), seed=105 + 10 * i))
    cases.append(Case("ragged-17x23", "projective", 3, 1, (17, 23), (17, 23), seed=150))
    cases.append(Case("no-align-corners", "rotate12", 2, 5, (48, 64), (48, 64), align_corners=False, seed=160))
    return cases


def ones_cases():
    return [Case(f"ones-{kind}", kind, 2, 1, (48, 64), (48, 64), ones=True, seed=200 + 10 * i) for i, kind in enumerate(ADMITTED)]


def rejected_cases():
    return [Case(f"{kind}", kind, 2, 3, (48, 64), (48, 64), seed=300 + 10 * i) for i, kind in enumerate(REJECTED)]


def model_h_matrices(hw):
    """The model-level test's homographies, one admitted kind per item of a B=2 batch"""
    return matrices(["projective", "translate"], hw)
