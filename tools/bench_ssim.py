"""Times MS-SSIM on the HIP path against the same op sequence as float32 torch ops (F.conv2d groups, F.avg_pool2d) on the same GPU.

For each shape: ms_ssim forward, forward + backward of (1 - ms_ssim).sum() (gradient for X), and both for the torch-op sequence;
device events around `--steps` calls after `--warmup` calls; the median of five windows.  Compulsory traffic: X and Y read once, the
pooled levels written and read once (forward); the backward adds X, Y and the pyramid read again, dX written, and the gradient
pyramid written and read.  `--only hip|torch` runs one side (for a kernel trace of it)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from masic_amd import ssim as S  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_ms_ssim(X, Y, data_range=1.0):
    """0.2.1's op sequence in float32 torch ops."""
    C = X.shape[1]
    g = torch.tensor(S.gaussian_taps(11, 1.5), dtype=torch.float32, device=X.device)
    wh, ww = g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), g.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    w = torch.tensor(WEIGHTS, dtype=torch.float32, device=X.device)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def G(x):
        return F.conv2d(F.conv2d(x, wh, groups=C), ww, groups=C)

    mcs = []
    for i in range(len(WEIGHTS)):
        mu1, mu2 = G(X), G(Y)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1, s2, s12 = G(X * X) - mu1_sq, G(Y * Y) - mu2_sq, G(X * Y) - mu1_mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
        ssim_pc, cs = torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)
        if i < len(WEIGHTS) - 1:
            mcs.append(torch.relu(cs))
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    v = torch.prod(torch.stack(mcs + [torch.relu(ssim_pc)], 0) ** w.view(-1, 1, 1), 0)
    return v.mean()


def compulsory_bytes(N, C, H, W, levels=5):
    P, pyr = N * C, 0
    h, w = H, W
    for _ in range(levels - 1):
        h, w = (h + 1) // 2, (w + 1) // 2
        pyr += P * h * w
    fwd = 4 * (2 * P * H * W + 2 * 2 * pyr)
    bwd = 4 * (2 * P * H * W + 2 * pyr + P * H * W + 2 * pyr)
    return fwd, fwd + bwd


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / steps)
    return sorted(res)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--shape", action="append", default=None, help="NxCxHxW (repeatable); default 8x3x512x512 and 1x3x1216x2176")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.shape or ["8x3x512x512", "1x3x1216x2176"])]
    for shape in shapes:
        gen = torch.Generator().manual_seed(0)
        Y = torch.rand(shape, generator=gen)
        X = (Y + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1)
        X, Y = X.cuda(), Y.cuda()
        Xg = X.clone().requires_grad_(True)
        fb_bytes = compulsory_bytes(*shape)
        row = {"shape": "x".join(map(str, shape)), "compulsory_MB": {"fwd": fb_bytes[0] / 1e6, "fwd_bwd": fb_bytes[1] / 1e6}}

        def hip_f():
            with torch.no_grad():
                return S.ms_ssim(X, Y, data_range=1)

        def hip_fb():
            (1 - S.ms_ssim(Xg, Y, data_range=1)).sum().backward()

        def torch_f():
            with torch.no_grad():
                return torch_ms_ssim(X, Y)

        def torch_fb():
            (1 - torch_ms_ssim(Xg, Y)).sum().backward()

        runs = {}
        if a.only in (None, "hip"):
            runs.update(hip_fwd_us=hip_f, hip_fwd_bwd_us=hip_fb)
        if a.only in (None, "torch"):
            runs.update(torch_fwd_us=torch_f, torch_fwd_bwd_us=torch_fb)
        for k, fn in runs.items():
            row[k] = round(timed(fn, a.steps, a.warmup), 1)
        if "hip_fwd_us" in row:
            row["hip_fwd_TBps"] = round(fb_bytes[0] / row["hip_fwd_us"] / 1e6, 2)
            row["hip_fwd_bwd_TBps"] = round(fb_bytes[1] / row["hip_fwd_bwd_us"] / 1e6, 2)
            row["compulsory_fwd_us_at_6.3TBps"] = round(fb_bytes[0] / 6.3e6, 1)
        if "hip_fwd_us" in row and "torch_fwd_us" in row:
            row["speedup_fwd"] = round(row["torch_fwd_us"] / row["hip_fwd_us"], 1)
            row["speedup_fwd_bwd"] = round(row["torch_fwd_bwd_us"] / row["hip_fwd_bwd_us"], 1)
        if a.only is None:
            with torch.no_grad():
                row["hip_minus_torch"] = float(S.ms_ssim(X, Y, data_range=1) - torch_ms_ssim(X, Y))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
