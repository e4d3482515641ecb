"""What the gradient with respect to h_matrix costs: a training-mode forward + rate_distortion + backward of HSIC(128,192,5) with and
without h_matrix.requires_grad, and the warp's matrix-gradient kernel alone against its compulsory traffic (source and incoming gradient
read once: 50 MB at 8 x 3 x 512 x 512).

Device events around `--steps` calls after `--warmup` calls; the median of five windows.  One JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)
import MASIC  # noqa: E402
from masic_amd import homography, nn as mnn, ops, synth  # noqa: E402
from masic_amd.loss import rate_distortion  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", default="bf16", choices=("f32", "bf16"))
    a = ap.parse_args()
    B, H, W = a.batch, a.size, a.size
    x1, x2, hm = (t.cuda() for t in synth.synth_inputs(B, H, W, seed=3))

    # ---- the kernel alone (both launches of ops.warp_perspective_bwd_matrix, then the chain's adjoint)
    g_dst = torch.randn_like(x1)
    minv, _ = homography.warp_matrices(hm, (H, W), (H, W), device=True)
    traffic = 2 * x1.numel() * 4
    for name, fn in (("warp_perspective_bwd_matrix", lambda: ops.warp_perspective_bwd_matrix(x1, minv, g_dst)),
                     ("warp_perspective_bwd_matrix+sum", lambda: ops.warp_perspective_bwd_matrix(x1, minv, g_dst, want_sum=True)),
                     ("warp_perspective_fwd (for scale)", lambda: ops.warp_perspective(x1, minv, (H, W)))):
        us = timed(fn, 20 * a.steps, a.warmup)
        print(json.dumps({"kernel": name, "shape": f"{B}x3x{H}x{W}", "us": round(us, 1), "compulsory_MB": traffic / 1e6,
                          "TBps": round(traffic / us / 1e6, 2), "compulsory_us_at_6.3TBps": round(traffic / 6.3e6, 1)}), flush=True)
    part, total = ops.warp_perspective_bwd_matrix(x1, minv, g_dst, want_sum=True)
    us = timed(lambda: ops.warp_matrix_bwd(hm, (H, W), (H, W), g_fwd=part), 20 * a.steps, a.warmup)
    print(json.dumps({"kernel": "warp_matrix_bwd", "slots": part.shape[1], "B": B, "us": round(us, 1)}), flush=True)
    us = timed(lambda: ops.warp_matrix_bwd(hm, (H, W), (H, W), g_fwd=total, g_inv=total), 20 * a.steps, a.warmup)
    print(json.dumps({"kernel": "warp_matrix_bwd", "slots": 1, "both_chains": True, "B": B, "us": round(us, 1)}), flush=True)

    # ---- the training step
    mnn.set_precision(a.precision)
    try:
        net = MASIC.HSIC(128, 192, 5)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=3))
        net = net.cuda().train()

        def step(h):
            for _, p in net.named_parameters():
                p.grad = None
            h.grad = None
            out = net(x1, x2, h)
            rate_distortion(out, x1, x2, 0.01)["loss"].backward()

        h_det, h_grad = hm.clone(), hm.clone().requires_grad_(True)
        t_det = timed(lambda: step(h_det), a.steps, a.warmup)
        t_grad = timed(lambda: step(h_grad), a.steps, a.warmup)
        t_det2 = timed(lambda: step(h_det), a.steps, a.warmup)
        print(json.dumps({"step": "forward + rate_distortion + backward", "model": "HSIC(128,192,5)", "shape": f"{B}x3x{H}x{W}", "precision": a.precision,
                          "h_matrix_detached_ms": round(t_det / 1e3, 3), "h_matrix_requires_grad_ms": round(t_grad / 1e3, 3),
                          "h_matrix_detached_again_ms": round(t_det2 / 1e3, 3), "extra_ms": round((t_grad - 0.5 * (t_det + t_det2)) / 1e3, 3),
                          "h_grad_finite": bool(torch.isfinite(h_grad.grad).all())}), flush=True)
    finally:
        mnn.set_precision("f32")


if __name__ == "__main__":
    main()
