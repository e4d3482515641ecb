"""Times the LPIPS forward (AlexNet trunk) on the HIP path, launch by launch, beside the same op sequence as float32 torch ops on the
same GPU.

For each shape: every stage of `lpips.LPIPS.forward` on its own (the first layer with the scaling folded in, the two max-pools,
layers 2-5, the five distance launches + the finishing launch) and the whole forward; for torch the same stages on the same
[2N, ...] tensors (scaling ops + F.conv2d + relu, F.max_pool2d, F.conv2d + relu, normalise / square / 1x1 convolution / mean), and
the whole sequence.  Device events around `--steps` calls after `--warmup` calls; the median of five windows; microseconds.
Weights are torch's default initialisation (`pnet_rand=True`, `pretrained=False`): no trained weights ship with the repository, and
the times do not depend on them.  `--only hip|torch` runs one side (for a kernel trace of it).

Then the loss: forward + backward (`net(y, x).sum().backward()`) with only `x` requiring grad (the training case, a chain of N images)
and with both pictures requiring grad (2N images), beside torch autograd through the same float32 restatement run as lpips runs it
(the trunk once per picture tensor, so autograd prunes the side that needs no gradient); and the 12 launches of the backward schedule
one by one for both chains."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lpips  # noqa: E402
from masic_amd import lpips as L  # noqa: E402
from masic_amd import ops  # noqa: E402

STAGES = ("conv1 3->64 k11 s4 (+scaling)", "maxpool 3/2 (64 ch)", "conv2 64->192 k5", "maxpool 3/2 (192 ch)", "conv3 192->384 k3",
          "conv4 384->256 k3", "conv5 256->256 k3", "distance x5 + finish", "whole forward")


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


def torch_normalize(f):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)


def torch_distance(taps, lins):
    val = 0
    for f, w in zip(taps, lins):
        d = (torch_normalize(f[0::2]) - torch_normalize(f[1::2])) ** 2
        val = val + F.conv2d(d, w).mean([2, 3], keepdim=True)
    return val


def backward_rows(a, net, convs, lins, y, x, taps, row, torch_taps, conv1_flop):
    """Forward + backward of the loss for both chains beside torch autograd, then the backward schedule launch by launch."""
    sl, N = net.scaling_layer, y.shape[0]

    def hip_loss(need0):
        yy, xx = y.detach().requires_grad_(need0), x.detach().requires_grad_(True)
        net(yy, xx).sum().backward()
        return yy.grad, xx.grad

    def torch_loss(need0):
        yy, xx = y.detach().requires_grad_(need0), x.detach().requires_grad_(True)
        with torch.set_grad_enabled(need0):
            t0 = torch_taps(yy)
        t1, val = torch_taps(xx), 0
        for f0, f1, w in zip(t0, t1, lins):
            val = val + F.conv2d((torch_normalize(f0) - torch_normalize(f1)) ** 2, w).mean([2, 3], keepdim=True)
        val.sum().backward()
        return yy.grad, xx.grad

    print(f"{'forward + backward':<34}{'hip us':>10}{'torch us':>10}{'torch/hip':>10}")
    for name, need0 in (("fwd + bwd, x requires grad", False), ("fwd + bwd, both require grad", True)):
        th = timed(lambda: hip_loss(need0), a.steps, a.warmup) if a.only in (None, "hip") else None
        tt = timed(lambda: torch_loss(need0), a.steps, a.warmup) if a.only in (None, "torch") else None
        row[name] = {"hip_us": th and round(th, 1), "torch_us": tt and round(tt, 1)}
        ratio = f"{tt / th:10.2f}" if th and tt else f"{'':>10}"
        print(f"{name:<34}{(f'{th:10.1f}' if th else f'{chr(45):>10}')}{(f'{tt:10.1f}' if tt else f'{chr(45):>10}')}{ratio}", flush=True)
        if a.only is None:
            gh, gt = hip_loss(need0)[1], torch_loss(need0)[1]
            row[name]["hip_vs_torch_relative"] = float((gh - gt).abs().max() / gt.abs().max())
    if a.only == "torch":
        return
    gout = torch.full((6, N), 0.5, device="cuda")
    packedb = ops.pack_lpips_conv1_bwd_weight(convs[0].weight.detach())
    H, W = y.shape[2:]
    cols = {}
    for sides in (2, 3):
        unit, stride, off = (2, 1, 0) if sides == 3 else (1, 2, sides - 1)
        stages, g = [], None
        for t in range(4, -1, -1):
            fn = lambda t=t, gin=g: ops.lpips_dist_bwd(taps[t], lins[t], gout, t, sides, g_in=gin)      # noqa: E731
            g = fn()
            stages.append((f"distance bwd tap {t} ({row['taps'][t]})", fn))
            if t:
                fn = lambda t=t, gi=g: L._conv_dgrad(convs[t], gi, unit)                                  # noqa: E731
                g = fn()
                stages.append((f"conv{t + 1} input gradient", fn))
                if t in (1, 2):
                    fn = lambda t=t, gi=g: ops.maxpool3s2_bwd(taps[t - 1], gi, stride, off)               # noqa: E731
                    g = fn()
                    stages.append((f"maxpool bwd ({taps[t - 1].shape[1]} ch)", fn))
        stages.append(("conv1 input gradient (+scaling)", lambda gi=g: ops.lpips_conv1_bwd(gi, packedb, sl.scale, H, W, False, sides)))
        cols[sides] = [(name, timed(fn, a.steps, a.warmup)) for name, fn in stages]
    print(f"{'backward launch':<38}{'N images us':>12}{'2N images us':>13}")
    for (name, one), (_, two) in zip(cols[2], cols[3]):
        row["bwd " + name] = {"one_sided_us": round(one, 1), "two_sided_us": round(two, 1)}
        print(f"{'  ' + name:<38}{one:12.1f}{two:13.1f}", flush=True)
    print(f"{'  sum':<38}{sum(v for _, v in cols[2]):12.1f}{sum(v for _, v in cols[3]):13.1f}")
    row["conv1_bwd_TFLOPs_useful"] = round(conv1_flop / cols[3][-1][1] / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--shape", action="append", default=None, help="NxCxHxW (repeatable); default 8x3x512x512 and 1x3x1216x2176")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.shape or ["8x3x512x512", "1x3x1216x2176"])]
    torch.manual_seed(0)
    net = lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False).cuda()
    convs = [net.net.conv(s) for s in range(1, 6)]
    lins = [net.lins[i].weight.detach() for i in range(5)]
    sl = net.scaling_layer
    for shape in shapes:
        gen = torch.Generator().manual_seed(0)
        y = torch.rand(shape, generator=gen)
        x = (y + 0.05 * torch.randn(shape, generator=gen)).clamp(0, 1)
        x, y = x.cuda(), y.cuda()
        both = torch.stack([y, x], 1).flatten(0, 1).contiguous()          # images 2n, 2n + 1 as the HIP path orders them
        with torch.no_grad():
            taps = net.features(y, x)
            pools = [ops.maxpool3s2(taps[0]), ops.maxpool3s2(taps[1])]
            packed1 = ops.pack_lpips_conv1_weight(convs[0].weight.detach())

            def tconv(i, t):
                c = convs[i]
                return F.relu(F.conv2d(t, c.weight, c.bias, stride=c.stride, padding=c.padding))

            def torch_taps(pictures):
                t, out = (pictures - sl.shift) / sl.scale, []
                for i in range(5):
                    if i in (1, 2):
                        t = F.max_pool2d(t, 3, 2)
                    t = tconv(i, t)
                    out.append(t)
                return out

            def torch_forward():
                return torch_distance(torch_taps(both), lins)

            hip = (lambda: ops.lpips_conv1(y, x, packed1, convs[0].bias.detach(), sl.shift, sl.scale, False),
                   lambda: ops.maxpool3s2(taps[0]), lambda: L._conv_relu(convs[1], pools[0]),
                   lambda: ops.maxpool3s2(taps[1]), lambda: L._conv_relu(convs[2], pools[1]),
                   lambda: L._conv_relu(convs[3], taps[2]), lambda: L._conv_relu(convs[4], taps[3]),
                   lambda: ops.lpips_distance(taps, lins), lambda: net(y, x))
            tor = (lambda: tconv(0, (both - sl.shift) / sl.scale),
                   lambda: F.max_pool2d(taps[0], 3, 2), lambda: tconv(1, pools[0]),
                   lambda: F.max_pool2d(taps[1], 3, 2), lambda: tconv(2, pools[1]),
                   lambda: tconv(3, taps[2]), lambda: tconv(4, taps[3]),
                   lambda: torch_distance(taps, lins), torch_forward)
            row = {"shape": "x".join(map(str, shape)), "taps": ["x".join(map(str, t.shape[1:])) for t in taps]}
            print(f"## {row['shape']}: taps {row['taps']} (batch of {2 * shape[0]} images)")
            print(f"{'stage':<34}{'hip us':>10}{'torch us':>10}{'torch/hip':>10}")
            for name, fh, ft in zip(STAGES, hip, tor):
                th = timed(fh, a.steps, a.warmup) if a.only in (None, "hip") else None
                tt = timed(ft, a.steps, a.warmup) if a.only in (None, "torch") else None
                row[name] = {"hip_us": th and round(th, 1), "torch_us": tt and round(tt, 1)}
                ratio = f"{tt / th:10.2f}" if th and tt else f"{'':>10}"
                print(f"{name:<34}{(f'{th:10.1f}' if th else f'{chr(45):>10}')}{(f'{tt:10.1f}' if tt else f'{chr(45):>10}')}{ratio}", flush=True)
            if a.only in (None, "hip"):          # the six launches of the distance stage one by one (straight through the C ABI)
                import ctypes
                from masic_amd._lib import lib
                N = shape[0]
                hw = [t.shape[2] * t.shape[3] for t in taps]
                nch = [lib.masic_lpips_dist_chunks(m) for m in hw]
                part = torch.zeros(N * sum(nch), dtype=torch.float64, device="cuda")
                out = torch.empty((6, N), dtype=torch.float32, device="cuda")
                for i, (t, w) in enumerate(zip(taps, lins)):
                    us = timed(lambda: lib.masic_lpips_dist_fwd(ops._p(t), ops._p(w), ops._p(part), N, t.shape[1], hw[i], ops._stream()),
                               a.steps, a.warmup)
                    row[f"distance tap {i}"] = {"hip_us": round(us, 1)}
                    print(f"{'  distance tap ' + str(i) + ' (' + row['taps'][i] + ')':<34}{us:10.1f}")
                us = timed(lambda: lib.masic_lpips_finish(ops._p(part), (ctypes.c_int * 5)(*nch), (ctypes.c_int * 5)(*hw), N, ops._p(out),
                                                          ops._stream()), a.steps, a.warmup)
                row["finish"] = {"hip_us": round(us, 1)}
                print(f"{'  finish':<34}{us:10.1f}")
            if a.only is None:
                v, r = net(y, x), torch_forward()
                row["hip_vs_torch_relative"] = float(((v - r).abs() / r.abs()).max())
            conv1_flop = 2.0 * 2 * shape[0] * 64 * 363 * taps[0].shape[2] * taps[0].shape[3]
            if a.only in (None, "hip"):
                row["conv1_TFLOPs_useful"] = round(conv1_flop / row[STAGES[0]]["hip_us"] / 1e6, 1)
        backward_rows(a, net, convs, lins, y, x, taps, row, torch_taps, conv1_flop)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
