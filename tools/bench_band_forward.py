#!/usr/bin/env python3
"""What HSIC.band_rows costs in time: the eval forward and the training step with the banded context models (run on the GPU box).

    python tools/bench_band_forward.py [--batch 8 --size 512 --band-rows 0,16,8 --iters 30 --warmup 5]

HSIC(128,192,5) with synthetic weights and bf16 operands.  Per band_rows: the median device time of the eager eval forward (under
no_grad) and of train.train_step, and the fold / unfold launches one call of each makes (counted at masic_amd.bandfold; 0 at
band_rows = 0: nothing new is launched there).  The convolution itself runs on [B T, M, S, w] instead of [B, M, h, w]: the same pixels
when S divides h."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--band-rows", default="0,16,8")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import MASIC
    from masic_amd import bandfold, nn as mnn, synth, train
    dev = torch.device("cuda", 0)
    x1, x2, hm = (t.to(dev) for t in synth.synth_inputs(args.batch, args.size, args.size, seed=100))
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=100))
    net = net.to(dev)
    net.update()
    opt, aopt = train.make_optimizers(net)
    calls = {"fold": 0, "unfold": 0}
    fold, unfold = bandfold.fold, bandfold.unfold

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    bandfold.fold, bandfold.unfold = counted("fold", fold), counted("unfold", unfold)

    def launches(fn):
        calls["fold"] = calls["unfold"] = 0
        fn()
        return calls["fold"], calls["unfold"]

    def forward():
        with torch.no_grad():
            net(x1, x2, hm)

    def step():
        train.train_step(net, opt, aopt, x1, x2, hm, 0.01)

    mnn.set_precision("bf16")
    try:
        print(f"| band_rows | eval forward ms (median, min .. max) | fold + unfold launches | training step ms (median, min .. max) | fold + unfold launches |\n"
              "|---|---|---|---|---|")
        for S in (int(v) for v in args.band_rows.split(",")):
            net.band_rows = S
            net.eval()
            fwd, n_fwd = _median_ms(forward, args.iters, args.warmup), launches(forward)
            net.train()
            trn, n_trn = _median_ms(step, args.iters, args.warmup), launches(step)
            print(f"| {S} | {fwd[0]:.3f} ({fwd[1]:.3f} .. {fwd[2]:.3f}) | {n_fwd[0]} + {n_fwd[1]} | {trn[0]:.3f} ({trn[1]:.3f} .. {trn[2]:.3f}) | "
                  f"{n_trn[0]} + {n_trn[1]} |", flush=True)
    finally:
        mnn.set_precision("f32")
        bandfold.fold, bandfold.unfold = fold, unfold


if __name__ == "__main__":
    main()
