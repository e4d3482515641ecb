#!/usr/bin/env python3
"""Encoder-side latent refinement measured on a briefly trained model (masic_amd/refine.py).

    python tools/bench_refine.py [--train-steps 300 --lmbda 0.0932 --batch 8 --size 512 --steps 0,10,50,200 --lr 0.1 --out table.txt]

Trains the default-init HSIC(128,192,5) as tools/train_converge.py does (bf16 operands, the synthetic consistent pairs), then, on B
held-out pairs of size x size, for every number of refinement steps: cost_best / cost_start (the true objective, mean over the pairs),
the bytes of the real files (HSIC.compress_batch(latents=...)), the PSNR of both views from the pictures HSIC.decompress_batch returns
(mean of the per-pair values), and the time of the call; for the longest run the true objective at every check.  The time of one
refinement step and of one true-objective check come from two runs of --time-steps steps, one that checks once and one that checks at
every step; beside them the training step of the same model at the same shape (masic_amd.train.train_step: forward + backward with
weight gradients + two Adams), measured in the same run.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--lmbda", type=float, default=0.0932)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", default="0,10,50,200")
    ap.add_argument("--lr", default=None, help="comma-separated Adam step sizes (default: masic_amd.refine.DEFAULT_LR)")
    ap.add_argument("--time-steps", type=int, default=20)
    ap.add_argument("--precision", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine: needs an MI355X -- the library has no CPU path")
    from masic_amd import nn as mnn, refine, synth, trainrun
    from masic_amd.train import make_optimizers, train_step
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    lrs = [refine.DEFAULT_LR] if args.lr is None else [float(v) for v in args.lr.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    net = trainrun.default_init(device=dev)
    pool = trainrun.batch_pool(16, 4, 256, 256, dev)
    _, dt = _timed(lambda: trainrun.train(net, args.train_steps, pool, args.lmbda, precision=args.precision))
    say(f"model: HSIC(128,192,5), default init + {args.train_steps} training steps at 4 x 256 x 256, lmbda {args.lmbda}, {args.precision} operands "
        f"({dt:.1f} s)")
    x1, x2, hm = trainrun.consistent_pair(*(t.to(dev) for t in synth.synth_inputs(B, S, S, seed=9001)), seed=9001)
    mnn.set_precision(args.precision)
    try:
        net.eval()
        net.update(force=True)
        say(f"pairs: {B} held-out synthetic pairs of {S} x {S}; objective J = bits / (H W) + lmbda 255^2 (MSE1 + MSE2) per pair, mean over the pairs")
        say()
        say(f"{'lr':>6} {'steps':>6} {'J_best/J_start':>15} {'J_start':>9} {'J_best':>9} {'file bytes':>11} {'bpp':>8} {'PSNR1 dB':>9} {'PSNR2 dB':>9} {'refine s':>9}")
        traces = []
        for lr in lrs:
            for steps in (int(v) for v in args.steps.split(",")):
                cfg = refine.RefineConfig(steps=steps, lr=lr, check_every=5)
                tr = []
                lat, t_ref = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, cfg, trace=tr))
                if steps == max(int(v) for v in args.steps.split(",")):
                    traces.append((lr, tr))
                with tempfile.TemporaryDirectory(prefix="masic_refine_") as tmp, torch.no_grad():
                    names = [f"p{i}" for i in range(B)]
                    enc = net.compress_batch(x1, x2, hm, names, tmp, latents=lat)
                    dec = net.decompress_batch(names, hm, tmp)
                    exact = all(torch.equal(enc[k], dec[k]) for k in ("x1_hat", "x2_hat"))
                nbytes = sum(enc["bytes"])
                psnr = []
                for xh, x in ((dec["x1_hat"], x1), (dec["x2_hat"], x2)):
                    mse = ((xh.clamp(0, 1) - x) ** 2).flatten(1).mean(dim=1).double()
                    psnr.append(float((10.0 * torch.log10(1.0 / mse)).mean()))
                cs, cb = float(lat.cost_start.mean()), float(lat.cost_best.mean())
                say(f"{lr:>6g} {steps:>6d} {float((lat.cost_best / lat.cost_start).mean()):>15.4f} {cs:>9.4f} {cb:>9.4f} {nbytes:>11d} "
                    f"{nbytes * 8.0 / (B * S * S):>8.4f} {psnr[0]:>9.3f} {psnr[1]:>9.3f} {t_ref:>9.2f}" + ("" if exact else "   DECODE MISMATCH"))
        say()
        say("the true objective at the checks of the longest run (step:J, mean over the pairs):")
        for lr, tr in traces:
            say(f"  lr {lr:g}: " + " ".join(f"{s}:{float(j.mean()):.1f}" for s, j in tr))
        # ---- time of a step and of a check
        T = args.time_steps
        refine.refine_latents(net, x1, x2, hm, args.lmbda, refine.RefineConfig(steps=3, lr=lrs[0], check_every=1))          # warm-up
        _, t_once = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, refine.RefineConfig(steps=T, lr=lrs[0], check_every=T)))
        _, t_every = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, refine.RefineConfig(steps=T, lr=lrs[0], check_every=1)))
        _, t_zero = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, refine.RefineConfig(steps=0)))
        check_ms = (t_every - t_once) / (T - 1) * 1e3                       # T checks against 1 (the check at the start is in both)
        step_ms = (t_once - t_zero - check_ms * 1e-3) / T * 1e3           # t_zero: the analysis transforms and the check at the start
        # ---- the training step of the same model at the same shape
        net.train()
        opt, aopt = make_optimizers(net)
        for _ in range(3):
            train_step(net, opt, aopt, x1, x2, hm, args.lmbda, None)
        _, t_train = _timed(lambda: [train_step(net, opt, aopt, x1, x2, hm, args.lmbda, None) for _ in range(T)])
        train_ms = t_train / T * 1e3
        say()
        say(f"time at {B} x {S} x {S}, {args.precision} operands ({T} steps each, host clock around a device synchronisation):")
        say(f"  refinement step (noise + surrogate forward + input-gradient backward + Adam)   {step_ms:8.2f} ms")
        say(f"  true-objective check (eval path from the latents + keep-best)                  {check_ms:8.2f} ms")
        say(f"  training step of the same model (weight gradients, two Adams)                  {train_ms:8.2f} ms")
        say(f"  refinement step / training step                                                {step_ms / train_ms:8.2f}")
    finally:
        mnn.set_precision("f32")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
