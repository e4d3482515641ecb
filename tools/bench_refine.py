#!/usr/bin/env python3
"""Encoder-side latent refinement measured on a briefly trained model (masic_amd/refine.py).

    python tools/bench_refine.py [--train-steps 300 --lmbda 0.0932 --batch 8 --size 512 --steps 0,10,50,200 --lr 0.1 --out table.txt]
                                 [--budget-rel 1.0,0.75 [--budget-gain 0.5,1,2]]

Trains the default-init HSIC(128,192,5) as tools/train_converge.py does (bf16 operands, the synthetic consistent pairs), then, on B
held-out pairs of size x size, for every number of refinement steps: cost_best / cost_start (the true objective, mean over the pairs),
the bytes of the real files (HSIC.compress_batch(latents=...)), the PSNR of both views from the pictures HSIC.decompress_batch returns
(mean of the per-pair values), and the time of the call; for the longest run the true objective at every check.  The time of one
refinement step and of one true-objective check come from two runs of --time-steps steps, one that checks once and one that checks at
every step; beside them the training step of the same model at the same shape (masic_amd.train.train_step: forward + backward with
weight gradients + two Adams), measured in the same run.

--budget-rel: rows of the refinement under a bit budget (RefineConfig(budget_rel=...)) next to unbudgeted rows of the same model, for
every gain of --budget-gain: the pairs' budget and achieved estimated bits, how many pairs end feasible, MSE1 + MSE2, the bytes of the
real files and their ratio to the estimated bits, PSNR, mu at the end and the time of the call; then the time of a budgeted step against
the unbudgeted one, in alternating runs.
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


def _coded(net, x1, x2, hm, lat):
    """the real files of the latents -> (bytes per pair, PSNR1, PSNR2 of the decoded pictures, decode == encode)"""
    B = x1.shape[0]
    with tempfile.TemporaryDirectory(prefix="masic_refine_") as tmp, torch.no_grad():
        names = [f"p{i}" for i in range(B)]
        enc = net.compress_batch(x1, x2, hm, names, tmp, latents=lat)
        dec = net.decompress_batch(names, hm, tmp)
        exact = all(torch.equal(enc[k], dec[k]) for k in ("x1_hat", "x2_hat"))
    psnr = []
    for xh, x in ((dec["x1_hat"], x1), (dec["x2_hat"], x2)):
        mse = ((xh.clamp(0, 1) - x) ** 2).flatten(1).mean(dim=1).double()
        psnr.append(float((10.0 * torch.log10(1.0 / mse)).mean()))
    return enc["bytes"], psnr[0], psnr[1], exact


def _estimate(net, x1, x2, hm, lat):
    """(estimated bits, MSE1 + MSE2) per pair of four latents, as refine_latents evaluates them"""
    from masic_amd import metrics, ops, refine
    from masic_amd.homography import warp_matrices
    B, _, H, W = x1.shape
    with torch.no_grad():
        m_fwd = torch.cat([warp_matrices(hm[i:i + 1], (H, W), (H, W), want_inverse=True)[0] for i in range(B)]).contiguous()
        gates = net.mask2weights_unit(ops.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))).contiguous()
        out = net._eval_from_latents(*lat[:4], m_fwd, gates)
        L = out["likelihoods"]
        rows = metrics.pair_rd(out["x1_hat"].contiguous(), x1, out["x2_hat"].contiguous(), x2, [L[k].contiguous() for k in ("y1", "y2", "z1", "z2")])
        return refine.bits_and_mse(rows, 3 * H * W)


def _budget_tables(args, net, x1, x2, hm, lr, say):
    from masic_amd import refine
    B = x1.shape[0]
    rels = [float(v) for v in args.budget_rel.split(",")]
    gains = [refine.DEFAULT_BUDGET_GAIN] if args.budget_gain is None else [float(v) for v in args.budget_gain.split(",")]
    steps_list = [int(v) for v in args.steps.split(",")]
    say()
    say(f"refinement under a bit budget (lr {lr:g}, check every 5): estimated bits are the loop's own, summed over the {B} pairs; feasible = pairs "
        "whose estimate is within their budget; D = MSE1 + MSE2, mean over the pairs")
    say(f"{'gain':>5} {'rel':>5} {'steps':>6} {'budget bits':>12} {'est. bits':>12} {'feasible':>9} {'D x 1e3':>9} {'file bytes':>11} {'file/est':>9} "
        f"{'PSNR1 dB':>9} {'PSNR2 dB':>9} {'mu min .. max':>17} {'refine s':>9}")

    def row(gain, rel, steps, lat, t_ref, r, d, target, mu):
        nbytes, p1, p2, exact = _coded(net, x1, x2, hm, lat)
        feas = "-" if target is None else f"{int((r <= target).sum())}/{B}"
        say(f"{gain:>5} {rel:>5} {steps:>6d} {'-' if target is None else format(float(target.sum()), '.0f'):>12} {float(r.sum()):>12.0f} {feas:>9} "
            f"{float(d.mean()) * 1e3:>9.4f} {sum(nbytes):>11d} {sum(nbytes) * 8.0 / float(r.sum()):>9.4f} {p1:>9.3f} {p2:>9.3f} "
            f"{'-' if mu is None else format(float(mu.min()), '.3f') + ' .. ' + format(float(mu.max()), '.3f'):>17} {t_ref:>9.2f}"
            + ("" if exact else "   DECODE MISMATCH"))
        return [n * 8.0 / float(v) for n, v in zip(nbytes, r)]

    ratios = []
    for steps in steps_list:
        lat, t_ref = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, refine.RefineConfig(steps=steps, lr=lr, check_every=5)))
        r, d = _estimate(net, x1, x2, hm, lat)
        ratios += row("-", "-", steps, lat, t_ref, r, d, None, None)
    for gain in gains:
        for rel in rels:
            for steps in (v for v in steps_list if v > 0):
                cfg = refine.RefineConfig(steps=steps, lr=lr, check_every=5, budget_rel=rel, budget_gain=gain)
                lat, t_ref = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, cfg))
                ratios += row(f"{gain:g}", f"{rel:g}", steps, lat, t_ref, lat.bits_best, lat.mse_best, lat.target_bits, lat.mu)
    say(f"file bits / estimated bits per pair over all rows: min {min(ratios):.4f}  mean {sum(ratios) / len(ratios):.4f}  max {max(ratios):.4f}")
    # ---- the budgeted step against the unbudgeted one: alternating runs of T steps with one check, less the call of 0 steps
    T = args.time_steps
    plain = lambda n: refine.RefineConfig(steps=n, lr=lr, check_every=max(n, 1))
    budget = lambda n: refine.RefineConfig(steps=n, lr=lr, check_every=max(n, 1), budget_rel=1.0)
    for cfg in (plain(3), budget(3)):
        refine.refine_latents(net, x1, x2, hm, args.lmbda, cfg)                # warm-up
    ms = {"unbudgeted": [], "budgeted": []}
    for _ in range(args.time_runs):
        for name, make in (("unbudgeted", plain), ("budgeted", budget)):
            _, t0 = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, make(0)))
            _, t1 = _timed(lambda: refine.refine_latents(net, x1, x2, hm, args.lmbda, make(T)))
            ms[name].append((t1 - t0) / T * 1e3)
    say()
    say(f"time of a refinement step, {args.time_runs} alternating runs of {T} steps with one check each, less the call of 0 steps (ms per step):")
    for name, v in ms.items():
        say(f"  {name:<11} " + " ".join(f"{t:6.2f}" for t in v) + f"   median {sorted(v)[len(v) // 2]:6.2f}  spread {max(v) - min(v):5.2f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--lmbda", type=float, default=0.0932)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", default="0,10,50,200")
    ap.add_argument("--lr", default=None, help="comma-separated Adam step sizes (default: masic_amd.refine.DEFAULT_LR)")
    ap.add_argument("--time-steps", type=int, default=20)
    ap.add_argument("--budget-rel", default=None, help="comma-separated budget_rel values: adds the table of the budgeted refinement")
    ap.add_argument("--budget-gain", default=None, help="comma-separated budget_gain values (default: masic_amd.refine.DEFAULT_BUDGET_GAIN)")
    ap.add_argument("--time-runs", type=int, default=5, help="alternating runs of the budgeted and the unbudgeted step")
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
                per_pair, *psnr, exact = _coded(net, x1, x2, hm, lat)
                nbytes = sum(per_pair)
                cs, cb = float(lat.cost_start.mean()), float(lat.cost_best.mean())
                say(f"{lr:>6g} {steps:>6d} {float((lat.cost_best / lat.cost_start).mean()):>15.4f} {cs:>9.4f} {cb:>9.4f} {nbytes:>11d} "
                    f"{nbytes * 8.0 / (B * S * S):>8.4f} {psnr[0]:>9.3f} {psnr[1]:>9.3f} {t_ref:>9.2f}" + ("" if exact else "   DECODE MISMATCH"))
        say()
        say("the true objective at the checks of the longest run (step:J, mean over the pairs):")
        for lr, tr in traces:
            say(f"  lr {lr:g}: " + " ".join(f"{s}:{float(j.mean()):.1f}" for s, j in tr))
        if args.budget_rel:
            _budget_tables(args, net, x1, x2, hm, lrs[0], say)          # before the training steps below move the model
            say()
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
