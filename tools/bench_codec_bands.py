#!/usr/bin/env python3
"""What the row bands of the y bitstream cost in bytes: HSIC.compress_batch(..., band_rows=S) on a briefly TRAINED model (run on the GPU
box).

    python tools/bench_codec_bands.py [--steps 400 --batch 4 --size 256 --lmbda 0.0932 --pairs 4 --band-rows 0,16,8,4,2,1 --out x.json]

With band_rows = S the first two rows of every band of S latent rows code without the rows above them: fewer
decode steps, more bytes.  How many more depends on how much the context model has learned to take from those rows -- synthetic weights
have a random context model and say nothing -- so this tool trains HSIC(128,192,5) from the default init for --steps steps with the
helpers of masic_amd/trainrun.py (as tools/train_converge.py does; bf16 operands, the same pool of consistent synthetic pairs), then
codes --pairs held-out 512 x 512 pairs with every band_rows and prints bytes per pair (both files; and the .bin alone) beside the
row of band_rows = 0.  The latents do not depend on band_rows: the reconstructions of every row must be those of the first, bit for
bit (asserted), so both views' PSNR is printed once.  Every row is decoded and checked against its encode."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")


def _psnr(a, b):
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--lmbda", type=float, default=0.0932)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--band-rows", default="0,16,8,4,2,1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from masic_amd import nn as mnn, synth, trainrun
    dev = torch.device("cuda", 0)
    pool = trainrun.batch_pool(args.pool, args.batch, args.size, args.size, dev)
    net = trainrun.default_init(device=dev)
    t0 = time.perf_counter()
    losses, _, _ = trainrun.train(net, args.steps, pool, args.lmbda, precision="bf16", lr=args.lr, log=max(1, args.steps // 5))
    print(f"trained {args.steps} steps (batch {args.batch}, {args.size}x{args.size}, lambda {args.lmbda}) in {time.perf_counter() - t0:.1f} s: "
          f"loss {losses[0][0]:.2f} -> {losses[-1][0]:.2f}, bpp {losses[0][1]:.3f} -> {losses[-1][1]:.3f}", flush=True)
    x1, x2, hm = trainrun.consistent_pair(*(t.to(dev) for t in synth.synth_inputs(args.pairs, 512, 512, seed=9001)), seed=9001)
    names = [f"p{i}" for i in range(args.pairs)]
    d = tempfile.mkdtemp()
    rows, first = [], None
    mnn.set_precision("bf16")
    try:
        net.eval()
        net.update(force=True)
        with torch.no_grad():
            for S in (int(v) for v in args.band_rows.split(",")):
                enc = net.compress_batch(x1, x2, hm, names, d, band_rows=S)
                dec = net.decompress_batch(names, hm, d)
                assert all(torch.equal(enc[k], dec[k]) for k in FIELDS), f"round trip at band_rows {S}"
                if first is None:
                    first = enc
                    print(f"held-out {args.pairs} x 512x512: PSNR {_psnr(enc['x1_hat'], x1):.2f} / {_psnr(enc['x2_hat'], x2):.2f} dB (every row)")
                assert all(torch.equal(enc[k], first[k]) for k in FIELDS), f"band_rows {S} changed a latent or a reconstruction"
                nbin = sum(os.path.getsize(os.path.join(d, n + ".bin")) for n in names) / args.pairs
                rows.append({"band_rows": S, "bytes_per_pair": sum(enc["bytes"]) / args.pairs, "bin_bytes_per_pair": nbin,
                             "bpp": sum(enc["bpp"]) / args.pairs, "steps_per_view": 32 + 3 * ((S if 0 < S < 32 else 32) - 1)})
    finally:
        mnn.set_precision("f32")
    base = rows[0]
    print("\n| band_rows | decode steps per view | bytes/pair | y streams (.bin) bytes/pair | bpp | vs first row |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['band_rows']} | {r['steps_per_view']} | {r['bytes_per_pair']:.0f} | {r['bin_bytes_per_pair']:.0f} | {r['bpp']:.4f} | "
              f"{r['bytes_per_pair'] / base['bytes_per_pair'] - 1.0:+.2%} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"args": vars(args), "rows": rows, "loss_first_last": [losses[0], losses[-1]]}, f, indent=1)


if __name__ == "__main__":
    main()
