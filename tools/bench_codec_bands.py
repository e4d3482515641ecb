#!/usr/bin/env python3
"""What the row bands of the y bitstream cost in bytes: HSIC.compress_batch(..., band_rows=S) on a briefly TRAINED model (run on the GPU
box).

    python tools/bench_codec_bands.py [--steps 400 --batch 4 --size 256 --lmbda 0.0932 --pairs 4 --band-rows 0,16,8,4,2,1
        --train-band-rows S --out x.json]

With band_rows = S the first two rows of every band of S latent rows code without the rows above them: fewer
decode steps, more bytes.  How many more depends on how much the context model has learned to take from those rows -- synthetic weights
have a random context model and say nothing -- so this tool trains HSIC(128,192,5) from the default init for --steps steps with the
helpers of masic_amd/trainrun.py (as tools/train_converge.py does; bf16 operands, the same pool of consistent synthetic pairs), then
codes --pairs held-out 512 x 512 pairs with every band_rows and prints bytes per pair (both files; and the .bin alone) beside the
row of band_rows = 0.  The latents do not depend on band_rows: the reconstructions of every row must be those of the first, bit for
bit (asserted), so both views' PSNR is printed once.  Every row is decoded and checked against its encode.

--train-band-rows S: a SECOND model, from the same initialisation on the same batches and noise, trained with HSIC.band_rows = S (the
training graph's context models do not see across the top edge of a band of S latent rows; DESIGN.md section 8.1 "Row bands in the
model") -- whether training for the band tops buys back the bytes they cost.  Every row then holds the bytes per pair of both models.
Beside the coded y streams the table prints the model's own estimate of them, -sum log2 of the y likelihoods of the eval forward, with
HSIC.band_rows at the row's band_rows (the banded estimate) and at 0 (the unbanded one, whatever the file)."""
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


def _y_bits(net, x1, x2, hm, S):
    """the estimated bits per pair of the two y streams with the model's band_rows at S"""
    from masic_amd import bands
    with bands.model_band_rows(net, S):
        L = net(x1, x2, hm)["likelihoods"]
    return float(-(torch.log2(L["y1"].double()).sum() + torch.log2(L["y2"].double()).sum())) / x1.shape[0]


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
    ap.add_argument("--train-band-rows", type=int, default=0, help="train a second model with HSIC.band_rows at this value (0: one model)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from masic_amd import nn as mnn, synth, trainrun
    dev = torch.device("cuda", 0)
    pool = trainrun.batch_pool(args.pool, args.batch, args.size, args.size, dev)
    models = []                                     # (trained with band_rows, net, losses)
    for trained_for in [0] + ([args.train_band_rows] if args.train_band_rows else []):
        net = trainrun.default_init(device=dev)
        net.band_rows = trained_for
        t0 = time.perf_counter()
        losses, _, _ = trainrun.train(net, args.steps, pool, args.lmbda, precision="bf16", lr=args.lr, log=max(1, args.steps // 5))
        net.band_rows = 0
        print(f"trained {args.steps} steps with band_rows {trained_for} (batch {args.batch}, {args.size}x{args.size}, lambda {args.lmbda}) in "
              f"{time.perf_counter() - t0:.1f} s: loss {losses[0][0]:.2f} -> {losses[-1][0]:.2f}, bpp {losses[0][1]:.3f} -> {losses[-1][1]:.3f}",
              flush=True)
        models.append((trained_for, net, losses))
    x1, x2, hm = trainrun.consistent_pair(*(t.to(dev) for t in synth.synth_inputs(args.pairs, 512, 512, seed=9001)), seed=9001)
    names = [f"p{i}" for i in range(args.pairs)]
    d = tempfile.mkdtemp()
    tables = []
    mnn.set_precision("bf16")
    try:
        for trained_for, net, _ in models:
            rows, first = [], None
            net.eval()
            net.update(force=True)
            with torch.no_grad():
                unbanded = _y_bits(net, x1, x2, hm, 0)
                for S in (int(v) for v in args.band_rows.split(",")):
                    enc = net.compress_batch(x1, x2, hm, names, d, band_rows=S)
                    dec = net.decompress_batch(names, hm, d)
                    assert all(torch.equal(enc[k], dec[k]) for k in FIELDS), f"round trip at band_rows {S}"
                    if first is None:
                        first = enc
                        print(f"model trained with band_rows {trained_for}, held-out {args.pairs} x 512x512: PSNR {_psnr(enc['x1_hat'], x1):.2f} / "
                              f"{_psnr(enc['x2_hat'], x2):.2f} dB (every row)")
                    assert all(torch.equal(enc[k], first[k]) for k in FIELDS), f"band_rows {S} changed a latent or a reconstruction"
                    nbin = sum(os.path.getsize(os.path.join(d, n + ".bin")) for n in names) / args.pairs
                    rows.append({"band_rows": S, "bytes_per_pair": sum(enc["bytes"]) / args.pairs, "bin_bytes_per_pair": nbin,
                                 "bpp": sum(enc["bpp"]) / args.pairs, "steps_per_view": 32 + 3 * ((S if 0 < S < 32 else 32) - 1),
                                 "y_bits_banded_estimate": _y_bits(net, x1, x2, hm, S), "y_bits_unbanded_estimate": unbanded})
            tables.append(rows)
    finally:
        mnn.set_precision("f32")
    for (trained_for, _, _), rows in zip(models, tables):
        base = rows[0]
        print(f"\nmodel trained with band_rows {trained_for}\n"
              "| band_rows | decode steps per view | bytes/pair | y streams (.bin) bytes/pair | bpp | vs first row | y streams bits | banded estimate "
              "(vs coded) | unbanded estimate (vs coded) |\n|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            bits = 8.0 * r["bin_bytes_per_pair"]
            print(f"| {r['band_rows']} | {r['steps_per_view']} | {r['bytes_per_pair']:.0f} | {r['bin_bytes_per_pair']:.0f} | {r['bpp']:.4f} | "
                  f"{r['bytes_per_pair'] / base['bytes_per_pair'] - 1.0:+.2%} | {bits:.0f} | {r['y_bits_banded_estimate']:.0f} "
                  f"({r['y_bits_banded_estimate'] / bits - 1.0:+.2%}) | {r['y_bits_unbanded_estimate']:.0f} ({r['y_bits_unbanded_estimate'] / bits - 1.0:+.2%}) |")
    if len(tables) == 2:
        print(f"\n| band_rows | bytes/pair, trained with 0 | bytes/pair, trained with {models[1][0]} | second vs first | second vs the first model's "
              "band_rows 0 |\n|---|---|---|---|---|")
        for a, b in zip(*tables):
            print(f"| {a['band_rows']} | {a['bytes_per_pair']:.0f} | {b['bytes_per_pair']:.0f} | {b['bytes_per_pair'] / a['bytes_per_pair'] - 1.0:+.2%} | "
                  f"{b['bytes_per_pair'] / tables[0][0]['bytes_per_pair'] - 1.0:+.2%} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"args": vars(args), "models": [{"trained_with_band_rows": m[0], "rows": rows, "loss_first_last": [m[2][0], m[2][-1]]}
                                                      for m, rows in zip(models, tables)]}, f, indent=1)


if __name__ == "__main__":
    main()
