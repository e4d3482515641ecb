"""HSIC.compress_batch / decompress_batch: encode and decode time per pair at B = 1, 2, 4, 8 (run on the GPU box).

HSIC(128,192,5), bf16 operands, synthetic weights and pairs (masic_amd.synth).  Every (size, B) is warmed up first; each timed run is
wall time around one call that ends in a device synchronise; the table holds the median of --runs runs divided by B.  The
single-pair methods are the B = 1 case behind a thin wrapper: their time is printed beside the B = 1 row and should equal it.  Every decode is checked against its encode.
  python tools/bench_codec_batch.py [--sizes 512x512,1216x2176] [--batches 1,2,4,8] [--runs 5] [--json out.json] [--no-verify]
                                    [--band-rows 0,8,4,2]
--band-rows adds a row per value: HSIC.compress_batch(..., band_rows=S) codes the y latents in independent bands of S latent rows,
w + 3 (S - 1) decode steps instead of w + 3 (h - 1) (0: off).  Synthetic weights: the bytes of these rows say nothing about the rate cost
(tools/bench_codec_bands.py measures that on a trained model).
--no-verify leaves out the decoder's final-state check (codec.decode_views verify=False): the cost of the check is the difference.
  python tools/bench_codec_batch.py --profile-one 512x512:8      (one decode_batch, for rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

import MASIC  # noqa: E402
from masic_amd import nn as mnn, synth  # noqa: E402

FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")


def _timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def _model():
    mnn.set_precision("bf16")
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=100))
    net = net.cuda().eval()
    net.update()
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1216x2176")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-one", default=None)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--band-rows", default="0")
    args = ap.parse_args()
    if args.no_verify:
        import functools
        from masic_amd import codec
        codec.decode_views = functools.partial(codec.decode_views, verify=False)
    bands = [int(v) for v in args.band_rows.split(",")]
    net = _model()
    d = tempfile.mkdtemp()
    if args.profile_one:
        size, B = args.profile_one.split(":")
        H, W = (int(v) for v in size.split("x"))
        B = int(B)
        x1, x2, hm = (t.cuda() for t in synth.synth_inputs(B, H, W, seed=100))
        names = [f"p{i}" for i in range(B)]
        with torch.no_grad():
            net.compress_batch(x1, x2, hm, names, d)
            net.decompress_batch(names, hm, d)
            t, _ = _timed(lambda: net.decompress_batch(names, hm, d))
        print(f"profile run: decode {H}x{W} B={B}: {1e3 * t / B:.2f} ms per pair")
        return
    rows = []
    with torch.no_grad():
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            Bmax = max(int(b) for b in args.batches.split(","))
            x1a, x2a, hma = (t.cuda() for t in synth.synth_inputs(Bmax, H, W, seed=100))
            # the single-pair methods (the B = 1 case of the same implementation)
            net.compress(x1a[:1], x2a[:1], hma[:1], "single", d)
            net.decompress(None, None, hma[:1], "single", d)
            se = statistics.median(_timed(lambda: net.compress(x1a[:1], x2a[:1], hma[:1], "single", d))[0] for _ in range(args.runs))
            sd = statistics.median(_timed(lambda: net.decompress(None, None, hma[:1], "single", d))[0] for _ in range(args.runs))
            print(f"{H}x{W} single-pair compress {1e3 * se:.2f} ms, decompress {1e3 * sd:.2f} ms", flush=True)
            for B, S in ((int(b), S) for b in args.batches.split(",") for S in bands):
                x1, x2, hm = x1a[:B], x2a[:B], hma[:B]
                names = [f"b{B}_{i}" for i in range(B)]
                kw = {"band_rows": S} if S else {}
                enc = net.compress_batch(x1, x2, hm, names, d, **kw)               # warm-up (allocator, weight packs, step lists)
                dec = net.decompress_batch(names, hm, d)
                assert all(torch.equal(enc[k], dec[k]) for k in FIELDS), "round trip"
                te = [_timed(lambda: net.compress_batch(x1, x2, hm, names, d, **kw))[0] for _ in range(args.runs)]
                td = [_timed(lambda: net.decompress_batch(names, hm, d))[0] for _ in range(args.runs)]
                row = {"size": f"{H}x{W}", "B": B, "band_rows": S, "encode_ms_per_pair": 1e3 * statistics.median(te) / B,
                       "decode_ms_per_pair": 1e3 * statistics.median(td) / B, "single_encode_ms": 1e3 * se, "single_decode_ms": 1e3 * sd,
                       "decode_ms_per_pair_runs": [1e3 * t / B for t in td], "bytes_per_pair": sum(enc["bytes"]) / B}
                rows.append(row)
                print(f"{H}x{W} B={B} band_rows={S}: encode {row['encode_ms_per_pair']:.2f} ms/pair, decode {row['decode_ms_per_pair']:.2f} ms/pair "
                      f"(runs {1e3 * min(td) / B:.2f} .. {1e3 * max(td) / B:.2f}; {row['bytes_per_pair']:.0f} bytes/pair)", flush=True)
            del x1a, x2a, hma
            torch.cuda.empty_cache()
    print("\n| size | B | band_rows | encode ms/pair | decode ms/pair (runs) | bytes/pair |\n|---|---|---|---|---|---|")
    for r in rows:
        runs = r["decode_ms_per_pair_runs"]
        print(f"| {r['size']} | {r['B']} | {r['band_rows']} | {r['encode_ms_per_pair']:.2f} | {r['decode_ms_per_pair']:.2f} "
              f"({min(runs):.2f} .. {max(runs):.2f}) | {r['bytes_per_pair']:.0f} |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
