"""Times and grades the weight-free patch aligner (masic_amd/align.py: one HIP launch, one workgroup per pair) and, beside it, the UDH
homography net it can stand in for.

Time: `align_patches` at patch size 128 for B = 1 and B = 8, eager and as a captured graph replayed, alternated inside one process; a
sample is `--inner` back-to-back calls between two device events, the figure the median of `--samples` (>= 20) samples with the
spread (min - max).  The net's forward (tools/bench_udh.py's `udh_hip`) is timed in the same loop when `--udh-weights` is given,
with random weights of the same shapes otherwise (its time does not depend on them).

Where the time goes: the same call at B = 1 with other iteration counts (no step; 30 or 60 steps on the 32 x 32 level only; 15 on the
64 x 64 level only; 10 on the finest only), from which the cost of the search and of one step per level follow by subtraction.

Quality, on the synthetic sets of tests/align_ref.py (a smooth random texture, a translation up to +-tmax px plus +-jitter px per
corner coordinate, 2 % noise; 2 textures x `--seeds` seeds per set): the mean corner error in pixels and `ops.udh_photo_loss`, the
loss the net is trained on, at the estimate, at the truth and at delta = 0.  The same two figures for the net when `--udh-weights`
names a state dict of coremasic/mywork/model.py: Net.

One JSON line per figure on stdout and in `--out` (default profiles/align_bench.txt)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import model as udh  # noqa: E402
from masic_amd import align, ops  # noqa: E402
from tests import align_ref as R  # noqa: E402

SETS = ((16, 4), (32, 4), (40, 8), (45, 0), (0, 8))          # (tmax, jitter); the last is stage 2 alone from delta0 = 0
LINES = []


def emit(rec):
    line = json.dumps(rec)
    LINES.append(line)
    print(line, flush=True)
    return rec


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def summary(name, ms, **extra):
    rec = {"name": name, "median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5),
           "samples": len(ms)}
    rec.update(extra)
    return emit(rec)


def captured(fn, check):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    torch.cuda.synchronize()
    check(out)
    return graph


def photo_loss(a, b, delta, P):
    s = R.square(P, torch.float32).to(a.device)[None]
    return [float(ops.udh_photo_loss(a[i:i + 1], ops.udh_photo_matrix(s, delta[i:i + 1].contiguous(), (P, P), (P, P)), b[i:i + 1]))
            for i in range(a.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--udh-weights", default=None, help="state dict of coremasic/mywork/model.py: Net (torch.save)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_align: no GPU; nothing here is measured on a CPU")
    dev, P = "cuda", args.patch
    torch.manual_seed(0)
    net = udh.Net(patch_size=P).to(dev).eval()
    if args.udh_weights:
        net.load_state_dict(torch.load(args.udh_weights, map_location=dev))

    # ---- time per call
    for B in args.batches:
        a, b, _ = R.make_set(P, (2.5, 4.0), 32, 4, range((B + 1) // 2))
        a, b = a[:B].to(dev), b[:B].to(dev)
        with torch.no_grad():
            for _ in range(args.warmup):
                want, info = align.align_patches(a, b)
                net(a, b)
            graph = captured(lambda: align.align_patches(a, b)[0], lambda out: torch.equal(out, want) or sys.exit("graph differs"))
            variants = {"align_eager": lambda: align.align_patches(a, b), "align_graph": graph.replay, "udh_net_eager": lambda: net(a, b)}
            times = {k: [] for k in variants}
            for _ in range(args.samples):
                for k, fn in variants.items():
                    times[k].append(sample(fn, args.inner))
        for k, v in times.items():
            summary(k, v, B=B, patch=P, status=info[:, 3].tolist() if k.startswith("align") else None,
                    trained_weights=bool(args.udh_weights) if k.startswith("udh") else None)

    # ---- what a step costs on each level: B = 1, the same call with other iteration counts (coarse to fine)
    a, b, _ = R.make_set(P, (2.5,), 32, 4, (0,))
    a, b = a.to(dev), b.to(dev)
    zero = torch.zeros((1, 4, 2), device=dev)
    triples = {"no_search_no_step": (zero, (0, 0, 0)), "search_no_step": (None, (0, 0, 0)), "search_30_0_0": (None, (30, 0, 0)),
               "search_60_0_0": (None, (60, 0, 0)), "search_0_15_0": (None, (0, 15, 0)), "search_0_0_10": (None, (0, 0, 10)),
               "search_30_15_10": (None, (30, 15, 10))}
    fns = {k: (lambda s=s, it=it: align.align_patches(a, b, s, iters=it)) for k, (s, it) in triples.items()}
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in fns}
        for _ in range(args.samples):
            for k, fn in fns.items():
                times[k].append(sample(fn, args.inner))
    med = {k: statistics.median(v) * 1e3 for k, v in times.items()}
    emit({"name": "align_call_us_by_iters", "B": 1, "patch": P, **{k: round(v, 1) for k, v in med.items()}})
    if P == 128:
        emit({"name": "align_step_us_by_level", "B": 1, "patch": P,
              "level_32": round((med["search_60_0_0"] - med["search_30_0_0"]) / 30, 2),
              "level_64": round((med["search_0_15_0"] - med["search_no_step"]) / 15, 2),
              "level_128": round((med["search_0_0_10"] - med["search_no_step"]) / 10, 2),
              "search": round(med["search_no_step"] - med["no_search_no_step"], 1)})

    # ---- quality
    for tmax, jitter in SETS:
        a, b, truth = R.make_set(P, (2.5, 4.0), tmax, jitter, range(args.seeds))
        a, b, truth = a.to(dev), b.to(dev), truth.float().to(dev)
        zero = torch.zeros_like(truth)
        with torch.no_grad():
            delta, info = align.align_patches(a, b, None if tmax else zero)
            rows = [("align", delta)] + ([("udh_net", net(a, b))] if args.udh_weights else [])
            base = {"at_truth": photo_loss(a, b, truth, P), "at_zero": photo_loss(a, b, zero, P)}
            for name, d in rows:
                err = R.corner_error(d.cpu(), truth.cpu())
                loss = photo_loss(a, b, d, P)
                emit({"name": f"{name}_quality", "patch": P, "tmax": tmax, "jitter": jitter, "search": bool(tmax), "cases": int(a.shape[0]),
                      "corner_error_px_mean": round(float(err.mean()), 5), "corner_error_px_max": round(float(err.max()), 5),
                      "photo_loss_mean": round(statistics.mean(loss), 5), "photo_loss_at_truth_mean": round(statistics.mean(base["at_truth"]), 5),
                      "photo_loss_at_zero_mean": round(statistics.mean(base["at_zero"]), 5),
                      "status": info[:, 3].tolist() if name == "align" else None})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
