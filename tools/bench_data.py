"""What a training batch costs when the dataset lives in device memory (masic_amd/data.py; run on the GPU box):

  1. DeviceStereoFolder.batch: 8 pairs cropped to 512 x 512 out of synthetic 860 x 1080 pictures (InStereo2K's size), --pairs of them so
     that the arena (5.6 MB a pair) is larger than the L2 and the 256 MB last-level cache; every batch takes other pairs at other
     windows, in the dataset's own random order.
  2. The same batches the only way the library could make them before: ops.pair_prep per view (2 calls = 4 launches a pair) on the
     pictures already on the device, stacked into the batch tensors.  The two paths are compared bit for bit first.
  3. The two kernels alone (device events over back-to-back launches, each launch on other pairs) against the bytes they must move,
     as a share of the 6.3 TB/s this chip streams.
  4. With --step: the training step the batches feed (HSIC(128,192,5), bf16 operands, masic_amd.train.train_step, h_matrix from a
     default-initialised homography net), and the batch as a share of it.

Times: device events around --iters batches issued back to back (the device's time per batch), and the host clock around the same
loop ending in a synchronise (what a training loop would see if it did nothing else; its inverse is the batches/s figure).

  python tools/bench_data.py [--pairs 64] [--iters 200] [--runs 3] [--step] [--out profiles/data_bench.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from masic_amd import data, ops  # noqa: E402
from masic_amd._lib import check, lib  # noqa: E402

H0, W0, CROP, B = 860, 1080, (512, 512), 8
STREAM = 6.3e12          # bytes/s this chip streams


def _dataset(pairs, seed=0):
    rng = np.random.default_rng(seed)
    lefts = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(pairs)]
    rights = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(pairs)]
    return data.DeviceStereoFolder.from_arrays(lefts, rights, patch_size=CROP, seed=seed)


def _plan(ds, iters, seed=1):
    """(indices, draws) per batch: every pair of the dataset in turn, shuffled, at the reference's random windows"""
    import random
    rng, order, plan = random.Random(seed), [], []
    for _ in range(iters):
        if len(order) < B:
            more = list(range(len(ds)))
            rng.shuffle(more)
            order += more
        index, order = order[:B], order[B:]
        plan.append((index, data.draw_items(rng, [ds.sizes[i] for i in index], CROP)))
    return plan


def _timed_loop(fn, plan):
    """(device us per batch, host us per batch of a loop that ends in a synchronise)"""
    for item in plan[:3]:
        fn(*item)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    for item in plan:
        fn(*item)
    b.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    return 1e3 * a.elapsed_time(b) / len(plan), 1e6 * wall / len(plan)


def _pair_prep_batch(ds, views):
    def run(index, draws):
        d1, d2, h1, h2 = [], [], [], []
        for i, (sh, sw, x, y) in zip(index, draws):
            for side, pics, homos in ((0, d1, h1), (1, d2, h2)):
                pic, patch = ops.pair_prep(views[2 * i + side], (sh, sw), CROP, ds.homopic, (x, y), ds.homopatch)
                pics.append(pic)
                homos.append(patch)
        return torch.stack(d1), torch.stack(d2), torch.stack(h1), torch.stack(h2)
    return run


def _kernels_alone(ds, plan, say):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    P, hp = 2 * B, ds.homopatch
    planes = torch.empty((P, 3) + CROP, device="cuda")
    patches = torch.empty((P, 1, hp, hp), device="cuda")
    tables = []
    for index, draws in plan:
        rows = ops.check_view_descriptors(ds.descriptors(index, draws), ds.arena.numel(), CROP, ds.homopic, hp)
        tables.append(torch.from_numpy(ops.pack_view_descriptors(rows)).cuda())
    st = ops._stream()

    def events(planes_arg, patches_arg):
        call = lambda t: check(lib.masic_views_prep(p(ds.arena), ds.arena.numel(), p(t), P, CROP[0], CROP[1], planes_arg, ds.homopic, hp, patches_arg, st))
        for t in tables[:3]:
            call(t)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in tables:
            call(t)
        b.record()
        torch.cuda.synchronize()
        return 1e-3 * a.elapsed_time(b) / len(tables)

    t_pl, t_pa = events(p(planes), None), events(None, p(patches))
    b_pl = P * CROP[0] * CROP[1] * (3 + 12)
    least = b_pl / STREAM
    say(f"crop kernel alone:  {1e6 * t_pl:.1f} us per batch of {P} views, {b_pl / 1e6:.1f} MB (3 B read + 12 B written a pixel) = "
        f"{b_pl / t_pl / 1e12:.2f} TB/s = {100 * least / t_pl:.0f} % of the {STREAM / 1e12:.1f} TB/s streaming rate ({1e6 * least:.1f} us)")
    say(f"patch kernel alone: {1e6 * t_pa:.1f} us per batch of {P} views ({P * hp * hp * 4 / 1e6:.2f} MB written; a gather of the crop, "
        f"launch-sized)")


def _step(ds, plan, say, steps=30):
    import MASIC  # noqa: F401
    import model
    from masic_amd import nn as mnn, trainrun
    from masic_amd.train import make_optimizers, train_step
    net = trainrun.default_init(device="cuda").train()
    torch.manual_seed(0)
    udh = model.Net().cuda().eval()
    opt, aopt = make_optimizers(net)
    mnn.set_precision("bf16")
    try:
        def one(index, draws, with_batch):
            b = ds.batch(index, draws=draws) if with_batch else fixed
            train_step(net, opt, aopt, b.d1, b.d2, b.h_matrix(udh), 0.0932)
        fixed = ds.batch(*plan[0])
        res = {}
        for with_batch in (False, True, False, True):
            for item in plan[:5]:
                one(*item, with_batch)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            a.record()
            for item in plan[:steps]:
                one(*item, with_batch)
            e.record()
            torch.cuda.synchronize()
            res.setdefault(with_batch, []).append((a.elapsed_time(e) / steps, 1e3 * (time.perf_counter() - t) / steps))
        for with_batch, label in ((False, "step on one resident batch      "), (True, "step with a fresh batch each time")):
            say(f"{label}: " + ", ".join(f"{d:.2f} ms device / {w:.2f} ms wall" for d, w in res[with_batch]))
        return min(w for _, w in res[False])
    finally:
        mnn.set_precision("f32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data: needs an MI355X; nothing is measured without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.perf_counter()
    ds = _dataset(args.pairs)
    torch.cuda.synchronize()
    say(f"dataset: {len(ds)} pairs of {H0} x {W0}, arena {ds.nbytes / 1e6:.0f} MB (built from arrays in {time.perf_counter() - t:.1f} s); "
        f"batch = {B} pairs cropped to {CROP[0]} x {CROP[1]}, {args.iters} batches a run, {args.runs} runs alternating the two paths")
    plan = _plan(ds, args.iters)
    flat = ds.offsets.reshape(-1)
    views = [ds.arena[int(o):int(o) + H0 * W0 * 3].view(H0, W0, 3) for o in flat]
    new = lambda index, draws: ds.batch(index, draws=draws)
    old = _pair_prep_batch(ds, views)
    for index, draws in plan[:4]:                                      # the two paths give the same bits
        b, o = new(index, draws), old(index, draws)
        assert all(torch.equal(x, y) for x, y in zip(b[:4], o)), "the two paths differ"
    say("the two paths agree bit for bit on the first 4 batches")
    res = {"new": [], "old": []}
    for _ in range(args.runs):
        res["new"].append(_timed_loop(new, plan))
        res["old"].append(_timed_loop(old, plan))
    med = {k: (statistics.median(d for d, _ in v), statistics.median(w for _, w in v)) for k, v in res.items()}
    for k, label in (("new", "DeviceStereoFolder.batch (2 launches + 2 small copies)"), ("old", f"ops.pair_prep x {2 * B} + 4 stacks ({4 * B + 4} launches)    ")):
        say(f"{label}: device {med[k][0]:.1f} us per batch, host loop {med[k][1]:.1f} us per batch = {1e6 / med[k][1]:.0f} batches/s "
            f"({B * 1e6 / med[k][1]:.0f} pairs/s); runs: " + ", ".join(f"{d:.1f}/{w:.1f}" for d, w in res[k]))
    say(f"ratio old / new: device {med['old'][0] / med['new'][0]:.1f} x, host loop {med['old'][1] / med['new'][1]:.1f} x")
    _kernels_alone(ds, plan, say)
    if args.step:
        step_ms = _step(ds, plan, say)
        say(f"a batch is {100 * med['new'][1] / 1e3 / step_ms:.2f} % of the {step_ms:.2f} ms step it feeds by its host loop time, "
            f"{100 * med['new'][0] / 1e3 / step_ms:.2f} % by its device time (before: {100 * med['old'][1] / 1e3 / step_ms:.1f} % / "
            f"{100 * med['old'][0] / 1e3 / step_ms:.1f} %)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
