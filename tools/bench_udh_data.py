"""What a UDH training batch costs when it is cut on the GPU (DeviceStereoFolder.udh_batch; run on the GPU box):

  1. udh_batch: 8 pairs, pic_size 256, patch 128, rho 45, out of synthetic 860 x 1080 pictures (InStereo2K's size); every batch takes other
     pairs at other windows.  Device time (events around --iters batches issued back to back) and host-loop time (the host clock around the
     same loop ending in a synchronise).
  2. The two launches alone, descriptors already on the device: 8 views of 256 x 256 (img_a), 16 views of 128 x 128 (the patches).
  3. The same batch made by the host chain the reference uses -- PIL resize, crop, normalise, grey, windows (tests/udh_data_ref.py) -- on
     this process's CPUs (a thread pool over the 16 pictures of a batch; PIL releases the GIL while it resamples), stacked and uploaded.
     The pictures are decoded already, which favours the host chain: the reference also opens and decodes two PNGs per item.
     The two paths are compared bit for bit first.
  4. One UDH training step at the same batch (udh_train.Net(128), photometric loss, backward, Adam: the udh_hip_step_adam figure of
     tools/bench_udh_train.py), and each batch time as a share of it.

  python tools/bench_udh_data.py [--pairs 24] [--iters 100] [--host-iters 5] [--samples 20] [--out profiles/udh_data_bench.txt]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from masic_amd import data, ops, udh_data, udh_train  # noqa: E402
from masic_amd._lib import check, lib  # noqa: E402
from tests import udh_data_ref as R  # noqa: E402

H0, W0, B, S, P, RHO = 860, 1080, 8, 256, 128, 45


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_udh_data: needs an MI355X; nothing is measured without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    lefts = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(args.pairs)]
    rights = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(args.pairs)]
    ds = data.DeviceStereoFolder.from_arrays(lefts, rights, patch_size=(256, 256), seed=0)
    cpus = max(1, min(16, len(os.sched_getaffinity(0))))
    say(f"dataset: {len(ds)} pairs of {H0} x {W0}, arena {ds.nbytes / 1e6:.0f} MB; batch = {B} pairs, pic_size {S}, patch {P}, rho {RHO}; "
        f"{args.iters} batches a run, {args.runs} runs; host chain on {cpus} threads")
    prng, order, plan = random.Random(1), [], []
    for _ in range(args.iters):
        if len(order) < B:
            more = list(range(len(ds)))
            prng.shuffle(more)
            order += more
        index, order = order[:B], order[B:]
        plan.append((index, udh_data.draw_udh_items(prng, B, S, P, RHO)))
    ds.udh_tables(S)

    def device_batch(index, draws):
        return ds.udh_batch(index, draws=draws, pic_size=S, patch_size=P, rho=RHO)

    pool = ThreadPoolExecutor(cpus)

    def host_batch(index, draws):
        def view(k):
            i, side = divmod(k, 2)
            g = R.grey_picture((lefts, rights)[side][index[i]], S)
            x, y = draws[i]
            return g, g[:, y:y + P, x:x + P]
        views = list(pool.map(view, range(2 * B)))
        img_a = torch.stack([views[2 * i][0] for i in range(B)]).pin_memory().to("cuda", non_blocking=True)
        patch_a = torch.stack([views[2 * i][1] for i in range(B)]).pin_memory().to("cuda", non_blocking=True)
        patch_b = torch.stack([views[2 * i + 1][1] for i in range(B)]).pin_memory().to("cuda", non_blocking=True)
        corners = torch.from_numpy(udh_data.corners_of(draws, P)).pin_memory().to("cuda", non_blocking=True)
        return img_a, patch_a, patch_b, corners

    for index, draws in plan[:2]:
        b, h = device_batch(index, draws), host_batch(index, draws)
        assert all(torch.equal(x, y) for x, y in zip((b.img_a, b.patch_a, b.patch_b, b.corners), h)), "the two paths differ"
    say("the device batch and the host chain agree bit for bit on the first 2 batches")

    dev_runs = [_timed_loop(device_batch, plan) for _ in range(args.runs)]
    dev_us, host_us = statistics.median(d for d, _ in dev_runs), statistics.median(w for _, w in dev_runs)
    say(f"udh_batch (2 launches + 2 small copies): device {dev_us:.1f} us per batch, host loop {host_us:.1f} us per batch = "
        f"{1e6 / host_us:.0f} batches/s; runs: " + ", ".join(f"{d:.1f}/{w:.1f}" for d, w in dev_runs))

    # the two launches alone
    pp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tables = ds.udh_tables(S)
    st = ops._stream()
    descs = []
    for index, draws in plan:
        sizes = [ds.sizes[i] for i in index]
        left, right = [int(ds.offsets[i, 0]) for i in index], [int(ds.offsets[i, 1]) for i in index]
        full = ops.check_udh_view_descriptors(tables.rows(left, sizes, [(0, 0)] * B), ds.arena.numel(), tables.words.numel(), (S, S), S)
        win = ops.check_udh_view_descriptors(tables.rows(left + right, sizes * 2, list(draws) * 2), ds.arena.numel(), tables.words.numel(), (P, P), S)
        descs.append((torch.from_numpy(ops.pack_udh_view_descriptors(full)).cuda(), torch.from_numpy(ops.pack_udh_view_descriptors(win)).cuda()))
    imgs, patches = torch.empty((B, 1, S, S), device="cuda"), torch.empty((2 * B, 1, P, P), device="cuda")

    def events(which):
        def call(d):
            if which == 0:
                check(lib.masic_udh_views_prep(pp(ds.arena), ds.arena.numel(), pp(tables.words), tables.words.numel(), pp(d[0]), B, S, S, S, pp(imgs), st))
            else:
                check(lib.masic_udh_views_prep(pp(ds.arena), ds.arena.numel(), pp(tables.words), tables.words.numel(), pp(d[1]), 2 * B, P, P, S, pp(patches), st))
        for d in descs[:3]:
            call(d)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for d in descs:
            call(d)
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / len(descs)

    k_img = statistics.median(events(0) for _ in range(args.runs))
    k_pat = statistics.median(events(1) for _ in range(args.runs))
    say(f"kernel alone: {B} views of {S} x {S}: {k_img:.1f} us; {2 * B} views of {P} x {P}: {k_pat:.1f} us; together {k_img + k_pat:.1f} us per batch")

    host_plan = plan[:max(args.host_iters, 4)]
    _, chain_us = _timed_loop(host_batch, host_plan)
    say(f"host chain (PIL, {cpus} threads, pictures decoded already, + upload): {chain_us / 1e3:.2f} ms per batch = {chain_us / host_us:.0f} x the host loop "
        f"of udh_batch")

    # the training step the batch feeds
    torch.manual_seed(0)
    net = udh_train.Net(patch_size=P).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, foreach=False, fused=False)
    fixed = device_batch(*plan[0])

    def step(b):
        net.zero_grad(set_to_none=True)
        loss = udh_train.photometric_loss(net(b.patch_a, b.patch_b), b.img_a, b.patch_b, b.corners)
        loss.backward()
        opt.step()

    def sample(fn, inner=3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        for k in range(inner):
            fn(k)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner, 1e3 * (time.perf_counter() - t) / inner

    for k in range(3):
        step(fixed)
    resident = [sample(lambda k: step(fixed)) for _ in range(args.samples)]
    fresh = [sample(lambda k: step(device_batch(*plan[(3 * j + k) % len(plan)]))) for j in range(args.samples)]
    step_ms = statistics.median(d for d, _ in resident)
    say(f"UDH training step (Net({P}), B = {B}, loss, backward, Adam) on one resident batch: device {step_ms:.3f} ms (min {min(d for d, _ in resident):.3f}, "
        f"max {max(d for d, _ in resident):.3f}), wall {statistics.median(w for _, w in resident):.3f} ms; with a fresh udh_batch each step: device "
        f"{statistics.median(d for d, _ in fresh):.3f} ms, wall {statistics.median(w for _, w in fresh):.3f} ms")
    say(f"share of the step: udh_batch {100 * dev_us / 1e3 / step_ms:.2f} % by device time, {100 * host_us / 1e3 / step_ms:.2f} % by host loop time; "
        f"the host chain {100 * chain_us / 1e3 / step_ms:.0f} %")
    print(json.dumps({"name": "udh_data_bench", "B": B, "pic_size": S, "patch": P, "batch_device_us": round(dev_us, 2), "batch_host_us": round(host_us, 2),
                      "kernel_img_us": round(k_img, 2), "kernel_patch_us": round(k_pat, 2), "host_chain_ms": round(chain_us / 1e3, 3),
                      "step_ms": round(step_ms, 4)}), flush=True)
    pool.shutdown()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
