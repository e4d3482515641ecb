"""Times the UDH homography net (coremasic/mywork/model.py: 13 HIP launches) against what a user had before it existed: the same
architecture as a stock float32 torch.nn.Sequential (nn.Conv2d / MaxPool2d / Linear -> MIOpen, ATen, rocBLAS) on the same GPU.

At patch size 128 and B = 8 and B = 1: the new forward, the same forward replayed as a captured graph, and the stock baseline.  The
three are alternated inside one process; a sample is `--inner` back-to-back calls between two device events, and the figure is the
median of `--samples` (>= 20) samples per variant, with the spread (min - max).  Nothing is tuned on either side: torch's defaults
(MIOpen's find mode included) are what a user gets.

Linear 1's weight stream: udh_fc alone (its partial-sum kernel, the finishing kernel and two allocations), bytes = the float32
weight (134 MB at patch 128), (a) called back to back -- 134 MB fits the 256 MB Infinity Cache, so this is partly a cache figure --
and (b) after a 1 GB sweep that evicts it, which is how the layer meets its weight inside a codec step.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import model as udh  # noqa: E402
from masic_amd import ops  # noqa: E402


class StockNet(nn.Module):
    """The reference architecture in stock torch modules (eval mode: the Dropout layers are identities and are left out)."""

    def __init__(self, patch_size):
        super().__init__()
        layers, cin = [], 2
        for cout, pool in ((64, True), (64, True), (128, True), (128, False)):
            layers += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(), nn.Conv2d(cout, cout, 3, padding=1), nn.ReLU()]
            if pool:
                layers.append(nn.MaxPool2d(2, 2))
            cin = cout
        layers += [nn.Flatten(), nn.Linear(128 * (patch_size // 8) ** 2, 1024), nn.ReLU(), nn.Linear(1024, 8)]
        self.seq = nn.Sequential(*layers)

    def forward(self, a, b):
        return self.seq(torch.cat((a, b), dim=1)).view(-1, 4, 2)


def copy_weights(net, stock):
    src = [t for _, t in net.state_dict().items()]
    dst = [t for _, t in stock.state_dict().items()]
    assert len(src) == len(dst) == 20
    with torch.no_grad():
        for s, d in zip(src, dst):
            d.copy_(s)


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
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples must be at least 20")
    dev = "cuda"
    torch.manual_seed(0)
    p = args.patch
    net = udh.Net(patch_size=p).to(dev).eval()
    stock = StockNet(p).to(dev).eval()
    copy_weights(net, stock)
    l1, l2 = net.fc[2], net.fc[5]
    wbytes = l1.weight.numel() * 4
    flush = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev)

    for B in args.batches:
        a = torch.randn(B, 1, p, p, device=dev)
        b = torch.randn(B, 1, p, p, device=dev)
        with torch.no_grad():
            for _ in range(args.warmup):
                new, ref = net(a, b), stock(a, b)
            dev_rel = float((new - ref).abs().max() / ref.abs().max())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                net(a, b)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gout = net(a, b)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gout, new)
            variants = {"udh_hip": lambda: net(a, b), "udh_hip_graph": graph.replay, "stock_torch": lambda: stock(a, b)}
            times = {k: [] for k in variants}
            for _ in range(args.samples):
                for k, fn in variants.items():
                    times[k].append(sample(fn, args.inner))
            recs = {k: summary(k, v, B=B, patch=p) for k, v in times.items()}
            print(json.dumps({"name": "udh_vs_stock", "B": B, "patch": p, "max_deviation_of_peak": dev_rel,
                              "hip_over_stock": round(recs["udh_hip"]["median_ms"] / recs["stock_torch"]["median_ms"], 4),
                              "graph_over_stock": round(recs["udh_hip_graph"]["median_ms"] / recs["stock_torch"]["median_ms"], 4)}), flush=True)

            x = net.features(a, b)[-1]
            fc = lambda: ops.udh_fc(x, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach())  # noqa: E731
            stock_fc = lambda: stock.seq[-1](torch.relu(stock.seq[-3](x.view(B, -1))))  # noqa: E731
            warm = [sample(fc, args.inner) for _ in range(args.samples)]
            warm_stock = [sample(stock_fc, args.inner) for _ in range(args.samples)]
            cold, cold_stock = [], []
            for _ in range(args.samples):
                flush.fill_(1.0)
                cold.append(sample(fc, 1))
                flush.fill_(1.0)
                cold_stock.append(sample(stock_fc, 1))
            for name, ms in (("linear_hip_back_to_back", warm), ("linear_stock_back_to_back", warm_stock),
                             ("linear_hip_after_sweep", cold), ("linear_stock_after_sweep", cold_stock)):
                summary(name, ms, B=B, patch=p, weight_bytes=wbytes,
                        weight_TB_per_s=round(wbytes / (statistics.median(ms) * 1e-3) / 1e12, 3))


if __name__ == "__main__":
    main()
