"""Times one training step of the UDH homography net (udh/udh/model.py -> masic_amd/udh_train.py) against what a user had before
it existed: the same net as stock float32 torch modules (MIOpen, ATen, rocBLAS; Dropout included) with the plain-torch photometric
loss of tests/udh_train_ref.py, autograd and the same optimizer, on the same GPU.

At patch size 128, B = 8 and B = 32: forward + loss + backward, and the same with Adam.step() (unfused), for both sides.  The
variants are alternated inside one process; a sample is `--inner` back-to-back steps between two device events, and the figure is
the median of `--samples` (>= 20) samples per variant, with the spread (min - max) -- the method of tools/bench_udh.py.  Nothing is
tuned on either side.  If stock convolutions are not available on the machine the baseline is skipped with a message.

The linear-backward launch on its own (ops.udh_fc_bwd: the head kernel, the streaming pass over Linear 1's weight, six
allocations): bytes = one read plus one write of the float32 weight (268 MB at patch 128), (a) called back to back and (b) after a
1 GB sweep that evicts the weight from the 256 MB Infinity Cache.  One JSON line per figure."""
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
from masic_amd import ops, udh_train  # noqa: E402
from tests import udh_train_ref as TR  # noqa: E402


class StockNet(nn.Module):
    """The reference architecture in stock torch modules, Dropout layers included (they are active in training mode)."""

    def __init__(self, patch_size):
        super().__init__()
        layers, cin = [], 2
        for cout, pool in ((64, True), (64, True), (128, True), (128, False)):
            layers += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(), nn.Conv2d(cout, cout, 3, padding=1), nn.ReLU()]
            if pool:
                layers.append(nn.MaxPool2d(2, 2))
            cin = cout
        layers += [nn.Flatten(), nn.Dropout(0.5), nn.Linear(128 * (patch_size // 8) ** 2, 1024), nn.ReLU(), nn.Dropout(0.5), nn.Linear(1024, 8)]
        self.seq = nn.Sequential(*layers)

    def forward(self, a, b):
        return self.seq(torch.cat((a, b), dim=1)).view(-1, 4, 2)


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


def make_step(net, loss_fn, batch, opt):
    a, b, img, pb, corners = batch

    def step():
        net.zero_grad(set_to_none=True)
        loss = loss_fn(net(a, b), img, pb, corners)
        loss.backward()
        if opt is not None:
            opt.step()
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-stock", action="store_true")
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples must be at least 20")
    dev = "cuda"
    torch.manual_seed(0)
    p = args.patch
    img_hw = (p + p // 4, p + p // 8)
    net = udh_train.Net(patch_size=p).to(dev).train()
    stock = None
    if not args.no_stock:
        try:
            stock = StockNet(p).to(dev).train()
            with torch.no_grad():
                for s, d in zip(net.state_dict().values(), stock.state_dict().values()):
                    d.copy_(s)
            stock(torch.zeros(1, 1, p, p, device=dev), torch.zeros(1, 1, p, p, device=dev)).sum().backward()
        except Exception as e:  # noqa: BLE001
            print(json.dumps({"name": "stock_torch", "skipped": f"stock convolutions are not available here: {type(e).__name__}: {e}"[:300]}), flush=True)
            stock = None
    l1, l2 = net.fc[2], net.fc[5]
    wbytes = l1.weight.numel() * 4
    flush = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev)

    for B in args.batches:
        a = torch.randn(B, 1, p, p, device=dev)
        b = torch.randn(B, 1, p, p, device=dev)
        img, pb, corners = (t.to(dev) for t in TR.loss_inputs(range(100, 100 + B), img_hw, (p, p), 10.0))
        batch = (a, b, img, pb, corners)
        variants = {"udh_hip_step": make_step(net, udh_train.photometric_loss, batch, None),
                    "udh_hip_step_adam": make_step(net, udh_train.photometric_loss, batch, torch.optim.Adam(net.parameters(), lr=1e-4, foreach=False, fused=False))}
        if stock is not None:
            variants["stock_torch_step"] = make_step(stock, TR.photometric_loss, batch, None)
            variants["stock_torch_step_adam"] = make_step(stock, TR.photometric_loss, batch,
                                                          torch.optim.Adam(stock.parameters(), lr=1e-4, foreach=False, fused=False))
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.samples):
            for k, fn in variants.items():
                times[k].append(sample(fn, args.inner))
        recs = {k: summary(k, v, B=B, patch=p) for k, v in times.items()}
        if stock is not None:
            print(json.dumps({"name": "udh_train_vs_stock", "B": B, "patch": p,
                              "hip_over_stock": round(recs["udh_hip_step"]["median_ms"] / recs["stock_torch_step"]["median_ms"], 4),
                              "hip_over_stock_adam": round(recs["udh_hip_step_adam"]["median_ms"] / recs["stock_torch_step_adam"]["median_ms"], 4)}),
                  flush=True)

        K, N = l1.weight.shape[1], l1.weight.shape[0]
        x = torch.randn(B, K, device=dev)
        m1, m2 = net.draw_masks(B, dev)
        w1, b1, w2, b2 = l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach()
        xd, hidden, _ = ops.udh_fc_train(x, w1, b1, w2, b2, m1, m2)
        gout = torch.randn(B, 8, device=dev)
        bwd = lambda: ops.udh_fc_bwd(gout, xd, hidden, w1, w2, m1, m2)  # noqa: E731
        warm = [sample(bwd, args.inner) for _ in range(args.samples)]
        cold = []
        for _ in range(args.samples):
            flush.fill_(1.0)
            cold.append(sample(bwd, 1))
        for name, ms in (("linear_bwd_back_to_back", warm), ("linear_bwd_after_sweep", cold)):
            summary(name, ms, B=B, patch=p, bytes=2 * wbytes, TB_per_s=round(2 * wbytes / (statistics.median(ms) * 1e-3) / 1e12, 3))


if __name__ == "__main__":
    main()
