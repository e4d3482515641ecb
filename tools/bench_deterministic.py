"""Cost of the deterministic mode (masic_amd/determinism.py): the HSIC training step (masic_amd.train.train_step, HSIC(128,192,5), bf16
operands) and the CQE training step (masic_amd.train.cqe_train_step) at 8 x 3 x 512 x 512, with the mode off and on.

Per step and mode: the median of five windows of `--steps` steps after `--warmup` steps (device events), and the deterministic
workspace the wrappers hold per stream afterwards.  `--only default|det` times one mode (for a kernel trace of it under
`rocprofv3 --kernel-trace --stats`); `--stats FILE [FILE]` instead summarises such traces (the rocpd results.db, or a kernel_stats.csv):
launches per step and the time of the weight-gradient kernels per step (`--steps-traced` = warmup + 5 x steps of the traced run)."""
import argparse
import csv
import json
import os
import re
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "coremasic", "mywork"))

WGRAD = ("conv_wgrad", "wgrad3x3_f16k", "wgrad1x1_f16k", "wgrad_pic", "wgrad_small", "wgrad_transpose", "wgrad3_transpose",
         "wgrad_slab_transpose", "wgrad1x1_finish", "warp_bwd", "warp_det")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) / steps)
    return sorted(res)[2]


def steps():
    import MASIC
    from masic_amd import nn as mnn, synth
    from masic_amd.train import cqe_train_step, make_optimizers, train_step
    mnn.set_precision("bf16")
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=100))
    net = net.cuda().train()
    x1, x2, hm = (t.cuda() for t in synth.synth_inputs(8, 512, 512, seed=100))
    opt, aopt = make_optimizers(net, fused=True)
    hsic = lambda: train_step(net, opt, aopt, x1, x2, hm, 0.01)
    net_e = MASIC.HSIC(128, 192, 5)
    net_e.load_state_dict(synth.synth_state_dict(net_e.state_dict(), seed=100))
    net_e = net_e.cuda().eval()
    en = MASIC.Independent_EN()
    en.load_state_dict(synth.synth_state_dict(en.state_dict(), seed=101))
    en = en.cuda().train()
    eopt = torch.optim.Adam(list(en.parameters()), lr=1e-4, fused=True)
    cqe = lambda: cqe_train_step(net_e, en, eopt, x1, x2, hm, 0.01)
    return {"hsic_train_step": hsic, "cqe_train_step": cqe}


def stats(files, n_steps):
    """kernel_stats.csv (rocprofv3 --stats) -> launches per step and the weight-gradient kernels' time per step"""
    out = {}
    for f in files:
        if f.endswith(".db"):
            rows = [{"Name": n, "Calls": 1, "TotalDurationNs": e - s} for n, s, e in sqlite3.connect(f).execute("select name, start, end from kernels")]
        else:
            rows = list(csv.DictReader(open(f)))
        calls = sum(int(r["Calls"]) for r in rows)
        kern = {}
        for r in rows:
            name = re.sub(r"\(.*", "", r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")).strip()
            if any(k in r["Name"] for k in WGRAD):
                k = kern.setdefault(name, [0, 0.0])
                k[0] += int(r["Calls"])
                k[1] += float(r["TotalDurationNs"]) / 1e3
        out[f] = {"launches_per_step": round(calls / n_steps, 1),
                  "wgrad_kernels_us_per_step": {k: {"calls": round(v[0] / n_steps, 1), "us": round(v[1] / n_steps, 1)}
                                                for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("default", "det"), default=None)
    ap.add_argument("--which", choices=("hsic_train_step", "cqe_train_step"), action="append", default=None)
    ap.add_argument("--stats", nargs="+", default=None)
    ap.add_argument("--steps-traced", type=int, default=0)
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats, a.steps_traced), indent=1))
        return
    from masic_amd import ops
    from masic_amd.determinism import deterministic
    fns = steps()
    for name in a.which or list(fns):
        row = {"step": name, "shape": "8x3x512x512", "operands": "bf16"}
        for mode in ("default", "det"):
            if a.only not in (None, mode):
                continue
            ops._WS.clear()
            torch.cuda.empty_cache()
            with deterministic(mode == "det"):
                row[mode + "_ms"] = round(timed(fns[name], a.steps, a.warmup), 2)
            if mode == "det":
                per = ops.det_workspace_bytes()
                row["det_workspace_MiB_per_stream"] = {str(k[1]): round(v / 2 ** 20, 1) for k, v in per.items()}
                row["det_largest_layer_MiB"] = round(max(ws.numel() * 4 for k, ws in ops._WS.items() if k[0] == "det") / 2 ** 20, 1)
        if "default_ms" in row and "det_ms" in row:
            row["det_over_default"] = round(row["det_ms"] / row["default_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
