#!/usr/bin/env python3
"""Train the homography net (UDH) on a folder of stereo pictures: the loop of the reference's udh/udh/train.py without Lightning --
HomographyModel.training_step (delta = model(patch_a, patch_b); photometric_loss(delta, img_a, patch_b, corners)) and its Adam -- on this
library: the pictures decoded once into device memory (masic_amd.data.DeviceStereoFolder), every batch of the reference's
SyntheticDataset cut from them by two launches (udh_batches), the net and the loss of masic_amd/udh_train.py.

    python tools/train_udh_folder.py -d /data/instereo2k [--split train --pic-size 256 --patch-size 128 --rho 45 --batch-size 8
        --epochs 1 --steps N -lr 1e-4 --seed 0 --save homo_best.pth.tar]

<dataset>/<split>/left/* and <dataset>/<split>/right/* pair up by name.  --save writes {'state_dict': net.state_dict()}: the 20 tensors
coremasic/mywork/model.py:Net loads with load_state_dict, and the file tools/train_folder.py --homopath reads."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-d", "--dataset", required=True)
    ap.add_argument("-da", "--dataset-add", default="")
    ap.add_argument("--split", default="train")
    ap.add_argument("--pic-size", type=int, default=256)
    ap.add_argument("--patch-size", type=int, default=128)
    ap.add_argument("--rho", type=int, default=45)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="stop after this many steps (0: run the epochs)")
    ap.add_argument("-lr", "--learning-rate", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-bytes", type=int, default=64 << 30)
    ap.add_argument("--save", default=None, help="write {'state_dict': ...} of the trained net here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_udh_folder: needs an MI355X -- the library has no CPU path")
    from masic_amd import data, udh_train
    device = torch.device("cuda", 0)
    t = time.perf_counter()
    ds = data.DeviceStereoFolder(args.dataset, args.split, patch_size=(1, 1), root_add=args.dataset_add, seed=args.seed, device=device,
                                 max_bytes=args.max_bytes)      # (the codec-side crop is not used here; 1 x 1 fits every picture)
    print(f"{len(ds)} pairs, {ds.nbytes / 1e6:.0f} MB on the device ({time.perf_counter() - t:.1f} s)")
    if len(ds) < args.batch_size:
        raise SystemExit(f"train_udh_folder: {len(ds)} pairs do not fill a batch of {args.batch_size}")
    torch.manual_seed(args.seed)
    net = udh_train.Net(patch_size=args.patch_size).to(device).train()
    optimizer = torch.optim.Adam(net.parameters(), lr=args.learning_rate)          # train.py: configure_optimizers
    kw = dict(pic_size=args.pic_size, patch_size=args.patch_size, rho=args.rho)
    per_epoch = len(ds) // args.batch_size
    step, t, loss = 0, time.perf_counter(), None
    for epoch in range(args.epochs):
        for i, b in enumerate(ds.udh_batches(args.batch_size, **kw)):
            optimizer.zero_grad()
            delta = net(b.patch_a, b.patch_b)
            loss = udh_train.photometric_loss(delta, b.img_a, b.patch_b, b.corners)
            loss.backward()
            optimizer.step()
            if i % 10 == 0:
                print(f"Train epoch {epoch}: [{i * args.batch_size}/{len(ds)} ({100. * i / per_epoch:.0f}%)]\tLoss: {loss.item():.5f}", flush=True)
            step += 1
            if args.steps and step >= args.steps:
                break
        if args.steps and step >= args.steps:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    print(f"{step} steps in {dt:.1f} s ({1e3 * dt / max(step, 1):.1f} ms a step, {step * args.batch_size / dt:.0f} pairs/s), last loss {loss.item():.5f}")
    if args.save:
        torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "steps": step}, args.save)
        print("saved", args.save)


if __name__ == "__main__":
    main()
