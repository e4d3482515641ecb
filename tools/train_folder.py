#!/usr/bin/env python3
"""Train the codec stage on a folder of stereo pictures: the loop of the reference's driver (coremasic/mywork/newtrain_codec_real.py:
105-161, train_epoch) on this library -- the pictures decoded once into device memory (masic_amd.data.DeviceStereoFolder), every batch
cut from them by two launches, h_matrix from the frozen homography net, one masic_amd.train.train_step per batch.

    python tools/train_folder.py -d /data/instereo2k [--split train --patch-size 512 512 --batch-size 8 --steps 300 --lambda 0.01
        --homopath homo_best.pth.tar --dataset-add DIR --precision bf16 --seed 0 --band-rows S --save checkpoint.pth.tar]

<dataset>/<split>/left/* and <dataset>/<split>/right/* pair up by name, as the reference's ImageFolder lists them.  The log line is the
reference's, every 10th iteration.  --homopath: a checkpoint of the reference's HomographyModel ({'state_dict': ...}, keys 'model.*');
without one the net keeps its initialisation, as the reference's driver goes on "homo from none".  --band-rows S: train for files coded
with compress(..., band_rows=S) -- HSIC.band_rows = S, the context models of the training graph do not see across the top edge of a
band of S latent rows (0, the default: the unbanded model)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def load_homography_net(path, patch_size, device):
    import model
    net = model.Net(patch_size=patch_size)
    print("intput homopath:", path)
    if path and os.path.exists(path):
        state = torch.load(path, map_location="cpu")
        state = state.get("state_dict", state)
        net.load_state_dict({(k[len("model."):] if k.startswith("model.") else k): v for k, v in state.items()})
        print("load homo model ok")
    else:
        print("homo from none")
    return net.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-d", "--dataset", required=True)
    ap.add_argument("-da", "--dataset-add", default="")
    ap.add_argument("--split", default="train")
    ap.add_argument("--patch-size", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lambda", dest="lmbda", type=float, default=1e-2)
    ap.add_argument("-lr", "--learning-rate", type=float, default=1e-4)
    ap.add_argument("--aux-learning-rate", type=float, default=1e-3)
    ap.add_argument("--homopath", default="homo_best.pth.tar")
    ap.add_argument("--precision", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-bytes", type=int, default=64 << 30)
    ap.add_argument("--band-rows", type=int, default=0, help="HSIC.band_rows while training: the row bands of the files the model is trained for")
    ap.add_argument("--save", default=None, help="write {'state_dict': ...} of the trained codec here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_folder: needs an MI355X -- the library has no CPU path")
    import MASIC
    from masic_amd import data, nn as mnn
    from masic_amd.train import make_optimizers, train_step
    device = torch.device("cuda", 0)
    t = time.perf_counter()
    ds = data.DeviceStereoFolder(args.dataset, args.split, tuple(args.patch_size), root_add=args.dataset_add, seed=args.seed, device=device,
                                 max_bytes=args.max_bytes)
    print(f"{len(ds)} pairs, {ds.nbytes / 1e6:.0f} MB on the device, crops of {ds.crop[0]} x {ds.crop[1]} ({time.perf_counter() - t:.1f} s)")
    if len(ds) < args.batch_size:
        raise SystemExit(f"train_folder: {len(ds)} pairs do not fill a batch of {args.batch_size}")
    nethomo = load_homography_net(args.homopath, ds.homopatch, device)
    torch.manual_seed(args.seed)
    net = MASIC.HSIC(N=128, M=192, K=5).to(device).train()
    net.band_rows = args.band_rows
    optimizer, aux_optimizer = make_optimizers(net, lr=args.learning_rate, aux_lr=args.aux_learning_rate)
    print("lambda:", args.lmbda)
    per_epoch = len(ds) // args.batch_size
    mnn.set_precision(args.precision)
    step, epoch, t = 0, 0, time.perf_counter()
    try:
        while step < args.steps:
            for i, b in enumerate(ds.batches(args.batch_size)):
                out_criterion, aux_loss = train_step(net, optimizer, aux_optimizer, b.d1, b.d2, b.h_matrix(nethomo), args.lmbda)
                if i % 10 == 0:
                    print(f'Train epoch {epoch}: ['
                          f'{i * args.batch_size}/{len(ds)}'
                          f' ({100. * i / per_epoch:.0f}%)]'
                          f'\tLoss: {out_criterion["loss"].item():.3f} |'
                          f'\tMSE loss: {out_criterion["mse_loss"].item():.5f} |'
                          f'\tBpp loss: {out_criterion["bpp_loss"].item():.2f} |'
                          f'\tAux loss: {aux_loss.item():.2f}', flush=True)
                step += 1
                if step >= args.steps:
                    break
            epoch += 1
    finally:
        mnn.set_precision("f32")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    print(f"{step} steps in {dt:.1f} s ({1e3 * dt / step:.1f} ms a step, {step * args.batch_size / dt:.0f} pairs/s)")
    if args.save:
        torch.save({"state_dict": net.state_dict(), "steps": step, "lambda": args.lmbda, "band_rows": net.band_rows}, args.save)


if __name__ == "__main__":
    main()
