#!/usr/bin/env python3
"""Evaluate a codec checkpoint on a folder's test split: the reference's test drivers (coremasic/mywork/test2_real.py, test3_real.py)
on this library -- masic_amd.evaluate.evaluate_folder (rate from the likelihoods) or, with --files, evaluate_files (real .msf files).

    python tools/eval_folder.py -d /data/instereo2k --checkpoint checkpoint.pth.tar [--homopath homo_best.pth.tar | --aligner]
        [--cqe second_checkpoint.pth.tar] [--split test] [--patch-size 256 256] [--batch-size 8] [--files] [--band-rows S] [--model-band-rows S]
        [--refine-steps K --refine-lmbda L [--refine-lr R] [--refine-budget-bpp X | --refine-budget-rel X]] [--precision bf16] [--lpips-weights alex.pth] [--json report.json] [--timing]

--checkpoint: what tools/train_folder.py --save writes ({'state_dict': ...} of MASIC.HSIC; --nmk for another width than 128 192 5).
--aligner: masic_amd.align.PatchAligner in place of a trained homography net.  The line printed is Report.line(): fields 'Label: value'
separated by '|' after 'Test epoch 0:'.  --json: the per-pair table.  --timing: the device time of evaluate.pair_metrics on one batch
beside that of the B per-slice loss.rate_distortion calls it replaces.  --refine-steps (with --files): the encoder refines every pair's
latents for that many Adam steps before coding (masic_amd.refine; --refine-lmbda: the rate-distortion weight the checkpoint was
trained with, --refine-lr: Adam's step size, default the library's).  --refine-budget-bpp X: every pair may cost at most X estimated
bits per pixel of its padded size; --refine-budget-rel X: at most X times the estimated bits of its unrefined latents (1.0: refine, but
never to more bits) -- RefineConfig's budget_bpp / budget_rel.  --band-rows S: how --files codes (StereoCodec's band_rows).
--model-band-rows S, in either mode: HSIC.band_rows = S, the file the model ESTIMATES -- the rate evaluate_folder reports, and the rate
the refinement and its budget descend and constrain, are those of files coded with band_rows = S."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _state(path):
    state = torch.load(path, map_location="cpu")
    return state.get("state_dict", state)


def time_pair_metrics(hsic, homo, ds, batch_size, reps=20):
    """(ms of one pair_metrics call, ms of the B per-slice rate_distortion calls) on the first batch's forward output, device time
    between two events, the median of `reps` after three warm-up rounds"""
    from masic_amd import evaluate
    from masic_amd.loss import rate_distortion
    b = next(ds.batches(batch_size, shuffle=False, drop_last=False))
    B = b.d1.shape[0]
    with torch.no_grad():
        out = hsic(b.d1, b.d2, b.h_matrix(homo))
        out = {"x1_hat": out["x1_hat"].clone(), "x2_hat": out["x2_hat"].clone(),
               "likelihoods": {k: v.clone() for k, v in out["likelihoods"].items()}}
        slices = [({"x1_hat": out["x1_hat"][i:i + 1], "x2_hat": out["x2_hat"][i:i + 1],
                    "likelihoods": {k: v[i:i + 1] for k, v in out["likelihoods"].items()}}, b.d1[i:i + 1], b.d2[i:i + 1]) for i in range(B)]

        def batched():
            evaluate.pair_metrics(out, b.d1, b.d2)

        def per_slice():
            for o, d1, d2 in slices:
                rate_distortion(o, d1, d2, 0.01)

        times = []
        for fn in (batched, per_slice):
            ms = []
            for r in range(reps + 3):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                end.record()
                end.synchronize()
                if r >= 3:
                    ms.append(start.elapsed_time(end))
            times.append(sorted(ms)[len(ms) // 2])
    return B, times[0], times[1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-d", "--dataset", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--nmk", type=int, nargs=3, default=(128, 192, 5), metavar=("N", "M", "K"))
    ap.add_argument("--homopath", default=None)
    ap.add_argument("--aligner", action="store_true")
    ap.add_argument("--cqe", default=None)
    ap.add_argument("--split", default="test")
    ap.add_argument("--patch-size", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--band-rows", type=int, default=0, help="--files: the row bands the files are coded with")
    ap.add_argument("--model-band-rows", type=int, default=0, help="HSIC.band_rows: the row bands of the file the model estimates (and refines for)")
    ap.add_argument("--refine-steps", type=int, default=0, help="--files: Adam steps of encoder-side latent refinement per batch (0: off)")
    ap.add_argument("--refine-lr", type=float, default=None, help="Adam's step size (default: masic_amd.refine.DEFAULT_LR)")
    ap.add_argument("--refine-lmbda", type=float, default=None, help="the rate-distortion weight of the checkpoint; needed with --refine-steps")
    ap.add_argument("--refine-budget-bpp", type=float, default=None, help="with --refine-steps: a pair's estimated bits per pixel at most")
    ap.add_argument("--refine-budget-rel", type=float, default=None, help="with --refine-steps: a pair's estimated bits at most this "
                                                                          "multiple of its unrefined latents'")
    ap.add_argument("--precision", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--metrics", nargs="*", default=None, help="psnr ms_ssim lpips (default: psnr ms_ssim, and lpips with --lpips-weights)")
    ap.add_argument("--lpips-weights", default=None, help="the lin-layer weights (alex.pth) of lpips.LPIPS; the trunk's come from "
                                                          "where lpips.LPIPS looks for them")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-dir", default=None, help="--files: keep the .msf files here")
    ap.add_argument("--json", default=None)
    ap.add_argument("--timing", action="store_true")
    args = ap.parse_args(argv)
    if args.aligner and args.homopath:
        raise SystemExit("eval_folder: --homopath and --aligner exclude each other")
    if args.refine_steps and not args.files:
        raise SystemExit("eval_folder: --refine-steps refines what is coded: it needs --files")
    if args.refine_steps and args.refine_lmbda is None:
        raise SystemExit("eval_folder: --refine-steps needs --refine-lmbda, the rate-distortion weight the checkpoint was trained with")
    if (args.refine_budget_bpp is not None or args.refine_budget_rel is not None) and not args.refine_steps:
        raise SystemExit("eval_folder: --refine-budget-bpp / --refine-budget-rel constrain the refinement: they need --refine-steps")
    if args.refine_budget_bpp is not None and args.refine_budget_rel is not None:
        raise SystemExit("eval_folder: --refine-budget-bpp and --refine-budget-rel exclude each other")
    if not torch.cuda.is_available():
        raise SystemExit("eval_folder: needs an MI355X -- the library has no CPU path")
    import MASIC
    from masic_amd import StereoCodec, data, evaluate, nn as mnn
    device = torch.device("cuda", 0)
    N, M, K = args.nmk
    hsic = MASIC.HSIC(N=N, M=M, K=K)
    hsic.load_state_dict(_state(args.checkpoint))
    hsic = hsic.to(device).eval()
    hsic.update()
    hsic.band_rows = args.model_band_rows
    if args.aligner:
        from masic_amd.align import PatchAligner
        homo = PatchAligner().to(device).eval()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from train_folder import load_homography_net
        homo = load_homography_net(args.homopath, 128, device)
    cqe = None
    if args.cqe:
        cqe = MASIC.Independent_EN()
        cqe.load_state_dict(_state(args.cqe))
        cqe = cqe.to(device).eval()
    lpips_fn = None
    if args.lpips_weights:
        import lpips
        lpips_fn = lpips.LPIPS(net="alex", spatial=False, model_path=args.lpips_weights, verbose=False).to(device).eval()
    metrics = tuple(args.metrics) if args.metrics is not None else ("psnr", "ms_ssim") + (("lpips",) if lpips_fn is not None else ())
    before = mnn.get_precision()
    mnn.set_precision(args.precision)
    try:
        if args.files:
            refine = None
            if args.refine_steps:
                from masic_amd.refine import DEFAULT_LR, RefineConfig
                refine = RefineConfig(steps=args.refine_steps, lr=DEFAULT_LR if args.refine_lr is None else args.refine_lr, lmbda=args.refine_lmbda,
                                      budget_bpp=args.refine_budget_bpp, budget_rel=args.refine_budget_rel)
            codec = StereoCodec(hsic, homo, cqe, band_rows=args.band_rows, refine=refine)
            report = evaluate.evaluate_files(codec, args.dataset, args.split, args.batch_size, enhance=cqe is not None, metrics=metrics,
                                             lpips_fn=lpips_fn, out_dir=args.out_dir)
        else:
            report = evaluate.evaluate_folder(hsic, homo, args.dataset, args.split, tuple(args.patch_size), args.batch_size, cqe=cqe,
                                              metrics=metrics, lpips_fn=lpips_fn, seed=args.seed)
        print(report.line(), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                f.write(report.to_json())
        if args.timing:
            ds = data.DeviceStereoFolder(args.dataset, args.split, tuple(args.patch_size), seed=args.seed, device=device)
            B, batched, per_slice = time_pair_metrics(hsic, homo, ds, args.batch_size)
            print(f"timing: B = {B}, crops of {ds.crop[0]} x {ds.crop[1]}: pair_metrics {1e3 * batched:.1f} us, "
                  f"{B} per-slice rate_distortion calls {1e3 * per_slice:.1f} us ({per_slice / batched:.1f} x)", flush=True)
    finally:
        mnn.set_precision(before)
    return report


if __name__ == "__main__":
    main()
