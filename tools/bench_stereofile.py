"""What the stereo file layer costs (masic_amd/stereofile.py; run on the GPU box):

  1. ops.pairs_prep's two kernels and ops.planes_to_u8 alone, device-event time over --iters back-to-back launches, against the bytes
     they move (uint8 side + float32 side; P = 2 B pictures).  Stacks whose planes fit the 256 MB last-level cache are marked.
  2. StereoCodec.encode / decode per pair at 512x512 and 375x1242, B = 1 and 8, bf16 operands, HSIC(128,192,5) with synthetic weights
     and a default-initialised homography net; beside them HSIC.compress_batch / decompress_batch on the SAME padded planes with the
     same h_matrix given: the difference is the layer (prep, homography net, container, temporary files, planes_to_u8).
     Wall time around one call that ends in a device synchronise, median of --runs.
  3. At masic_amd.trainrun's trained operating point (600 bf16 steps on 4 x 256 x 256): bpp and PSNR of the same pairs coded with the
     matrix of the quantised offsets and with the matrix of the unquantised ones.

  python tools/bench_stereofile.py [--runs 5] [--iters 200] [--skip-trained]"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "coremasic", "mywork")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import MASIC  # noqa: E402
import model  # noqa: E402
from masic_amd import StereoCodec, nn as mnn, ops, stereofile as SF, synth  # noqa: E402
from masic_amd._lib import check, lib  # noqa: E402

SIZES = ((512, 512), (375, 1242))
LMBDA = 0.0932


def _timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def _events(fn, iters):
    """ms per call over `iters` back-to-back calls between two device events (after a warm-up of 3)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _pictures(B, H, W, seed):
    x1, x2, _ = synth.synth_inputs(B, H, W, seed=seed)
    u8 = lambda x: torch.from_numpy(np.ascontiguousarray(np.rint(x.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).cuda()
    return u8(x1), u8(x2)


def kernels(iters):
    print("## kernels alone (device events; GB/s over the bytes each kernel must move)")
    print("| picture | P | planes kernel us | GB/s | patches kernel us | planes_to_u8 us | GB/s | planes in cache |")
    print("|---|---|---|---|---|---|---|---|")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for H0, W0 in SIZES:
        H, W = SF.padded_hw(H0, W0)
        for P in (2, 16, 128):
            pics = torch.randint(0, 256, (P, H0, W0, 3), dtype=torch.uint8, device="cuda")
            planes = torch.empty((P, 3, H, W), device="cuda")
            patches = torch.empty((P, 1, 128, 128), device="cuda")
            back = torch.empty_like(pics)
            st = ops._stream()
            t_pl = _events(lambda: check(lib.masic_pairs_prep(p(pics), P, H0, W0, H, W, p(planes), 256, 64, 64, 128, None, st)), iters)
            t_pa = _events(lambda: check(lib.masic_pairs_prep(p(pics), P, H0, W0, H, W, None, 256, 64, 64, 128, p(patches), st)), iters)
            t_u8 = _events(lambda: check(lib.masic_planes_to_u8(p(planes), P, H, W, H0, W0, p(back), st)), iters)
            assert torch.equal(back, pics)
            b_pl = P * (H0 * W0 * 3 + 3 * H * W * 4)
            b_u8 = P * (H0 * W0 * 3 + 3 * H0 * W0 * 4)
            print(f"| {H0}x{W0} | {P} | {1e3 * t_pl:.1f} | {b_pl / t_pl / 1e6:.0f} | {1e3 * t_pa:.1f} | {1e3 * t_u8:.1f} | {b_u8 / t_u8 / 1e6:.0f} | "
                  f"{'yes' if planes.numel() * 4 < 256e6 else 'no'} |", flush=True)
            del pics, planes, patches, back
    torch.cuda.empty_cache()


def layer(runs):
    print("\n## encode / decode per pair, bf16 operands (wall time, median of %d)" % runs)
    print("| picture | B | encode ms | compress_batch ms | layer ms | decode ms | decompress_batch ms | layer ms | file bytes | of them header |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    mnn.set_precision("bf16")
    hsic = MASIC.HSIC(128, 192, 5)
    hsic.load_state_dict(synth.synth_state_dict(hsic.state_dict(), seed=100))
    hsic = hsic.cuda().eval()
    hsic.update()
    torch.manual_seed(0)
    udh = model.Net().cuda().eval()
    sc = StereoCodec(hsic, udh)
    med = lambda f: statistics.median(_timed(f)[0] for _ in range(runs))
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        for H0, W0 in SIZES:
            for B in (1, 8):
                left, right = _pictures(B, H0, W0, seed=100)
                names = [f"p{i}" for i in range(B)]
                try:
                    enc = sc.encode(left, right, names, d)                               # warm-up
                except ValueError as e:                                                  # e.g. non-finite latents of the synthetic weights
                    print(f"| {H0}x{W0} | {B} | not measured: {e} |", flush=True)
                    continue
                dec = sc.decode(names, d)
                assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
                planes = ops.pairs_prep(torch.cat((left, right))).planes
                hm = enc["h_matrix"]
                inner = [f"i{i}" for i in range(B)]
                hsic.compress_batch(planes[:B], planes[B:], hm, inner, d)
                hsic.decompress_batch(inner, hm, d)
                te, tc = med(lambda: sc.encode(left, right, names, d)), med(lambda: hsic.compress_batch(planes[:B], planes[B:], hm, inner, d))
                td, tu = med(lambda: sc.decode(names, d)), med(lambda: hsic.decompress_batch(inner, hm, d))
                ms = lambda t: 1e3 * t / B
                print(f"| {H0}x{W0} | {B} | {ms(te):.2f} | {ms(tc):.2f} | {ms(te - tc):.2f} | {ms(td):.2f} | {ms(tu):.2f} | {ms(td - tu):.2f} | "
                      f"{sum(enc['bytes']) / B:.0f} | {SF.HEADER_BYTES} |", flush=True)
    mnn.set_precision("f32")


def trained():
    from masic_amd import trainrun
    print("\n## quantised against unquantised matrix at the trained operating point (600 bf16 steps, 4 x 256 x 256)")
    pool = trainrun.batch_pool(16, 4, 256, 256, "cuda", seed=8300)
    net = trainrun.default_init(device="cuda")
    losses, _, _ = trainrun.train(net, 600, pool, LMBDA, precision="bf16")
    net.eval()
    net.update(force=True)
    print(f"trained: loss {losses[0][0]:.0f} -> {losses[-1][0]:.1f}")
    mnn.set_precision("bf16")
    torch.manual_seed(0)
    udh = model.Net().cuda().eval()
    B, H0, W0 = 4, 250, 250
    held = trainrun.consistent_pair(*(t.cuda() for t in synth.synth_inputs(B, H0, W0, seed=8301)), seed=8301)
    left, right = (ops.planes_to_u8(t.contiguous(), (H0, W0)) for t in held[:2])
    planes, patches = ops.pairs_prep(torch.cat((left, right)))
    psnr = lambda a, b: float(-10 * torch.log10(((a[..., :H0, :W0] - b[..., :H0, :W0]) ** 2).mean()))
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        delta = torch.cat([udh(patches[i:i + 1], patches[B + i:B + i + 1]) for i in range(B)])
        q = SF.quantise(delta.reshape(B, 8).cpu().numpy())
        s = float(SF.HOMOPATCH)
        corners = torch.tensor([[0.0, 0.0], [s, 0.0], [s, s], [0.0, s]], device="cuda").repeat(B, 1, 1)
        mats = {"quantised": SF.h_matrix_from_offsets(q, (H0, W0), "cuda"),
                "unquantised": ops.homography_from_corners(corners, delta, (H0, W0), (SF.HOMOPIC, SF.HOMOPIC))}
        print(f"offsets: max |delta| {float(delta.abs().max()):.3f} px, max |delta - q/64| {float(np.abs(SF.dequantise(q) - delta.reshape(B, 8).cpu().numpy()).max()):.5f} px, "
              f"max |h_q - h| {float((mats['quantised'] - mats['unquantised']).abs().max()):.2e}")
        for name, hm in mats.items():
            out = net.compress_batch(planes[:B], planes[B:], hm, [f"{name}{i}" for i in range(B)], d)
            bpp = sum(out["bytes"]) * 8.0 / (B * H0 * W0)
            print(f"{name:12s}: {sum(out['bytes'])} bytes in the inner files of {B} pairs = {bpp:.5f} bpp over {H0}x{W0}; "
                  f"PSNR left {psnr(out['x1_hat'], planes[:B]):.4f} dB, right {psnr(out['x2_hat'], planes[B:]):.4f} dB")
        print(f"the stereo header adds {SF.HEADER_BYTES} bytes a pair = {SF.HEADER_BYTES * 8.0 / (H0 * W0):.5f} bpp at {H0}x{W0}")
    mnn.set_precision("f32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-trained", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stereofile: needs an MI355X; nothing is measured without one")
    kernels(args.iters)
    layer(args.runs)
    if not args.skip_trained:
        trained()


if __name__ == "__main__":
    main()
