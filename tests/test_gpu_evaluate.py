"""GPU tests (-m gpu) of the test-split evaluation (masic_amd/evaluate.py, tools/eval_folder.py) on five 192 x 256 stereo pairs written
as PNG files, with the small model and the UDH net of tests/test_gpu_stereofile.py.  The per-pair rate and distortion are compared with
== against loss.rate_distortion on the one-pair slices of the SAME forward outputs, taken through forward hooks; that a batch's forward
outputs equal the one-pair forward's is a property of other kernels and is not asserted here."""
import json
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import udh_weights as UW
from tests.test_cpu_evaluate import ROOT, parse_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, PAIRS = 192, 256, 5
NMK, SEED, PREC = (32, 48, 3), 21, "bf16"
NAMES = [f"{i:03d}.png" for i in range(PAIRS)]
_CACHE = {}


def _pair(i, h, w):
    """a smooth ramp plus seeded noise; the right view is the left one shifted by a few pixels"""
    rng = np.random.default_rng(100 + i)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([40 + 150.0 * xx / w + 10 * i, 200 - 120.0 * yy / h, 60 + 60.0 * (xx + yy) / (h + w)], axis=2)
    left = np.clip(np.rint(ramp + rng.normal(0, 5, ramp.shape)), 0, 255).astype(np.uint8)
    return left, np.roll(left, -(2 + i), axis=1)


def _write(root, name, left, right):
    from PIL import Image
    for side, pic in (("left", left), ("right", right)):
        os.makedirs(os.path.join(root, "test", side), exist_ok=True)
        Image.fromarray(pic).save(os.path.join(root, "test", side, name))


def _state_dict():
    import MASIC
    from masic_amd import synth
    return synth.synth_state_dict(MASIC.HSIC(*NMK).state_dict(), seed=SEED)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """(folder, hsic, udh); masic_amd.nn's precision is bf16 while this module's tests run"""
    import MASIC
    import model
    from masic_amd import nn as mnn
    root = str(tmp_path_factory.mktemp("split"))
    for i, name in enumerate(NAMES):
        _write(root, name, *_pair(i, H, W))
    mnn.set_precision(PREC)
    try:
        hsic = MASIC.HSIC(*NMK)
        hsic.load_state_dict(_state_dict())
        hsic = hsic.to(DEV).eval()
        hsic.update()
        udh = model.Net(patch_size=128).to(DEV).eval()
        UW.fill(udh, UW.WEIGHT_SEED)
        yield root, hsic, udh
    finally:
        mnn.set_precision("f32")


def _clone(out):
    return {"x1_hat": out["x1_hat"].clone(), "x2_hat": out["x2_hat"].clone(),
            **({"likelihoods": {k: v.clone() for k, v in out["likelihoods"].items()}} if "likelihoods" in out else {})}


def _hooked(module, run):
    """run() with every forward call of `module` recorded: [(inputs, output)], cloned"""
    calls = []
    handle = module.register_forward_hook(lambda m, args, out: calls.append((tuple(a.clone() for a in args), _clone(out))))
    try:
        return run(), calls
    finally:
        handle.remove()


def _estimate(env, **kw):
    from masic_amd import evaluate
    root, hsic, udh = env
    if "estimate" not in _CACHE:
        _CACHE["estimate"] = _hooked(hsic, lambda: evaluate.evaluate_folder(hsic, udh, root, patch_size=(H, W), batch_size=2))
    return _CACHE["estimate"]


def test_estimate_mode_has_rate_distortions_own_numbers_per_pair(env):
    from masic_amd import nn as mnn
    from masic_amd.loss import rate_distortion
    from pytorch_msssim import ms_ssim
    report, calls = _estimate(env)
    assert report.mode == "estimate" and report.n == PAIRS and report.names == NAMES and report.roundtrip_exact is None
    assert [c[0][0].shape[0] for c in calls] == [2, 2, 1]                    # every pair once, the last batch short
    assert mnn.get_precision() == PREC
    i = 0
    with torch.no_grad():
        for (d1, d2, _), out in calls:
            assert d1.shape[1:] == (3, H, W)
            ms1 = ms_ssim(out["x1_hat"], d1, data_range=1, size_average=False).double().cpu().numpy()
            ms2 = ms_ssim(out["x2_hat"], d2, data_range=1, size_average=False).double().cpu().numpy()
            for b in range(d1.shape[0]):
                one = {"x1_hat": out["x1_hat"][b:b + 1], "x2_hat": out["x2_hat"][b:b + 1],
                       "likelihoods": {k: v[b:b + 1] for k, v in out["likelihoods"].items()}}
                rd = rate_distortion(one, d1[b:b + 1], d2[b:b + 1], 0.01)
                p = {k: v[i] for k, v in report.pairs.items()}
                print(NAMES[i], {k: float(v) for k, v in p.items()})
                assert p["mse1"] == float(rd["mse1"]) and p["mse2"] == float(rd["mse2"])
                for k in ("y1", "y2", "z1", "z2"):
                    assert p["bpp_" + k] == float(rd["bpp_" + k]) and p["bpp_" + k] > 0, k
                assert p["bpp1"] == float(rd["bpp_y1"] + rd["bpp_z1"]) and p["bpp2"] == float(rd["bpp_y2"] + rd["bpp_z2"])
                assert np.float32(p["bpp"]) == np.float32(rd["bpp_loss"].item())          # rate_distortion rounds its sum to float32
                assert p["bpp"] == float(((rd["bpp_y1"] + rd["bpp_y2"]) + rd["bpp_z1"]) + rd["bpp_z2"])
                assert abs(p["psnr1"] - float(rd["psnr1"])) < 1e-12 and abs(p["psnr2"] - float(rd["psnr2"])) < 1e-12
                assert p["psnr"] == (p["psnr1"] + p["psnr2"]) / 2
                assert p["ms_ssim1"] == ms1[b] and p["ms_ssim2"] == ms2[b] and p["ms_ssim"] == (ms1[b] + ms2[b]) / 2
                i += 1
    assert i == PAIRS
    for k, v in report.pairs.items():
        assert v.dtype == np.float64 and v.shape == (PAIRS,) and report.mean[k] == float(np.mean(v)), k
    assert len(set(report.pairs["mse1"])) == PAIRS                          # five different pictures, five different values
    got = parse_line(report.line())
    assert got["Pairs"] == PAIRS and got["PSNR (dB)"] == round((report.mean["psnr1"] + report.mean["psnr2"]) / 2, 3)
    assert got["Bpp loss"] == round(report.mean["bpp"] / 2, 4) and got["BPP1"] == round(report.mean["bpp1"], 3)


def test_estimate_mode_repeats_and_restores_training_flags(env):
    from masic_amd import evaluate, nn as mnn
    root, hsic, udh = env
    first, _ = _estimate(env)
    hsic.train()
    udh.train()
    try:
        again = evaluate.evaluate_folder(hsic, udh, root, patch_size=(H, W), batch_size=2)
        assert all(m.training for m in hsic.modules()) and all(m.training for m in udh.modules())
    finally:
        hsic.eval()
        udh.eval()
    assert mnn.get_precision() == PREC
    assert again.names == first.names and set(again.pairs) == set(first.pairs)
    for k in first.pairs:
        assert np.array_equal(again.pairs[k], first.pairs[k]), k
    # another batch size regroups the pairs, nothing else: psnr only, one batch of five
    five = evaluate.evaluate_folder(hsic, udh, root, patch_size=(H, W), batch_size=8, metrics=("psnr",))
    assert five.n == PAIRS and "ms_ssim" not in five.pairs and "MS-SSIM" not in five.line()


def test_estimate_mode_with_the_enhancement_net(env):
    """the rate is the codec's, the distortion comes from the enhanced pictures"""
    import MASIC
    from masic_amd import evaluate, ops, synth
    root, hsic, udh = env
    plain, _ = _estimate(env)
    cqe = MASIC.Independent_EN()
    cqe.load_state_dict(synth.synth_state_dict(cqe.state_dict(), seed=101))
    cqe = cqe.to(DEV).eval()
    (report, en_calls), codec_calls = _hooked(hsic, lambda: _hooked(cqe, lambda: evaluate.evaluate_folder(
        hsic, udh, root, patch_size=(H, W), batch_size=2, cqe=cqe, metrics=("psnr",))))
    assert not cqe.training and [c[0][0].shape[0] for c in en_calls] == [2, 2, 1]
    for k in ("bpp_y1", "bpp_y2", "bpp_z1", "bpp_z2", "bpp1", "bpp2", "bpp"):
        assert np.array_equal(report.pairs[k], plain.pairs[k]), k
    i = 0
    for ((d1, d2, h), codec_out), ((x1_in, x2_in, h_in), en_out) in zip(codec_calls, en_calls):
        assert torch.equal(x1_in, codec_out["x1_hat"]) and torch.equal(x2_in, codec_out["x2_hat"]) and torch.equal(h_in, h)
        for b in range(d1.shape[0]):
            assert report.pairs["mse1"][i] == float(ops.sse(en_out["x1_hat"][b:b + 1].contiguous(), d1[b:b + 1]) / d1[b:b + 1].numel())
            assert report.pairs["mse2"][i] == float(ops.sse(en_out["x2_hat"][b:b + 1].contiguous(), d2[b:b + 1]) / d2[b:b + 1].numel())
            i += 1
    assert i == PAIRS and not np.array_equal(report.pairs["mse1"], plain.pairs["mse1"])


def test_pair_metrics_without_likelihoods(env):
    from masic_amd import evaluate
    _, calls = _estimate(env)
    (d1, d2, _), out = calls[0]
    full = evaluate.pair_metrics(out, d1, d2)
    only = evaluate.pair_metrics({"x1_hat": out["x1_hat"], "x2_hat": out["x2_hat"]}, d1, d2)
    assert sorted(only) == ["mse1", "mse2"] and len(full) == 9
    for k, v in full.items():
        assert v.dtype == torch.float64 and v.shape == (2,) and v.is_cuda, k
    assert torch.equal(only["mse1"], full["mse1"]) and torch.equal(only["mse2"], full["mse2"])


def _np_psnr(decoded, original):
    d = decoded.astype(np.int64) - original.astype(np.int64)
    mse = (d * d).sum() / (original.size * 255 ** 2)
    return mse, (100.0 if mse < 1.0e-10 else 20 * math.log10(1 / math.sqrt(mse)))


def test_files_mode(env, tmp_path):
    from masic_amd import StereoCodec, data, evaluate
    root, hsic, udh = env
    out_dir = str(tmp_path / "msf")
    report = evaluate.evaluate_files(StereoCodec(hsic, udh), root, batch_size=2, out_dir=out_dir)
    _CACHE["files"] = report
    assert report.mode == "files" and report.n == PAIRS and report.names == NAMES and report.roundtrip_exact is True
    assert sorted(os.listdir(out_dir)) == [n + ".msf" for n in NAMES]        # left where the caller asked for them
    dec = StereoCodec(hsic).decode(NAMES, out_dir)
    left, right = dec["left"].cpu().numpy(), dec["right"].cpu().numpy()
    for i, n in enumerate(NAMES):
        size = os.path.getsize(os.path.join(out_dir, n + ".msf"))
        assert report.pairs["bytes"][i] == size and report.pairs["bpp"][i] == 8 * size / (H * W)
        for v, pics, side in (("1", left, "left"), ("2", right, "right")):
            mse, psnr = _np_psnr(pics[i], data.decode_rgb8(os.path.join(root, "test", side, n)))
            print(n, side, size, mse, psnr)
            assert report.pairs["mse" + v][i] == mse and 0 < mse < 1
            assert abs(report.pairs["psnr" + v][i] - psnr) <= 1e-15 * psnr          # two float64 logarithms: an ulp or two
    assert "ms_ssim" in report.pairs and np.all(report.pairs["ms_ssim"] <= 1)
    got = parse_line(report.line())
    assert list(got) == ["Pairs", "PSNR (dB)", "BPP", "MS-SSIM", "MS-SSIM1", "MS-SSIM2", "PSNR1", "PSNR2"]
    assert got["BPP"] == round(report.mean["bpp"] / 2, 3)


def test_files_mode_groups_pictures_by_size(env, tmp_path):
    from masic_amd import StereoCodec, evaluate
    root, hsic, udh = env
    mixed = str(tmp_path / "mixed")
    shutil.copytree(os.path.join(root, "test"), os.path.join(mixed, "test"))
    _write(mixed, "005.png", *_pair(5, 128, 192))
    codec, calls = StereoCodec(hsic, udh), []
    encode = codec.encode
    codec.encode = lambda left, right, names, path: (calls.append((list(names), tuple(left.shape))), encode(left, right, names, path))[1]
    report = evaluate.evaluate_files(codec, mixed, batch_size=8, metrics=("psnr",))
    assert calls == [(NAMES, (5, H, W, 3)), (["005.png"], (1, 128, 192, 3))]
    assert report.names == NAMES + ["005.png"] and report.n == 6 and report.roundtrip_exact is True
    assert report.pairs["bpp"][5] == 8 * report.pairs["bytes"][5] / (128 * 192)
    if "files" in _CACHE:                                                   # a pair's file does not depend on its batch mates
        assert np.array_equal(report.pairs["bytes"][:5], _CACHE["files"].pairs["bytes"])
        assert np.array_equal(report.pairs["mse1"][:5], _CACHE["files"].pairs["mse1"])
    with pytest.raises(ValueError, match="005.png is 128 x 192"):
        evaluate.evaluate_files(codec, mixed, batch_size=8, metrics=("psnr", "ms_ssim"))
    assert len(calls) == 2                                                  # refused before anything ran


def test_the_command_line_tool(env, tmp_path, capsys):
    """tools/eval_folder.py on a checkpoint as tools/train_folder.py --save writes it: the line it prints is the report's, and the
    test's parser reads it back"""
    from masic_amd import evaluate, nn as mnn
    from masic_amd.align import PatchAligner
    root, hsic, _ = env
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_folder
    finally:
        sys.path.pop(0)
    ckpt, table = str(tmp_path / "checkpoint.pth.tar"), str(tmp_path / "report.json")
    torch.save({"state_dict": _state_dict(), "steps": 0, "lambda": 0.01}, ckpt)
    eval_folder.main(["-d", root, "--checkpoint", ckpt, "--nmk", *map(str, NMK), "--aligner", "--patch-size", str(H), str(W),
                      "--batch-size", "2", "--precision", PREC, "--json", table])
    assert mnn.get_precision() == PREC
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test epoch 0:")]
    assert len(lines) == 1
    want = evaluate.evaluate_folder(hsic, PatchAligner().to(DEV).eval(), root, patch_size=(H, W), batch_size=2)
    assert lines[0] == want.line()
    got = parse_line(lines[0])
    assert got["Pairs"] == PAIRS and got["PSNR1"] == round(want.mean["psnr1"], 3) and got["MS-SSIM"] == round(want.mean["ms_ssim"], 4)
    with open(table) as f:
        d = json.load(f)
    assert d["names"] == NAMES and d["pairs"]["bpp"] == list(want.pairs["bpp"])
