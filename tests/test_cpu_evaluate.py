"""What the test-split evaluation answers without a GPU: the host-side answers of masic_amd/metrics.py's entry points (include/masic_metrics.h
and its binding are a row of tests/test_cpu_side_headers.py), the arithmetic and
the summary line of masic_amd.evaluate.Report, and every refusal of evaluate_folder / evaluate_files / pair_metrics that happens before
a launch.  The kernels and the two loops run in tests/test_gpu_metrics.py and tests/test_gpu_evaluate.py."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_line(line):
    """The small parser of the summary line: the text after 'Test epoch 0:', fields at '|', label and value at ':'"""
    assert "\n" not in line
    fields = line.split("Test epoch 0:")[-1].split("|")
    out = {}
    for f in fields:
        label, value = f.strip().split(":")
        out[label.strip()] = float(value.strip())
    return out


# ------------------------------------------------------------------------------------------ the entry points
def test_workspace_sizes_need_no_gpu():
    """pair_rd keeps masic_rd_loss's six rows of partials per image (so the partition of a slice is masic_sse's); 0 for a B the entry
    points refuse"""
    from masic_amd import _lib
    lib = _lib.lib
    assert lib.masic_metrics_pair_rd_workspace_bytes(1) == lib.masic_rd_loss_workspace_bytes() == 6 * lib.masic_reduce_workspace_bytes()
    assert lib.masic_metrics_pair_rd_workspace_bytes(5) == 5 * lib.masic_rd_loss_workspace_bytes()
    assert lib.masic_metrics_u8_sse_workspace_bytes(3) == 3 * 256 * 8
    for bad in (0, -1, 65536):
        assert lib.masic_metrics_pair_rd_workspace_bytes(bad) == 0 and lib.masic_metrics_u8_sse_workspace_bytes(bad) == 0


def test_argument_errors_launch_nothing():
    """the refusals come before the launches, so they are reached without a device: null pointers, nliks, B, P, n"""
    from masic_amd import _lib
    lib, one = _lib.lib, ctypes.c_void_p(64)
    liks, cnt = (ctypes.c_void_p * 4)(64, 64, 64, 64), (ctypes.c_size_t * 4)(1, 1, 1, 1)
    ok = [one, one, one, one, 4, liks, cnt, 4, 1, one, one, None]
    for k, v in ((0, None), (3, None), (9, None), (10, None), (7, 5), (7, -1), (8, 0), (8, 65536), (5, None)):
        args = list(ok)
        args[k] = v
        assert lib.masic_metrics_pair_rd(*args) == _lib.ERR_ARG, (k, v)
    liks[2] = None
    assert lib.masic_metrics_pair_rd(*ok) == _lib.ERR_ARG
    assert b"null likelihood" in lib.masic_last_error()
    ok = [one, one, 16, 1, one, one, None]
    for k, v in ((0, None), (1, None), (4, None), (5, None), (2, 0), (3, 0), (3, 65536)):
        args = list(ok)
        args[k] = v
        assert lib.masic_metrics_u8_sse(*args) == _lib.ERR_ARG, (k, v)


# ------------------------------------------------------------------------------------------ the report
MSE1 = np.array([1e-3, 4e-3, 2.5e-4])
MSE2 = np.array([2e-3, 1e-3, 1e-2])
BPP = {"bpp_y1": np.array([0.20, 0.30, 0.10]), "bpp_y2": np.array([0.10, 0.20, 0.05]), "bpp_z1": np.array([0.010, 0.020, 0.030]),
       "bpp_z2": np.array([0.005, 0.004, 0.003])}


def _estimate_report(**more):
    from masic_amd.evaluate import Report
    cols = {"mse1": MSE1, "mse2": MSE2, **BPP}
    cols["bpp1"], cols["bpp2"] = BPP["bpp_y1"] + BPP["bpp_z1"], BPP["bpp_y2"] + BPP["bpp_z2"]
    cols["bpp"] = BPP["bpp_y1"] + BPP["bpp_y2"] + BPP["bpp_z1"] + BPP["bpp_z2"]
    cols.update(more)
    return Report(["a.png", "b.png", "c.png"], cols, "estimate")


def test_report_arithmetic():
    r = _estimate_report(ms_ssim1=np.array([0.9, 0.95, 0.99]), ms_ssim2=np.array([0.8, 0.85, 0.97]))
    assert r.n == 3 and r.names == ["a.png", "b.png", "c.png"] and r.mode == "estimate" and r.roundtrip_exact is None
    want1 = np.array([10 * math.log10(1 / m) for m in MSE1])
    assert np.allclose(r.pairs["psnr1"], want1, rtol=1e-15, atol=0) and abs(r.pairs["psnr1"][0] - 30.0) < 1e-12
    assert np.array_equal(r.pairs["psnr"], (r.pairs["psnr1"] + r.pairs["psnr2"]) / 2)
    assert np.array_equal(r.pairs["ms_ssim"], (r.pairs["ms_ssim1"] + r.pairs["ms_ssim2"]) / 2)
    for k, v in r.pairs.items():
        assert v.dtype == np.float64 and r.mean[k] == float(np.mean(v)), k
    # the mean of the per-pair PSNRs, not the PSNR of the mean mse
    assert abs(r.mean["psnr1"] - 10 * math.log10(1 / MSE1.mean())) > 0.5
    f = dict((label, value) for label, value, _ in r.fields())
    assert f["PSNR (dB)"] == (r.mean["psnr1"] + r.mean["psnr2"]) / 2
    assert f["Bpp loss"] == r.mean["bpp"] / 2 and "BPP" not in f
    assert f["BPP1"] == r.mean["bpp1"] and f["BPP2"] == r.mean["bpp2"]
    with pytest.raises(ValueError, match="2 values for 3 pairs"):
        _estimate_report(ms_ssim1=np.zeros(2))
    from masic_amd.evaluate import Report
    with pytest.raises(ValueError, match="mode"):
        Report(["a"], {"mse1": [1.0], "mse2": [1.0]}, "guess")


def test_files_mode_psnr_and_its_cap():
    from masic_amd.evaluate import Report, psnr_from_mse_u8
    n = 5 * 7 * 3
    sse = np.array([0.0, 1.0, 12345.0])
    mse = sse / (n * 255 ** 2)
    r = Report(["a", "b", "c"], {"mse1": mse, "mse2": mse[::-1].copy(), "bpp": np.array([1.0, 2.0, 4.5])}, "files", roundtrip_exact=True)
    want = [100.0] + [20 * math.log10(1 / math.sqrt(m)) for m in mse[1:]]
    assert np.allclose(r.pairs["psnr1"], want, rtol=1e-15, atol=0) and r.pairs["psnr1"][0] == 100.0 and r.pairs["psnr2"][2] == 100.0
    assert psnr_from_mse_u8(0.99e-10) == 100.0 and psnr_from_mse_u8(1.0e-10) < 100.0 + 1e-9
    assert r.roundtrip_exact is True


def test_line_is_read_back_by_a_small_parser():
    r = _estimate_report(ms_ssim1=np.array([0.9, 0.95, 0.99]), ms_ssim2=np.array([0.8, 0.85, 0.97]))
    line = r.line()
    assert line.startswith("Test epoch 0: ") and r.line(epoch=3).startswith("Test epoch 3: ")
    got = parse_line(line)
    assert list(got) == ["Pairs", "PSNR (dB)", "Bpp loss", "MS-SSIM", "MS-SSIM1", "MS-SSIM2", "PSNR1", "PSNR2", "BPP1", "BPP2"]
    m = r.mean
    assert got["Pairs"] == 3
    assert got["PSNR (dB)"] == round((m["psnr1"] + m["psnr2"]) / 2, 3) and got["Bpp loss"] == round(m["bpp"] / 2, 4)
    assert got["MS-SSIM"] == round(m["ms_ssim"], 4) and got["MS-SSIM1"] == round(m["ms_ssim1"], 4) and got["MS-SSIM2"] == round(m["ms_ssim2"], 4)
    assert got["PSNR1"] == round(m["psnr1"], 3) and got["PSNR2"] == round(m["psnr2"], 3)
    assert got["BPP1"] == round(m["bpp1"], 3) and got["BPP2"] == round(m["bpp2"], 3)
    # with LPIPS measured, its three fields follow MS-SSIM's
    r = _estimate_report(lpips1=np.array([0.1, 0.2, 0.3]), lpips2=np.array([0.3, 0.2, 0.4]))
    got = parse_line(r.line())
    assert list(got) == ["Pairs", "PSNR (dB)", "Bpp loss", "LPIPS", "LPIPS1", "LPIPS2", "PSNR1", "PSNR2", "BPP1", "BPP2"]
    assert got["LPIPS"] == round(r.mean["lpips"], 4) == 0.25 and got["LPIPS2"] == 0.3


def test_files_mode_line_has_no_per_view_rate():
    from masic_amd.evaluate import Report
    r = Report(["a", "b"], {"mse1": [1e-3, 2e-3], "mse2": [1e-3, 1e-3], "bpp": [0.5, 0.7], "bytes": [100, 140]}, "files", roundtrip_exact=True)
    got = parse_line(r.line())
    assert list(got) == ["Pairs", "PSNR (dB)", "BPP", "PSNR1", "PSNR2"]
    assert got["BPP"] == round(0.6 / 2, 3) and "BPP1" not in r.line() and "Bpp loss" not in r.line()
    # a distortion-only estimate (the CQE stage's criterion) has no rate fields at all
    r = Report(["a"], {"mse1": [1e-3], "mse2": [1e-3]}, "estimate")
    assert list(parse_line(r.line())) == ["Pairs", "PSNR (dB)", "PSNR1", "PSNR2"]


def test_json_round_trip():
    from masic_amd.evaluate import Report
    r = _estimate_report(ms_ssim1=np.array([0.9, 0.95, 0.99]), ms_ssim2=np.array([0.8, 0.85, 0.97]))
    text = r.to_json()
    d = json.loads(text)
    assert d["mode"] == "estimate" and d["n"] == 3 and d["names"] == r.names and d["mean"] == r.mean
    back = Report.from_json(text)
    assert back.names == r.names and back.mode == r.mode and back.mean == r.mean and set(back.pairs) == set(r.pairs)
    for k in r.pairs:
        assert np.array_equal(back.pairs[k], r.pairs[k]), k
    assert back.line() == r.line() and back.to_json() == text


# ------------------------------------------------------------------------------------------ refusals before any launch
class _Cpu(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


class _ClaimsCuda(torch.nn.Module):
    """parameters that claim a device: the refusals that follow the device's read nothing else of the module"""
    def parameters(self, recurse=True):
        class P:
            device = torch.device("cuda", 0)
        return iter([P()])


def _folder(tmp_path, hw=(64, 96), n=2):
    from PIL import Image
    for side in ("left", "right"):
        os.makedirs(tmp_path / "test" / side)
        for i in range(n):
            Image.fromarray(np.full((hw[0], hw[1], 3), 10 * i, dtype=np.uint8)).save(tmp_path / "test" / side / f"{i:03d}.png")
    return str(tmp_path)


def test_estimate_mode_refusals(tmp_path):
    from masic_amd import evaluate
    root = _folder(tmp_path)
    with pytest.raises(ValueError, match="unknown metric 'ssim'"):
        evaluate.evaluate_folder(_Cpu(), _Cpu(), root, metrics=("psnr", "ssim"))
    with pytest.raises(ValueError, match="'lpips' needs lpips_fn"):
        evaluate.evaluate_folder(_Cpu(), _Cpu(), root, metrics=("psnr", "lpips"))
    with pytest.raises(ValueError, match="batch_size"):
        evaluate.evaluate_folder(_Cpu(), _Cpu(), root, batch_size=0)
    with pytest.raises(RuntimeError, match="hsic module must live on a CUDA"):
        evaluate.evaluate_folder(_Cpu(), _Cpu(), root, metrics=("psnr",))
    with pytest.raises(RuntimeError, match="Invalid directory"):
        evaluate.evaluate_folder(_ClaimsCuda(), _ClaimsCuda(), str(tmp_path / "nowhere"), metrics=("psnr",))


def test_ms_ssim_needs_176_pixels(tmp_path):
    """refused from the pictures' headers, with modules that would fail at their first use"""
    from masic_amd import evaluate
    Cuda = _ClaimsCuda
    root = _folder(tmp_path, hw=(175, 300))
    with pytest.raises(ValueError, match=r"'ms_ssim' needs pictures of at least 176 x 176.*the crop of 000.png is 175 x 256"):
        evaluate.evaluate_folder(Cuda(), Cuda(), root, patch_size=(256, 256))
    with pytest.raises(ValueError, match="is 175 x 300"):
        evaluate.evaluate_files(_codec(Cuda()), root)
    evaluate._check_ms_ssim(("psnr", "ms_ssim"), (176, 176), "x", "t")
    evaluate._check_ms_ssim(("psnr",), (8, 8), "x", "t")


def _codec(hsic, udh=True, cqe=None):
    from masic_amd import StereoCodec
    return StereoCodec(hsic, hsic if udh else None, cqe)


def test_files_mode_refusals(tmp_path):
    from masic_amd import evaluate
    root = _folder(tmp_path)
    with pytest.raises(ValueError, match="unknown metric"):
        evaluate.evaluate_files(_codec(_Cpu()), root, metrics=("bpp",))
    with pytest.raises(ValueError, match="'lpips' needs lpips_fn"):
        evaluate.evaluate_files(_codec(_Cpu()), root, metrics=("lpips",))
    with pytest.raises(RuntimeError, match="cannot encode"):
        evaluate.evaluate_files(_codec(_Cpu(), udh=False), root, metrics=("psnr",))
    with pytest.raises(RuntimeError, match="enhance=True needs the enhancement network"):
        evaluate.evaluate_files(_codec(_Cpu()), root, metrics=("psnr",), enhance=True)
    with pytest.raises(RuntimeError, match="must live on a CUDA"):
        evaluate.evaluate_files(_codec(_Cpu()), root, metrics=("psnr",))
    with pytest.raises(RuntimeError, match="Invalid directory"):
        evaluate.evaluate_files(_codec(_ClaimsCuda()), root, split="val", metrics=("psnr",))


def test_cpu_tensors_are_refused():
    from masic_amd import evaluate, metrics
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.pair_metrics({"x1_hat": x, "x2_hat": x}, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.pair_rd(x, x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.u8_sse(torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="likelihoods"):
        evaluate.pair_metrics({"x1_hat": x, "x2_hat": x, "likelihoods": {"y1": x}}, x, x)


def test_eval_mode_sets_every_flag_back():
    from masic_amd import evaluate
    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Sequential(torch.nn.Dropout()))
    net.train()
    net[1].eval()                      # a mixed module: the inner Sequential and its Dropout stay in eval mode afterwards
    flags = [m.training for m in net.modules()]
    with pytest.raises(KeyError):
        with evaluate._eval_mode(net, None, "not a module"):
            assert not any(m.training for m in net.modules())
            raise KeyError("x")
    assert [m.training for m in net.modules()] == flags and flags == [True, True, False, False]
