"""Shared by tests/test_cpu_udh_train.py and tests/test_gpu_udh_train.py: the cases of tests/golden/udh_train.npz, their inputs
rebuilt from the recorded seeds, and the comparison rule (error over the tensor's peak against max(1e-4, 2 x the reference's own
float32 floor); large tensors by 512 sampled entries and the L2 norm, as tests/test_gpu_cqe.py)."""
import importlib.util
import os

import numpy as np
import torch

from tests import udh_train_ref as TR
from tests import udh_weights as UW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((32, 3, (40, 48), "eval"), (32, 3, (40, 48), "train"), (64, 9, (80, 96), "train"), (128, 1, (160, 144), "eval"))
RHO = {32: 6.0, 64: 10.0, 128: 10.0}
GTOL = 1e-4


def load_udh_model():
    """udh/udh/model.py by file path: its module name collides with the codec-side `model`."""
    spec = importlib.util.spec_from_file_location("udh_train_model", os.path.join(ROOT, "udh", "udh", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_inputs(fx, index):
    """(a, b, img_a, patch_b, corners, masks or None) of fixture case `index`, rebuilt from its seeds (CPU float32; masks uint8)."""
    p, B, img_hw, mode = CASES[index]
    key = f"c{index}/"
    a, b = TR.patch_batch(fx[key + "patch_seeds"], p)
    img, pb, corners = TR.loss_inputs(fx[key + "seeds"], img_hw, (p, p), RHO[p])
    masks = None
    if mode == "train":
        k = 128 * (p // 8) ** 2
        masks = (torch.from_numpy(np.unpackbits(fx[key + "m1"], axis=1)[:, :k].copy()), torch.from_numpy(np.unpackbits(fx[key + "m2"], axis=1)[:, :1024].copy()))
    return a, b, img, pb, corners, masks


def check(fx, index, name, got, worst):
    """Error of `got` against fixture entry c<index>/<name> in units of its tolerance; sampled entries + L2 norm for large tensors."""
    key = f"c{index}/{name}"
    assert got is not None, key
    got = got.detach().cpu()
    if key in fx:
        ref = torch.from_numpy(fx[key])
        assert tuple(got.shape) == tuple(ref.shape), key
        e = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
    else:
        idx, ref = torch.from_numpy(fx[key + "@idx"]), torch.from_numpy(fx[key + "@val"])
        e = float((got.reshape(-1)[idx] - ref).abs().max()) / (float(fx[key + "@absmax"]) + 1e-30)
        e = max(e, abs(float(got.double().norm()) / (float(fx[key + "@norm"]) + 1e-300) - 1.0))
    tol = max(GTOL, 2.0 * float(fx[f"c{index}/floor/{name}"]))
    assert np.isfinite(e), key
    e /= tol
    if e > worst[0]:
        worst[0], worst[1] = e, key
    return e


def check_step(fx, index, loss, delta, grads, what):
    worst = [0.0, ""]
    check(fx, index, "loss", loss.reshape(()), worst)
    check(fx, index, "delta", delta, worst)
    assert len(grads) == 20
    for n, g in grads.items():
        check(fx, index, "g/" + n, g, worst)
    print(f"{what} case {index} {CASES[index]}: worst error / tolerance {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst
