"""Writes tests/golden/udh_net.npz: outputs of the REFERENCE's UDH homography net (coremasic/mywork/model.py: Net) on the CPU for
seeded weights and inputs (tests/udh_weights.py).  Needs the reference tree and oracle/_ref (`make -C oracle ref`); run from the
repository root:  python tests/golden/make_udh_goldens.py

Per case (patch_size, B): the float32 `delta`, the float64 `delta` of `net.double()` (the reference's own rounding floor), and
the four block outputs sampled at every 7th element.  Per patch size: the state-dict names and shapes and each tensor's float64
sum and first four values.  Inputs and weights are not stored: both sides rebuild them from the seeds."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import udh_weights as UW  # noqa: E402


def load_reference_model():
    ref_import.load()                                  # installs the kornia / torchvision stand-ins the file imports
    path = os.path.join(ref_import.REF, "coremasic", "mywork", "model.py")
    spec = importlib.util.spec_from_file_location("model_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    M = load_reference_model()
    out = {}
    nets = {}
    for p in sorted({p for p, _ in UW.CASES} | {32, 64, 128}):
        net = M.Net(patch_size=p).eval()
        arrays = UW.fill(net, UW.WEIGHT_SEED)
        nets[p] = net
        names = list(arrays)
        shapes = np.zeros((len(names), 4), dtype=np.int64)
        sums = np.zeros(len(names), dtype=np.float64)
        heads = np.zeros((len(names), 4), dtype=np.float32)
        for i, n in enumerate(names):
            shapes[i, :arrays[n].ndim] = arrays[n].shape
            sums[i], heads[i] = UW.fingerprint(arrays[n])
        out[f"w{p}/names"] = np.array(names)
        out[f"w{p}/shapes"] = shapes
        out[f"w{p}/sum"] = sums
        out[f"w{p}/head"] = heads
    for p, B in UW.CASES:
        net = nets[p]
        a, b = UW.patches(UW.case_seed(p, B), B, p)
        with torch.no_grad():
            x = torch.cat((a, b), dim=1)
            for i, blk in enumerate(net.cnn):
                x = blk(x)
                out[f"c{p}_{B}/block{i}"] = x.reshape(-1)[::UW.SAMPLE_STRIDE].numpy().copy()
            d32 = net(a, b)
            d64 = net.double()(a.double(), b.double())
            net.float()
            UW.fill(net, UW.WEIGHT_SEED)               # (float -> double -> float is exact, refilled anyway)
        out[f"c{p}_{B}/delta"] = d32.numpy().copy()
        out[f"c{p}_{B}/delta64"] = d64.numpy().copy()
        peak = float(d64.abs().max())
        print(f"case p={p} B={B}: peak |delta| {peak:.3f}, float32 vs float64 {float((d32.double() - d64).abs().max()) / peak:.2e} of peak")
    path = os.path.join(ROOT, "tests", "golden", "udh_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
