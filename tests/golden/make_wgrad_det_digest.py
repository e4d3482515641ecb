"""SHA-256 of every deterministic weight gradient over the case lists of tests/test_gpu_determinism.py (NCHW_CASES, K3_CASES,
GEMM1_CASES) -> tests/golden/wgrad_det_digest.json.  Needs an MI355X.  Deterministic mode is bitwise reproducible, so a library whose
kernels, grids and split counts are those of the recording reproduces every digest.  Inputs: a CPU torch.Generator seeded per case,
copied to the device.  The committed file was written by this script run on commit 37681ab, the commit BEFORE the weight-gradient
host side became a plan and a table (plan_wgrad, WGRAD_ROWS, wg3_run, wg1_run); regenerate it only from a commit whose bits are meant to
become the new reference.

    python tests/golden/make_wgrad_det_digest.py

tests/test_gpu_determinism.py::test_det_digests_are_the_recorded imports digests() from here."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "wgrad_det_digest.json")


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def digests(nchw_cases, k3_cases, gemm1_cases, dev="cuda"):
    """{case id: sha256 hex of dW (and of the bias sums behind it where there are any)} in deterministic mode"""
    import torch
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16, PREC_F32
    from masic_amd.determinism import deterministic
    out = {}
    with deterministic():
        for i, (prec, name, B, Cin, H, W, Cout, k, s, tr, masked, act) in enumerate(nchw_cases):
            d = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=tr, prec=PREC_BF16 if prec == "bf16" else PREC_F32)
            g = torch.Generator().manual_seed(1000 + i)
            x = (2.0 * torch.randn(B, Cin, H, W, generator=g)).to(dev)
            dy = torch.randn(B, Cout, d.Ho, d.Wo, generator=g).to(dev)
            wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
            out[f"nchw/{prec}-{name}"] = _sha(ops.conv2d_wgrad(x, dy, d, wshape))
            if prec == "bf16" and ops.conv2d_wgrad_b16_supported(d):
                out[f"nchw/{prec}-{name}/in16"] = _sha(ops.conv2d_wgrad(x.bfloat16(), dy.bfloat16(), d, wshape))
        for i, (KS, B, Cin, Cout, H, W) in enumerate(k3_cases):
            g = torch.Generator().manual_seed(2000 + i)
            x16 = ops.nchw_to_f16k(torch.randn(B, Cin, H, W, generator=g).to(dev))
            g16 = ops.nchw_to_f16k(torch.randn(B, Cout, H, W, generator=g).to(dev))
            fn = ops.conv3x3_wgrad_f16k if KS == 3 else ops.conv5x5_wgrad_f16k
            out[f"k{KS}/{B}-{Cin}-{Cout}-{H}-{W}"] = _sha(fn(x16, g16, B, Cin, Cout, H, W))
        for i, (B, Cout, Cin, H, W) in enumerate(gemm1_cases):
            g = torch.Generator().manual_seed(3000 + i)
            x16 = ops.nchw_to_f16k((1.5 * torch.randn(B, Cin, H, W, generator=g)).to(dev))
            g16 = ops.nchw_to_f16k(torch.randn(B, Cout, H, W, generator=g).to(dev))
            key = f"k1/{B}-{Cout}-{Cin}-{H}-{W}"
            out[key + "/bias0"] = _sha(ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W))
            out[key + "/bias1"] = _sha(*ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W, bias_of=1))
            out[key + "/bias2"] = _sha(*ops.gemm_wgrad_f16k(x16, g16, B, Cin, Cout, H * W, bias_of=2))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "coremasic", "mywork"))
    import torch  # noqa: F401  (before the library: both then share torch's HIP runtime)
    from masic_amd import _lib
    from tests.test_gpu_determinism import GEMM1_CASES, K3_CASES, NCHW_CASES
    D = digests(NCHW_CASES, K3_CASES, GEMM1_CASES)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        json.dump(D, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(D)} digests (library {_lib.LIB_PATH})")
