"""SHA-256 of ops.conv2d / ops.conv2d_f16k_out outputs, one case per entry of CONV_ROWS (masic_amd/csrc/conv.hip) and a few forms on top
-> tests/golden/conv_fwd_digest.json.  Needs an MI355X.  These kernels use no atomics, so a library whose kernels, grids and arguments
are those of the recording reproduces every digest.  Inputs: a CPU torch.Generator seeded per case, copied to the device.  The
committed file was written by this script run on commit b955ed7, the commit BEFORE the host side of conv.hip became a plan and a
table (plan_conv, CONV_ROWS); regenerate it only from a commit whose bits are meant to become the new reference.

    python tests/golden/make_conv_fwd_digest.py

Each case is the smallest shape of a search over kinds, channels, sizes and batches that selects its kernel; the widest tiles need
>= 512 / 768 workgroups, so their outputs are tens of MB: an output above 1 MiB is folded on the device before it is hashed (exact
integer sums of its 32-bit words over rows of 4096, plain and weighted by the row number -- any changed word changes a sum).  The
kernel a case was recorded on is part of the case and of the JSON; tests/test_cpu_conv_plan.py holds the plan to it without a GPU.
tests/test_gpu_conv_digest.py imports cases() and digests() from here."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "conv_fwd_digest.json")
GATE, RES1, RES2, F16K_OUT = 1, 2, 4, 8          # MASIC_CONV_*
RELU, SOFTMAX = 1, 3                             # MASIC_ACT_*

# (kernel, B, Cin, H, W, Cout, k, stride, transposed, masked, prec, in_op): the plain form, no activation, whole buffers
ROW_CASES = [
    ("conv5s1_small<4>", 1, 3, 4, 4, 3, 5, 1, 0, 0, 0, 0),
    ("conv5s1_small<8>", 1, 3, 4, 4, 8, 5, 1, 0, 0, 0, 0),
    ("conv_direct_f32<3>", 1, 3, 4, 4, 3, 3, 2, 0, 0, 0, 0),
    ("conv_direct_f32<8>", 1, 3, 4, 4, 8, 3, 2, 0, 0, 0, 0),
    ("conv_igemm_bf16<1, 1, 2, 0, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<1, 1, 2, 0, true>", 1, 2, 4, 4, 12, 1, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<1, 1, 2, 1, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<1, 1, 2, 1, true>", 1, 2, 4, 4, 12, 1, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<1, 1, 2, 2, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<1, 1, 2, 2, true>", 1, 2, 4, 4, 12, 1, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<1, 3, 2, 0, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<1, 3, 2, 0, true>", 1, 4, 4, 4, 96, 1, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<1, 3, 2, 1, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<1, 3, 2, 1, true>", 1, 4, 4, 4, 96, 1, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<1, 3, 2, 2, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<1, 3, 2, 2, true>", 1, 4, 4, 4, 96, 1, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 1, 0, false>", 1, 32, 4, 4, 64, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 1, 0, true>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 1, 1, false>", 1, 32, 4, 4, 64, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 1, 1, true>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 1, 2, false>", 1, 32, 4, 4, 64, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 1, 2, true>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 2, 0, false>", 2, 4, 256, 256, 128, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 2, 0, true>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 2, 1, false>", 2, 4, 256, 256, 128, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 2, 1, true>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 2, 2, false>", 2, 4, 256, 256, 128, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 2, 2, true>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 4, 0, false>", 3, 32, 256, 256, 64, 3, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 4, 0, true>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 1, 4, 1, false>", 3, 32, 256, 256, 64, 3, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 4, 1, true>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 1, 4, 2, false>", 3, 32, 256, 256, 64, 3, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 1, 4, 2, true>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 2, 2, 0, false>", 3, 4, 256, 384, 128, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 2, 2, 0, true>", 2, 4, 128, 256, 128, 3, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 2, 2, 1, false>", 3, 4, 256, 384, 128, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 2, 2, 1, true>", 2, 4, 128, 256, 128, 3, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 2, 2, 2, false>", 3, 4, 256, 384, 128, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 2, 2, 2, true>", 2, 4, 128, 256, 128, 3, 1, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 2, 4, 0, false>", 3, 4, 384, 512, 128, 3, 2, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 2, 4, 0, true>", 3, 4, 128, 128, 128, 1, 1, 0, 0, 1, 0),
    ("conv_igemm_bf16<2, 2, 4, 1, false>", 3, 4, 384, 512, 128, 3, 2, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 2, 4, 1, true>", 3, 4, 128, 128, 128, 1, 1, 0, 0, 1, 1),
    ("conv_igemm_bf16<2, 2, 4, 2, false>", 3, 4, 384, 512, 128, 3, 2, 0, 0, 1, 2),
    ("conv_igemm_bf16<2, 2, 4, 2, true>", 3, 4, 128, 128, 128, 1, 1, 0, 0, 1, 2),
    ("conv_igemm_f32<1, 1, 2, 0, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 0, 0),
    ("conv_igemm_f32<1, 1, 2, 0, true>", 1, 4, 4, 4, 12, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<1, 1, 2, 1, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 0, 1),
    ("conv_igemm_f32<1, 1, 2, 2, false>", 1, 2, 4, 4, 12, 3, 2, 0, 0, 0, 2),
    ("conv_igemm_f32<1, 3, 2, 0, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 0, 0),
    ("conv_igemm_f32<1, 3, 2, 0, true>", 1, 4, 4, 4, 96, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<1, 3, 2, 1, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 0, 1),
    ("conv_igemm_f32<1, 3, 2, 2, false>", 1, 4, 4, 4, 96, 3, 2, 0, 0, 0, 2),
    ("conv_igemm_f32<2, 1, 1, 0, false>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 1, 0, true>", 1, 4, 4, 4, 64, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 1, 1, false>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 0, 1),
    ("conv_igemm_f32<2, 1, 1, 2, false>", 1, 4, 4, 4, 64, 3, 2, 0, 0, 0, 2),
    ("conv_igemm_f32<2, 1, 2, 0, false>", 2, 4, 128, 128, 128, 3, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 2, 0, true>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 2, 1, false>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 0, 1),
    ("conv_igemm_f32<2, 1, 2, 2, false>", 2, 4, 128, 128, 128, 1, 1, 0, 0, 0, 2),
    ("conv_igemm_f32<2, 1, 4, 0, false>", 3, 4, 256, 256, 64, 3, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 4, 0, true>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 1, 4, 1, false>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 0, 1),
    ("conv_igemm_f32<2, 1, 4, 2, false>", 3, 4, 256, 256, 64, 1, 1, 0, 0, 0, 2),
    ("conv_igemm_f32<2, 2, 2, 0, false>", 2, 4, 128, 256, 128, 3, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 2, 2, 0, true>", 2, 4, 128, 256, 128, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 2, 2, 1, false>", 2, 4, 128, 256, 128, 1, 1, 0, 0, 0, 1),
    ("conv_igemm_f32<2, 2, 2, 2, false>", 2, 4, 128, 256, 128, 1, 1, 0, 0, 0, 2),
    ("conv_igemm_f32<2, 2, 4, 0, false>", 2, 4, 256, 256, 128, 3, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 2, 4, 0, true>", 2, 4, 256, 256, 128, 1, 1, 0, 0, 0, 0),
    ("conv_igemm_f32<2, 2, 4, 1, false>", 2, 4, 256, 256, 128, 1, 1, 0, 0, 0, 1),
    ("conv_igemm_f32<2, 2, 4, 2, false>", 2, 4, 256, 256, 128, 1, 1, 0, 0, 0, 2),
    ("deconv5s2_small_cout", 1, 16, 4, 4, 4, 5, 2, 1, 0, 0, 0),
]
# name -> (kernel, (B, Cin, H, W, Cout, k, stride, transposed, masked, prec, in_op), form, act, (in_ctot, in_coff, out_ctot, out_coff) or None)
FORM_CASES = {
    "igemm gate + two residuals, relu, partial tiles": ("conv_igemm_f32<2, 1, 1, 0, false>", (2, 24, 34, 18, 40, 3, 1, 0, 0, 0, 0), GATE | RES1 | RES2, RELU, None),
    "igemm bf16 gate + two residuals": ("conv_igemm_bf16<1, 1, 2, 0, false>", (2, 24, 16, 12, 32, 3, 1, 0, 0, 1, 0), GATE | RES1 | RES2, 0, None),
    "channel views, transposed 5x5 s2, bf16": ("conv_igemm_bf16<1, 1, 2, 0, false>", (2, 32, 8, 16, 32, 5, 2, 1, 0, 1, 0), 0, 0, (40, 8, 48, 16)),
    "channel views, masked 5x5": ("conv_igemm_f32<2, 1, 1, 2, false>", (1, 48, 16, 12, 64, 5, 1, 0, 1, 0, 2), 0, 0, (50, 2, 70, 3)),
    "odd size, partial tile, 3x3 s2": ("conv_igemm_f32<1, 3, 2, 0, false>", (3, 5, 13, 19, 70, 3, 2, 0, 0, 0, 0), 0, 0, None),
    "odd size, direct softmax with gate": ("conv_direct_f32<3>", (2, 16, 13, 19, 3, 3, 1, 0, 0, 0, 0), GATE, SOFTMAX, None),
    "direct, transposed 3x3, two residuals": ("conv_direct_f32<8>", (2, 12, 9, 7, 6, 3, 1, 1, 0, 0, 1), RES1 | RES2, 0, None),
    "deconv 128 -> 3, partial tiles": ("deconv5s2_small_cout", (2, 128, 34, 18, 3, 5, 2, 1, 0, 0, 0), 0, 0, None),
    "conv5s1 gate + residual, odd size": ("conv5s1_small<4>", (2, 6, 13, 19, 3, 5, 1, 0, 0, 0, 0), GATE | RES1, 0, None),
    "F16K output, transposed 5x5 s2": ("conv_igemm_bf16<2, 1, 1, 0, true>", (2, 32, 16, 12, 64, 5, 2, 1, 0, 1, 0), F16K_OUT, RELU, None),
    "F16K output into a wider buffer": ("conv_igemm_bf16<1, 1, 2, 0, true>", (1, 16, 8, 16, 32, 3, 1, 0, 0, 1, 0), F16K_OUT, 0, (16, 0, 64, 16)),
}


def cases():
    out = [{"name": kernel, "kernel": kernel, "shape": tuple(t), "form": 0, "act": 0, "view": None} for kernel, *t in ROW_CASES]
    out += [{"name": n, "kernel": k, "shape": t, "form": f, "act": a, "view": v} for n, (k, t, f, a, v) in FORM_CASES.items()]
    return out


def form_of(c):
    return c["form"]


def desc_of(c):
    from masic_amd import ops
    B, Cin, H, W, Cout, k, s, tr, masked, prec, in_op = c["shape"]
    in_ctot, in_coff, out_ctot, out_coff = c["view"] or (Cin, 0, Cout, 0)
    return ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=bool(tr), masked=bool(masked), in_ctot=in_ctot, in_coff=in_coff,
                              out_ctot=out_ctot, out_coff=out_coff, in_op=in_op, act=c["act"], gate_ctot=2 if c["form"] & GATE else 0,
                              gate_c=1 if c["form"] & GATE else 0, prec=prec)


def _sha(t):
    import torch
    t = t.contiguous().view(-1).view(torch.int32)
    if t.numel() > (1 << 18):
        rows = torch.nn.functional.pad(t, (0, -t.numel() % 4096)).view(-1, 4096).to(torch.int64)
        weight = torch.arange(1, rows.shape[0] + 1, device=t.device, dtype=torch.int64)[:, None]
        t = torch.stack([rows.sum(0), (rows * weight).sum(0)])
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digests(dev="cuda"):
    """{case name: sha256 hex of the output buffer}; a float32 output buffer is pre-filled, so channels outside a view are hashed too"""
    import torch
    from masic_amd import ops
    out = {}
    for i, c in enumerate(cases()):
        d = desc_of(c)
        B, Cin, H, W, Cout, k, s, tr, masked, prec, in_op = c["shape"]
        g = torch.Generator().manual_seed(4000 + i)
        x = (2.0 * torch.randn(B, d.in_ctot, H, W, generator=g)).to(dev)
        w = (torch.randn((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), generator=g) * (Cin * k * k) ** -0.5).to(dev)
        bias = torch.randn(Cout, generator=g).to(dev)
        gate, res1, res2 = (torch.rand(shape, generator=g).to(dev) if c["form"] & bit else None
                            for bit, shape in ((GATE, (B, 2, d.Ho, d.Wo)), (RES1, (B, Cout, d.Ho, d.Wo)), (RES2, (B, Cout, d.Ho, d.Wo))))
        packed = ops.pack_conv_weight(w, d)
        if c["form"] & F16K_OUT:
            y = ops.conv2d_f16k_out(x, packed, bias, d)
            if c["view"]:      # (the call writes its own channels only: hash those records)
                y = y.view(B, d.out_ctot // 16, d.Ho * d.Wo, 16)[:, d.out_coff // 16:(d.out_coff + Cout) // 16]
            y = y.contiguous().view(-1).view(torch.int32)
        else:
            y = torch.full((B, d.out_ctot, d.Ho, d.Wo), 0.5, device=dev)
            ops.conv2d(x, packed, bias, d, out=y, gate=gate, res1=res1, res2=res2)
        out[c["name"]] = _sha(y)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "coremasic", "mywork"))
    import torch  # noqa: F401  (before the library: both then share torch's HIP runtime)
    from masic_amd import _lib
    D = digests()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        json.dump({"cases": {c["name"]: {"kernel": c["kernel"], "sha256": D[c["name"]]} for c in cases()}}, f, indent=0)
        f.write("\n")
    print(f"{out}: {len(D)} digests (library {_lib.LIB_PATH})")
