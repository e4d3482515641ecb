"""SHA-256 of the outputs of the four F16K kernel families -- conv_f16k / conv_f16k_multi (csrc/conv_f16k.hip), the first analysis
layer (csrc/conv_a.hip), the 1x1 GEMMs (csrc/gemm_f16k.hip) and the resident 3x3 kernel (csrc/conv3x3_resident.hip) -- one case per
entry point and form -> tests/golden/f16k_digest.json.  Needs an MI355X.  These kernels use no atomics, so a library whose kernels,
grids and arguments are those of the recording reproduces every digest.  Inputs: a CPU torch.Generator seeded per case, copied to the
device.  The committed file was written by this script run on commit 5ff276d, the commit BEFORE the four families got a source file
each (all of them were conv_f16k.hip then); regenerate it only from a commit whose bits are meant to become the new reference.

    python tests/golden/make_f16k_digest.py

Every case is at the smallest shape that still has a partial tile or a second co-block: 20 x 24 outputs under 8 x 32 / 16 x 16 tiles,
192 output channels (a full and a half 128-channel block), 480 pixels under the GEMMs' 256-pixel tiles; the resident kernel takes whole
tiles only and gets a second workgroup round instead (288 tiles on 256 persistent workgroups).  The conv_f16k cases carry the kernel
they were recorded on (masic_conv_f16k_kernel_name, asked on the host: kernels()); an output above 1 MiB is folded on the device before
it is hashed, as in make_conv_fwd_digest.py.  tests/test_gpu_f16k_digest.py imports kernels() and digests() from here."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "f16k_digest.json")
RELU, LEAKY = 1, 2                               # MASIC_ACT_*
BF16, FP8 = 1, 2                                 # MASIC_PREC_*
GDN, NOSPLIT, MULTI = 1, 2, 4                    # MASIC_F16K_*


def _desc(B, Cin, H, W, Cout, k, s, tr=False, prec=BF16, **kw):
    from masic_amd import ops
    kw.setdefault("in_ctot", Cin)
    return ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=tr, prec=prec, **kw)


# name -> (descriptor arguments, masic_conv_f16k_kernel_name flags): the conv_f16k cases, whose kernel is a function of the shape
F16K_DESCS = {
    "conv_f16k s2 5x5 128->128 + GDN": (dict(B=1, Cin=128, H=40, W=48, Cout=128, k=5, s=2, out_ctot=128), GDN),
    "conv_f16k transposed s2 5x5 + IGDN, y16_pre": (dict(B=1, Cin=128, H=10, W=12, Cout=128, k=5, s=2, tr=True, out_ctot=128), GDN),
    "conv_f16k 3x3 64->64 res_ex: mask, two residuals, y_pre": (dict(B=2, Cin=64, H=20, W=24, Cout=64, k=3, s=1, out_ctot=64, act=LEAKY), 0),
    "conv_f16k float32 NCHW channel view + gate": (dict(B=1, Cin=128, H=40, W=48, Cout=192, k=5, s=2, out_ctot=200, out_coff=3, act=RELU,
                                                        gate_ctot=2, gate_c=1), 0),
    "conv_f16k few channels + res32": (dict(B=2, Cin=96, H=20, W=24, Cout=32, k=3, s=1), NOSPLIT),
    "conv_f16k depth-to-space": (dict(B=2, Cin=128, H=10, W=12, Cout=32, k=3, s=1), NOSPLIT),
    "conv_f16k_multi four outputs + gate": (dict(B=1, Cin=128, H=40, W=48, Cout=192, k=5, s=2), MULTI),
    "conv_f16k fp8 operands -> F16K": (dict(B=1, Cin=128, H=40, W=48, Cout=128, k=5, s=2, out_ctot=128, prec=FP8), 0),
}


def kernels():
    """{conv_f16k case: the kernel the current library runs it on}: host code only, no GPU"""
    import torch  # noqa: F401  (before the library: both then share torch's HIP runtime)
    from masic_amd import _lib
    out, buf = {}, ctypes.create_string_buffer(96)
    for name, (kw, flags) in F16K_DESCS.items():
        rc = _lib.lib.masic_conv_f16k_kernel_name(ctypes.byref(_desc(**kw)), flags, buf, len(buf))
        out[name] = buf.value.decode() if rc == 0 else None
    return out


def _fold(t):
    import torch
    t = t.contiguous().view(-1)
    t = t.view(torch.int32) if t.element_size() * t.numel() % 4 == 0 else t
    if t.dtype == torch.int32 and t.numel() > (1 << 18):
        rows = torch.nn.functional.pad(t, (0, -t.numel() % 4096)).view(-1, 4096).to(torch.int64)
        weight = torch.arange(1, rows.shape[0] + 1, device=t.device, dtype=torch.int64)[:, None]
        t = torch.stack([rows.sum(0), (rows * weight).sum(0)])
    return t.cpu().numpy().tobytes()


def _sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(_fold(t))
    return h.hexdigest()


class _Rand:
    """the inputs of one case: CPU generator, seeded per case"""

    def __init__(self, seed, dev):
        import torch
        self.g, self.dev, self.torch = torch.Generator().manual_seed(seed), dev, torch

    def n(self, *shape, scale=1.0):
        return (scale * self.torch.randn(*shape, generator=self.g)).to(self.dev)

    def u(self, *shape, lo=0.0, hi=1.0):
        return (lo + (hi - lo) * self.torch.rand(*shape, generator=self.g)).to(self.dev)

    def f16k(self, B, C, H, W, scale=1.0):
        from masic_amd import ops
        return ops.nchw_to_f16k(self.n(B, C, H, W, scale=scale))

    def weight(self, d, scale=1.0):
        shape = (d.Cin, d.Cout, d.KH, d.KW) if d.transposed else (d.Cout, d.Cin, d.KH, d.KW)
        return self.n(*shape, scale=scale * (d.Cin * d.KH * d.KW) ** -0.5)

    def gdn(self, C=128):
        from masic_amd import ops
        return ops.pack_gdn_f16k(self.u(C, lo=0.5, hi=1.5), self.u(C, C, hi=0.2).contiguous())


# ---- conv_f16k / conv_f16k_multi
def _f16k_gdn(name, r):
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, w, b, gp = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.weight(d), r.n(d.Cout), r.gdn()
    return [ops.conv2d_f16k(x, ops.pack_conv_f16k_weight(w, d), b, d, gdn=(gp, False))]


def _f16k_igdn_dual(name, r):
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, w, b, gp = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.weight(d, 2.0), r.n(d.Cout), r.gdn()
    return list(ops.conv2d_f16k_gdn_dual(x, ops.pack_conv_f16k_weight(w, d), b, d, (gp, True), products=1))


def _f16k_res_ex(name, r):
    import torch
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, w, b = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.weight(d), r.n(d.Cout)
    res1, res2, mask = (r.f16k(d.B, 80, d.Ho, d.Wo) for _ in range(3))         # res_ctot = 80 > Cout
    y_pre = torch.full((d.B * 80 * d.Ho * d.Wo,), 0x1234, dtype=torch.int16, device=r.dev)
    y = ops.conv2d_f16k_res(x, ops.pack_conv_f16k_weight(w, d), b, d, res1=res1, res2=res2, res_ctot=80, mask=mask, mask_slope=0.01, y_pre=y_pre)
    return [y, y_pre]


def _f16k_nchw_view_gate(name, r):
    import torch
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, w, b = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.weight(d), r.n(d.Cout)
    gate = r.u(d.B, d.gate_ctot, d.Ho, d.Wo)
    y = torch.full((d.B, d.out_ctot, d.Ho, d.Wo), 0.5, device=r.dev)
    ops.conv2d_f16k(x, ops.pack_conv_f16k_weight(w, d), b, d, out_nchw=y, gate=gate)
    return [y]


def _f16k_few(name, r):
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, b = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.n(32)
    w = r.weight(d)
    w[3:] = 0.0
    b[3:] = 0.0
    return [ops.conv2d_f16k_few(x, ops.pack_conv_f16k_weight(w, d), b, d, 3, res32=r.n(d.B, 3, d.Ho, d.Wo))]


def _f16k_d2s(name, r):
    import torch
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x = r.f16k(d.B, d.Cin, d.Hi, d.Wi)
    wc, bc = ops.deconv_s2_as_conv_weight_dev(r.n(d.Cin, 3, 5, 5, scale=(d.Cin * 25) ** -0.5), r.n(3))
    y = torch.full((d.B, 5, 2 * d.Hi, 2 * d.Wi), 0.5, device=r.dev)
    ops.conv2d_f16k_d2s(x, ops.pack_conv_f16k_weight(wc, d), bc, d, 3, out=y, out_coff=1)
    return [y]


def _f16k_multi(name, r):
    import torch
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x, w, b = r.f16k(d.B, d.Cin, d.Hi, d.Wi), r.weight(d, 4.0), r.n(d.Cout)
    gate = r.u(d.B, 3, d.Ho, d.Wo)
    cat = torch.full((d.B * 224 * d.Ho * d.Wo,), 0x1234, dtype=torch.int16, device=r.dev)
    out = ops.conv2d_f16k_multi(x, ops.pack_conv_f16k_weight(w, d), b, d, round16=cat, round16_ctot=224, round16_coff=16, gate=gate, gate_c=2)
    return [out[k] for k in ("y32", "round32", "round16", "abs16")]


def _f16k_fp8(name, r):
    from masic_amd import ops
    d = _desc(**F16K_DESCS[name][0])
    x8 = ops.nchw_to_f8k(r.n(d.B, d.Cin, d.Hi, d.Wi), 0.02)
    wp, ws = ops.pack_conv_f8k_weight(r.weight(d), d)
    return [ops.conv2d_f8k(x8, wp, (ws * 0.02).contiguous(), r.n(d.Cout), d, out="f16k")]


# ---- first analysis layer: channels 3..5 of a six-channel picture, 40 x 48 -> 20 x 24 (8 x 32 tiles).  The launcher takes the
# wave-private kernel conv_a_gdn_f16k_w for a single-product GDN with an F16K output on an input of W % 4 == 0, and conv_a_gdn_f16k for
# everything else: W = 50 below, and every other form.
def _conv_a(form, W=48):
    def run(name, r):
        from masic_amd import ops
        x = r.u(2, 6, 40, W)
        wp = ops.pack_conv_a_weight(r.n(128, 3, 5, 5, scale=75 ** -0.5))
        b, gp = r.n(128), (r.gdn(), False)
        if form == "gdn":
            return [ops.conv_a_gdn_f16k(x, wp, b, gp, in_coff=3)[0]]
        if form == "x3":
            ops.set_fused_gdn_products(3)
            try:
                return [ops.conv_a_gdn_f16k(x, wp, b, gp, in_coff=3)[0]]
            finally:
                ops.set_fused_gdn_products(1)
        if form == "dual":
            return list(ops.conv_a_gdn_dual(x, wp, b, gp, in_coff=3, products=1)[:2])
        if form == "f8k":
            return [ops.conv_a_gdn_f8k(x, wp, b, gp, 0.05, in_coff=3)[0]]
        return [ops.conv_a_f16k(x, wp, b, in_coff=3)[0]]
    return run


# ---- 1x1 layers: 480 pixels (two 256-pixel tiles, the second partial), 192 output channels (two co-blocks, the second half full)
def _gemm_bf16(B, nchw):
    def run(name, r):
        import torch
        from masic_amd import ops
        x, w, b = r.f16k(B, 128, 20, 24), r.n(192, 128, scale=128 ** -0.5), r.n(192)
        wp = ops.pack_gemm_f16k_weight(w, 128, 192, False)
        if not nchw:
            return [ops.gemm_f16k(x, wp, b, B, 128, 192, 20, 24, LEAKY)]
        y = torch.full((B, 200, 20, 24), 0.5, device=r.dev)
        ops.gemm_f16k(x, wp, b, B, 128, 192, 20, 24, RELU, out_nchw=y, out_coff=5)
        return [y]
    return run


def _gemm_layers(r, shapes, B):
    from masic_amd import ops
    layers = []
    for Cin, Cout, act, out in shapes:
        x, w, b = r.f16k(B, Cin, 20, 24), r.n(Cout, Cin, scale=Cin ** -0.5), r.n(Cout)
        layers.append(dict(x=x, wp=ops.pack_gemm_f16k_weight(w, Cin, Cout, False), bias=b, Cin=Cin, Cout=Cout, act=act, out=out, out_scale=0.05))
    return layers


def _gemm_group3(name, r):
    from masic_amd import ops
    return ops.gemm_f16k_group(_gemm_layers(r, [(128, 192, LEAKY, "f16k"), (192, 96, 0, "nchw"), (64, 288, RELU, "f16k")], 2), 2, 20, 24)


def _gemm_f8_out(name, r):
    from masic_amd import ops
    return ops.gemm_f16k_group(_gemm_layers(r, [(128, 192, LEAKY, "f8k")], 2), 2, 20, 24)


def _gemm_fp8(name, r):
    from masic_amd import ops
    x8 = ops.nchw_to_f8k(r.n(2, 128, 20, 24), 0.02)
    wp, ws = ops.pack_gemm_f8k_weight(r.n(192, 128, scale=128 ** -0.5), 128, 192, False)
    return [ops.gemm_f8k(x8, wp, (ws * 0.02).contiguous(), r.n(192), 2, 128, 192, 20, 24, LEAKY, out="f16k")]


# ---- resident 3x3
def _c3(B, Cin, Cout, H, W, form):
    def run(name, r):
        from masic_amd import ops
        x = r.f16k(B, Cin, H, W)
        wp = ops.pack_conv3x3_resident_weight(r.n(Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5))
        b = r.n(Cout)
        if form == "plain":
            return [ops.conv3x3_resident(x, wp, b, B, Cin, Cout, H, W, act=LEAKY)]
        res1, res2, mask = (r.f16k(B, Cout, H, W) for _ in range(3))
        if form == "res":
            y_pre = r.f16k(B, Cout, H, W)
            return [ops.conv3x3_resident(x, wp, b, B, Cin, Cout, H, W, act=LEAKY, res1=res1, res2=res2, res_ctot=Cout, mask=mask, mask_slope=0.01,
                                         y_pre=y_pre), y_pre]
        out, mask2 = [], r.f16k(B, Cout, H, W)
        for sum_of in (1, 2):
            out += list(ops.conv3x3_resident(x, wp, b, B, Cin, Cout, H, W, res1=res1, res2=res2, res_ctot=Cout, mask=mask, mask_slope=0.01,
                                             mask2=mask2, mask2_slope=0.0, sum_of=sum_of))
        return out
    return run


CASES = {
    "conv_f16k s2 5x5 128->128 + GDN": _f16k_gdn,
    "conv_f16k transposed s2 5x5 + IGDN, y16_pre": _f16k_igdn_dual,
    "conv_f16k 3x3 64->64 res_ex: mask, two residuals, y_pre": _f16k_res_ex,
    "conv_f16k float32 NCHW channel view + gate": _f16k_nchw_view_gate,
    "conv_f16k few channels + res32": _f16k_few,
    "conv_f16k depth-to-space": _f16k_d2s,
    "conv_f16k_multi four outputs + gate": _f16k_multi,
    "conv_f16k fp8 operands -> F16K": _f16k_fp8,
    "conv_a_gdn_f16k_w: in_ctot 6, in_coff 3": _conv_a("gdn"),
    "conv_a_gdn_f16k: in_ctot 6, in_coff 3, W = 50": _conv_a("gdn", W=50),
    "conv_a_gdn_f16k dual (y_pre)": _conv_a("dual"),
    "conv_a_fwd (no GDN)": _conv_a("plain"),
    "conv_a_gdn_f16k fp8 output": _conv_a("f8k"),
    "conv_a_gdn_f16k products = 3": _conv_a("x3"),
    "gemm_f16k2 128->192, B = 2": _gemm_bf16(2, False),
    "gemm_f16k2 128->192, B = 9, float32 NCHW view": _gemm_bf16(9, True),
    "gemm_f16k2 three-layer group": _gemm_group3,
    "gemm_f16k<2> bf16 operands, fp8 output": _gemm_f8_out,
    "gemm_f16k<4, true> fp8 operands": _gemm_fp8,
    "conv3x3_resident 3->32, 16x32": _c3(2, 3, 32, 16, 32, "plain"),
    "conv3x3_resident 32->32, mask + residuals + y_pre": _c3(2, 32, 32, 16, 32, "res"),
    "conv3x3_resident 64->64 ex: y2, sum_of 1 and 2, 8x32": _c3(2, 64, 64, 8, 32, "ex"),
    "conv3x3_resident 64->64, 288 tiles on 256 workgroups": _c3(3, 64, 64, 64, 384, "plain"),
}
assert set(F16K_DESCS) <= set(CASES)


def digests(dev="cuda"):
    """{case name: sha256 hex of the output buffers}; a buffer written through a view is pre-filled, so what lies outside it is hashed too"""
    import torch
    from masic_amd import ops
    products = ops._FUSED_GDN_PRODUCTS
    ops.set_fused_gdn_products(1)
    try:
        out = {name: _sha(fn(name, _Rand(7000 + i, dev))) for i, (name, fn) in enumerate(CASES.items())}
        torch.cuda.synchronize()
    finally:
        ops.set_fused_gdn_products(products)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "coremasic", "mywork"))
    import torch  # noqa: F401  (before the library: both then share torch's HIP runtime)
    from masic_amd import _lib
    D, K = digests(), kernels()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        json.dump({"cases": {n: {"kernel": K.get(n), "sha256": D[n]} for n in CASES}}, f, indent=0)
        f.write("\n")
    print(f"{out}: {len(D)} digests (library {_lib.LIB_PATH})")
