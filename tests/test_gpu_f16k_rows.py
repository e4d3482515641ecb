"""Every kernel instantiation of F16K_ROWS (masic_amd/csrc/conv_f16k.hip) and every epilogue form of its entry points against the
float64 reference of tests/f16k_ref.py: one hard case per row (ragged tiles in both directions, a batch, a patch ring that wraps,
padding taps, a partly empty co-block, a sub-block past the last channel -- tests/f16k_row_cases.py: the table and the search that
wrote it), the geometry the table does not force, and the forms.  tests/test_cpu_f16k_rows.py holds every case to its kernel and to
its properties without a GPU.

Each row and geometry case runs twice.
(a) Whole-number operands (f16k_ref.inputs(integers=True)) under the asserted bound max|x| max|w| Cin k k + max|bias| < 2^24: every
    partial sum is exact in float32 in any order, so the float32 NCHW output must equal the float64 reference bit for bit and the F16K
    output that reference rounded once to bf16.  GDN rows: the pre-GDN output of gdn_dual.  The two fp8 GDN rows have no gdn_dual (it
    takes no dequantisation scales): they run an inverse GDN with gamma^ = 0, beta^ = 1, i.e. y = x * sqrt(0 + 1) -- the norm is an
    exact 1, the square root of 1 is 1 and x * 1 is x -- and must equal the reference bit for bit as well, float32 and F16K.  Multi
    rows: all four layouts, with half-integer biases so that round() meets ties and -0.
(b) Real-valued operands, float32 NCHW output, the project's gates: 2e-5 of the reference's peak for the convolution, 5e-5 for the
    three-product GDN, 2^-9 for the one-product GDN.  The one-product form rounds gamma^ and x^2 to bf16 and may be off by 2^-8 q of
    the peak, q = f16k_ref.one_product_share <= 1 the part of the norm that is gamma^ x^2: 2^-9 follows for a correct kernel only
    where q <= 1/2.  It is therefore asserted twice: on the operands as drawn against f16k_ref.one_product_bound(q) = 2^-8 q + 2^-14
    (q from the reference alone; 0.85 ... 1 here), and against 2^-9 itself on the same operands times the power of two at which
    q <= 0.45.  Multi rows: y32 at 2e-5; round32, round16 and abs16 are held bit for bit to what they promise of the y32 the kernel
    stored -- for those three layouts run (a) alone is the comparison with the reference.
Forms: exact where the float32 epilogue is replicated (whole-number operands and residuals, power-of-two gates, ReLU); the leaky /
mask-slope case at 2^-8; gdn_dual into a view bit for bit before the GDN on whole numbers, and on real operands at the F16K gates
(2^-8 before the GDN; after it 2^-8 + one_product_bound(q) as drawn and 2^-8 + 2^-9 scaled).  Everything outside an
output view keeps its prefill exactly.  Measured errors: DESIGN.md section 2.2."""
import ctypes

import numpy as np
import pytest
import torch

from tests import f16k_ref as R
from tests import f16k_row_cases as T
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS = T.row_cases() + T.geometry_cases()
FORMS = T.form_cases()


def _dev(t):
    return None if t is None else t.to(DEV)


def _packed(c, x, w, d):
    """(input buffer, packed weights, dequantisation scales or None) on the device"""
    from masic_amd import ops
    if c.prec == R.PREC_FP8:
        wp, ws = ops.pack_conv_f8k_weight(_dev(w), d)
        return _dev(R.to_f8k(x)), wp, ws           # unit input scale: the scales of the call are the weight scales
    return _dev(R.to_f16k(x)), ops.pack_conv_f16k_weight(_dev(w), d), None


def _conv(c, x16, wp, ws, bias, d, out, gdn=None):
    from masic_amd import ops
    if c.prec == R.PREC_FP8:
        return ops.conv2d_f8k(x16, wp, ws, _dev(bias), d, out=out, gdn=gdn)
    return ops.conv2d_f16k(x16, wp, _dev(bias), d, want_nchw=out == "nchw", gdn=gdn)


def _gdn_params(seed, identity=False):
    from masic_amd import synth
    if identity:
        return torch.ones(128), torch.zeros(128, 128)
    rs = np.random.RandomState(seed)
    return synth.synth_tensor("g.beta", (128,), rs), synth.synth_tensor("g.gamma", (128, 128), rs)


def _report(entry, run, gate, err):
    print(f"f16k_rows | {entry.id} | {entry.kernel} | {tuple(entry.case[:9])} | {run} | gate {gate} | error {err:.3e}")


def _multi_bias(bias):
    return bias + 0.5 * (torch.arange(bias.numel()) % 2).float()


def _check_multi(entry, out, v64, gate, exact, cat=None):
    """the four layouts of conv_f16k_multi: exact -> against the reference bit for bit; else y32 at the gate and the rest as functions of it"""
    c = entry.case
    Ho, Wo = R.out_hw(c)
    y32 = out["y32"].cpu()
    if exact:
        ref = R.multi_ref(v64, gate)
        assert torch.equal(y32, ref["y32"]), f"{entry.id}: y32"
    else:
        e = assert_close(y32, v64, entry.id + ": y32", 2e-5)
        _report(entry, "(b) real operands, y32", "2.0e-05", e)
        ref = R.multi_ref(y32.double(), gate)
    assert torch.equal(R.bits(out["round32"].cpu()), R.bits(ref["round32"])), f"{entry.id}: round32 (ties to even, the sign of zero)"
    assert torch.equal(R.bits(R.from_f16k(out["abs16"], c.B, c.Cout, Ho, Wo)), R.bits(ref["abs16"])), f"{entry.id}: abs16"
    if cat is None:
        assert torch.equal(R.bits(R.from_f16k(out["round16"], c.B, c.Cout, Ho, Wo)), R.bits(ref["round16"])), f"{entry.id}: round16"
    else:
        ctot, coff = cat
        want = R.in_view(ref["round16"], ctot, coff)
        assert torch.equal(R.bits(R.from_f16k(out["round16"], c.B, ctot, Ho, Wo)), R.bits(want)), f"{entry.id}: gated round16 view, prefill outside"


@pytest.mark.parametrize("entry", LAYERS, ids=[e.id for e in LAYERS])
def test_f16k_row_vs_float64(entry):
    from masic_amd import ops
    c, seed = entry.case, T.seed_of(entry)
    r = T.row_params(entry.kernel)
    Ho, Wo = R.out_hw(c)
    d = R.desc_of(c)
    assert T.plan(c)[0] == entry.kernel

    # ---- (a) whole-number operands: exact
    x, w, bias = R.inputs(c, seed, integers=True)
    if r["MULTI"]:
        bias = _multi_bias(bias)
    assert R.exact_bound(c, x, w, bias) < 2 ** 24, "every partial sum must be a float32 integer (half-integer for the multi rows)"
    ref = R.conv64(c, x, w, bias)
    x16, wp, ws = _packed(c, x, w, d)
    if r["MULTI"]:
        _check_multi(entry, ops.conv2d_f16k_multi(x16, wp, _dev(bias), d), ref, None, True)
        _report(entry, "(a) whole numbers, four layouts", "exact", 0.0)
    elif r["GDN"] and not r["F8"]:
        gp = ops.pack_gdn_f16k(*[_dev(t) for t in _gdn_params(seed)])
        pre, _ = ops.conv2d_f16k_gdn_dual(x16, wp, _dev(bias), d, (gp, bool(c.transposed)))
        got = R.from_f16k(pre, c.B, c.Cout, Ho, Wo)
        _report(entry, "(a) whole numbers, pre-GDN F16K", "exact", rel_err(got.float(), ref.bfloat16().float()))
        assert torch.equal(got.float(), ref.bfloat16().float()), f"{entry.id}: pre-GDN output of gdn_dual"
    elif r["GDN"]:
        gp = ops.pack_gdn_f16k(*[_dev(t) for t in _gdn_params(seed, identity=True)])
        y32 = _conv(c, x16, wp, ws, bias, d, "nchw", gdn=(gp, True)).cpu()
        y16 = R.from_f16k(_conv(c, x16, wp, ws, bias, d, "f16k", gdn=(gp, True)), c.B, c.Cout, Ho, Wo)
        _report(entry, "(a) whole numbers, identity inverse GDN, float32 NCHW and F16K", "exact", max(rel_err(y32, ref), rel_err(y16.float(), ref.bfloat16().float())))
        assert torch.equal(y32.double(), ref), f"{entry.id}: x * sqrt(0 + 1), float32 NCHW"
        assert torch.equal(y16.float(), ref.bfloat16().float()), f"{entry.id}: x * sqrt(0 + 1), F16K"
    else:
        y32 = _conv(c, x16, wp, ws, bias, d, "nchw").cpu()
        y16 = R.from_f16k(_conv(c, x16, wp, ws, bias, d, "f16k"), c.B, c.Cout, Ho, Wo)
        _report(entry, "(a) whole numbers, float32 NCHW and F16K", "exact", max(rel_err(y32, ref), rel_err(y16.float(), ref.bfloat16().float())))
        assert torch.equal(y32.double(), ref), f"{entry.id}: exact operands, exact sums: float32 NCHW"
        assert torch.equal(y16.float(), ref.bfloat16().float()), f"{entry.id}: exact operands, exact sums: only the one bf16 rounding is left"

    # ---- (b) real-valued operands: the project's gates
    x, w, bias = R.inputs(c, seed + 500)
    ref = R.conv64(c, x, w, bias)
    x16, wp, ws = _packed(c, x, w, d)
    if r["MULTI"]:
        _check_multi(entry, ops.conv2d_f16k_multi(x16, wp, _dev(bias), d), ref, None, False)
    elif r["GDN"]:
        beta, gamma = _gdn_params(seed)
        inverse = bool(c.transposed)
        gref = R.gdn64(ref, beta, gamma, inverse)
        gp = ops.pack_gdn_f16k(_dev(beta), _dev(gamma))
        products = ops._FUSED_GDN_PRODUCTS
        try:
            ops.set_fused_gdn_products(3)
            e = rel_err(_conv(c, x16, wp, ws, bias, d, "nchw", gdn=(gp, inverse)), gref)
            _report(entry, f"(b) real operands, 3-product {'I' if inverse else ''}GDN", "5.0e-05", e)
            assert e <= 5e-5, f"{entry.id}: 3-product GDN: {e:.3e} > 5e-5"
            # one product: on the same operands against the bound derived for them, and against the gate itself on operands scaled by the
            # power of two s at which it is derived (f16k_ref.one_product_share) -- x and the bias times s; fp8 rows take s as the input
            # scale of the dequantisation factors
            ops.set_fused_gdn_products(1)
            e = rel_err(_conv(c, x16, wp, ws, bias, d, "nchw", gdn=(gp, inverse)), gref)
            q1 = R.one_product_share(ref, beta, gamma, inverse)
            _report(entry, f"(b) real operands, 1-product {'I' if inverse else ''}GDN (share {q1:.2f})", f"{R.one_product_bound(q1):.2e}", e)
            assert e <= R.one_product_bound(q1), f"{entry.id}: 1-product GDN: {e:.3e} > 2^-8 * {q1:.3f} + 2^-14"
            s = R.one_product_scale(ref, beta, gamma, inverse)
            q = R.one_product_share(s * ref, beta, gamma, inverse)
            assert q <= 0.45
            if c.prec == R.PREC_FP8:
                xs, wss = x16, (ws * s).contiguous()
            else:
                xs, wss = _dev(R.to_f16k(x * s)), None
            es = rel_err(_conv(c, xs, wp, wss, bias * s, d, "nchw", gdn=(gp, inverse)), R.gdn64(s * ref, beta, gamma, inverse))
            _report(entry, f"(b) real operands times {s:g}, 1-product {'I' if inverse else ''}GDN (share {q:.2f})", "2^-9", es)
            assert es <= 2.0 ** -9, f"{entry.id}: 1-product GDN: {es:.3e} > 2^-9"
        finally:
            ops.set_fused_gdn_products(products)
    else:
        y32 = _conv(c, x16, wp, ws, bias, d, "nchw")
        e = rel_err(y32, ref)
        _report(entry, "(b) real operands, float32 NCHW", "2.0e-05", e)
        assert_close(y32, ref, entry.id, 2e-5)


# ------------------------------------------------------------------------------------------------ the forms
def _ints(g, shape, top):
    return torch.randint(-top, top + 1, shape, generator=g).float()


def _gates(g, shape):
    return torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0])[torch.randint(0, 5, shape, generator=g)]


def _prefilled16(n):
    return torch.full((n,), R.PREFILL_BITS, dtype=torch.int16, device=DEV)


@pytest.mark.parametrize("entry", FORMS, ids=[e.id for e in FORMS])
def test_f16k_form_vs_float64(entry):
    from masic_amd import ops
    c, seed, what = entry.case, T.seed_of(entry), entry.id[len("form "):]
    B, C = c.B, c.Cout
    Ho, Wo = R.out_hw(c)
    g = torch.Generator().manual_seed(seed + 1)
    assert T.plan(c)[0] == entry.kernel
    real = what.startswith(("res_ex leaky", "gdn_dual"))
    x, w, bias = R.inputs(c, seed, integers=not real)
    if what.startswith("few"):
        w[3:], bias[3:] = 0.0, 0.0
    if what.startswith("depth"):
        wt, bt = _ints(g, (c.Cin, 3, 5, 5), 4), _ints(g, (3,), 20)
        w, bias = R.d2s_weight(wt, bt)
    if what.startswith("multi"):
        bias = _multi_bias(bias)
    if not real:
        assert R.exact_bound(c, x, w, bias) < 2 ** 24
    x16 = _dev(R.to_f16k(x))

    if what.startswith("res_ex"):
        leaky = c.act == R.ACT_LEAKY
        slope = 0.01 if leaky else 0.0
        d = R.desc_of(c, out_ctot=96, out_coff=16)
        wp = ops.pack_conv_f16k_weight(_dev(w), d)
        draw = (lambda: torch.randn(B, 80, Ho, Wo, generator=g).bfloat16().float()) if leaky else (lambda: _ints(g, (B, 80, Ho, Wo), 64))
        res1, res2 = draw(), draw()
        mask = draw() if leaky else _ints(g, (B, 80, Ho, Wo), 2)       # (whole numbers: zeros among them, act'(0) is the slope)
        y16, pre16 = _prefilled16(B * 96 * Ho * Wo), _prefilled16(B * 80 * Ho * Wo)
        ops.conv2d_f16k_res(x16, wp, _dev(bias), d, y16=y16, res1=_dev(R.to_f16k(res1)), res2=_dev(R.to_f16k(res2)), res_ctot=80,
                            mask=_dev(R.to_f16k(mask)), mask_slope=slope, y_pre=pre16)
        v, pre = R.epilogue32(R.conv64(c, x, w, bias), c.act, mask=mask[:, :C], slope=slope, res1=res1[:, :C], res2=res2[:, :C])
        y, yp = R.from_f16k(y16, B, 96, Ho, Wo).float(), R.from_f16k(pre16, B, 80, Ho, Wo).float()
        assert bool((y[:, :16] == R.PREFILL).all()) and bool((y[:, 16 + C:] == R.PREFILL).all()) and bool((yp[:, C:] == R.PREFILL).all()), "prefill"
        if leaky:
            err = max(rel_err(y[:, 16:16 + C], v.double()), rel_err(yp[:, :C], pre.double()))
            _report(entry, "real operands, y and y_pre F16K", "2^-8", err)
            assert_close(y[:, 16:16 + C], v.double(), what + ": y", 2.0 ** -8)
            assert_close(yp[:, :C], pre.double(), what + ": y_pre", 2.0 ** -8)
            return
        else:
            assert torch.equal(y[:, 16:16 + C], v.bfloat16().float()) and torch.equal(yp[:, :C], pre.bfloat16().float()), what
    elif what.startswith("few"):
        d = R.desc_of(c)
        res32 = _ints(g, (B, 3, Ho, Wo), 100)
        y = ops.conv2d_f16k_few(x16, ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias), d, 3, res32=_dev(res32))
        assert torch.equal(y.cpu(), R.few_ref(R.conv64(c, x, w, bias), c.act, res32, 3)), what
    elif what.startswith("depth"):
        d = R.desc_of(c)
        out = torch.full((B, 5, 2 * c.H, 2 * c.W), R.PREFILL, device=DEV)
        ops.conv2d_f16k_d2s(x16, ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias), d, 3, out=out, out_coff=1)
        ref = torch.nn.functional.conv_transpose2d(x.double(), wt.double(), bt.double(), stride=2, padding=2, output_padding=1)
        assert torch.equal(out.cpu().double(), R.in_view(ref, 5, 1)), what
    elif what.startswith("gdn_dual"):
        d = R.desc_of(c, out_ctot=160, out_coff=16)
        beta, gamma = _gdn_params(seed)
        gp = ops.pack_gdn_f16k(_dev(beta), _dev(gamma))

        def dual(xx, bb):
            """(pre-GDN, GDN) of one launch into prefilled buffers of 160 channels, as float32 NCHW; everything outside the view checked"""
            x16, bd = _dev(R.to_f16k(xx)), _dev(bb)
            pre16, y16 = _prefilled16(B * 160 * Ho * Wo), _prefilled16(B * 160 * Ho * Wo)
            ops.check(ops.lib.masic_conv_f16k_gdn_dual_fwd(ops._p(x16), ops._p(wp), ops._p(bd), ops._p(gp), ops._gdn_flags(False, 1), ops._p(pre16),
                                                           ops._p(y16), ctypes.byref(d), ops._stream()), "conv_f16k_gdn_dual_fwd")
            pre, y = R.from_f16k(pre16, B, 160, Ho, Wo).float(), R.from_f16k(y16, B, 160, Ho, Wo).float()
            for t in (pre, y):
                assert bool((t[:, :16] == R.PREFILL).all()) and bool((t[:, 16 + C:] == R.PREFILL).all()), "prefill"
            return pre[:, 16:16 + C], y[:, 16:16 + C]

        # whole numbers (same weights rounded as f16k_ref.inputs does): conv + bias and one rounding to bf16, bit for bit in the view
        xi, wi, bi = R.inputs(c, seed, integers=True)
        assert R.exact_bound(c, xi, wi, bi) < 2 ** 24
        wp = ops.pack_conv_f16k_weight(_dev(wi), d)
        pre, _ = dual(xi, bi)
        _report(entry, "whole numbers, pre-GDN F16K", "exact", rel_err(pre, R.conv64(c, xi, wi, bi).bfloat16().float()))
        assert torch.equal(pre, R.conv64(c, xi, wi, bi).bfloat16().float()), what + ": pre-GDN, whole numbers"
        # real operands as drawn, then times the power of two at which the one-product gate is derived (f16k_ref.one_product_share)
        wp = ops.pack_conv_f16k_weight(_dev(w), d)
        ref = R.conv64(c, x, w, bias)
        s = R.one_product_scale(ref, beta, gamma, False)
        for sc in (1.0, s):
            rs, q = sc * ref, R.one_product_share(sc * ref, beta, gamma, False)
            gate, text = (2.0 ** -8 + R.one_product_bound(q), f"2^-8 + {R.one_product_bound(q):.2e}") if sc == 1.0 else (2.0 ** -8 + 2.0 ** -9, "2^-8 + 2^-9")
            assert sc == 1.0 or q <= 0.45
            pre, y = dual(x * sc, bias * sc)
            gref = R.gdn64(rs, beta, gamma, False)
            _report(entry, f"real operands times {sc:g}, pre-GDN F16K", "2^-8", rel_err(pre, rs))
            _report(entry, f"real operands times {sc:g}, 1-product GDN, F16K (share {q:.2f})", text, rel_err(y, gref))
            assert_close(pre, rs, what + ": pre-GDN", 2.0 ** -8)
            assert_close(y, gref, what + ": GDN", gate)
        return
    elif what.startswith("gated F16K"):
        d = R.desc_of(c, out_ctot=192, out_coff=16, gate_ctot=3, gate_c=1)
        gate = _gates(g, (B, 3, Ho, Wo))
        buf = _prefilled16(B * 192 * Ho * Wo)
        ops.conv2d_f16k(x16, ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias), d, out16=buf, gate=_dev(gate))
        v, _ = R.epilogue32(R.conv64(c, x, w, bias), c.act, gate=gate[:, 1:2])
        assert torch.equal(R.from_f16k(buf, B, 192, Ho, Wo).float(), R.in_view(v.bfloat16().float(), 192, 16)), what
    elif what.startswith("gated float32"):
        d = R.desc_of(c, out_ctot=200, out_coff=3, gate_ctot=2, gate_c=1)
        gate = _gates(g, (B, 2, Ho, Wo))
        out = torch.full((B, 200, Ho, Wo), R.PREFILL, device=DEV)
        ops.conv2d_f16k(x16, ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias), d, out_nchw=out, gate=_dev(gate))
        v, _ = R.epilogue32(R.conv64(c, x, w, bias), c.act, gate=gate[:, 1:2])
        assert torch.equal(out.cpu(), R.in_view(v, 200, 3)), what
    elif what.startswith("fp8 output"):
        d = R.desc_of(c, out_ctot=224, out_coff=32)
        ref = R.conv64(c, x, w, bias).float()
        scale = 2.0 ** int(np.ceil(np.log2(float(ref.abs().max()) / 448.0)))       # a power of two: v / scale is exact
        y8 = torch.full((B * 224 * Ho * Wo,), 0x38, dtype=torch.uint8, device=DEV)  # e4m3 1.0
        wp, bd = ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias)      # (named: they must outlive the launch)
        ops.check(ops.lib.masic_conv_f8k_fwd(ops._p(x16), ops._p(wp), None, ops._p(bd), None, None, 0, None, None, ops._p(y8), 1.0 / scale, ctypes.byref(d),
                                             ops._stream()), "conv_f8k_fwd")
        got = R.from_f8k(y8, B, 224, Ho, Wo)
        assert torch.equal(got * scale, R.in_view(R.fp8_out_ref(ref, scale), 224, 32, scale)), what
    else:
        assert what.startswith("multi")
        d = R.desc_of(c)
        gate = _gates(g, (B, 3, Ho, Wo))
        cat = _prefilled16(B * 224 * Ho * Wo)
        out = ops.conv2d_f16k_multi(x16, ops.pack_conv_f16k_weight(_dev(w), d), _dev(bias), d, round16=cat, round16_ctot=224, round16_coff=16,
                                    gate=_dev(gate), gate_c=2)
        _check_multi(entry, out, R.conv64(c, x, w, bias), gate[:, 2:3], True, cat=(224, 16))
    _report(entry, "whole numbers", "exact", 0.0)
