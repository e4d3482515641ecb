"""Every persistent-workgroup kernel with more tiles than workgroups, against float64 (tests/tile_loop_cases.py: the shapes and what
makes them hard; tests/test_cpu_tile_loops.py holds them to that without a GPU).  The small-shape tests of these kernels run every
workgroup's loop body once; here the prologue prefetch of the second tile, the in-loop prefetch, the ring wrap and the counted waits on
the back edge decide values that are checked.

conv_a (8 forms) and the resident 3x3 kernel (5 channel pairs, plain and EX) run twice, as tests/test_gpu_f16k_rows.py does:
(a) whole-number operands under an asserted exact_bound < 2^24: every partial sum is a float32 integer in any order, so the F16K
    output must equal the float64 reference rounded once to bf16, bit for bit -- conv_a: the plain convolution, the pre-GDN output of
    the dual form, and the GDN forms through an inverse GDN with gamma^ = 0, beta^ = 1 (y = x sqrt(0 + 1)), one- and three-product,
    F16K and fp8 (f16k_ref.fp8_out_ref at a power-of-two scale); resident: y, y_pre, y2 with whole-number residuals and masks, ReLU or
    no activation and mask slope 0 (the float32 epilogue of f16k_ref.epilogue32 is exact), the prefill outside the output view, and
    the channel sums, exact in any order because the reference's sum of |stored value| per channel is asserted < 2^24.
(b) real operands at the project's gates: conv_a 2^-8 before the GDN, 2^-8 + one_product_bound(q) after it as drawn and 2^-8 + 2^-9
    on the operands times one_product_scale, 2^-8 + 5e-5 for the three-product form (the fp8 store has no gate of its own: run (a)
    is its check); resident: LeakyReLU and mask slope 0.01 at 2^-8 of the peak (y2 too: where mask2 > 0 it is bf16(y) itself, elsewhere
    two roundings of a value a hundred times below the peak).
gdn_fwd: 2e-5 (float32), 5e-5 (bf16x3), 2^-8 (F16K store), both directions.
gdn_bwd: the float64 emulation with the kernel's roundings (f16k_ref.gdn_bwd_emulation) at 2e-3 of the peak and float64 autograd at
    3e-2, the gates of test_gdn_backward_fused_bf16; dx, d beta, d gamma bit for bit across the four operand combinations; the F16K and
    bf16 dx = the float32 dx rounded once; the channel sums at 1e-5 of max sum |dx|.
pic_wgrad: 2e-5 of the peak against float64 conv2d_weight on the bf16-rounded operands, both layer orientations, and the q channel view.
(c) selective support for the two reductions, where one lost tile would be diluted in a sum over 65 000 pixels: g (gdn_bwd) / p
    (pic_wgrad) is zero outside three tiles -- the first of the second round (index = the plan's grid), the first of the last round,
    the ragged last one -- and d gamma, d beta, the channel sums and dW must be that set's contribution alone, at the same gates of its
    own peak; dx must be exactly zero off the set.
One report line per check: kernel, shape, ntiles/grid, run, gate, measured error."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f16k_ref as R
from tests import tile_loop_cases as T
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _family(name):
    return [c for c in T.CASES if c.family == name]


def _ids(cases):
    return [T.case_id(c) for c in cases]


def _report(c, run, gate, err):
    m, v, _ = T.plan(c)
    assert m.kernel == c.kernel and v["ntiles"] > m.grid[0]
    print(f"tile_loops | {c.kernel} | {tuple(c.shape)} | {v['ntiles']}/{m.grid[0]} | {run} | gate {gate} | error {err:.3e}")


def _hold(c, run, got, ref, gate, text=None):
    """report, then assert max |got - ref| <= gate * max |ref|"""
    e = rel_err(got, ref)
    _report(c, run, text or f"{gate:.1e}", e)
    assert e <= gate, f"{T.case_id(c)}: {run}: {e:.3e} > {text or gate}"


def _same(c, run, got, want):
    """report, then assert equality of two device tensors (whole numbers: -0 does not occur apart from products with a zero slope)"""
    bad = int((got != want).sum())
    _report(c, run, "exact", float((got.double() - want.double()).abs().max()) / max(float(want.abs().max()), 1.0))
    assert bad == 0, f"{T.case_id(c)}: {run}: {bad} of {want.numel()} elements differ"


def _to16(x):
    """float32 NCHW on the CPU -> F16K on the device, packed by the reference's own torch ops"""
    return R.to_f16k(x).to(DEV)


def _nchw(y16, B, C, H, W):
    """F16K buffer on the device -> float32 NCHW on the device (the layout of f16k_ref.from_f16k, torch ops)"""
    return y16.view(torch.bfloat16).reshape(B, C // 16, H * W, 16).permute(0, 1, 3, 2).reshape(B, C, H, W).float()


def _prefilled16(n):
    return torch.full((n,), R.PREFILL_BITS, dtype=torch.int16, device=DEV)


def _gdn_params(seed, identity=False):
    from masic_amd import synth
    if identity:
        return torch.ones(128), torch.zeros(128, 128)
    rs = np.random.RandomState(seed)
    return synth.synth_tensor("g.beta", (128,), rs), synth.synth_tensor("g.gamma", (128, 128), rs)


# ------------------------------------------------------------------------------------------------ conv_a
def _conv_a_case(shape):
    B, Hi, Wi = shape
    return R.case_of((B, 3, Hi, Wi, 128, 5, 2, 0, 0), view=(6, 3))


@functools.lru_cache(maxsize=None)
def _conv_a_operands(shape, integers):
    """(x, w, bias, conv + bias in float64) -- shared by the forms of one input width, never written to"""
    rc = _conv_a_case(shape)
    x, w, bias = R.inputs(rc, 4100 + shape[2] + (0 if integers else 500), integers=integers)
    if integers:
        assert R.exact_bound(rc, x, w, bias) < 2 ** 24, "every partial sum must be a float32 integer"
    return x, w, bias, R.conv64(rc, x, w, bias)


@functools.lru_cache(maxsize=None)
def _conv_a_gdn_refs(shape):
    """real operands: (beta, gamma, GDN of conv + bias, its one-product share q, the scale s, the share at s, the GDN of s (conv + bias))"""
    ref = _conv_a_operands(shape, False)[3]
    beta, gamma = _gdn_params(4200 + shape[2])
    s = R.one_product_scale(ref, beta, gamma, False)
    return (beta, gamma, R.gdn64(ref, beta, gamma, False), R.one_product_share(ref, beta, gamma, False), s,
            R.one_product_share(s * ref, beta, gamma, False), R.gdn64(s * ref, beta, gamma, False))


def _run_conv_a(c, x, w, bias, gdn=None, out_scale=None):
    """the outputs of the form of case c: {"y" / "pre": float32 NCHW on the device, "y8": decoded fp8 on the CPU}; gdn = (beta, gamma, inverse)"""
    from masic_amd import ops
    has_gdn, products, out = c.form
    B, Hi, Wi = c.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    xd, wp, bd = x.to(DEV), ops.pack_conv_a_weight(w.to(DEV)), bias.to(DEV)
    assert T.plan(c, x_aligned16=int(xd.data_ptr() % 16 == 0))[0].kernel == c.kernel
    if not has_gdn:
        return {"y": _nchw(ops.conv_a_f16k(xd, wp, bd, in_coff=3)[0], B, 128, Ho, Wo)}
    gp = (ops.pack_gdn_f16k(gdn[0].to(DEV), gdn[1].to(DEV)), gdn[2])
    before = ops._FUSED_GDN_PRODUCTS
    try:
        ops.set_fused_gdn_products(products)
        if out == 0:
            return {"y": _nchw(ops.conv_a_gdn_f16k(xd, wp, bd, gp, in_coff=3)[0], B, 128, Ho, Wo)}
        if out == 1:
            return {"y8": R.from_f8k(ops.conv_a_gdn_f8k(xd, wp, bd, gp, out_scale, in_coff=3)[0], B, 128, Ho, Wo)}
        pre, y, _, _ = ops.conv_a_gdn_dual(xd, wp, bd, gp, in_coff=3, products=products)
        return {"pre": _nchw(pre, B, 128, Ho, Wo), "y": _nchw(y, B, 128, Ho, Wo)}
    finally:
        ops.set_fused_gdn_products(before)


@pytest.mark.parametrize("c", _family("conv_a"), ids=_ids(_family("conv_a")))
def test_conv_a_tile_loop(c):
    has_gdn, products, out = c.form
    # ---- (a) whole numbers: bit for bit
    x, w, bias, ref = _conv_a_operands(c.shape, True)
    want = ref.bfloat16().float().to(DEV)
    ident = _gdn_params(0, identity=True) + (True,)
    if out == 1:
        scale = 2.0 ** int(np.ceil(np.log2(float(ref.abs().max()) / 448.0)))
        got = _run_conv_a(c, x, w, bias, ident, out_scale=scale)["y8"]
        _same(c, f"(a) whole numbers, identity inverse GDN, fp8 at scale {scale:g}", got * scale, R.fp8_out_ref(ref.float(), scale))
    else:
        res = _run_conv_a(c, x, w, bias, ident)
        for k in sorted(res):
            _same(c, "(a) whole numbers, " + ("pre-GDN F16K" if k == "pre" else "F16K" + (", identity inverse GDN" if has_gdn else "")), res[k], want)
    # ---- (b) real operands: the project's gates
    if out == 1:
        return
    x, w, bias, ref = _conv_a_operands(c.shape, False)
    if not has_gdn:
        _hold(c, "(b) real operands, F16K", _run_conv_a(c, x, w, bias)["y"], ref, 2.0 ** -8, "2^-8")
        return
    beta, gamma, gref, q1, s, qs, gref_s = _conv_a_gdn_refs(c.shape)
    res = _run_conv_a(c, x, w, bias, (beta, gamma, False))
    if "pre" in res:
        _hold(c, "(b) real operands, pre-GDN F16K", res["pre"], ref, 2.0 ** -8, "2^-8")
    if products == 3:
        _hold(c, "(b) real operands, 3-product GDN, F16K", res["y"], gref, 2.0 ** -8 + 5e-5, "2^-8 + 5e-5")
        return
    _hold(c, f"(b) real operands, 1-product GDN, F16K (share {q1:.2f})", res["y"], gref, 2.0 ** -8 + R.one_product_bound(q1), f"2^-8 + {R.one_product_bound(q1):.2e}")
    assert qs <= 0.45
    res = _run_conv_a(c, x * s, w, bias * s, (beta, gamma, False))
    if "pre" in res:
        _hold(c, f"(b) real operands times {s:g}, pre-GDN F16K", res["pre"], s * ref, 2.0 ** -8, "2^-8")
    _hold(c, f"(b) real operands times {s:g}, 1-product GDN, F16K (share {qs:.2f})", res["y"], gref_s, 2.0 ** -8 + 2.0 ** -9, "2^-8 + 2^-9")


# ------------------------------------------------------------------------------------------------ the resident 3x3 kernel
def _ints(g, shape, top):
    return torch.randint(-top, top + 1, shape, generator=g).float()


def _c3_real_cin(ci, C):
    return ci if ci > 16 else (6 if C == 32 else 3)      # one record per pixel holds a 6- or 3-channel picture


@functools.lru_cache(maxsize=None)
def _c3_operands(shape, integers, transposed=False):
    """(f16k_ref case, x [B, CI, H, W] with finite values in the padding channels, w, bias, conv + bias in float64)"""
    B, ci, C, H, W = shape
    cin = _c3_real_cin(ci, C)
    rc = R.case_of((B, cin, H, W, C, 3, 1, int(transposed), 0), view=(ci, 0))
    g = torch.Generator().manual_seed(4300 + ci + C + 7 * integers + 13 * transposed)
    if integers:
        x = _ints(g, (B, ci, H, W), 3)
        w = torch.tensor([-1.0, 0.0, 0.0, 0.0, 1.0])[torch.randint(0, 5, (C, cin, 3, 3), generator=g)]
        bias = _ints(g, (C,), 20)
        assert R.exact_bound(rc, x, w, bias) < 2 ** 24
    else:
        x = (2.0 * torch.randn(B, ci, H, W, generator=g)).bfloat16().float()
        w = (torch.randn(C, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).bfloat16().float()
        bias = torch.randn(C, generator=g)
    return rc, x, w, bias, R.conv64(rc, x, w, bias)


def _c3_side(g, shape, integers, top):
    return _ints(g, shape, top) if integers else torch.randn(shape, generator=g).bfloat16().float()


def _c3_run(c, integers, act, transposed=False):
    """one forward-form launch (mask, y_pre, two residuals, output view) and, for an EX case, the two EX launches (mask2 / y2, sum_of 1 and 2);
    returns [(what, got on the device, float32 reference on the CPU)] and [(what, sums on the device, float64 sums)]"""
    from masic_amd import ops
    B, ci, C, H, W = c.shape
    ex = c.form[0]
    rc, x, w, bias, v64 = _c3_operands(c.shape, integers, transposed)
    cin = rc.Cin
    assert ops.conv3x3_resident_supported(B, cin, C, H, W)
    slope = 0.0 if integers else 0.01
    RT, OT, OC = C + 16, C + 32, 16
    g = torch.Generator().manual_seed(4400 + ci + C + int(integers))
    res1, res2 = _c3_side(g, (B, RT, H, W), integers, 64), _c3_side(g, (B, RT, H, W), integers, 64)
    mask, mask2 = _c3_side(g, (B, RT, H, W), integers, 2), _c3_side(g, (B, RT, H, W), integers, 2)      # (whole numbers: zeros among them)
    v, pre = R.epilogue32(v64, act, mask=mask[:, :C], slope=slope, res1=res1[:, :C], res2=res2[:, :C])
    x16, wp, bd = _to16(x), ops.pack_conv3x3_resident_weight(w.to(DEV), transposed=transposed), bias.to(DEV)
    r1, r2, m1, m2 = _to16(res1), _to16(res2), _to16(mask), _to16(mask2)
    views, sums = [], []
    want_y, want_pre = R.in_view(v.bfloat16().float(), OT, OC), R.in_view(pre.bfloat16().float(), RT, 0)
    for sum_of in ((1, 2) if ex else (0,)):
        y16, pre16 = _prefilled16(B * OT * H * W), _prefilled16(B * RT * H * W)
        out = ops.conv3x3_resident(x16, wp, bd, B, cin, C, H, W, act=act, y16=y16, out_ctot=OT, out_coff=OC, in_ctot=ci, res1=r1, res2=r2, res_ctot=RT,
                                   mask=m1, mask_slope=slope, y_pre=pre16, mask2=m2 if ex else None, mask2_slope=slope, sum_of=sum_of)
        tag = f", sum_of {sum_of}" if ex else ""
        views += [("y into a view" + tag, _nchw(y16, B, OT, H, W), want_y if integers else v), ("y_pre" + tag, _nchw(pre16, B, RT, H, W), want_pre if integers else pre)]
        if ex:
            y2 = v.bfloat16().float() * torch.where(mask2[:, :C] > 0, torch.tensor(1.0), torch.tensor(slope, dtype=torch.float32))
            views.append(("y2" + tag, _nchw(out[1], B, RT, H, W)[:, :C], y2.bfloat16().float() if integers else y2))
            stored = pre.bfloat16().double() if sum_of == 1 else y2.bfloat16().double()
            if integers:
                assert float(stored.abs().sum((0, 2, 3)).max()) < 2 ** 24, "the channel sums must be exact in float32 in any order"
            sums.append((f"channel sums, sum_of {sum_of}", out[2], stored.sum((0, 2, 3))))
    return views, sums


def _c3_check(c, act, transposed=False):
    B, ci, C, H, W = c.shape
    form = ("input-gradient form (transposed pack), " if transposed else "") + ("EX" if c.form[0] else "forward form")
    # ---- (a) whole numbers
    views, sums = _c3_run(c, True, act, transposed)
    for what, got, want in views:
        _same(c, f"(a) whole numbers, {form}, act {act}, {what}", got, want.to(DEV))       # (the views: prefill outside included)
    for what, got, want in sums:
        _same(c, f"(a) whole numbers, {form}, {what}", got.double(), want.to(DEV))
    # ---- (b) LeakyReLU, mask slope 0.01, real operands
    views, _ = _c3_run(c, False, R.ACT_LEAKY, transposed)
    for what, got, want in views:
        if got.shape[1] != C:           # a view: the prefill outside it exactly, the layer's channels at the gate
            off = 16 if what.startswith("y into") else 0
            outside = torch.cat([got[:, :off], got[:, off + C:]], 1)
            assert bool((outside == R.PREFILL).all()), f"{T.case_id(c)}: {what}: prefill"
            got = got[:, off:off + C]
        _hold(c, f"(b) real operands, {form}, LeakyReLU, mask slope 0.01, {what}", got, want, 2.0 ** -8, "2^-8")


@pytest.mark.parametrize("c", _family("resident"), ids=_ids(_family("resident")))
def test_resident_tile_loop(c):
    B, ci, C, H, W = c.shape
    ex = c.form[0]
    _c3_check(c, R.ACT_RELU if (C == 32) != bool(ex) else R.ACT_NONE)       # ReLU and no activation each meet both widths and both EX settings


@pytest.mark.parametrize("c", [c for c in _family("resident") if c.shape[1] == c.shape[2] and not c.form[0]],
                         ids=_ids([c for c in _family("resident") if c.shape[1] == c.shape[2] and not c.form[0]]))
def test_resident_tile_loop_input_gradient_form(c):
    _c3_check(c, R.ACT_NONE, transposed=True)


# ------------------------------------------------------------------------------------------------ gdn_fwd
@functools.lru_cache(maxsize=None)
def _gdn_fwd_ref(shape, inverse):
    g = torch.Generator().manual_seed(4500 + int(inverse))
    x = 3.0 * torch.randn(shape, generator=g)
    beta, gamma = _gdn_params(4501)
    return x, beta, gamma, R.gdn64(x.double(), beta, gamma, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("c", _family("gdn_fwd"), ids=_ids(_family("gdn_fwd")))
def test_gdn_fwd_tile_loop(c, inverse):
    from masic_amd import ops
    prec, out_f16k = c.form
    x, beta, gamma, ref = _gdn_fwd_ref(c.shape, inverse)
    xd, bd, gd = x.to(DEV), beta.to(DEV), gamma.to(DEV)
    name = "inverse GDN" if inverse else "GDN"
    if out_f16k:
        _hold(c, f"real operands, {name}, F16K store", _nchw(ops.gdn_f16k(xd, bd, gd, inverse=inverse), *c.shape), ref, 2.0 ** -8, "2^-8")
    elif prec == T.PREC_BF16:
        _hold(c, f"real operands, {name}, bf16x3", ops.gdn(xd, bd, gd, inverse=inverse, prec=T.PREC_BF16), ref, 5e-5)
    else:
        _hold(c, f"real operands, {name}, float32", ops.gdn(xd, bd, gd, inverse=inverse, prec=T.PREC_F32), ref, 2e-5)


# ------------------------------------------------------------------------------------------------ gdn_bwd
def _rows(t):
    """NCHW -> [128, B H W]"""
    return t.permute(1, 0, 2, 3).reshape(128, -1)


def _gdn_bwd_params():
    beta, gamma = _gdn_params(4600)
    gamma[0, 1], gamma[1, 0], beta[0] = 1e-7, 1e-7, 1e-5        # stored parameters below their bound: the LowerBound rule
    return beta, gamma


@functools.lru_cache(maxsize=None)
def _gdn_bwd_operands(shape, inverse):
    """bf16-representable x and g (so that all four operand combinations see the same values), the parameters, the emulation, autograd"""
    g = torch.Generator().manual_seed(4601 + int(inverse))
    x = (3.0 * torch.randn(shape, generator=g)).bfloat16().float()
    go = torch.randn(shape, generator=g).bfloat16().float()
    beta, gamma = _gdn_bwd_params()
    return x, go, beta, gamma, R.gdn_bwd_emulation(_rows(x), _rows(go), beta, gamma, inverse), R.gdn_bwd_autograd64(_rows(x), _rows(go), beta, gamma, inverse)


def _gdn_bwd_call(c, x, go, beta, gamma, inverse, **want):
    from masic_amd import ops
    xf, gf, _ = c.form
    return ops.gdn_bwd_fused_ex(_to16(x) if xf else x.to(DEV), _to16(go) if gf else go.to(DEV), c.shape, beta.to(DEV), gamma.to(DEV), inverse=inverse, beta_min=1e-6, **want)


@functools.lru_cache(maxsize=None)
def _gdn_bwd_base(inverse):
    """(dx, d beta, d gamma) of the float32-operand kernel, on the device: what the other three operand combinations must repeat bit for bit"""
    c = _family("gdn_bwd")[0]
    assert c.form[:2] == (0, 0)
    x, go, beta, gamma, _, _ = _gdn_bwd_operands(c.shape, inverse)
    gx, _, _, gb, gg = _gdn_bwd_call(c, x, go, beta, gamma, inverse, want_nchw=True, want_f16k=False, want_sum=False)
    return gx, gb, gg


def _hold_grads(c, run, got, emu, ref):
    """the two gates of test_gdn_backward_fused_bf16 on (dx [128, pixels], d beta, d gamma): 2e-3 of the float64 autograd result's peak
    against the emulation, 3e-2 against autograd itself"""
    for name, a, e, r in zip(("dx", "d beta", "d gamma"), got, emu, ref):
        peak = float(r.abs().max())
        ee, er = float((a.double().cpu() - e).abs().max()) / peak, float((a.double().cpu() - r).abs().max()) / peak
        _report(c, f"{run}, {name} against the emulation", "2.0e-03", ee)
        _report(c, f"{run}, {name} against float64 autograd", "3.0e-02", er)
        assert ee <= 2e-3 and er <= 3e-2, f"{T.case_id(c)}: {run}: {name}: {ee:.3e} of the peak from the emulation, {er:.3e} from autograd"


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("c", _family("gdn_bwd"), ids=_ids(_family("gdn_bwd")))
def test_gdn_bwd_tile_loop(c, inverse):
    B, C, H, W = c.shape
    x, go, beta, gamma, emu, auto = _gdn_bwd_operands(c.shape, inverse)
    name = "inverse GDN" if inverse else "GDN"
    gx, gx16, gs, gb, gg = _gdn_bwd_call(c, x, go, beta, gamma, inverse, want_nchw=True, want_f16k=True, want_sum=True)
    _hold_grads(c, f"(b) real operands, {name}", (_rows(gx), gb, gg), emu[:3], auto)
    gx0, gb0, gg0 = _gdn_bwd_base(inverse)
    assert torch.equal(gx, gx0) and torch.equal(gb, gb0) and torch.equal(gg, gg0), "dx, d beta, d gamma: bit for bit across the operand combinations"
    assert torch.equal(_nchw(gx16, B, C, H, W), gx.bfloat16().float()), "F16K dx = float32 dx rounded once"
    gxb, _, none_sum, gb2, gg2 = _gdn_bwd_call(c, x, go, beta, gamma, inverse, want_nchw=True, want_f16k=False, want_sum=False, want_b16=True)
    assert none_sum is None and gxb.dtype == torch.bfloat16 and torch.equal(gxb, gx.bfloat16()), "bf16 dx = float32 dx rounded once"
    assert torch.equal(gb2, gb) and torch.equal(gg2, gg), "the reduce pass without the channel sums"
    es = float((gs.double() - gx.double().sum((0, 2, 3))).abs().max()) / float(gx.double().abs().sum((0, 2, 3)).max())
    _report(c, f"(b) real operands, {name}, channel sums of dx", "1.0e-05", es)
    assert es <= 1e-5, f"{T.case_id(c)}: channel sums of dx: {es:.3e} of max sum |dx|"


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("c", _family("gdn_bwd"), ids=_ids(_family("gdn_bwd")))
def test_gdn_bwd_selective_support(c, inverse):
    B, C, H, W = c.shape
    m, v, _ = T.plan(c)
    x, go, beta, gamma, _, _ = _gdn_bwd_operands(c.shape, inverse)
    tiles = T.selective_tiles(c)
    on = torch.zeros(v["npix"], dtype=torch.bool)
    for t in tiles:
        on[128 * t:128 * (t + 1)] = True                     # (the last tile: clipped at the pixel count)
    assert 0 < int(on[128 * tiles[-1]:].sum()) < 128, "the last tile is ragged"
    gsel = (go.permute(0, 2, 3, 1).reshape(-1, 128) * on[:, None]).reshape(B, H, W, 128).permute(0, 3, 1, 2).contiguous()
    gx, _, gs, gb, gg = _gdn_bwd_call(c, x, gsel, beta, gamma, inverse, want_nchw=True, want_f16k=False, want_sum=True)
    xs, gsub = _rows(x)[:, on], _rows(go)[:, on]
    emu, auto = R.gdn_bwd_emulation(xs, gsub, beta, gamma, inverse), R.gdn_bwd_autograd64(xs, gsub, beta, gamma, inverse)
    rows = _rows(gx).cpu()
    assert bool((rows[:, ~on] == 0).all()), "dx is exactly zero where g is"
    _hold_grads(c, f"(c) g on tiles {tiles} of {v['ntiles']}, {'inverse GDN' if inverse else 'GDN'}", (rows[:, on], gb, gg), emu[:3], auto)
    es = float((gs.double().cpu() - rows.double().sum(1)).abs().max()) / float(rows.double().abs().sum(1).max())
    _report(c, f"(c) g on tiles {tiles}, channel sums of dx", "1.0e-05", es)
    assert es <= 1e-5


# ------------------------------------------------------------------------------------------------ pic_wgrad
@functools.lru_cache(maxsize=None)
def _pic_operands(shape):
    B, Hc, Wc = shape
    g = torch.Generator().manual_seed(4700)
    p = torch.randn(B, 128, Hc, Wc, generator=g).bfloat16().float()
    q6 = 2.0 * torch.randn(B, 6, 2 * Hc, 2 * Wc, generator=g)
    return p, q6


def _pic_ref(p, q):
    """float64 dW [128, 3, 5, 5] of both layers from the bf16-rounded operands: Conv2d(3 -> 128) (x = q, dy = p) by conv2d_weight,
    ConvTranspose2d(128 -> 3) (x = p, dy = q) by autograd"""
    pd, qd = p.bfloat16().double(), q.bfloat16().double()
    conv = torch.nn.grad.conv2d_weight(qd, (128, 3, 5, 5), pd, stride=2, padding=2)
    wt = torch.zeros(128, 3, 5, 5, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(pd, wt, None, stride=2, padding=2, output_padding=1).backward(qd)
    return conv, wt.grad


def _pic_hold(c, run, got, p, q):
    conv, deconv = _pic_ref(p, q)
    _hold(c, run + ", Conv2d(3 -> 128)", got.view(128, 3, 5, 5), conv, 2e-5)
    _hold(c, run + ", ConvTranspose2d(128 -> 3)", got.view(128, 3, 5, 5), deconv, 2e-5)


@pytest.mark.parametrize("c", _family("pic_wgrad"), ids=_ids(_family("pic_wgrad")))
def test_pic_wgrad_tile_loop(c):
    from masic_amd import ops
    B, Hc, Wc = c.shape
    p, q6 = _pic_operands(c.shape)
    q = q6[:, 2:5].contiguous()
    p16 = _to16(p)
    got = ops.pic_wgrad_f16k(p16, q.to(DEV), B, Hc, Wc)
    _pic_hold(c, "(b) real operands", got, p, q)
    assert torch.equal(ops.pic_wgrad_f16k(p16, q6.to(DEV), B, Hc, Wc, q_coff=2), got), "channels 2 .. 4 of a six-channel tensor"


@pytest.mark.parametrize("c", _family("pic_wgrad"), ids=_ids(_family("pic_wgrad")))
def test_pic_wgrad_selective_support(c):
    from masic_amd import ops
    B, Hc, Wc = c.shape
    m, v, _ = T.plan(c)
    p, q6 = _pic_operands(c.shape)
    q = q6[:, 2:5].contiguous()
    chunks = T.selective_tiles(c)
    psel = torch.zeros(B, 128, Hc * Wc)
    for k in chunks:
        b, p0 = k // v["tiles_per_image"], (k % v["tiles_per_image"]) * 64
        psel[b, :, p0:p0 + 64] = p.reshape(B, 128, -1)[b, :, p0:p0 + 64]
    assert 0 < Hc * Wc - (chunks[-1] % v["tiles_per_image"]) * 64 < 64, "the last chunk is ragged"
    psel = psel.reshape(B, 128, Hc, Wc)
    got = ops.pic_wgrad_f16k(_to16(psel), q.to(DEV), B, Hc, Wc)
    _pic_hold(c, f"(c) p on chunks {chunks} of {v['ntiles']}", got, psel, q)
