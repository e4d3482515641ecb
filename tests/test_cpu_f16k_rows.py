"""The cases of tests/test_gpu_f16k_rows.py without a GPU: each still selects the kernel instantiation it is filed under with the flags
it is filed under (masic_conv_f16k_plan_name: a host query), the row cases between them cover the whole of F16K_ROWS, each has the
properties that make it hard (tests/f16k_row_cases.py) or names the rule that forbids one, the search still writes the committed table,
the plan query agrees with masic_conv_f16k_kernel_name over the sweep of the plan golden, the reciprocal multipliers the launcher
builds from the plan's integers divide exactly, and the reference of tests/f16k_ref.py agrees with independent forms."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from masic_amd import _lib
from tests import f16k_ref as R
from tests import f16k_row_cases as T

ROWS, GEOMETRY, FORMS = T.row_cases(), T.geometry_cases(), T.form_cases()
CASES = ROWS + GEOMETRY + FORMS
IDS = [c.id for c in CASES]


def _golden_sweep():
    spec = importlib.util.spec_from_file_location("make_f16k_plan_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_f16k_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ selection and properties
def test_row_cases_cover_the_table():
    names = T.table_names()
    assert len(names) == len(set(names)) == 26
    assert [e.kernel for e in ROWS] == names, "one case per instantiation, in the table's order"
    covered = {T.plan(e.case)[0] for e in ROWS}
    print(f"{len(covered & set(names))} of {len(names)} instantiations of F16K_ROWS covered")
    assert covered == set(names)
    # the flags a row is reached with are the ones it serves
    for e in ROWS:
        r = T.row_params(e.kernel)
        assert e.case.flags == (R.F16K_GDN if r["GDN"] else R.F16K_MULTI if r["MULTI"] else 0), e.id
        assert (e.case.prec == R.PREC_FP8) == r["F8"], e.id


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_selects_its_kernel(case):
    p = T.plan(case.case)
    assert p is not None and p[0] == case.kernel, (case.id, p)
    name, grid, v = p
    c = case.case
    # the line is consistent with itself and with the tap counts the properties use
    assert v["spc"] == [-(-t // v["T"]) for t in R.phase_taps(c)] and len(v["spc"]) == v["nphase"]
    assert grid == (-(-v["ntiles"] // 8) * 8 * v["nphase"], v["ncb"] * v["msplit"], c.B) and v["block"] == 512
    r = T.row_params(name)
    assert all(v[k] == r[k] for k in ("KS", "T", "D", "L", "NP")) and v["xcd_images"] == int(c.B % 8 == 0)
    assert v["nchunks"] * v["KS"] * (32 if r["F8"] else 16) == c.Cin and v["ncb"] == -(-c.Cout // 128)
    Hp, Wp = T.plane(c)
    assert v["tiles_w"] == -(-Wp // v["TW"]) and v["ntiles"] == v["tiles_w"] * -(-Hp // v["TH"])


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_row_case_is_hard(case):
    """every property of tests/f16k_row_cases.py, from the plan line's integers; a property a case lacks is named in the case together
    with the rule of choose_f16k / plan_f16k that forbids it, and only a rule the row's own parameters invoke may be named"""
    props = T.properties(case.case)
    missing = {n for n, v in props.items() if not v}
    assert missing == set(case.waived), (case.id, props)
    r = T.row_params(case.kernel)
    assert ("past" in props) == (r["NM"] < 4 and r["D"] != 1 and r["NP"] == 1), "a row of 4 / msplit accumulator tiles runs under msplit > 1"
    allowed = T.waivable(case.kernel)
    assert all(allowed.get(n) == why and len(why) > 20 for n, why in case.waived.items()), case.id


def test_geometry_and_form_cases_are_what_they_say():
    g = {e.id[len("geometry "):]: (e, T.plan(e.case)[2]) for e in GEOMETRY}
    maps = [(e.kernel, v["xcd_images"]) for what, (e, v) in g.items() if what.startswith("block map")]
    assert {x for k, x in maps if k == "conv_f16k<1, 5, 2, 6, 1, false, 2, 1, false>"} == {0, 1}, "the same kernel under both block-to-tile maps"
    assert any(T.row_params(k)["NP"] > 1 and x == 0 for k, x in maps), "a large-tile row at a batch that is no multiple of 8"
    assert {v["TW"] for what, (e, v) in g.items() if what.startswith("TW = ")} == {8, 16}
    assert {v["TW"] for what, (e, v) in g.items() if what.startswith("TW = ") and e.case.stride == 2} == {8, 16}
    tr = [e.case for e, _ in g.values() if e.case.transposed]
    assert tr and all(R.phase_taps(c) == [9, 6, 6, 4] for c in tr)
    assert any(e.case.masked and e.case.k == 5 and R.phase_taps(e.case) == [12] for e, _ in g.values())
    assert sum(1 for e, _ in g.values() if e.case.view and e.case.view[1] > 0 and e.case.view[0] > e.case.view[1] + e.case.Cin) == 2
    for e in FORMS:       # two tiles along each axis, the last ones partial
        p = T.properties(e.case)
        assert p["batch"] and p["tiles"] and p["ragged_h"] and p["ragged_w"], e.id
    assert len(FORMS) == 9


def test_the_search_writes_the_committed_table():
    assert T.search() == T.ROW_CASES


# ------------------------------------------------------------------------------------------------ the plan query
@functools.lru_cache(maxsize=None)
def _sweep_answers():
    """[(descriptor row, flags, masic_conv_f16k_kernel_name's code and name, masic_conv_f16k_plan_name's code and line)] over the golden sweep"""
    G, out = _golden_sweep(), []
    for row in G.sweep():
        for flags in (0, 1, 2, 4):
            d = G.desc_of(row)
            rc_k, name = G.kernel_name(_lib.lib, d, flags)
            buf = ctypes.create_string_buffer(b"?" * 255, 256)
            rc_p = _lib.lib.masic_conv_f16k_plan_name(ctypes.byref(d), flags, buf, 256)
            out.append((tuple(int(v) for v in row), flags, rc_k, name, rc_p, buf.value.decode()))
    return out


def test_plan_name_agrees_with_kernel_name_over_the_golden_sweep():
    n_ok = 0
    for row, flags, rc_k, name, rc_p, line in _sweep_answers():
        assert rc_p == rc_k, (row, flags, rc_p, rc_k)
        if rc_k != 0:
            assert line == "", "an empty buffer on refusal"
            continue
        assert line.endswith("\n") and T.parse(line)[0] == name, (row, flags, line, name)
        n_ok += 1
    assert n_ok > 1000
    # unknown flags, no buffer and a buffer too small are refused, the last two with the buffer left empty
    G, lib = _golden_sweep(), _lib.lib
    d = G.desc_of(G.sweep()[0])
    buf = ctypes.create_string_buffer(b"?" * 255, 256)
    assert lib.masic_conv_f16k_plan_name(ctypes.byref(d), 8, buf, 256) != 0 and buf.value == b""
    assert lib.masic_conv_f16k_plan_name(ctypes.byref(d), 0, None, 0) != 0
    row = next(r for r in G.sweep() if G.kernel_name(lib, G.desc_of(r), 0)[0] == 0)
    buf = ctypes.create_string_buffer(b"?" * 255, 256)
    assert lib.masic_conv_f16k_plan_name(ctypes.byref(G.desc_of(row)), 0, buf, 40) != 0 and buf.value == b""


def test_reciprocal_multipliers_divide_exactly():
    """f16k_launch hands the kernel ceil(2^32 / d) for d = PW, PWh and NPIXp / 32, and the kernel takes x / d as __umulhi(x, magic) for
    the pixel and DMA-instruction indices of the patch maps, all below 2 NPIXp (conv_f16k.hip, geometry-dependent setup: q = grp * 64 +
    lane < 64 NPIXp / 32, pp and rem below NPIXp, I < 4 NPI <= 48).  Integer arithmetic only: for every divisor of the sweep's and the
    tables' plan lines and every dividend below the largest 2 NPIXp it is used with, the multiplier gives the true quotient."""
    lines = {a[5] for a in _sweep_answers() if a[4] == 0 and a[5]} | {T.plan_line(e.case)[1] for e in CASES}
    bound = {}
    for line in lines:
        v = T.parse(line)[2]
        assert v["NPIXp"] % 32 == 0 and v["PWh"] == (v["PW"] + 1) // 2
        for d in (v["PW"], v["PWh"], v["NPIXp"] // 32):
            bound[d] = max(bound.get(d, 0), 2 * v["NPIXp"])
    assert len(bound) >= 10
    for d, top in sorted(bound.items()):
        magic = ((1 << 32) + d - 1) // d
        assert magic < (1 << 32)
        x = np.arange(top, dtype=np.uint64)
        assert np.array_equal((x * np.uint64(magic)) >> np.uint64(32), x // np.uint64(d)), (d, top)
    print(f"{len(bound)} divisors {min(bound)} .. {max(bound)}, dividends below {max(bound.values())}")


# ------------------------------------------------------------------------------------------------ the reference against independent forms
TINY = [("conv 3x3", (2, 16, 5, 7, 32, 3, 1, 0, 0), None), ("conv 5x5 stride 2", (1, 16, 9, 6, 32, 5, 2, 0, 0), None),
        ("conv 3x3 stride 2 of a view", (1, 16, 6, 7, 32, 3, 2, 0, 0), (48, 16)), ("transposed 5x5 stride 2", (2, 16, 4, 5, 32, 5, 2, 1, 0), None),
        ("masked 5x5", (1, 16, 6, 6, 32, 5, 1, 0, 1), None)]


@pytest.mark.parametrize("integers", [False, True])
@pytest.mark.parametrize("prec", [R.PREC_BF16, R.PREC_FP8])
@pytest.mark.parametrize("what,shape,view", TINY, ids=[t[0] for t in TINY])
def test_reference_layer_is_the_modules(what, shape, view, prec, integers):
    """conv64 == the layer as torch.nn modules in float64 (a masked one: torch.nn.Conv2d under the mask buffer of
    compressai.layers.MaskedConv2d) on the viewed input; the operands are exact in the operand format"""
    from compressai.layers import MaskedConv2d
    c = R.case_of(shape, prec, view=view)
    x, w, bias = R.inputs(c, 11, integers)
    if prec == R.PREC_BF16:
        assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w)
    else:
        assert torch.equal(x.to(torch.float8_e4m3fn).float(), x)
        scale = w.abs().amax(dim=(0, 2, 3) if c.transposed else (1, 2, 3)) / 448.0
        ws = w / scale.view((1, -1, 1, 1) if c.transposed else (-1, 1, 1, 1))
        # the weights over their per-channel scale are e4m3 values: exactly with unit scales, else up to the float32 rounding of 2 / 448
        q = ws.to(torch.float8_e4m3fn).float()
        assert float((q - ws).abs().max()) <= 2.0 ** -20 * 448 and torch.equal((q.double() / (1.0 if integers else 224.0)).float(), w)
        assert not integers or (bool((scale == 1.0).all()) and torch.equal(q, ws)), "unit scales"
    if integers:
        assert all(torch.equal(torch.round(t), t) for t in (x, w, bias)) and R.exact_bound(c, x, w, bias) < 2 ** 24
    kw = dict(kernel_size=c.k, stride=c.stride, padding=c.k // 2)
    mod = (torch.nn.ConvTranspose2d(c.Cin, c.Cout, output_padding=c.stride - 1, **kw) if c.transposed else torch.nn.Conv2d(c.Cin, c.Cout, **kw)).double()
    with torch.no_grad():
        mod.weight.copy_(w.double())
        if c.masked:
            mod.weight.mul_(MaskedConv2d(c.Cin, c.Cout, **kw).mask.double())
        mod.bias.copy_(bias.double())
        off = view[1] if view else 0
        want = mod(x[:, off:off + c.Cin].double())
    got = R.conv64(c, x, w, bias)
    assert tuple(got.shape) == (c.B, c.Cout) + R.out_hw(c) and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert R.macs(c) > 0 and len(R.phase_taps(c)) == (4 if c.transposed else 1)


def test_reference_epilogue_in_closed_form():
    one = lambda v: torch.full((1, 1, 1, 1), float(v), dtype=torch.float32)
    d = lambda v: one(v).double()
    # relu before the gate, the gate not on the residuals, the mask factor before y_pre, the residuals after it
    y, pre = R.epilogue32(d(-2), R.ACT_RELU, gate=one(-1), res1=one(3), res2=one(4))
    assert float(y) == 7.0 and float(pre) == 0.0
    y, pre = R.epilogue32(d(8), R.ACT_RELU, gate=one(0.5), mask=one(-1), slope=0.25, res1=one(3), res2=one(4))
    assert float(pre) == 1.0 and float(y) == 8.0
    y, pre = R.epilogue32(d(8), R.ACT_NONE, mask=one(0), slope=0.0, res1=one(3))       # act'(0) is the slope: `mask > 0 ? 1 : slope`
    assert float(pre) == 0.0 and float(y) == 3.0
    y, pre = R.epilogue32(d(-3), R.ACT_LEAKY, mask=one(2), slope=0.01)
    assert float(y) == float(torch.tensor(-3.0) * torch.tensor(0.01)) and y.dtype == torch.float32
    # float32, in order: (1 + 2^-24) + 2^-24 is 1 in float32 twice over, and 1 + 2^-23 in one float64 sum
    y, _ = R.epilogue32(d(1), R.ACT_NONE, res1=one(2.0 ** -24), res2=one(2.0 ** -24))
    assert float(y) == 1.0
    # one rounding to bf16, ties to even: 257 -> 256, 259 -> 260
    assert [float(v) for v in torch.tensor([257.0, 259.0]).bfloat16()] == [256.0, 260.0]
    # the view keeps its prefill
    v = R.in_view(torch.ones(1, 2, 1, 1), 5, 2)
    assert v[0, :, 0, 0].tolist() == [0.5, 0.5, 1.0, 1.0, 0.5]


def test_reference_layouts_multi_few_d2s_fp8_and_gdn():
    g = torch.Generator().manual_seed(3)
    # F16K: element (b, c, p) lies at ((b C/16 + c/16) HW + p) 16 + c % 16; F8K likewise with 32
    x = torch.randn(2, 32, 3, 5, generator=g).bfloat16().float()
    flat = R.to_f16k(x).view(torch.bfloat16).float()
    for b, ch, p in ((0, 0, 0), (1, 17, 7), (1, 31, 14)):
        assert float(flat[((b * 2 + ch // 16) * 15 + p) * 16 + ch % 16]) == float(x[b, ch].reshape(-1)[p])
    assert torch.equal(R.from_f16k(R.to_f16k(x), 2, 32, 3, 5).float(), x)
    x8 = R._pick(R.FP8_X, (2, 64, 3, 5), g)
    flat = R.to_f8k(x8).view(torch.float8_e4m3fn).float()
    assert float(flat[((1 * 2 + 1) * 15 + 7) * 32 + 9]) == float(x8[1, 41].reshape(-1)[7])
    assert torch.equal(R.from_f8k(R.to_f8k(x8), 2, 64, 3, 5), x8)
    # multi: ties to even, -0 kept, the gate after the rounding, one rounding to bf16
    v = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -0.25, 300.5, -3.0]).reshape(1, 8, 1, 1).double()
    m = R.multi_ref(v, gate=torch.full((1, 1, 1, 1), 0.5))
    assert m["round32"].flatten().tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, -0.0, 300.0, -3.0]
    assert R.bits(m["round32"]).flatten()[3].item() == -2 ** 31 and R.bits(m["round32"]).flatten()[0].item() == 0
    assert m["round16"].float().flatten().tolist() == [0.0, 1.0, 1.0, -0.0, -1.0, -0.0, 150.0, -1.5]
    assert R.bits(m["round16"]).flatten()[5].item() == -2 ** 15
    assert m["abs16"].float().flatten().tolist() == [0.5, 1.5, 2.5, 0.5, 1.5, 0.25, 300.0, 3.0] and torch.equal(m["y32"].double(), v)
    # few channels: act, then the float32 residual, channels 0 .. C-1
    f = R.few_ref(torch.tensor([-1.0, 2.0, 5.0]).reshape(1, 3, 1, 1).double(), R.ACT_RELU, torch.ones(1, 2, 1, 1), 2)
    assert f.flatten().tolist() == [1.0, 3.0]
    # depth-to-space: the 3x3 convolution to channels 4c + 2ph + pw, pixel-shuffled, is the transposed 5x5 stride-2 convolution
    w, b, t = torch.randn(16, 3, 5, 5, generator=g).double(), torch.randn(3, generator=g).double(), torch.randn(2, 16, 4, 5, generator=g).double()
    wc, bc = R.d2s_weight(w, b)
    assert wc.dtype == torch.float32
    wc, bc = R.d2s_weight(w.float(), b.float())
    y = F.pixel_shuffle(F.conv2d(t, wc.double(), bc.double(), padding=1)[:, :12], 2)
    want = F.conv_transpose2d(t, w.float().double(), b.float().double(), stride=2, padding=2, output_padding=1)
    assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max()) and float(wc[12:].abs().max()) == 0.0
    # fp8 output: round to nearest even on the e4m3 grid (steps of 2 from 16 to 32: 17 -> 16, 19 -> 20), saturating
    assert R.fp8_out_ref(torch.tensor([17.0, 19.0, 1000.0, -0.0625]), 1.0).tolist() == [16.0, 20.0, 448.0, -0.0625]
    assert R.fp8_out_ref(torch.tensor([34.0]), 2.0).tolist() == [32.0]
    # GDN: x rsqrt(beta^ + gamma^ x^2) with the stored parameters' reparametrisation (lower bound, square, minus the pedestal)
    ped = 2.0 ** -36
    beta, gamma, t = 0.5 + torch.rand(4, generator=g), 0.1 * torch.rand(4, 4, generator=g), torch.randn(2, 4, 3, 3, generator=g).double()
    bh = torch.clamp(beta.double(), min=(1e-6 + ped) ** 0.5) ** 2 - ped
    gh = torch.clamp(gamma.double(), min=ped ** 0.5) ** 2 - ped
    nrm = torch.einsum("ij,bjhw->bihw", gh, t * t) + bh.view(1, -1, 1, 1)
    assert float((R.gdn64(t, beta, gamma, False) - t / nrm.sqrt()).abs().max()) < 1e-13
    assert float((R.gdn64(t, beta, gamma, True) - t * nrm.sqrt()).abs().max()) < 1e-13
    # the one-product form's share of the norm and the bound derived from it: none of it with gamma^ = 0, all of it as x grows
    assert R.one_product_share(t, torch.ones(4), torch.zeros(4, 4), False) == 0.0 and R.one_product_share(1e4 * t, beta, gamma, True) > 0.999
    assert 0.3 < R.one_product_share(R.one_product_scale(8 * t, beta, gamma, False) * 8 * t, beta, gamma, False) <= 0.45
    assert R.one_product_bound(0.45) < 2.0 ** -9 < R.one_product_bound(0.5) and R.one_product_bound(1.0) == 2.0 ** -8 + 2.0 ** -14
    # the identity inverse GDN of the fp8 GDN rows: gamma stored 0 -> gamma^ = 0, beta stored 1 -> beta^ = 1 in float32
    assert float(torch.tensor(1.0, dtype=torch.float32) ** 2 - torch.tensor(ped, dtype=torch.float32)) == 1.0
    assert float((R.gdn64(t, torch.ones(4), torch.zeros(4, 4), True) - t).abs().max()) < 1e-10
