"""The cases of tests/test_gpu_conv_rows.py and of tests/test_gpu_backward.py::test_conv_wgrad_packed2 without a GPU: each still
selects the kernel instantiation it is filed under (host plan queries), the row cases between them cover the whole of CONV_ROWS, each
has the properties that make it hard (tests/conv_row_cases.py) or names the rule that forbids one, the search still writes the
committed tables, the reference of tests/conv_ref.py agrees with independent forms, and every case leaves room under its gate."""
import ctypes

import pytest
import torch

from masic_amd import _lib
from tests import conv_ref as R
from tests import conv_row_cases as T

CASES = T.all_cases()
IDS = [c.id for c in CASES]


# ------------------------------------------------------------------------------------------------ selection and properties
def test_row_cases_cover_the_table():
    names = T.table_names()
    assert len(names) == len(set(names)) == 75
    rows = T.row_cases()
    assert [k for k, _, _ in rows] == names, "one case per instantiation, in the table's order"
    covered = {T.plan(c)[0] for _, c, _ in rows}
    print(f"{len(covered & set(names))} of {len(names)} instantiations of CONV_ROWS covered")
    assert covered == set(names)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_selects_its_kernel(case):
    p = T.plan(case.case)
    assert p is not None and p[0] == case.kernel, (case.id, p)


def test_extra_cases_cover_every_tile_shape():
    tiles = lambda cases: sorted(k.split("<")[0] + k.split("<")[1][:7] for k, _, _ in cases)
    want = sorted(f"{fam}{t[0]}, {t[1]}, {t[2]}" for fam in ("conv_igemm_f32", "conv_igemm_bf16") for t in T.TILES)
    assert tiles(T.transposed_cases()) == want and tiles(T.form_cases()) == want
    assert all(c.transposed and c.k == 5 and c.stride == 2 and T.plan(c)[2]["nphase"] == 4 for _, c, _ in T.transposed_cases())
    for _, c, _ in T.form_cases():
        in_ctot, in_coff, out_ctot, out_coff = c.view
        assert c.form == R.GATE | R.RES1 | R.RES2 and c.act != 0
        assert in_coff > 0 and in_coff + c.Cin < in_ctot and out_coff > 0 and out_coff + c.Cout < out_ctot, "channels on both sides of both views"
    f16k = [e.case for e in CASES if e.id.startswith("f16k-out ")]
    assert len(f16k) == 7 and all(c.form == R.F16K_OUT and c.prec == R.PREC_BF16 and c.view[2] > c.Cout for c in f16k)
    assert len(T.digest_form_cases()) == 11


HARD = [c for c in CASES if c.waived is not None]


@pytest.mark.parametrize("case", HARD, ids=[c.id for c in HARD])
def test_case_is_hard(case):
    """batch, ragged tile in both directions, more than one tile in both, ragged channel block, partial last K chunk -- from the plan
    line's integers; a property a case lacks is named in the case together with the rule of choose_cfg that forbids it"""
    name, kernel, c, waived = case.id, case.kernel, case.case, case.waived
    props = T.properties(c)
    assert {"batch", "ragged_h", "ragged_w", "tiles", "cout"} <= set(props) and ("k_chunks" in props) == kernel.startswith(("conv_igemm", "deconv"))
    missing = {n for n, v in props.items() if not v}
    assert missing == set(waived), (name, props)
    assert all(isinstance(r, str) and len(r) > 20 for r in waived.values())


def test_the_search_writes_the_committed_tables():
    rows, trans, forms = T.search()
    assert rows == T.ROW_CASES and trans == T.TRANSPOSED_CASES and forms == T.FORM_CASES


def test_wgrad_packed2_cases_select_the_four_instantiations():
    from masic_amd import ops
    from tests.test_gpu_backward import WGRAD_PACKED2_CASES
    want = {f"conv_wgrad_packed_f32<2, {bf}, {det}>" for bf in ("false", "true") for det in ("false", "true")}
    seen = set()
    for name, B, Cin, H, W, Cout, k, s, tr in WGRAD_PACKED2_CASES:
        per_case = set()
        for prec in (_lib.PREC_F32, _lib.PREC_BF16):
            d = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=tr, prec=prec)
            for flags in (_lib.WGRAD_CLEAN, _lib.WGRAD_DET):      # what ops.conv2d_wgrad calls by default and in deterministic mode
                buf = ctypes.create_string_buffer(1024)
                assert _lib.lib.masic_conv2d_wgrad_plan_name(ctypes.byref(d), flags, buf, 1024) == 0
                per_case |= {line.split(" | ")[0] for line in buf.value.decode().splitlines()} & want
        assert per_case == want, (name, per_case)
        seen |= per_case
    print(f"{len(seen)} of 4 conv_wgrad_packed_f32<2, ., .> instantiations covered")
    assert seen == want


# ------------------------------------------------------------------------------------------------ the reference against independent forms
SMALL = [c for c in CASES if c.case.B * c.case.Cout * R.out_hw(c.case)[0] * R.out_hw(c.case)[1] <= 1 << 18]


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_reference_layer_is_the_modules(case):
    """conv_ref without gate and residuals == the layer as torch.nn modules in float64 (a masked one: torch.nn.Conv2d under the mask
    buffer of compressai.layers.MaskedConv2d), on the viewed, transformed and (for bf16) rounded input"""
    from compressai.layers import MaskedConv2d
    c = case.case._replace(form=0)
    x, w, bias, _, _, _ = R.inputs(c, case.seed, case.integers)
    in_ctot, in_coff, out_ctot, out_coff = R.views(c)
    kw = dict(kernel_size=c.k, stride=c.stride, padding=c.k // 2)
    if c.transposed:
        mod = torch.nn.ConvTranspose2d(c.Cin, c.Cout, output_padding=c.stride - 1, **kw)
    else:
        mod = torch.nn.Conv2d(c.Cin, c.Cout, **kw)
    q = (lambda t: t.bfloat16().double()) if c.prec == R.PREC_BF16 else (lambda t: t.double())
    mod = mod.double()
    with torch.no_grad():
        mod.weight.copy_(q(w))
        if c.masked:      # (the package's MaskedConv2d runs on the device only: its mask buffer on a plain torch layer)
            mod.weight.mul_(MaskedConv2d(c.Cin, c.Cout, **kw).mask.double())
        mod.bias.copy_(bias.double())
        xv = x[:, in_coff:in_coff + c.Cin]
        xv = {0: xv, 1: xv.abs(), 2: torch.round(xv)}[c.in_op]
        act = {0: torch.nn.Identity(), 1: torch.nn.ReLU(), 2: torch.nn.LeakyReLU(0.01), 3: torch.nn.Softmax(dim=1)}[c.act]
        want = act(mod(q(xv)))
    got = R.conv_ref(c, x, w, bias)
    assert tuple(got.shape) == (c.B, out_ctot) + R.out_hw(c)
    assert float((got[:, out_coff:out_coff + c.Cout] - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("act", [0, 1, 2])
def test_reference_epilogue_and_views_in_closed_form(act):
    """a 1x1 layer with the identity as weight copies its input view: the whole output buffer follows in closed form --
    act(x[view] + bias) * gate[:, 1] + res1 + res2 inside the view, the prefill outside"""
    C, B, H, W = 5, 2, 3, 4
    c = R.Case(B, C, H, W, C, 1, 1, 0, 0, R.PREC_F32, 0, R.GATE | R.RES1 | R.RES2, act, (9, 3, 11, 4))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 9, H, W, generator=g).double()
    bias, gate = torch.randn(C, generator=g).double(), torch.randn(B, 2, H, W, generator=g).double()      # (gates of both signs)
    res1, res2 = torch.randn(B, C, H, W, generator=g).double(), torch.randn(B, C, H, W, generator=g).double()
    got = R.conv_ref(c, x, torch.eye(C).reshape(C, C, 1, 1), bias, gate, res1, res2)
    t = x[:, 3:8] + bias[None, :, None, None]
    t = {0: t, 1: t.clamp(min=0), 2: torch.where(t >= 0, t, 0.01 * t)}[act]
    want = torch.full((B, 11, H, W), R.PREFILL, dtype=torch.float64)
    want[:, 4:9] = t * gate[:, 1:2] + res1 + res2
    assert torch.equal(got, want)
    # the order, in numbers: relu before the gate (relu(-2) * -1 = 0, not relu(-2 * -1) = 2), and the gate not on the residuals
    c1 = R.Case(1, 1, 1, 1, 1, 1, 1, 0, 0, R.PREC_F32, 0, R.GATE | R.RES1 | R.RES2, R.ACT_RELU, None)
    one = lambda v: torch.full((1, 1, 1, 1), float(v))
    out = R.conv_ref(c1, one(-2), one(1), torch.zeros(1), torch.tensor([[[[9.0]], [[-1.0]]]]), one(3), one(4))
    assert float(out) == 7.0
    out = R.conv_ref(c1, one(2), one(1), torch.ones(1), torch.tensor([[[[9.0]], [[0.0]]]]), one(3), one(4))
    assert float(out) == 7.0
    # in_op: round half to even, |x|; bf16 operands are rounded after it
    c2 = R.Case(1, 1, 1, 1, 1, 1, 1, 0, 0, R.PREC_BF16, R.INOP_ROUND, 0, 0, None)
    assert float(R.conv_ref(c2, one(2.5), one(1), None)) == 2.0 and float(R.conv_ref(c2, one(3.5), one(1), None)) == 4.0
    assert float(R.conv_ref(c2._replace(in_op=R.INOP_ABS), one(-1.003), one(1), None)) == float(torch.tensor(1.003).bfloat16())
    # F16K output: the result rounded to bf16
    c3 = c2._replace(in_op=0, form=R.F16K_OUT)
    assert float(R.conv_ref(c3, one(1.0), one(1), torch.tensor([0.001]))) == 1.0


# ------------------------------------------------------------------------------------------------ room under the gate
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_on_the_cpu_is_within_a_quarter_of_the_gate(case):
    """the same reference evaluated in float32 (torch, CPU): a correct float32-accumulating kernel has this kind of error, and the gate
    leaves four times that"""
    from tests.util import rel_err
    name, kernel, c = case.id, case.kernel, case.case
    args = R.inputs(c, case.seed, case.integers)
    _, _, _, out_coff = R.views(c)
    own = slice(out_coff, out_coff + c.Cout)
    ref = R.conv_ref(c, *args)[:, own]
    f32 = R.conv_ref(c, *args, dtype=torch.float32)[:, own]
    e = rel_err(f32, ref)
    print(f"conv_rows floor | {name} | {kernel} | gate {R.gate_of(c):.3e} | float32 on the CPU {e:.3e}")
    assert e <= 0.25 * R.gate_of(c), (name, e)
