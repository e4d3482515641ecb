"""The plan of the NCHW convolutions (masic_amd/csrc/conv.hip: plan_conv, CONV_ROWS) against the launches of the if-ladders and launch
macros it replaced, recorded in tests/golden/conv_plan.npz (tests/golden/make_conv_plan_golden.py): the launch of every call of the
sweep -- kernel with all template arguments, grid, block, LDS bytes and the integers of its argument struct --, the return codes of
the refused forms and the three descriptor queries.  Host queries only."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

from masic_amd import _lib
from masic_amd._lib import CONV_F16K_OUT, CONV_GATE, CONV_RES1, CONV_RES2

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("make_conv_plan_golden")
dig = _load("make_conv_fwd_digest")

ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4
BUF = 256


def plan(d, form, n=BUF):
    buf = ctypes.create_string_buffer(n)
    rc = _lib.lib.masic_conv_plan_name(ctypes.byref(d), form, buf, n)
    return rc, buf.value.decode()


def table():
    """every (row, in_op, flag) the table holds -> name"""
    out, buf = {}, ctypes.create_string_buffer(96)
    row = 0
    while any(_lib.lib.masic_conv_row_name(row, op, f, buf, 96) == 0 for op in range(3) for f in range(2)):
        for op in range(3):
            for f in range(2):
                if _lib.lib.masic_conv_row_name(row, op, f, buf, 96) == 0:
                    out[(row, op, f)] = buf.value.decode()
        row += 1
    return out


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(HERE, "golden", "conv_plan.npz")))      # (every array read once)
    assert np.array_equal(g["sweep"], gen.sweep())
    assert np.array_equal(g["extra"], np.array([list(gen.desc_ints(d)) + [f] for d, f in gen.extra_cases()], np.int32))
    return g


@pytest.fixture(scope="module")
def calls():
    return gen.cases()


@pytest.fixture(scope="module")
def now(calls):
    """the current library's plans and queries over the golden's calls, packed like the golden"""
    plans = [plan(d, f) for d, f in calls]
    assert all(text == "" for rc, text in plans if rc != 0), "a refused form has no plan"
    A = gen.queries(_lib.lib, calls)
    A.update(gen.pack([(rc, gen.parse_plan_text(text)) for rc, text in plans]))
    return A


def _lines(A):
    names = [str(n) for n in A["names"]]
    return [(r[0], names[r[1]]) + tuple(r[2:]) for r in A["launches"].tolist()]


def test_launches_are_the_parents(golden, now):
    """call for call: same return code, same kernel instantiation, grid, block, LDS bytes and argument integers"""
    assert np.array_equal(golden["rc"], now["rc"])
    want, got = _lines(golden), _lines(now)
    assert len(want) == len(got) and len(want) > 40000
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, (len(bad), bad[:5])


def test_sweep_reaches_every_refusal_and_the_empty_output(golden, calls):
    rc, form = golden["rc"], np.array([f for _, f in calls])
    launched = np.zeros(len(rc), bool)
    launched[golden["launches"][:, 0]] = True
    assert set(rc.tolist()) == {0, ERR_SHAPE, ERR_UNSUPPORTED}
    for f in gen.FORMS:      # every form is accepted somewhere; every form but the plain one is refused somewhere for a non-fp8 layer
        prec = np.array([d.prec for d, _ in calls])
        assert ((form == f) & launched).any(), f
        assert f == 0 or ((form == f) & (rc == ERR_UNSUPPORTED) & (prec != gen.FP8)).any(), f
    assert ((rc == 0) & ~launched).sum() == 4      # the empty outputs of extra_cases: MASIC_OK, nothing launched


def test_queries_are_the_parents(golden, now, calls):
    """masic_conv_packed_bytes and masic_conv2d_f16k_out_supported everywhere; masic_conv_kernel_name wherever the plain form is
    launched.  The parent named a kernel for every well-formed descriptor, the fp8 ones included, which masic_conv2d_fwd has always
    refused: those names, and only those, are gone -- the corrected disagreement, counted."""
    assert np.array_equal(golden["packed_bytes"], now["packed_bytes"]) and (golden["packed_bytes"] > 0).sum() > 46000
    assert np.array_equal(golden["f16k_out_supported"], now["f16k_out_supported"]) and 1000 < golden["f16k_out_supported"].sum() < 40000
    was = [str(golden["kname_names"][i]) for i in golden["kname"]]
    is_ = [str(now["kname_names"][i]) for i in now["kname"]]
    differ = [i for i in range(len(calls)) if (was[i], int(golden["kname_rc"][i])) != (is_[i], int(now["kname_rc"][i]))]
    assert all(calls[i][0].prec == gen.FP8 and was[i] != "" and is_[i] == "" and now["kname_rc"][i] == ERR_UNSUPPORTED
               and golden["kname_rc"][i] == 0 for i in differ)
    assert len(differ) == sum(d.prec == gen.FP8 for d, _ in calls) == 64


def test_kernel_name_is_the_plain_plans_kernel(calls):
    """... but for conv5s1_small, which masic_conv_kernel_name has always printed without its template argument"""
    buf = ctypes.create_string_buffer(96)
    n = 0
    for d, form in calls:
        if form != 0:
            continue
        rc, text = plan(d, 0)
        assert _lib.lib.masic_conv_kernel_name(ctypes.byref(d), buf, 96) == rc
        if text:
            kernel = text.split(" | ")[0]
            assert buf.value.decode() == ("conv5s1_small" if kernel.startswith("conv5s1_small<") else kernel)
            n += 1
        else:
            assert rc != 0 or d.Ho <= 0
    assert n > 20000


def test_every_row_and_column_is_launched_by_the_sweep(golden, now):
    """7 tile shapes x (4 f32 + 6 bf16 instantiations), conv_direct_f32<3|8>, deconv5s2_small_cout, conv5s1_small<4|8> -- and the sweep
    launches nothing else, on the recording (every branch of the ladders was reached) and now."""
    names = table()
    assert len(names) == len(set(names.values())) == 7 * 4 + 7 * 6 + 5
    assert not any(n.startswith("conv_igemm_bf16<2, 2, 1,") or n.startswith("conv_igemm_f32<2, 2, 1,") for n in names.values())
    for A in (golden, now):
        assert set(A["names"]) == set(names.values())
        assert set(A["launches"][:, 1].tolist()) == set(range(len(A["names"])))


def test_digest_cases_select_their_kernels():
    """tests/golden/conv_fwd_digest.json (tests/test_gpu_conv_digest.py): one case per table entry, each still reaching the kernel it
    was recorded on"""
    with open(os.path.join(HERE, "golden", "conv_fwd_digest.json")) as f:
        want = json.load(f)["cases"]
    cases = dig.cases()
    assert [c["name"] for c in cases] == list(want)
    seen = set()
    for c in cases:
        rc, text = plan(dig.desc_of(c), dig.form_of(c))
        assert rc == 0 and text.split(" | ")[0] == want[c["name"]]["kernel"], c["name"]
        seen.add(want[c["name"]]["kernel"])
    assert seen == set(table().values())


def test_forms_without_an_entry_point_and_bad_arguments():
    from masic_amd import ops
    d = ops.make_conv_desc(2, 128, 16, 16, 128, 3, 3, 1, 1, prec=_lib.PREC_BF16)
    assert plan(d, CONV_F16K_OUT)[0] == 0 and plan(d, CONV_GATE | CONV_RES1 | CONV_RES2)[0] == 0
    assert plan(d, CONV_F16K_OUT | CONV_GATE) == (ERR_ARG, "")
    assert plan(d, 16) == (ERR_ARG, "")
    assert plan(d, 0, n=16) == (ERR_ARG, "")                                       # buffer too small: no partial plan
    assert plan(ops.make_conv_desc(2, 128, 16, 16, 128, 3, 3, 1, 1), CONV_F16K_OUT) == (ERR_UNSUPPORTED, "")
    assert plan(ops.make_conv_desc(2, 128, 16, 16, 3, 5, 5, 2, 2, transposed=True), CONV_GATE) == (ERR_UNSUPPORTED, "")
    assert plan(ops.make_conv_desc(2, 6, 16, 16, 3, 5, 5, 1, 2), CONV_RES1 | CONV_RES2) == (ERR_UNSUPPORTED, "")
    assert plan(ops.make_conv_desc(2, 6, 16, 16, 3, 5, 5, 1, 2), CONV_RES1)[0] == 0
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.masic_conv_row_name(0, 1, 1, buf, 96) == ERR_ARG               # conv_igemm_f32 has no VEC4 instantiation with an in_op
    assert _lib.lib.masic_conv_row_name(99, 0, 0, buf, 96) == ERR_ARG
