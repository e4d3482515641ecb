"""The weight-gradient plans (masic_amd/csrc/conv_wgrad.hip: plan_wgrad, WGRAD_ROWS; wgrad_f16k.hip: plan_wg3, plan_wg1, WG3_ROWS) against
the launches of the if-ladders they replaced, recorded in tests/golden/wgrad_plan.npz (tests/golden/make_wgrad_plan_golden.py): every
launch of every call of the sweep -- kernel with all template arguments, grid, block, LDS bytes, fill and finishing pass, in order --,
the return codes of the refused forms and the byte queries.  Host queries only."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from masic_amd import _lib
from masic_amd._lib import WGRAD_CLEAN, WGRAD_DET, WGRAD_IN16

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_wgrad_plan_golden", os.path.join(HERE, "golden", "make_wgrad_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4
BUF = 1024


def nchw_plan(d, flags, n=BUF):
    buf = ctypes.create_string_buffer(n)
    rc = _lib.lib.masic_conv2d_wgrad_plan_name(ctypes.byref(d), flags, buf, n)
    return rc, buf.value.decode()


def f16k_plan(row, n=BUF):
    buf = ctypes.create_string_buffer(n)
    rc = _lib.lib.masic_wgrad_f16k_plan_name(*(int(v) for v in row), buf, n)
    return rc, buf.value.decode()


def rows(query):
    out, buf = [], ctypes.create_string_buffer(96)
    for det in (0, 1):
        i = 0
        while query(i, det, buf, 96) == 0:
            out.append(buf.value.decode())
            i += 1
    return out


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "wgrad_plan.npz"))
    assert np.array_equal(g["nchw_sweep"], gen.nchw_sweep()) and np.array_equal(g["f16k_sweep"], gen.f16k_sweep())
    return g


@pytest.fixture(scope="module")
def now(golden):
    """the current library's plans and byte queries over the golden's sweeps, packed like the golden"""
    SN, SF = golden["nchw_sweep"], golden["f16k_sweep"]
    A = gen.byte_queries(_lib.lib, SN, SF)
    for prefix, plans in (("nchw_", [nchw_plan(gen.desc_of(r), int(r[9])) for r in SN]), ("f16k_", [f16k_plan(r) for r in SF])):
        assert all(text == "" for rc, text in plans if rc != 0), "a refused form has no plan"
        A.update(gen.pack(prefix, [(rc, gen.parse_plan_text(text)) for rc, text in plans]))
    return A


def _lines(A, prefix):
    L = A[prefix + "launches"]
    return [(int(r[0]), str(A[prefix + "names"][r[1]])) + tuple(int(v) for v in r[2:]) for r in L]


@pytest.mark.parametrize("prefix", ["nchw_", "f16k_"])
def test_launches_are_the_parents(golden, now, prefix):
    """line for line: same kernel instantiation, grid, block, LDS bytes, fill and finishing launches in the same order"""
    assert np.array_equal(golden[prefix + "rc"], now[prefix + "rc"])
    want, got = _lines(golden, prefix), _lines(now, prefix)
    assert len(want) == len(got) and len(want) > 2000
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, (len(bad), bad[:5])


def test_byte_queries_are_the_parents(golden, now):
    for k in ("ws_bytes", "det_bytes", "bf16in_supported", "f16k_det_bytes"):
        assert np.array_equal(golden[k], now[k]), k
    assert golden["bf16in_supported"].sum() > 500 and (golden["det_bytes"] > golden["ws_bytes"]).sum() > 1000


def test_sweep_reaches_refusals_and_every_form(golden):
    """the recording itself: refused forms of every kind, accepted calls of every flag word"""
    SN, SF = golden["nchw_sweep"], golden["f16k_sweep"]
    ok = golden["nchw_rc"] == 0
    assert {int(f) for f in SN[ok][:, 9]} == set(gen.NCHW_FLAGS)
    assert set(golden["nchw_rc"][~ok].tolist()) == {ERR_UNSUPPORTED}
    assert set(golden["f16k_rc"][-len(gen.F16K_REFUSED):].tolist()) == {ERR_ARG, ERR_UNSUPPORTED}
    assert (golden["f16k_rc"][:-len(gen.F16K_REFUSED)] == 0).all()
    assert {(int(k), int(f)) for k, f in SF[:, [0, 6]]} >= {(3, 0), (3, WGRAD_CLEAN), (3, WGRAD_DET), (5, 0), (5, WGRAD_CLEAN), (5, WGRAD_DET),
                                                          (1, 0), (1, WGRAD_DET)}


def test_every_row_of_both_tables_is_named_by_the_sweep(golden, now):
    """every row, in both columns, is launched by at least one sweep entry -- and the sweep launches nothing the tables do not hold, apart
    from the fills, the finishing passes and the 1x1 F16K kernel (two instantiations, no table).  The same on the recording: every
    branch of the ladders the tables replaced was reached."""
    aux_n = {"masic_zero_kernel", "wgrad_transpose_kernel", "wgrad_slab_transpose_kernel", "wgrad_small_finish"}
    aux_f = {"masic_zero_kernel", "wgrad3_transpose_kernel", "wgrad_slab_transpose_kernel", "wgrad1x1_finish", "wgrad1x1_f16k<false>",
             "wgrad1x1_f16k<true>"}
    rn, rf = rows(_lib.lib.masic_conv2d_wgrad_row_name), rows(_lib.lib.masic_wgrad_f16k_row_name)
    assert len(rn) == 30 and len(set(rn)) == 28       # 15 rows x 2 columns; the two small-channel rows hold one kernel in both
    assert len(rf) == len(set(rf)) == 16
    for A in (golden, now):
        assert set(A["nchw_names"]) - aux_n == set(rn)
        assert set(A["f16k_names"]) - aux_f == set(rf)
        assert set(A["nchw_names"]) >= aux_n and set(A["f16k_names"]) >= aux_f
        for prefix in ("nchw_", "f16k_"):      # every name of the list is used by a launch
            assert set(A[prefix + "launches"][:, 1].tolist()) == set(range(len(A[prefix + "names"])))


def test_forms_without_an_entry_point_and_bad_arguments():
    d = gen.desc_of(np.array((5, 2, 0, 128, 128, 64, 64, 2, 1, 0)))
    assert nchw_plan(d, WGRAD_IN16)[0] == 0
    assert nchw_plan(d, WGRAD_DET | WGRAD_CLEAN) == (ERR_ARG, "")
    assert nchw_plan(d, 8) == (ERR_ARG, "")
    assert nchw_plan(d, 0, n=16) == (ERR_ARG, "")                                  # buffer too small: no partial plan
    assert nchw_plan(gen.desc_of(np.array((3, 1, 0, 128, 128, 64, 64, 2, 1, 0))), WGRAD_IN16) == (ERR_UNSUPPORTED, "")
    d.in_coff = 1                                                                  # the input view leaves its buffer
    assert nchw_plan(d, 0) == (ERR_SHAPE, "") and _lib.lib.masic_conv2d_wgrad_bf16in_supported(ctypes.byref(d)) == 1
    assert f16k_plan((3, 2, 64, 64, 16, 16, WGRAD_DET | WGRAD_CLEAN)) == (ERR_ARG, "")
    assert f16k_plan((1, 0, 2, 64, 64, 256, WGRAD_CLEAN)) == (ERR_ARG, "")
    assert f16k_plan((3, 2, 64, 64, 16, 16, WGRAD_IN16)) == (ERR_ARG, "")
    assert f16k_plan((4, 2, 64, 64, 16, 16, 0)) == (ERR_ARG, "")
    rc, text = f16k_plan((3, 2, 64, 96, 16, 16, 0))
    assert rc == 0 and text.splitlines()[0].startswith("masic_zero_kernel | ") and text.splitlines()[-1].startswith("wgrad3_transpose_kernel | ")
