"""The conv_f16k dispatch table (masic_amd/csrc/conv_f16k.hip: F16K_ROWS, plan_f16k) against the decisions of the if-ladders it
replaced, pinned in tests/golden/f16k_plan.npz (tests/golden/make_f16k_plan_golden.py), and the forms the name query learnt with the
table (flag bits 1 and 2).  Host queries only."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from masic_amd import _lib
from masic_amd._lib import ACT_RELU, F16K_GDN, F16K_MULTI, F16K_NOSPLIT

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_f16k_plan_golden", os.path.join(HERE, "golden", "make_f16k_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ERR_UNSUPPORTED = -4
DELETED = "conv_f16k<2, 2, 1, 3, 1, false, 1, 1, false>"
NAME_RE = re.compile(r"conv_f16k<(\d), (\d), (\d), (\d), (\d), (true|false), (\d), (\d), (true|false)>$")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "f16k_plan.npz"))


@pytest.fixture(scope="module")
def now(golden):
    """The current library's answers over the golden's sweep, plus the names of flag words 2 and 4 per descriptor."""
    S = golden["sweep"]
    assert np.array_equal(S, gen.sweep())
    A = gen.answers(_lib.lib, S)
    A["nosplit"] = [gen.kernel_name(_lib.lib, gen.desc_of(r), F16K_NOSPLIT) for r in S]
    A["multi"] = [gen.kernel_name(_lib.lib, gen.desc_of(r), F16K_MULTI) for r in S]
    return A


def table_rows():
    rows, buf = [], ctypes.create_string_buffer(96)
    while _lib.lib.masic_conv_f16k_row_name(len(rows), buf, 96) == 0:
        rows.append(buf.value.decode())
    return rows


def test_answers_are_the_parents(golden, now):
    for k in ("supported", "packed_bytes", "multi_supported", "rc0", "rc1"):
        assert np.array_equal(golden[k], now[k]), k
    for k in ("name0", "name1"):
        assert np.array_equal(golden["names"][golden[k]], now["names"][now[k]]), k


def test_every_row_is_named_by_the_sweep(now):
    rows = table_rows()
    assert len(rows) == len(set(rows)) == 26 and DELETED not in rows
    seen = set(now["names"][now["name0"]]) | set(now["names"][now["name1"]]) | {n for _, n in now["nosplit"]} | {n for _, n in now["multi"]}
    seen.discard("")
    assert seen == set(rows), (sorted(set(rows) - seen), sorted(seen - set(rows)))


def test_unsplit_forms(now):
    """Flag bit 1 (depth-to-space, few-channel, fp8 output): the launcher runs these with msplit = 1, i.e. the flags-0 kernel with NM = 4
    wherever the co-block split had lowered it.  That is NM = 1 for Cout <= 32 on the stride-1 walk and 4 for Cout >= 64, with the two
    cases the launcher itself keeps apart: a strided layer to 32 channels never had NM = 1 (it runs NM = 4, three tiles idle), and the
    lite rows hold exactly Cout / 32 tiles (NM = 2 / 3) and are never split."""
    S, n0 = now["sweep"], now["names"][now["name0"]]
    checked = 0
    for row, name0, rc0, (rc, name) in zip(S, n0, now["rc0"], now["nosplit"]):
        if rc0 != 0:
            assert rc == ERR_UNSUPPORTED and name == ""
            continue
        m = NAME_RE.match(name0)
        lite, stride1_walk, cout = m.group(3) == "1", m.group(2) == "2", int(row[5])
        nm = int(m.group(7)) if lite else (1 if (cout <= 32 and stride1_walk) else 4)
        assert cout > 32 or not stride1_walk or int(m.group(7)) == 1
        want = name0[:m.start(7)] + str(nm) + name0[m.end(7):]
        assert (rc, name) == (0, want), (row, name0, name)
        checked += name != name0
    assert checked > 100        # the sweep has split layers


def test_multi_form(now):
    """Flag bit 2: conv_f16k_multi<NM of the flags-0 name> exactly where masic_conv_f16k_multi_supported says 1."""
    n0 = now["names"][now["name0"]]
    assert now["multi_supported"].sum() > 50
    for row, name0, ms, (rc, name) in zip(now["sweep"], n0, now["multi_supported"], now["multi"]):
        if ms:
            assert (rc, name) == (0, "conv_f16k_multi<%s>" % NAME_RE.match(name0).group(7)), (row, name0, name)
        else:
            assert (rc, name) == (ERR_UNSUPPORTED, ""), (row, name)
    assert {n for _, n in now["multi"]} == {"", "conv_f16k_multi<1>", "conv_f16k_multi<2>", "conv_f16k_multi<4>"}


def test_deleted_name_never_appears(now):
    for flags in (0, F16K_GDN, F16K_NOSPLIT, F16K_GDN | F16K_NOSPLIT, F16K_MULTI):
        for row in now["sweep"][::7]:
            assert gen.kernel_name(_lib.lib, gen.desc_of(row), flags)[1] != DELETED
    assert DELETED not in set(now["names"]) | {n for _, n in now["nosplit"]}


def test_refused_forms():
    """(descriptor, flags) pairs the launcher refuses have no name."""
    name = lambda row, flags, act=0: gen.kernel_name(_lib.lib, gen.desc_of(np.array(row), act), flags)
    s2_128_192, s2_128_128, s1_96_96 = (5, 2, 0, 0, 128, 192, 64, 64, 8, 1), (5, 2, 0, 0, 128, 128, 64, 64, 8, 1), (3, 1, 0, 0, 96, 96, 256, 256, 8, 1)
    assert name(s2_128_128, F16K_GDN) == (0, "conv_f16k<1, 5, 2, 6, 1, true, 4, 1, false>")
    assert name(s2_128_192, F16K_GDN) == (ERR_UNSUPPORTED, "")                       # fused GDN with Cout != 128
    assert name(s2_128_128, F16K_GDN, ACT_RELU) == (ERR_UNSUPPORTED, "")             # ... with an activation
    assert name(s1_96_96, 0) == (0, "conv_f16k<2, 2, 1, 3, 1, false, 3, 1, false>")
    assert name(s1_96_96, F16K_MULTI) == (ERR_UNSUPPORTED, "")                       # multi on another configuration
    assert name(s2_128_192, F16K_MULTI)[0] == 0
    assert name(s2_128_192, F16K_MULTI, ACT_RELU) == (ERR_UNSUPPORTED, "")           # multi with an activation
    assert name(s2_128_192, F16K_MULTI | F16K_NOSPLIT) == (ERR_UNSUPPORTED, "")      # multi is a form of its own
    assert name(s2_128_128, F16K_MULTI | F16K_GDN) == (ERR_UNSUPPORTED, "")
    assert name((5, 2, 0, 0, 128, 192, 64, 64, 8, 2), F16K_MULTI) == (ERR_UNSUPPORTED, "")   # multi with fp8 operands
    assert name(s2_128_128, 8)[0] == -1                                              # unknown flag: MASIC_ERR_ARG
