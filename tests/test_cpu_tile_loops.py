"""The tile-loop cases of tests/tile_loop_cases.py held to their kernels and properties, from the launchers' plan queries alone (host
code, no GPU): every case runs the kernel it is filed under with more tiles than workgroups, enough rounds for its pipeline to wrap,
a ragged last tile and a batch whose images one workgroup crosses -- or names the launcher rule that forbids the property.  The plan
queries themselves: one line per launch, the finishing passes included; refusals leave an empty buffer."""
import ctypes

import pytest

from tests import tile_loop_cases as T

IDS = [T.case_id(c) for c in T.CASES]


@pytest.mark.parametrize("c", T.CASES, ids=IDS)
def test_case_runs_its_kernel_past_the_grid_cap(c):
    m, v, _ = T.plan(c)
    assert m.kernel == c.kernel
    units = m.grid[0] * v.get("per_wg", 1)
    assert m.grid[1:] == (1, 1) and v["ntiles"] > units, "more tiles than the grid takes in one round"
    counts = [len(T.tiles_of(c, wg)) for wg in range(m.grid[0])]
    if c.family != "gdn_fwd" or v["per_wg"] == 1:
        assert sum(counts) == v["ntiles"], "tiles_of covers the tile list"
    assert max(counts) >= 2 and min(counts) < max(counts), "some workgroups run one tile more than others"


@pytest.mark.parametrize("c", T.CASES, ids=IDS)
def test_case_has_its_properties(c):
    p = T.properties(c)
    for name in ("rounds", "ragged", "batch"):
        if name in c.given_up:
            assert not p[name], f"{name} is given up ({c.given_up[name]}) but the plan line shows it"
        else:
            assert p[name], f"{name}: {T.plan(c)[0]}"
    assert all(k in p for k in c.given_up), "a rule is named for a property of the list"


def test_cases_cover_every_persistent_kernel():
    names = {c.kernel for c in T.CASES}
    assert {k for k, _, _ in T.CONV_A_FORMS} <= names and len(T.CONV_A_FORMS) == 8
    assert set(T.GDN_BWD_KERNELS.values()) <= names
    assert {f"conv3x3_resident_f16k<{ci}, {c}, {ex}>" for ci, c in T.C3_PAIRS for ex in ("false", "true")} <= names
    assert {"wgrad_pic_f16k", "gdn_mfma_c128", "gdn_bf16x3_c128"} <= names


def test_selective_tile_sets():
    for c in T.CASES:
        if c.family in ("gdn_bwd", "pic_wgrad"):
            m, v, _ = T.plan(c)
            s = T.selective_tiles(c)
            assert len(s) == 3 and s[0] == m.grid[0] and s[-1] == v["ntiles"] - 1 and s[1] % m.grid[0] == 0 and s[1] + m.grid[0] > s[2]


def test_conv_a_alignment_picks_the_kernel():
    """the wave-private kernel needs a 16-byte aligned input and Wi % 4 == 0; the same form falls to the shared-patch kernel otherwise"""
    c = T.CASES[0]
    assert c.kernel == "conv_a_gdn_f16k_w" and T.plan(c, x_aligned16=0)[0].kernel == "conv_a_gdn_f16k<false, 0>"
    assert T.plan(c._replace(shape=(29, 130, 66)))[0].kernel == "conv_a_gdn_f16k<false, 0>"
    small = T.plan(c._replace(shape=(1, 16, 64)))[0]
    assert small.grid == (1, 1, 1) and small.ints[0] == 1, "fewer tiles than the cap: one workgroup per tile"


def test_every_launch_has_a_line():
    """finishing and packing passes are launches too"""
    by = {c.kernel: c for c in T.CASES}
    names = lambda c: [l.kernel for l in T.plan(c)[2]]
    assert names(by["gdn_bwd_c128_wn<2>"]) == ["gdn_bwd_pack_kernel", "gdn_bwd_c128_wn<2>", "gdn_bwd_reduce_kernel"]
    assert names(by["wgrad_pic_f16k"]) == ["wgrad_pic_f16k", "wgrad_pic_finish"]
    assert names(by["conv3x3_resident_f16k<64, 64, true>"]) == ["conv3x3_resident_f16k<64, 64, true>", "c3_sum_finish_kernel"]
    assert names(by["conv3x3_resident_f16k<64, 64, false>"]) == ["conv3x3_resident_f16k<64, 64, false>"]
    assert names(by["conv_a_gdn_f16k_w"]) == ["conv_a_gdn_f16k_w"] and names(by["gdn_mfma_c128"]) == ["gdn_mfma_c128"]
    # the reduce pass adds a block row of 128 entries for the channel sums
    c = by["gdn_bwd_c128<false, false>"]
    with_sum, without = T.plan(c)[2][2], T.plan(c._replace(form=(0, 0, 0)))[2][2]
    assert with_sum.grid[0] == without.grid[0] + 128 // 32
    # the generic GDN kernel (any other channel count) has a line as well
    rc, text = T.plan_text("gdn_fwd", (2, 3, 5, 7, T.PREC_F32, 0))
    assert rc == 0 and T.parse(text)[0].kernel == "gdn_generic" and T.parse(text)[0].grid == (1, 2, 1)


REFUSED = [
    ("conv_a", (0, 130, 66, 1, 1, 1, 0)),           # B = 0
    ("conv_a", (2, 130, 66, 1, 0, 1, 2)),           # no GDN, pre-GDN output
    ("conv_a", (2, 130, 66, 1, 1, 2, 0)),           # two products
    ("gdn_bwd", (2, 64, 8, 8, 0, 0, 1)),            # C != 128
    ("gdn_bwd", (2, 128, 0, 8, 0, 0, 1)),
    ("pic_wgrad", (0, 8, 8)),
    ("pic_wgrad", (64, 512, 512)),                  # past 32-bit offsets
    ("resident", (2, 32, 32, 24, 64, 0, 0)),        # H % 16 != 0
    ("resident", (2, 64, 32, 16, 64, 0, 0)),        # Cin > Cout
    ("resident", (2, 32, 32, 16, 64, 0, 1)),        # sums without the EX form
    ("gdn_fwd", (2, 128, 5, 7, T.PREC_BF16, 1)),    # F16K output needs H W % 32 == 0
    ("gdn_fwd", (2, 600, 8, 8, T.PREC_F32, 0)),     # C > 512
]


@pytest.mark.parametrize("family,args", REFUSED, ids=[f"{f} {a}" for f, a in REFUSED])
def test_refused_shapes_leave_an_empty_buffer(family, args):
    rc, text = T.plan_text(family, args)
    assert rc != 0 and text == ""


@pytest.mark.parametrize("family", sorted(T.QUERY))
def test_buffer_rules(family):
    from masic_amd import _lib
    c = next(c for c in T.CASES if c.family == family)
    args = [int(v) for v in T.query_args(c)]
    fn = getattr(_lib.lib, T.QUERY[family])
    assert fn(*args, None, 0) != 0
    buf = ctypes.create_string_buffer(b"?" * 19, 20)
    assert fn(*args, buf, 20) != 0 and buf.value == b"", "a buffer too small is an error and left empty"
