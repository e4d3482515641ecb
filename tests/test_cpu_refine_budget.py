"""Latent refinement under a bit budget (masic_amd/refine.py), the parts that need no GPU: RefineConfig's budget fields, the host-side
argument checks of the three entry points of include/masic_budget.h (the header itself is a row of tests/test_cpu_side_headers.py), the
CPU restatement of the constrained keep-best and of the multiplier update (tests/budget_ref.py) with the guarantees they give, and the
admissibility of the budget the GPU loop test runs under."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from masic_amd.refine import MU_MAX, MU_MIN, RefinedToBudget          # the interface under test: the restatements below are of it
from tests import budget_ref as BR
from tests import refine_ref as R
from tests.test_cpu_refine import _encoder_latents

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- RefineConfig
def test_config_budget_defaults_are_off():
    from masic_amd.refine import DEFAULT_BUDGET_GAIN, RefineConfig
    c = RefineConfig()
    assert (c.budget_bpp, c.budget_rel, c.budget_gain, c.has_budget) == (None, None, DEFAULT_BUDGET_GAIN, False)
    assert c.budget_bpp_for(3) is None
    assert (MU_MIN, MU_MAX) == (2.0 ** -10, 2.0 ** 10) == (BR.MU_MIN, BR.MU_MAX)
    assert DEFAULT_BUDGET_GAIN in (0.5, 1.0, 2.0)


def test_config_accepts_budgets():
    from masic_amd.refine import RefineConfig
    c = RefineConfig(steps=5, budget_bpp=0.5)
    assert c.has_budget and c.budget_bpp == 0.5 and c.budget_bpp_for(3) == [0.5, 0.5, 0.5]
    c = RefineConfig(budget_bpp=(0.25, 1, 2.5), budget_gain=2)
    assert c.has_budget and c.budget_bpp_for(3) == [0.25, 1.0, 2.5] and c.budget_gain == 2.0
    c = RefineConfig(budget_rel=1)
    assert c.has_budget and c.budget_rel == 1.0 and c.budget_bpp is None
    for field in ("budget_bpp=[0.25, 1.0]", "budget_rel=None", "budget_gain=0.5"):
        assert field in repr(RefineConfig(budget_bpp=[0.25, 1.0], budget_gain=0.5))
    assert "budget_rel=0.75" in repr(RefineConfig(budget_rel=0.75))


@pytest.mark.parametrize("kw", [dict(budget_bpp=1.0, budget_rel=1.0), dict(budget_bpp=[1.0], budget_rel=0.5)]
                         + [{f: v} for f in ("budget_bpp", "budget_rel", "budget_gain") for v in (0, 0.0, -1.0, NAN, INF, -INF, True, False, "1")]
                         + [dict(budget_bpp=v) for v in ([], [1.0, 0.0], [1.0, NAN], [INF], [True], [-0.5, 1.0], ["1"])]
                         + [dict(budget_rel=[1.0]), dict(budget_gain=[1.0]), dict(budget_gain=None)])
def test_config_refuses_budgets(kw):
    from masic_amd.refine import RefineConfig
    with pytest.raises(ValueError, match="RefineConfig"):
        RefineConfig(**kw)


def test_config_budget_bpp_must_match_the_batch():
    from masic_amd.refine import RefineConfig
    with pytest.raises(ValueError, match=r"RefineConfig.*2 values for 3 pairs"):
        RefineConfig(budget_bpp=[1.0, 2.0]).budget_bpp_for(3)
    with pytest.raises(ValueError, match=r"^StereoCodec.encode: RefineConfig.*3 pairs"):
        RefineConfig(budget_bpp=[1.0, 2.0]).budget_bpp_for(3, "StereoCodec.encode")


def test_refined_to_budget_extends_refined():
    from masic_amd.refine import Refined
    assert Refined._fields == ("y1", "y2", "z1", "z2", "cost_start", "cost_best")
    assert RefinedToBudget._fields == Refined._fields + ("bits_start", "bits_best", "mse_start", "mse_best", "target_bits", "mu")
    assert issubclass(RefinedToBudget, tuple) and tuple(RefinedToBudget(*range(12))[:4]) == (0, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_bad_arguments_launch_nothing():
    """the argument checks are host code: null pointers, B out of range, a zero count, scalars outside their range"""
    from masic_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(16)
    four = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    n = (ctypes.c_size_t * 4)(1, 1, 1, 1)
    zero = (ctypes.c_size_t * 4)(1, 0, 1, 1)
    assert lib.masic_budget_select(None, four, n, 1, p, p, p, p, p, None) != 0
    assert lib.masic_budget_select(four, four, n, 1, p, p, None, p, p, None) != 0
    assert lib.masic_budget_select(four, four, zero, 1, p, p, p, p, p, None) != 0
    assert lib.masic_budget_select(four, four, n, 0, p, p, p, p, p, None) != 0
    assert lib.masic_budget_select(four, four, n, 65536, p, p, p, p, p, None) != 0
    assert b"budget_select" in lib.masic_last_error()
    assert lib.masic_budget_mu(None, p, p, 1, 1.0, 0.5, 2.0, None) != 0
    assert lib.masic_budget_mu(p, p, None, 1, 1.0, 0.5, 2.0, None) != 0
    assert lib.masic_budget_mu(p, p, p, 0, 1.0, 0.5, 2.0, None) != 0
    assert lib.masic_budget_mu(p, p, p, 65536, 1.0, 0.5, 2.0, None) != 0
    for gain, lo, hi in ((0.0, 0.5, 2.0), (-1.0, 0.5, 2.0), (NAN, 0.5, 2.0), (INF, 0.5, 2.0), (1.0, 0.0, 2.0), (1.0, NAN, 2.0), (1.0, 0.5, INF),
                         (1.0, 0.5, NAN), (1.0, -2.0, -1.0), (1.0, 2.0, 0.5)):
        assert lib.masic_budget_mu(p, p, p, 1, gain, lo, hi, None) != 0, (gain, lo, hi)
    assert b"budget_mu" in lib.masic_last_error()
    one = (ctypes.c_size_t * 1)(1)
    lik = (ctypes.c_void_p * 1)(16)
    assert lib.masic_budget_rd_seeds(None, p, p, p, 1, lik, one, 1, 1, 0.01, 1.0, None, None, p, p, lik, None) != 0
    assert lib.masic_budget_rd_seeds(p, p, p, p, 0, lik, one, 1, 1, 0.01, 1.0, None, None, p, p, lik, None) != 0
    assert lib.masic_budget_rd_seeds(p, p, p, p, 1, lik, one, 5, 1, 0.01, 1.0, None, None, p, p, lik, None) != 0
    assert lib.masic_budget_rd_seeds(p, p, p, p, 1, lik, one, 1, 0, 0.01, 1.0, None, None, p, p, lik, None) != 0
    assert lib.masic_budget_rd_seeds(p, p, p, p, 1, lik, one, 1, 1, 0.01, 0.0, None, None, p, p, lik, None) != 0
    assert lib.masic_budget_rd_seeds(p, p, p, p, 1, lik, (ctypes.c_size_t * 1)(0), 1, 1, 0.01, 1.0, None, None, p, p, lik, None) != 0
    assert b"budget_rd_seeds" in lib.masic_last_error()


# ---------------------------------------------------------------------------------------------------------------- the rule
T = 100.0
CANDIDATES = {"feasible": (90.0, 0.5), "feasible, worse D": (80.0, 0.9), "on the budget": (100.0, 0.5), "infeasible": (120.0, 0.1),
              "infeasible, more bits": (150.0, 0.1), "NaN R": (NAN, 0.1), "NaN D": (90.0, NAN), "NaN both": (NAN, NAN)}
KEPT = {"feasible": (95.0, 0.7), "on the budget": (100.0, 0.7), "infeasible": (130.0, 0.7)}


def test_rule_over_the_exhaustive_grid():
    """every kind of candidate against every kind of kept iterate, and the ties of each branch"""
    want = {("feasible", "feasible"): True, ("feasible", "on the budget"): True, ("feasible", "infeasible"): True,
            ("feasible, worse D", "feasible"): False, ("feasible, worse D", "on the budget"): False, ("feasible, worse D", "infeasible"): True,
            ("on the budget", "feasible"): True, ("on the budget", "on the budget"): True, ("on the budget", "infeasible"): True,
            ("infeasible", "feasible"): False, ("infeasible", "on the budget"): False, ("infeasible", "infeasible"): True,
            ("infeasible, more bits", "feasible"): False, ("infeasible, more bits", "on the budget"): False,
            ("infeasible, more bits", "infeasible"): False}
    for (cn, (r, d)), (kn, (rb, db)) in itertools.product(CANDIDATES.items(), KEPT.items()):
        got = BR.wins(r, d, T, rb, db)
        assert got == (False if "NaN" in cn else want[(cn, kn)]), (cn, kn)
    # ties: equality never replaces
    assert not BR.wins(95.0, 0.7, T, 95.0, 0.7)                     # the kept iterate itself
    assert not BR.wins(80.0, 0.7, T, 95.0, 0.7)                     # both feasible, equal D: fewer bits do not matter
    assert not BR.wins(130.0, 0.1, T, 130.0, 0.7)                   # both infeasible, equal R: a lower D does not matter
    assert BR.wins(129.0, 9.0, T, 130.0, 0.7)                       # both infeasible: R decides alone
    assert BR.wins(99.0, 0.69, T, 10.0, 0.7)                        # both feasible: D decides alone
    # a kept iterate that is itself NaN (a start that did not evaluate) counts as infeasible
    assert BR.wins(90.0, 0.5, T, NAN, NAN) and not BR.wins(120.0, 0.5, T, NAN, NAN)
    take, rb, db = BR.select([90.0, 120.0, NAN], [0.5, 0.1, 0.1], [T] * 3, [95.0, 95.0, 95.0], [0.7, 0.7, 0.7])
    assert take.tolist() == [True, False, False] and rb.tolist() == [90.0, 95.0, 95.0] and db.tolist() == [0.5, 0.7, 0.7]


@pytest.mark.parametrize("seed", range(20))
def test_rule_guarantees_over_random_sequences(seed):
    """section 8.10's guarantees: if any checked iterate, the start included, was feasible, the result is feasible (and is the
    feasible iterate of least D); if the start was feasible, D_best <= D_start; if nothing was feasible, R_best <= R_start"""
    rng = np.random.RandomState(seed)
    n = 30
    r = rng.choice([60.0, 80.0, 100.0, 100.5, 120.0, 150.0, NAN], size=n, p=[0.1, 0.1, 0.05, 0.1, 0.3, 0.3, 0.05])
    if seed % 3 == 0:
        r = np.where(r <= T, 110.0 + r, r)                          # nothing feasible
    d = rng.choice([0.2, 0.4, 0.4, 0.6, NAN], size=n)
    r[0], d[0] = (90.0 if seed % 2 else 140.0), 0.5                 # the start: finite, feasible or not
    rb, db = r[0], d[0]
    for k in range(1, n):
        if BR.wins(r[k], d[k], T, rb, db):
            rb, db = r[k], d[k]
    valid = ~(np.isnan(r) | np.isnan(d))
    feasible = valid & (r <= T)
    if feasible.any():
        assert rb <= T
        assert db == d[feasible].min()
    else:
        assert rb == r[valid].min() and rb <= r[0]
    if r[0] <= T:
        assert db <= d[0]
    assert not np.isnan(rb) and not np.isnan(db)


def test_mu_update_restated():
    mu = BR.mu_update([1.0, 1.0, 1.0, 2.0, 1.0, 2.0 ** -10, 2.0 ** 10], [100.0, 150.0, 50.0, NAN, 1e6, 1.0, 1e3], [100.0] * 7, 1.0)
    assert mu[0] == 1.0 and mu[1] == np.exp(0.5) and mu[2] == np.exp(-0.5) and mu[3] == 2.0
    assert mu[4] == BR.MU_MAX and mu[5] == BR.MU_MIN and mu[6] == BR.MU_MAX
    assert BR.mu_update([1.0], [150.0], [100.0], 2.0)[0] == np.exp(1.0)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_budget_fixture_is_admissible():
    """The float64 oracle budget loop on refine_ref.tiny_case(2) from the oracle encoder's latents (100 steps, lr 0.1, seed 3, a check
    every 5, gain 1): BUDGET_REL is the largest of 0.9 / 0.8 / 0.7 for which both pairs end feasible with R_best <= 0.98 T -- the
    margin the float32 kernels' loop (tests/test_gpu_refine_budget.py) is given.  Recorded here: R_best / T = 0.996, 0.999 at 0.9;
    0.996, 0.989 at 0.8; 0.912, 0.917 at 0.7."""
    c = R.tiny_case(2, torch.float64)
    lat = _encoder_latents(c)
    qualifies = {}
    for rel in (0.9, 0.8, 0.7):
        o = BR.oracle_budget_loop(c["sd"], lat, c["x1"], c["x2"], c["h_matrix"], c["K"], c["lmbda"], budget_rel=rel, **BR.LOOP)
        ratio = o["r_best"] / o["target"]
        print(f"budget_rel {rel}: R_start {o['r_start']}  T {o['target']}  R_best / T {ratio}  D_start {o['d_start']}  D_best {o['d_best']}  mu {o['mu']}")
        assert np.array_equal(o["target"], rel * o["r_start"]) and len(o["trace"]) == 21
        assert (o["r_best"] <= o["r_start"]).all()                  # the start is infeasible at every rel < 1: never more bits than it
        qualifies[rel] = bool((ratio <= 0.98).all())
        if qualifies[rel]:
            break
    assert any(qualifies.values()), qualifies
    assert BR.BUDGET_REL == max(rel for rel, ok in qualifies.items() if ok), qualifies
