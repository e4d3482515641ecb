"""tests/entropy_ref.py checked without a GPU and without the library: the float64 reference against the oracle in float64 and
against 40-digit arithmetic, the coverage conditions of the regimes, the tolerance table against the float32 oracle, and the teeth
of the ruler -- a float32 restatement of the kernels stays inside the table, each deliberate mutation of it does not."""
import math

import numpy as np
import pytest
import torch

from oracle import hsic_oracle as O
from tests import entropy_ref as R
from tests.util import scaled_err

MAIN = R.GMM_SHAPES[0]
KS = (1, 2, 5, 8)


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    """float32 reductions in one fixed order, as the table was measured."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def oracle_err():
    return R.measure_oracle(O)


@pytest.fixture
def f32_bounds(monkeypatch):
    """The oracle in float64 with the float32-valued bounds the kernels receive."""
    monkeypatch.setattr(O, "SCALE_BOUND", R.B_S)
    monkeypatch.setattr(O, "LIK_BOUND", R.B_L)


# ------------------------------------------------------------------------------------------------------------ reference cross-checks
@pytest.mark.parametrize("regime", R.GMM_REGIMES)
def test_gmm_reference_equals_float64_oracle(regime, f32_bounds):
    for K in KS:
        for shape in R.GMM_SHAPES:
            inp = R.gmm_inputs(regime, K, shape)
            for ymode in ("noise", "given"):
                yh = R.gmm_y_hat(inp, ymode)
                for logits in (True, False):
                    wts = inp["logits"] if logits else inp["weights"]
                    ref = R.gmm_ref(yh, inp["sigma"], inp["mu"], wts, K, logits)
                    got = R.gmm_oracle32(O, yh, inp["sigma"], inp["mu"], wts, K, logits, dtype=torch.float64)
                    for q in ("lik", "dy", "dsigma", "dmu", "dw") + (("dlogits", "w") if logits else ()):
                        e = scaled_err(got[q], *ref[q])
                        assert e <= 1e-12, f"{regime} K={K} {shape} {ymode} logits={logits} {q}: {e:.2e}"
                    e = scaled_err(-torch.log2(got["lik"]), *ref["bits"])
                    assert e <= 1e-12, f"{regime} K={K} bits: {e:.2e}"


def test_gmm_reference_positive_gradient_gates_equal_float64_oracle(f32_bounds):
    """sum(lik * g) with g of both signs: the likelihood gate blocks a positive g below the bound, the sigma gate a positive d sigma."""
    for regime in ("tail", "sharp"):
        inp = R.gmm_inputs(regime, 3, MAIN)
        g = torch.from_numpy(np.random.RandomState(3).standard_normal(size=MAIN).astype(np.float32))
        ref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], 3, True, g_lik=g)
        got = R.gmm_oracle32(O, inp["y"], inp["sigma"], inp["mu"], inp["logits"], 3, True, dtype=torch.float64, g_lik=g)
        for q in ("dy", "dsigma", "dmu", "dlogits"):
            assert scaled_err(got[q], *ref[q]) <= 1e-12, (regime, q)
        if regime == "tail":
            blocked = (ref["lik"][0] <= R.B_L) & (g > 0)
            assert int(blocked.sum()) > 10 and float(ref["dy"][0][blocked].abs().max()) == 0.0


@pytest.mark.parametrize("pset", R.EB_PSETS)
def test_bottleneck_reference_equals_float64_oracle(pset, f32_bounds):
    for regime in R.EB_REGIMES:
        for shape in ((3, 3, 2, 43), (1, 3, 1, 1)):
            table, quant = R.eb_params(pset, shape[0])
            inp = R.eb_inputs(regime, shape)
            for training in (True, False):
                zh = R.eb_quantize(inp["z"], quant[:, 0, 1], training, inp["noise"])
                ref = R.eb_ref(zh, table)
                got = R.eb_oracle32(O, inp["z"], table, quant, training, inp["noise"] if training else None, dtype=torch.float64)
                # (the oracle quantises in float64: round(z - med) + med need not be a float32, so eval compares at the oracle's own z_hat)
                if not training:
                    ref = R.eb_ref(got["z_hat"], table)
                for q in ("lik", "dz", "dparams") if training else ("lik",):
                    e = scaled_err(got[q], *ref[q])
                    assert e <= 1e-12, f"{pset} {regime} {shape} training={training} {q}: {e:.2e}"
    for C in R.AUX_CS:
        table, quant = R.eb_params(pset, C)
        ref, got = R.aux_ref(table, quant, target=R.AUX_TARGET), R.aux_oracle32(O, table, quant, dtype=torch.float64)
        for q in ("aux", "aux_dq"):
            assert scaled_err(got[q], *ref[q]) <= 1e-12, (pset, C, q)


def test_gmm_reference_at_40_digits():
    """A few hundred points of every regime: likelihood and the two derivative kernels of the closed form, in 40-digit arithmetic."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    Phi = lambda t: mp.erfc(-t / mp.sqrt(2)) / 2
    phi = lambda t: mp.exp(-t * t / 2) / mp.sqrt(2 * mp.pi)
    for regime in R.GMM_REGIMES:
        K, shape = 2, (1, 1, 7, 19)
        inp = R.gmm_inputs(regime, K, shape)
        ref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["weights"], K, logits=False, g_lik=-torch.ones(shape))
        lik, dmu, dsg = [], [], []
        for p in range(7 * 19):
            y = mp.mpf(float(inp["y"].reshape(-1)[p]))
            tot = mp.mpf(0)
            for k in range(K):
                sg, mu, w = (mp.mpf(float(inp[n].reshape(K, -1)[k, p])) for n in ("sigma", "mu", "weights"))
                s = max(sg, mp.mpf(R.B_S))
                d = y - mu
                ta, tb = (mp.mpf("0.5") - abs(d)) / s, (mp.mpf("-0.5") - abs(d)) / s
                tot += w * (Phi(ta) - Phi(tb))
                dmu.append(float(-mp.sign(d) * w * (phi(ta) - phi(tb)) / s))
                dsg.append(float(-w * (tb * phi(tb) - ta * phi(ta)) / s))
            lik.append(float(max(tot, mp.mpf(R.B_L))))
        order = lambda v: torch.tensor(v, dtype=torch.float64).reshape(-1, K).t().reshape(-1)
        assert scaled_err(torch.tensor(lik, dtype=torch.float64), *ref["lik"]) <= 1e-13, regime
        assert scaled_err(order(dmu), *ref["dmu"]) <= 1e-13, regime
        assert scaled_err(order(dsg), *ref["dsigma_raw"]) <= 1e-13, regime


def test_bottleneck_reference_at_40_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40

    def logits(row, x):
        v = [x]
        for l, (off, o, i) in enumerate(R._M_OFF):
            nxt = []
            for r in range(o):
                s = sum((row[off + r * i + c] if row[off + r * i + c] > 20 else mp.log(1 + mp.exp(row[off + r * i + c]))) * v[c] for c in range(i))
                s += row[R._B_OFF[l] + r]
                nxt.append(s + mp.tanh(row[R._F_OFF[l] + r]) * mp.tanh(s) if l < 4 else s)
            v = nxt
        return v[0]

    sig = lambda t: 1 / (1 + mp.exp(-t))
    for pset in R.EB_PSETS:
        table, quant = R.eb_params(pset, 1)
        row = [mp.mpf(float(t)) for t in table[0]]
        for regime in R.EB_REGIMES:
            z = R.eb_inputs(regime, (1, 3, 5, 17))["z"]
            ref = R.eb_ref(z, table)["lik"]
            got = []
            for v in z.reshape(-1)[:100]:
                lo, up = logits(row, mp.mpf(float(v)) - mp.mpf("0.5")), logits(row, mp.mpf(float(v)) + mp.mpf("0.5"))
                sg = -mp.sign(lo + up)
                got.append(float(max(abs(sig(sg * up) - sig(sg * lo)), mp.mpf(R.B_L))))
            e = scaled_err(torch.tensor(got, dtype=torch.float64), ref[0].reshape(-1)[:100], ref[1].reshape(-1)[:100])
            assert e <= 1e-12, (pset, regime, e)


# ------------------------------------------------------------------------------------------------------------ coverage conditions
def test_regime_coverage_conditions():
    """Conditions on the inputs (not measurements), on the float64 reference at the main shape."""
    for K in R.GMM_KS:
        inp = R.gmm_inputs("tail", K, MAIN)
        ref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], K)
        lik, bits = ref["lik"][0], ref["bits"][0]
        clamped = lik <= R.B_L
        assert float(clamped.double().mean()) >= 0.05, K
        assert float(((bits > 20) & ~clamped).double().mean()) >= 0.20, K
        assert float(lik.max()) > 0.1
        sg = R.gmm_inputs("sharp", K, MAIN)["sigma"]
        for v in R.SHARP_SIGMAS:
            assert int((sg == np.float32(v)).sum()) > 0, (K, v)
        assert R.SHARP_SIGMAS[2] < R.B_S == R.SHARP_SIGMAS[3] < R.SHARP_SIGMAS[4] and R.B_S < 0.11
        inp = R.gmm_inputs("flat", K, MAIN)
        assert float(R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], K)["lik"][0].min()) > R.B_L
        inp = R.gmm_inputs("ties", K, MAIN)
        d = (inp["y"].unsqueeze(1) - inp["mu"].reshape(MAIN[0], K, *MAIN[1:])).abs()
        assert int((d == 0).sum()) > 0 and int((d == 0.5).sum()) > 0 and int(((inp["y"] % 1.0) == 0.5).sum()) > 0
        if K > 1:
            inp = R.gmm_inputs("onehot", K, MAIN)
            top = inp["logits"].reshape(MAIN[0], K, -1).sort(dim=1).values
            assert float((top[:, -1] - top[:, -2]).min()) >= 40.0
            assert set(inp["weights"].unique().tolist()) == {0.0, 1.0}
    # every value is a float32, the bottleneck's parameter sets are what they say
    sat = R.eb_params("saturated", 3)[0]
    assert float(sat[:, :33].max()) > 88.8 and int((sat[:, :33] > 20).sum()) >= 12 and int((sat[:, :33] < -20).sum()) >= 18
    assert set(sat[:, 46:].abs().unique().tolist()) == {4.0}
    for regime, span in R.EB_REGIMES.items():
        z = R.eb_inputs(regime, (3, 3, 7, 37))["z"]
        assert 0.9 * span < float(z.abs().max()) <= span
    for pset in R.EB_PSETS:
        table, _ = R.eb_params(pset, 3)
        lik = {r: R.eb_ref(R.eb_inputs(r, (3, 3, 7, 37))["z"], table)["lik"][0] for r in R.EB_REGIMES}
        assert float(lik["core"].min()) > R.B_L and float(lik["tail"].min()) < 0.5 * float(lik["core"].min()), pset
        assert int((lik["far"] <= R.B_L).sum()) > 0 and int((lik["tail"] > R.B_L).sum()) > 0, pset


# ------------------------------------------------------------------------------------------------------------ the tolerance table
def test_tolerance_table_is_8x_the_float32_oracle(oracle_err):
    """Neither loosened nor stale: oracle_err <= TOL / 8 and TOL <= 32 max(oracle_err, 8 * 2^-24), for every entry; and the oracle's
    own error stays under 2^-10 (above that a scale would be missing a cancelled term)."""
    assert set(oracle_err) == set(R.TOL), sorted(set(oracle_err) ^ set(R.TOL))
    for regime, qs in oracle_err.items():
        assert set(qs) == set(R.TOL[regime]), regime
        for q, e in qs.items():
            tol = R.TOL[regime][q]
            print(f"{regime:10s} {q:8s} oracle {e:.3e}  TOL {tol:.2e}")
            assert tol >= R.TOL_FLOOR * (1 - 1e-6)
            assert e <= tol / 8, f"{regime}/{q}: oracle {e:.3e} > TOL/8 = {tol / 8:.3e}"
            assert tol <= 32 * max(e, 8 * R.EPS32), f"{regime}/{q}: TOL {tol:.3e} is stale (oracle {e:.3e})"
            assert e <= 2.0 ** -10, f"{regime}/{q}: the scale misses a cancelled term"


def test_oracle_bits_are_within_1e_4_bit(oracle_err):
    """In absolute terms: the float32 oracle's bits against the reference's, everywhere."""
    for regime in R.GMM_REGIMES:
        inp = R.gmm_inputs(regime, 5, MAIN)
        ref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], 5)
        got = R.gmm_oracle32(O, inp["y"], inp["sigma"], inp["mu"], inp["logits"], 5)
        assert float((got["bits"] - ref["bits"][0]).abs().max()) <= 1e-4, regime


# ------------------------------------------------------------------------------------------------------------ teeth
def _gmm_eval(fn, regime, K, logits):
    inp = R.gmm_inputs(regime, K, MAIN)
    yh = R.gmm_y_hat(inp, "noise")
    return fn(yh, inp["sigma"], inp["mu"], inp["logits"] if logits else inp["weights"], K, logits)


@pytest.mark.parametrize("regime", R.GMM_REGIMES)
def test_gmm_restatement_equals_the_oracle(regime):
    """The float32 restatement of gmm_fwd_kernel / gmm_bwd_kernel and the float32 oracle differ by at most TOL / 8, and the
    restatement itself is inside TOL.  (With the density taken as c * expf(-0.5f * t * t) instead of from erfcf's own argument, as
    gmm_bwd_kernel did, dy in `core` at K = 1 differs from the oracle by 9.5e-07 of the scale against TOL / 8 = 5.5e-07.)"""
    fails = []
    for K in KS:
        for logits in (True, False):
            ref = _gmm_eval(R.gmm_ref, regime, K, logits)
            orc = _gmm_eval(lambda *a: R.gmm_oracle32(O, *a), regime, K, logits)
            k32 = _gmm_eval(R.gmm_k32, regime, K, logits)
            for q in ("bits", "dy", "dsigma", "dmu", "dw") + (("dlogits", "w") if logits else ()):
                e, own, tol = scaled_err(k32[q], orc[q], ref[q][1]), scaled_err(k32[q], *ref[q]), R.TOL[regime][q]
                print(f"{regime} K={K} logits={logits} {q}: restatement - oracle {e:.3e} (TOL/8 {tol / 8:.3e}), restatement - reference {own:.3e}")
                assert own <= tol, f"{regime} K={K} logits={logits} {q}: the restatement is outside TOL: {own:.3e} > {tol:.3e}"
                if e > tol / 8:
                    fails.append(f"{regime} K={K} logits={logits} {q}: {e:.3e} > {tol / 8:.3e}")
    assert not fails, fails


# which regime and quantity must notice each mutation (it may show elsewhere too)
GMM_TEETH = {
    "no_reflection": ("tail", "bits"),
    "erfc_as_1_minus_erf": ("tail", "bits"),
    "phi_constant": ("core", "dy"),
    "dsigma_tb_term": ("core", "dsigma"),
    "softmax_no_dot": ("core", "dlogits"),
    "sigma_gate_gt": ("sharp", "dsigma"),
}
EB_TEETH = {
    "sign_fixed": ("eb_far", "bits"),
    "softplus_no_threshold": ("eb_core", "bits"),
    "tanh_derivative_1_minus_t": ("eb_core", "dparams"),
}


@pytest.mark.parametrize("mut", R.GMM_MUTATIONS)
def test_gmm_mutation_exceeds_the_table(mut):
    regime, q = GMM_TEETH[mut]
    worst = 0.0
    for K in KS:
        ref = _gmm_eval(R.gmm_ref, regime, K, True)
        got = _gmm_eval(lambda *a: R.gmm_k32(*a, mut=mut), regime, K, True)
        e = scaled_err(got[q], *ref[q])
        assert e > R.TOL[regime][q], f"{mut} K={K}: {regime}/{q} {e:.3e} <= TOL {R.TOL[regime][q]:.2e}"
        worst = max(worst, e)
    print(f"{mut}: {regime}/{q} {worst:.3e} against TOL {R.TOL[regime][q]:.2e}")


def _eb_eval(fn, pset, regime, shape=(3, 3, 2, 43)):
    table, quant = R.eb_params(pset, shape[0])
    inp = R.eb_inputs(regime, shape)
    return fn(R.eb_quantize(inp["z"], quant[:, 0, 1], True, inp["noise"]), table)


def test_bottleneck_restatement_equals_the_oracle():
    for pset in R.EB_PSETS:
        for regime in R.EB_REGIMES:
            shape = (3, 3, 2, 43)
            table, quant = R.eb_params(pset, 3)
            inp = R.eb_inputs(regime, shape)
            ref = _eb_eval(R.eb_ref, pset, regime)
            k32 = _eb_eval(R.eb_k32, pset, regime)
            orc = R.eb_oracle32(O, inp["z"], table, quant, True, inp["noise"])
            for q in ("bits", "dz", "dparams"):
                e = scaled_err(k32[q], orc[q], ref[q][1])
                assert e <= R.TOL["eb_" + regime][q] / 8, f"{pset} {regime} {q}: {e:.3e} > {R.TOL['eb_' + regime][q] / 8:.3e}"
        for C in R.AUX_CS:
            table, quant = R.eb_params(pset, C)
            ref, k32, orc = R.aux_ref(table, quant), R.aux_k32(table, quant), R.aux_oracle32(O, table, quant)
            for q in ("aux", "aux_dq"):
                e = scaled_err(k32[q], orc[q], ref[q][1])
                assert e <= R.TOL["eb_aux"][q] / 8, f"aux {pset} C={C} {q}: {e:.3e}"


@pytest.mark.parametrize("mut", R.EB_MUTATIONS)
def test_bottleneck_mutation_exceeds_the_table(mut):
    regime, q = EB_TEETH[mut]
    errs = {}
    for pset in R.EB_PSETS:
        ref = _eb_eval(R.eb_ref, pset, regime[3:])
        got = _eb_eval(lambda *a: R.eb_k32(*a, mut=mut), pset, regime[3:])
        errs[pset] = scaled_err(got[q], *ref[q])
    print(f"{mut}: {regime}/{q} {errs} against TOL {R.TOL[regime][q]:.2e}")
    assert max(errs.values()) > R.TOL[regime][q], f"{mut}: {errs}"


def test_scaled_err_sees_what_the_tensor_wide_ruler_does_not():
    """An element at 1e-6 wrong by a factor of 100 passes rel_err at 1e-4 and fails scaled_err by orders of magnitude."""
    from tests.util import rel_err
    ref = torch.tensor([1.0, 1e-6], dtype=torch.float64)
    got = torch.tensor([1.0, 1e-8], dtype=torch.float64)
    assert rel_err(got, ref) <= 1e-4
    assert scaled_err(got, ref, ref) > 0.9
    assert scaled_err(ref, ref, ref) == 0.0
    assert scaled_err(torch.tensor([float("nan"), 1e-6]), ref, ref) == math.inf
