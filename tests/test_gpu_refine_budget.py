"""GPU tests (-m gpu) of the latent refinement under a bit budget (masic_amd/refine.py, masic_amd/csrc/refine_budget.hip,
autograd.PairBudgetFn, HSIC.compress(latents=), StereoCodec(refine=)) against the CPU restatements of tests/budget_ref.py."""
import os

import numpy as np
import pytest
import torch

from tests import budget_ref as BR
from tests import refine_ref as R
from tests.test_gpu_refine import DEV, FIELDS, _assert_untouched, _files, _snapshot, _tensor, _tiny_net
from tests.util import rel_err

pytestmark = pytest.mark.gpu
NAN = float("nan")
SMALL = (1, 3, 4, 5)
GRID_CAP = 8192                                    # refine_slices.h: workgroups of a launch at most
_CACHE = {}


def _long(nt, B):
    """a per-pair length the bounded grid of a launch of nt tensors and B pairs needs two grid-stride passes for, with an odd tail"""
    return 4 * 256 * (GRID_CAP // (nt * B)) + 4 * 256 + 7


def _lens(n):
    """the per-pair lengths of the four tensors of one launch: n and three small ones, so that one launch mixes lengths"""
    return [n] + [m for m in (5, 3, 1, 4) if m != n][:3]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", SMALL + ("long",))
def test_seeds_closed_forms_and_rd_seeds_bits(n, B):
    """every element within 1e-6 of the float64 closed form (float32 results of float64 factors, as refine.rd_seeds is held to);
    mu = None and mu = ones give refine.rd_seeds' bits"""
    from masic_amd import refine
    n = _long(6, B) if n == "long" else n
    rng = np.random.RandomState(31 * B + n % 1000)
    ns = _lens(n)
    lmbda, hw = 0.0125, 37.0
    pics = [rng.uniform(0, 1, (B, n)).astype(np.float32) for _ in range(4)]
    liks = [rng.uniform(1e-6, 1.0, (B, m)).astype(np.float32) for m in ns]
    tp = [_tensor(B, n, s, a) for s, a in zip((1, 1, 0, 0), pics)]
    tl = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 2, 3), liks)]
    pd = [a.astype(np.float64) for a in pics]
    for g, mu in ((None, rng.uniform(0.01, 30.0, B)), (rng.uniform(0.5, 2.0, B), rng.uniform(0.01, 30.0, B)), (rng.uniform(0.5, 2.0, B), None)):
        g1, g2, gl = refine.budget_seeds(tp[0], tp[1], tp[2], tp[3], tl, lmbda, hw, None if g is None else _dev(g), None if mu is None else _dev(mu))
        gg, mm = np.ones(B) if g is None else g, np.ones(B) if mu is None else mu
        want1 = gg[:, None] * 2 * lmbda * 255.0 ** 2 * (pd[0] - pd[1]) / n
        want2 = gg[:, None] * 2 * lmbda * 255.0 ** 2 * (pd[2] - pd[3]) / n
        assert rel_err(g1.cpu(), torch.from_numpy(want1)) <= 1e-6 and rel_err(g2.cpu(), torch.from_numpy(want2)) <= 1e-6
        for k in range(4):
            want = -(gg * mm)[:, None] / (np.log(2.0) * hw * liks[k].astype(np.float64))
            err = float(np.max(np.abs(gl[k].cpu().numpy().astype(np.float64) - want) / np.abs(want)))       # every element to 1e-6 of itself
            assert err <= 1e-6, (k, err)
    for g in (None, _dev(rng.uniform(0.5, 2.0, B))):
        ref = refine.rd_seeds(tp[0], tp[1], tp[2], tp[3], tl, lmbda, hw, g)
        for mu in (None, torch.ones(B, dtype=torch.float64, device=DEV)):
            got = refine.budget_seeds(tp[0], tp[1], tp[2], tp[3], tl, lmbda, hw, g, mu)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
            for k in range(4):
                assert torch.equal(got[2][k], ref[2][k]), k


# one pair's (r_now, d_now, r_best, d_best) under the budget 100
TAKE = {"feasible against infeasible": (90.0, 0.5, 130.0, 0.7), "on the budget against infeasible": (100.0, 0.9, 130.0, 0.7),
        "both feasible, lower D": (99.0, 0.5, 95.0, 0.7), "both infeasible, fewer bits": (120.0, 0.9, 130.0, 0.7),
        "feasible against a NaN start": (90.0, 0.5, NAN, NAN)}
LEAVE = {"both feasible, higher D": (80.0, 0.9, 95.0, 0.7), "both feasible, equal D": (80.0, 0.7, 95.0, 0.7),
         "both infeasible, more bits": (150.0, 0.1, 130.0, 0.7), "both infeasible, equal R": (130.0, 0.1, 130.0, 0.7),
         "infeasible against feasible": (120.0, 0.1, 95.0, 0.7), "infeasible against on the budget": (100.5, 0.1, 100.0, 0.7),
         "the kept iterate itself": (95.0, 0.7, 95.0, 0.7), "NaN R": (NAN, 0.1, 130.0, 0.7), "NaN D": (90.0, NAN, 130.0, 0.7),
         "NaN both": (NAN, NAN, 130.0, 0.7), "infeasible against a NaN start": (120.0, 0.5, NAN, NAN)}


def _select_cases(B):
    cases = [(what, [v] * B, True) for what, v in TAKE.items()] + [(what, [v] * B, False) for what, v in LEAVE.items()]
    if B == 3:
        t, l = list(TAKE.values()), list(LEAVE.values())
        cases.append(("the middle pair only", [l[0], t[2], l[7]], None))
        cases.append(("the outer pairs", [t[0], l[4], t[3]], None))
    return cases


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", SMALL + ("long",))
def test_select_is_exact(n, B):
    """bit-exact against budget_ref.select over every branch of the rule, NaNs and ties; cur is never modified"""
    from masic_amd import refine
    n = _long(4, B) if n == "long" else n
    rng = np.random.RandomState(7 * B + n % 1000)
    ns = _lens(n)
    cur0 = [rng.standard_normal((B, m)).astype(np.float32) for m in ns]
    best0 = [rng.standard_normal((B, m)).astype(np.float32) for m in ns]
    cur = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 2, 3), cur0)]
    target = np.full(B, 100.0)
    cases = _select_cases(B)
    if n > 5:
        cases = cases[:1] + cases[5:6] + cases[-2:]                    # the long slices: one that copies, one that does not, the mixed ones
    for what, rows, all_take in cases:
        best = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 0, 2), best0)]          # tensors 2, 3: cur and best aligned differently
        r_now, d_now, rb, db = (np.array(col, dtype=np.float64) for col in zip(*rows))
        r_best, d_best = _dev(rb), _dev(db)
        refine.budget_select(cur, best, _dev(r_now), _dev(d_now), _dev(target), r_best, d_best)
        take, want_r, want_d = BR.select(r_now, d_now, target, rb, db)
        if all_take is not None:
            assert take.all() if all_take else not take.any(), what
        else:
            assert take.any() and not take.all(), what
        assert np.array_equal(r_best.cpu().numpy(), want_r, equal_nan=True) and np.array_equal(d_best.cpu().numpy(), want_d, equal_nan=True), what
        for k in range(4):
            want = np.where(take[:, None], cur0[k], best0[k])
            assert np.array_equal(best[k].cpu().numpy(), want), (what, k)
    for k in range(4):
        assert np.array_equal(cur[k].cpu().numpy(), cur0[k]), k


@pytest.mark.parametrize("B", (1, 3, 300))
def test_mu_update(B):
    """against numpy float64 to 1e-12 relative (a double exp and three flops are within a few 1e-16: the margin absorbs libm
    differences); both clamps are hit exactly; a NaN R leaves mu"""
    from masic_amd import refine
    rng = np.random.RandomState(B)
    mu0 = np.exp(rng.uniform(-5, 5, B))
    target = rng.uniform(1e3, 1e6, B)
    r = target * rng.uniform(0.2, 3.0, B)
    for gain in (0.5, 1.0, 2.0):
        mu = _dev(mu0)
        refine.budget_mu(mu, _dev(r), _dev(target), gain)
        want = BR.mu_update(mu0, r, target, gain)
        assert float(np.max(np.abs(mu.cpu().numpy() - want) / want)) <= 1e-12, gain
    # the clamps, exactly; NaN; R = T leaves mu bit for bit
    mu0 = np.resize([1000.0, 2.0 ** -9, 3.0, 7.0, 1.0, 2.0 ** 10, 2.0 ** -10], B)
    r = np.resize([200.0, 1.0, NAN, 100.0, 1e9, 100.0, 100.0], B)
    target = np.full(B, 100.0)
    mu = _dev(mu0)
    refine.budget_mu(mu, _dev(r), _dev(target), 1.0)
    want = np.resize([2.0 ** 10, 2.0 ** -10, 3.0, 7.0, 2.0 ** 10, 2.0 ** 10, 2.0 ** -10], B)
    assert np.array_equal(mu.cpu().numpy(), want) and np.array_equal(want, BR.mu_update(mu0, r, target, 1.0))
    mu = _dev(np.full(B, 1.5))
    refine.budget_mu(mu, _dev(np.full(B, 150.0)), _dev(target), 1.0, mu_min=1.0, mu_max=2.0)          # own clamp values
    assert np.array_equal(mu.cpu().numpy(), np.full(B, 2.0))


def test_budget_wrappers_refuse():
    from masic_amd import refine
    t = [torch.zeros(2, 5, device=DEV) for _ in range(4)]
    d = lambda n=2: torch.ones(n, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="four tensors"):
        refine.budget_select(t[:3], t, d(), d(), d(), d(), d())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.budget_select([x.cpu() for x in t], t, d(), d(), d(), d(), d())
    with pytest.raises(RuntimeError, match="shapes"):
        refine.budget_select(t, t[:3] + [torch.zeros(2, 6, device=DEV)], d(), d(), d(), d(), d())
    with pytest.raises(RuntimeError, match="r_now"):
        refine.budget_select(t, t, torch.zeros(2, device=DEV), d(), d(), d(), d())
    with pytest.raises(RuntimeError, match="target"):
        refine.budget_select(t, t, d(), d(), d(3), d(), d())
    with pytest.raises(RuntimeError, match="d_best"):
        refine.budget_select(t, t, d(), d(), d(), d(), d().cpu())
    with pytest.raises(RuntimeError, match="mu"):
        refine.budget_mu(torch.ones(2, device=DEV), d(), d(), 1.0)
    with pytest.raises(RuntimeError, match="r_now"):
        refine.budget_mu(d(), d(3), d(), 1.0)
    for gain, lo, hi in ((0.0, 0.5, 2.0), (NAN, 0.5, 2.0), (True, 0.5, 2.0), (1.0, 2.0, 0.5), (1.0, 0.0, 2.0), (1.0, 0.5, float("inf"))):
        with pytest.raises(RuntimeError, match="budget_mu"):
            refine.budget_mu(d(), d(), d(), gain, lo, hi)
    p = torch.zeros(2, 7, device=DEV)
    with pytest.raises(RuntimeError, match="mu"):
        refine.budget_seeds(p, p, p, p, t, 0.01, 4.0, None, d(3))
    with pytest.raises(RuntimeError, match="g must"):
        refine.budget_seeds(p, p, p, p, t, 0.01, 4.0, torch.ones(2, device=DEV), d())
    with pytest.raises(RuntimeError, match="at most 4"):
        refine.budget_seeds(p, p, p, p, t + t[:1], 0.01, 4.0)
    with pytest.raises(RuntimeError, match="float32"):
        refine.budget_seeds(p.double(), p, p, p, t, 0.01, 4.0)


# ------------------------------------------------------------------------------------------------ 2. the loop on the tiny net
def _setup():
    if "net" not in _CACHE:
        from masic_amd import nn as mnn
        try:
            net = _tiny_net("f32")
        finally:
            mnn.set_precision("f32")
        c = R.tiny_case(2, torch.float32)
        _CACHE.update(net=net, c=c, x=tuple(c[k].to(DEV) for k in ("x1", "x2", "h_matrix")))
    return _CACHE["net"], _CACHE["c"], _CACHE["x"]


def _config(**kw):
    from masic_amd import refine
    return refine.RefineConfig(**BR.LOOP, budget_gain=BR.GAIN, **kw)


def _true_rd(net, lat, x1, x2, hm):
    """(R, D) of the four latents as refine_latents evaluates them: pair_rd on HSIC._eval_from_latents"""
    from masic_amd import metrics, ops, refine
    from masic_amd.homography import warp_matrices
    B, _, H, W = x1.shape
    with torch.no_grad():
        m_fwd = torch.cat([warp_matrices(hm[i:i + 1], (H, W), (H, W), want_inverse=True)[0] for i in range(B)]).contiguous()
        gates = net.mask2weights_unit(ops.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))).contiguous()
        out = net._eval_from_latents(*lat, m_fwd, gates)
        L = out["likelihoods"]
        rows = metrics.pair_rd(out["x1_hat"].contiguous(), x1, out["x2_hat"].contiguous(), x2, [L[k].contiguous() for k in ("y1", "y2", "z1", "z2")])
        return refine.bits_and_mse(rows, 3 * H * W)


def _rel_one():
    """budget_rel = 1.0 on the tiny fixture, run twice: computed once for the tests below"""
    if "one" not in _CACHE:
        from masic_amd import refine
        net, c, (x1, x2, hm) = _setup()
        snap = _snapshot(net)
        a = refine.refine_latents(net, x1, x2, hm, c["lmbda"], _config(budget_rel=1.0))
        b = refine.refine_latents(net, x1, x2, hm, c["lmbda"], _config(budget_rel=1.0))
        torch.cuda.synchronize()
        _assert_untouched(net, snap)
        _CACHE["one"] = (a, b)
    return _CACHE["one"]


def test_no_budget_is_todays_call():
    """both budgets None (whatever budget_gain says): a Refined, torch.equal to the call of a config that names no budget field"""
    from masic_amd import refine
    net, c, (x1, x2, hm) = _setup()
    today = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig(**BR.LOOP))
    got = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig(**BR.LOOP, budget_bpp=None, budget_rel=None, budget_gain=2.0))
    assert type(today) is refine.Refined and type(got) is refine.Refined and len(got) == 6
    for k, name in enumerate(refine.Refined._fields):
        assert torch.equal(today[k], got[k]), name


def test_budget_rel_one_never_more_bits_never_worse():
    from masic_amd import refine
    net, c, (x1, x2, hm) = _setup()
    a, b = _rel_one()
    assert type(a) is refine.RefinedToBudget
    for k, name in enumerate(refine.RefinedToBudget._fields):
        assert torch.equal(a[k], b[k]), name                         # two identical calls are bit-equal
        assert a[k].is_cuda and (a[k].dtype == (torch.float32 if k < 4 else torch.float64)), name
    print("budget_rel 1.0: bits_start", a.bits_start.cpu().numpy(), "bits_best", a.bits_best.cpu().numpy(), "mse_start", a.mse_start.cpu().numpy(),
          "mse_best", a.mse_best.cpu().numpy(), "mu", a.mu.cpu().numpy())
    assert torch.equal(a.target_bits, a.bits_start)
    assert bool((a.bits_best <= a.target_bits).all()) and bool((a.mse_best <= a.mse_start).all())
    r, d = _true_rd(net, a[:4], x1, x2, hm)
    assert torch.equal(r, a.bits_best) and torch.equal(d, a.mse_best)
    hw = float(x1.shape[2] * x1.shape[3])
    for cost, bits, mse in ((a.cost_start, a.bits_start, a.mse_start), (a.cost_best, a.bits_best, a.mse_best)):
        assert torch.equal(cost, bits / hw + (c["lmbda"] * 255.0 ** 2) * mse)
    start = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig())
    assert float(rel_err(a.cost_start.cpu(), start.cost_start.cpu())) <= 1e-12          # the same objective, its float64 terms in another order


def test_budget_below_the_start_follows_the_restated_rule():
    """budget_rel = BUDGET_REL (tests/test_cpu_refine_budget.py pins it): the traced multiplier is budget_ref's update of the traced R,
    the kept iterate is budget_ref's selection over the traced (R, D), section 8.10's guarantees hold, and every pair the float64
    oracle loop finished feasible with its 2 % margin ends feasible here"""
    from masic_amd import refine
    net, c, (x1, x2, hm) = _setup()
    snap = _snapshot(net)
    trace = []
    out = refine.refine_latents(net, x1, x2, hm, c["lmbda"], _config(budget_rel=BR.BUDGET_REL), trace=trace)
    torch.cuda.synchronize()
    _assert_untouched(net, snap)
    target = out.target_bits.cpu().numpy()
    assert np.array_equal(target, BR.BUDGET_REL * out.bits_start.cpu().numpy())
    steps = [s for s, *_ in trace]
    assert steps == list(range(0, 101, 5))
    mu_prev, r_best, d_best = np.ones(2), None, None
    for s, r, d, mu in trace:
        r, d, mu = r.cpu().numpy(), d.cpu().numpy(), mu.cpu().numpy()
        print(f"step {s:3d}  R {r}  R / T {r / target}  D {d}  mu {mu}")
        want = BR.mu_update(mu_prev, r, target, BR.GAIN)
        assert float(np.max(np.abs(mu - want) / want)) <= 1e-12, s
        mu_prev = mu
        r_best, d_best = (r, d) if s == 0 else BR.select(r, d, target, r_best, d_best)[1:]
    assert np.array_equal(trace[0][1].cpu().numpy(), out.bits_start.cpu().numpy()) and np.array_equal(trace[0][2].cpu().numpy(), out.mse_start.cpu().numpy())
    assert np.array_equal(out.bits_best.cpu().numpy(), r_best) and np.array_equal(out.mse_best.cpu().numpy(), d_best)
    assert np.array_equal(out.mu.cpu().numpy(), mu_prev)
    all_r = np.stack([t[1].cpu().numpy() for t in trace])
    for b in range(2):
        if (all_r[:, b] <= target[b]).any():
            assert r_best[b] <= target[b], b
        else:
            assert r_best[b] <= all_r[0, b], b
    c64 = R.tiny_case(2, torch.float64)
    start = [t.cpu().double() for t in refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig())[:4]]
    o = BR.oracle_budget_loop(c64["sd"], start, c64["x1"], c64["x2"], c64["h_matrix"], c64["K"], c64["lmbda"], budget_rel=BR.BUDGET_REL, **BR.LOOP)
    margin = o["r_best"] <= 0.98 * o["target"]
    print("oracle: R_best / T", o["r_best"] / o["target"], "here", r_best / target, "D_best", o["d_best"], "here", d_best)
    assert margin.any()
    for b in range(2):
        if margin[b]:
            assert r_best[b] <= target[b], b


def test_budget_steps_zero_returns_the_encoders_latents():
    from masic_amd import refine
    net, c, (x1, x2, hm) = _setup()
    out = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig(steps=0, budget_rel=0.5, budget_gain=BR.GAIN))
    plain = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig())
    assert type(out) is refine.RefinedToBudget
    with torch.no_grad():
        for i in range(2):
            for got, want in zip(out[:4], net.latents(x1[i:i + 1], x2[i:i + 1], hm[i:i + 1])):
                assert torch.equal(got[i:i + 1], want)
    for k in range(4):
        assert torch.equal(out[k], plain[k])
    assert torch.equal(out.bits_best, out.bits_start) and torch.equal(out.mse_best, out.mse_start) and torch.equal(out.cost_best, out.cost_start)
    assert torch.equal(out.target_bits, 0.5 * out.bits_start)
    assert np.array_equal(out.mu.cpu().numpy(), BR.mu_update(np.ones(2), out.bits_start.cpu().numpy(), out.target_bits.cpu().numpy(), BR.GAIN))
    bpp = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig(steps=0, budget_bpp=[1.5, 2.0]))
    assert bpp.target_bits.cpu().tolist() == [1.5 * 64 * 64, 2.0 * 64 * 64]
    with pytest.raises(ValueError, match="3 values for 2 pairs"):
        refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig(steps=0, budget_bpp=[1.0, 1.0, 1.0]))


# ------------------------------------------------------------------------------------------------ 3. files
def test_files_from_budgeted_latents_round_trip(tmp_path):
    """the RefinedToBudget goes to compress / compress_batch as latents= and the files decode exactly; file bits beside estimated bits"""
    net, c, (x1, x2, hm) = _setup()
    a, _ = _rel_one()
    with torch.no_grad():
        enc = net.compress_batch(x1, x2, hm, ["r0", "r1"], str(tmp_path), latents=a)
        dec = net.decompress_batch(["r0", "r1"], hm, str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
        assert torch.equal(enc["y1_hat"], torch.round(a.y1)) and torch.equal(enc["y2_hat"], torch.round(a.y2))
        plain = net.compress_batch(x1, x2, hm, ["p0", "p1"], str(tmp_path))
        for i in range(2):
            print(f"pair {i}: file bits {enc['bytes'][i] * 8} (unrefined {plain['bytes'][i] * 8}), estimated bits {float(a.bits_best[i]):.1f} "
                  f"(unrefined {float(a.bits_start[i]):.1f}), budget {float(a.target_bits[i]):.1f}")
        one = type(a)(*[t[:1].contiguous() for t in a])
        e1 = net.compress(x1[:1], x2[:1], hm[:1], "s", str(tmp_path), latents=one)
        d1 = net.decompress(None, None, hm[:1], "s", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(e1[k], d1[k]), k
    assert len(_files(tmp_path, "s")[1]) > 0


def test_stereo_codec_refine_to_budget(tmp_path):
    from masic_amd import StereoCodec, nn as mnn, refine, synth
    from masic_amd.align import PatchAligner
    try:
        net, _, _ = _setup()
        udh = PatchAligner().to(DEV).eval()
        a, b, _ = synth.synth_inputs(2, 72, 100, seed=5)
        u8 = lambda x: torch.from_numpy(np.ascontiguousarray(np.rint(x.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).to(DEV)
        left, right = u8(a), u8(b)
        names = ["p", "q"]
        enc = StereoCodec(net, udh, refine=refine.RefineConfig(steps=20, lmbda=0.01, budget_rel=1.0)).encode(left, right, names, str(tmp_path))
        dec = StereoCodec(net).decode(names, str(tmp_path))
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert torch.equal(dec["x1_hat"], enc["x1_hat"]) and torch.equal(dec["x2_hat"], enc["x2_hat"])
        with pytest.raises(ValueError, match=r"StereoCodec.encode.*1 values for 2 pairs"):
            StereoCodec(net, udh, refine=refine.RefineConfig(steps=3, lmbda=0.01, budget_bpp=[1.0])).encode(left, right, ["u", "v"], str(tmp_path))
        assert not os.path.exists(os.path.join(str(tmp_path), "u.msf"))
    finally:
        mnn.set_precision("f32")


def test_full_width_bf16_budget_holds_and_exact_round_trip(tmp_path):
    """once at HSIC(128,192,5), 2 x 128 x 128, bf16 operands, budget_rel = 1.0: never more estimated bits and never a higher MSE than
    the start, and the files of the kept latents decode exactly"""
    import MASIC
    from masic_amd import nn as mnn, refine, synth
    try:
        mnn.set_precision("bf16")
        net = MASIC.HSIC(128, 192, 5)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=21))
        net = net.to(DEV).eval()
        net.update()
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(2, 128, 128, seed=21))
        snap = _snapshot(net)
        out = refine.refine_latents(net, x1, x2, hm, 0.01, refine.RefineConfig(steps=10, lr=0.1, check_every=5, budget_rel=1.0, budget_gain=BR.GAIN))
        torch.cuda.synchronize()
        _assert_untouched(net, snap)
        rs, rb, ds, db = (t.cpu().numpy() for t in (out.bits_start, out.bits_best, out.mse_start, out.mse_best))
        print("bf16 full width: bits_start", rs, "bits_best", rb, "mse_start", ds, "mse_best", db, "mu", out.mu.cpu().numpy())
        assert all(np.isfinite(v).all() for v in (rs, rb, ds, db))
        assert torch.equal(out.target_bits, out.bits_start) and (rb <= rs).all() and (db <= ds).all()
        with torch.no_grad():
            enc = net.compress_batch(x1, x2, hm, ["a", "b"], str(tmp_path), latents=out)
            dec = net.decompress_batch(["a", "b"], hm, str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
    finally:
        mnn.set_precision("f32")
