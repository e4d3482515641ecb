"""TEST INFRASTRUCTURE for the latent refinement under a bit budget (masic_amd/refine.py, include/masic_budget.h): independent
restatements on the CPU, numpy float64.

    wins / select        the constrained keep-best rule of masic_budget_select
    mu_update            the multiplier update of masic_budget_mu
    true_rd              (R [B] bits, D [B] = MSE1 + MSE2) of the eval-mode path of tests/refine_ref.py
    oracle_budget_loop   the budgeted loop on tests/refine_ref.py's graph

tests/refine_ref.py is imported, not edited: the gradient of J_b(mu) = mu_b bits_b / (H W) + lmbda 255^2 (MSE1_b + MSE2_b) for one pair
is mu_b times the gradient R.latent_grads returns for lmbda / mu_b on that pair's B = 1 slice.
"""
import numpy as np
import torch

from tests import refine_ref as R

MU_MIN, MU_MAX = 2.0 ** -10, 2.0 ** 10
BUDGET_REL = 0.7                 # pinned by tests/test_cpu_refine_budget.py::test_budget_fixture_is_admissible (it checks this value)
GAIN = 1.0                       # the gain the fixture's loops run with, whatever the library's default
LOOP = dict(steps=100, lr=0.1, check_every=5, seed=3)


def wins(r, d, t, r_best, d_best):
    """One pair: does the candidate (r, d) replace the kept (r_best, d_best) under the budget t?"""
    if np.isnan(r) or np.isnan(d):
        return False
    fc, fk = bool(r <= t), bool(r_best <= t)
    if fc and not fk:
        return True
    if fc and fk:
        return bool(d < d_best)
    if not fc and not fk:
        return bool(r < r_best)
    return False


def select(r, d, t, r_best, d_best):
    """float64 [B] arrays -> (take [B] bool, r_best', d_best')"""
    r, d, t, r_best, d_best = (np.asarray(a, dtype=np.float64) for a in (r, d, t, r_best, d_best))
    take = np.array([wins(*v) for v in zip(r, d, t, r_best, d_best)], dtype=bool)
    return take, np.where(take, r, r_best), np.where(take, d, d_best)


def mu_update(mu, r, t, gain, mu_min=MU_MIN, mu_max=MU_MAX):
    """float64 [B]: clamp(mu exp(gain (r / t - 1)), mu_min, mu_max); a NaN r leaves mu"""
    mu, r, t = (np.asarray(a, dtype=np.float64) for a in (mu, r, t))
    with np.errstate(over="ignore", invalid="ignore"):
        new = np.minimum(np.maximum(mu * np.exp(gain * (r / t - 1.0)), mu_min), mu_max)
    return np.where(np.isnan(r), mu, new)


def true_rd(sd, lat, x1, x2, h_matrix, K):
    """(R [B], D [B]) float64 numpy of the eval-mode path from the latents"""
    B = x1.shape[0]
    with torch.no_grad():
        out = R.forward_from_latents(sd, *lat, x1, h_matrix, None, K)
        bits = sum(-torch.log2(l).reshape(B, -1).sum(dim=1) for l in out["likelihoods"].values())
        mse = ((out["x1_hat"] - x1) ** 2).reshape(B, -1).mean(dim=1) + ((out["x2_hat"] - x2) ** 2).reshape(B, -1).mean(dim=1)
    return bits.double().numpy(), mse.double().numpy()


def oracle_budget_loop(sd, lat, x1, x2, h_matrix, K, lmbda, steps, lr, check_every=5, seed=0, pair_keys=None, budget_rel=None,
                       target=None, gain=GAIN):
    """The budgeted loop of masic_amd.refine.refine_latents -> dict of float64 numpy: r_start, d_start, target, r_best, d_best, mu [B]
    and trace, the list of (step, R, D, mu after the check's update)."""
    B = x1.shape[0]
    pair_keys = list(range(B)) if pair_keys is None else list(pair_keys)
    dt = x1.dtype
    cur = [t.detach().clone() for t in lat]
    ms, vs = [np.zeros(t.shape) for t in cur], [np.zeros(t.shape) for t in cur]
    r_start, d_start = true_rd(sd, cur, x1, x2, h_matrix, K)
    target = budget_rel * r_start if target is None else np.asarray(target, dtype=np.float64)
    mu = mu_update(np.ones(B), r_start, target, gain)
    r_best, d_best = r_start.copy(), d_start.copy()
    trace = [(0, r_start.copy(), d_start.copy(), mu.copy())]
    shapes = [tuple(t.shape) for t in cur]
    for s in range(1, steps + 1):
        noise = [torch.from_numpy(u).to(dt) for u in R.step_noise(shapes, s, seed, pair_keys)]
        grads = [np.zeros(shp) for shp in shapes]
        for b in range(B):
            one = slice(b, b + 1)
            g, _, _ = R.latent_grads(sd, [t[one] for t in cur], x1[one], x2[one], h_matrix[one], [u[one] for u in noise], K,
                                     lmbda / float(mu[b]))
            for k in range(4):
                grads[k][one] = float(mu[b]) * g[k].double().numpy()
        for k in range(4):
            p, ms[k], vs[k] = R.adam_step(cur[k].double().numpy(), grads[k], ms[k], vs[k], lr, s)
            cur[k] = torch.from_numpy(p).to(dt)
        if s % check_every == 0 or s == steps:
            r_now, d_now = true_rd(sd, cur, x1, x2, h_matrix, K)
            _, r_best, d_best = select(r_now, d_now, target, r_best, d_best)
            mu = mu_update(mu, r_now, target, gain)
            trace.append((s, r_now.copy(), d_now.copy(), mu.copy()))
    return dict(r_start=r_start, d_start=d_start, target=target, r_best=r_best, d_best=d_best, mu=mu, trace=trace)
