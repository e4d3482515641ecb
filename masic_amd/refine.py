"""Encoder-side latent refinement: smaller files from the same decoder (INTEGRATION.md "Latent refinement").

`HSIC.compress` rounds whatever the analysis transforms output, but the decoder never sees those transforms -- only round(y1),
round(y2) and the two z streams.  `refine_latents` therefore optimises the four latents of each pair against the pair's own
rate-distortion objective before they are coded; weights, decoder and file format stay as they are, and a file written from the result
(`HSIC.compress(..., latents=refined)`) decodes with today's `decompress`.

    refine_latents(hsic, x1, x2, h_matrix, lmbda, RefineConfig(steps=100))   -> Refined(y1, y2, z1, z2, cost_start, cost_best)

The loop: Adam on the latents (one launch per step for all four), gradient of the "mixed" surrogate `HSIC._forward_refine` -- rounded
values with an identity gradient wherever the decoder sees a rounded value, uniform noise where a likelihood is evaluated -- summed
over the pairs' objectives J_b = bits_b / (H W) + lmbda 255^2 (MSE1_b + MSE2_b) (autograd.PairRateDistortionFn: nothing is divided
by B).  Every `check_every` steps and at the last one the TRUE objective -- J_b on the eval-mode path from the latents, what the file
will cost and how the decoder will reconstruct -- is evaluated and the best iterate per pair is kept on the device; the host never
reads a cost inside the loop.  cost_best <= cost_start by construction, and steps = 0 returns the encoder's latents bit for bit.

The noise is the library's own (Philox4x32-10, keyed by seed and pair key, masic_refine_noise): torch's generators are not touched,
and a pair's noise does not depend on its batch mates.  The weights are frozen for the call (requires_grad off, restored after it):
no weight-, bias- or table-gradient launch runs and no parameter's .grad changes.

Limits.  The result of a pair is NOT promised to be bit-equal across batch compositions: several bf16 layers pick their kernels by
batch shape.  The surrogate and the check model the context model of HSIC.band_rows (0: the unbanded one): set it to the band_rows the
file will be coded with (bands.model_band_rows) and the loop descends and checks that file's rate; files coded with another band_rows
from refined latents decode exactly (the coder uses the final latents) but the rate the loop minimised is not theirs.  The bands are
those of the full-latent parameter form, not the pixel-list kernels' bf16 arithmetic.  fp8 operands are not supported.

Under a bit budget (RefineConfig(budget_bpp=...) or (budget_rel=...); both None: everything above, unchanged).  The objective
above follows lmbda wherever it leads -- on a model that sits at the wrong operating point to files three times the size
(profiles/refine_bench.txt).  With a budget the call solves, per pair b and independent of its batch mates,

    minimise D_b = MSE1_b + MSE2_b   subject to   R_b <= T_b

where R_b is the true estimated bits of the pair (minus the sum of the four metrics.pair_rd log columns / ln 2 on
HSIC._eval_from_latents) and T_b its budget in bits.  A step descends J_b(mu) = mu_b bits_b / (H W) + lmbda 255^2 (MSE1_b + MSE2_b)
(autograd.PairBudgetFn), mu float64 [B] on the device, 1 at the start.  At every check (the evaluation of the start is one), from the
one pair_rd call it makes:
  * the constrained keep-best (masic_budget_select): a candidate (R, D) replaces the kept iterate (R_best, D_best) iff neither value
    is NaN and  [candidate feasible, kept not]  or  [both feasible and D < D_best]  or  [both infeasible and R < R_best];
    equality never replaces and an infeasible candidate never replaces a feasible one;
  * then mu_b <- clamp(mu_b exp(budget_gain (R_b / T_b - 1)), MU_MIN, MU_MAX) (masic_budget_mu; a NaN R_b leaves mu_b).
By construction: if any checked iterate, the start included, was feasible, the result is feasible; if the start was feasible,
D_best <= D_start; if nothing was feasible, R_best <= R_start.  The call returns a RefinedToBudget.

Limits of the budget.  It is on the ESTIMATED bits of the context model of HSIC.band_rows, as the loop's rate is: file bytes exceed
the estimate by the container and coder overhead (measured: profiles/refine_budget_bench.txt), and a file coded with another
band_rows than the attribute is budgeted against the attribute's estimate.  fp8 is refused as without a budget.

The elementwise kernels are declared in include/masic_refine.h and include/masic_budget.h, side headers of libmasic_hip.so bound by
_lib.bind_header.  No CPU path.
"""
import collections
import ctypes
import math

import torch

from . import _lib

HEADER_PATH = _lib.header_path("masic_refine.h")
MAX_PAIRS = 65535                # the pair is a grid dimension of the kernels

SIGNATURES = _lib.bind_header(HEADER_PATH, "masic_refine_")          # name -> (restype, argtypes) of every prototype of masic_refine.h
BUDGET_HEADER_PATH = _lib.header_path("masic_budget.h")
BUDGET_SIGNATURES = _lib.bind_header(BUDGET_HEADER_PATH, "masic_budget_")          # likewise of masic_budget.h
MU_MIN, MU_MAX = 2.0 ** -10, 2.0 ** 10          # the clamp of the rate multiplier of the budgeted loop

# The default step size rests on tools/bench_refine.py's table (profiles/refine_bench.txt: a briefly trained full-width model, 8 pairs of
# 512 x 512, bf16): of 0.1 / 0.05 / 0.02, 0.05 reached the lowest true objective after 10 and after 50 steps and was within 0.2 % of
# the best (0.02) after 200.  On the tiny untrained fixture (tests/test_cpu_refine.py) 0.1 moves 8x further than 0.02 in 100 steps.
DEFAULT_LR = 0.05

# The default gain of the multiplier update rests on tools/bench_refine.py --budget-rel's table (profiles/refine_budget_bench.txt: the
# model and pairs of DEFAULT_LR's, budget_rel 1.0 and 0.75, 50 and 200 steps): of 0.5 / 1 / 2, gain 2 ended within the budget on 24 of the
# 32 pair-runs (1: 20, 0.5: 16), and where 1 and 2 were both feasible on every pair their MSE was level (12.86 against 13.19 x 1e-3 at 200).
DEFAULT_BUDGET_GAIN = 2.0

Refined = collections.namedtuple("Refined", "y1 y2 z1 z2 cost_start cost_best")
Refined.__doc__ = """The best iterate of refine_latents as float32 latents [B, ...] and the true objective of every pair at the start and at
that iterate (float64 [B] on the device).  HSIC.compress / compress_batch take it as `latents=`."""

RefinedToBudget = collections.namedtuple("RefinedToBudget", Refined._fields + ("bits_start", "bits_best", "mse_start", "mse_best",
                                                                              "target_bits", "mu"))
RefinedToBudget.__doc__ = """The kept iterate of refine_latents under a bit budget.  The first six fields are Refined's: cost_start / cost_best hold
the ordinary objective (mu = 1), bits / (H W) + lmbda 255^2 mse, of the start and of the kept iterate.  Then, float64 [B] on the device:
the true estimated bits R and MSE1 + MSE2 of the start and of the kept iterate, the pair's budget in bits and the multiplier at the end.
HSIC.compress / compress_batch take it as `latents=`."""


def _positive(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and 0.0 < float(v) < float("inf")


class RefineConfig:
    """steps: Adam steps (0: off -- the encoder's latents come back bit for bit); lr: Adam's step size (betas 0.9 / 0.999, eps 1e-8, no
    decay); check_every: the true objective is evaluated every that many steps (and at the last); seed: 0 .. 2^32 - 1, the first key
    word of the noise; pair_keys: one 0 .. 2^32 - 1 key per pair (None: the pair's index in the call) -- a pair refined under the same
    seed and key sees the same noise whatever its position; lmbda: the rate-distortion weight for callers that carry no lmbda of their
    own (StereoCodec, tools/eval_folder.py); refine_latents' own argument wins.
    The bit budget (at most one of the two; both None: no budget, the unconstrained loop): budget_bpp: a positive finite number, or
    one per pair -- the pair may cost at most that many estimated bits per pixel, bpp as this project defines it, bits / (H W) of the
    pictures refine_latents is given (StereoCodec: the padded size), so T_b = bpp H W; budget_rel: a positive finite number, T_b =
    budget_rel * the estimated bits of the unrefined latents -- 1.0: never more bits than those.  budget_gain: the gain of the
    multiplier update, mu_b <- mu_b exp(budget_gain (R_b / T_b - 1)) at every check."""

    def __init__(self, steps=0, lr=DEFAULT_LR, check_every=5, seed=0, pair_keys=None, lmbda=None, budget_bpp=None, budget_rel=None,
                 budget_gain=DEFAULT_BUDGET_GAIN):
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
            raise ValueError(f"RefineConfig: steps must be an integer >= 0, got {steps!r}")
        if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
            raise ValueError(f"RefineConfig: check_every must be an integer >= 1, got {check_every!r}")
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (0.0 < float(lr) < float("inf")):
            raise ValueError(f"RefineConfig: lr must be a positive finite number, got {lr!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"RefineConfig: seed must be an integer in 0 .. 2^32 - 1, got {seed!r}")
        if pair_keys is not None:
            pair_keys = [k for k in pair_keys]
            for k in pair_keys:
                if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 2 ** 32:
                    raise ValueError(f"RefineConfig: pair_keys must be integers in 0 .. 2^32 - 1, got {k!r}")
        if lmbda is not None and (isinstance(lmbda, bool) or not isinstance(lmbda, (int, float)) or not (0.0 < float(lmbda) < float("inf"))):
            raise ValueError(f"RefineConfig: lmbda must be a positive finite number or None, got {lmbda!r}")
        if budget_bpp is not None and budget_rel is not None:
            raise ValueError("RefineConfig: at most one of budget_bpp and budget_rel may be set")
        if budget_bpp is not None and not isinstance(budget_bpp, (bool, int, float)):
            if isinstance(budget_bpp, (str, bytes)) or not hasattr(budget_bpp, "__iter__"):
                raise ValueError(f"RefineConfig: budget_bpp must be a positive finite number, a sequence of them or None, got {budget_bpp!r}")
            budget_bpp = [v for v in budget_bpp]
            if not budget_bpp or not all(_positive(v) for v in budget_bpp):
                raise ValueError(f"RefineConfig: budget_bpp must hold positive finite numbers, one per pair, got {budget_bpp!r}")
            budget_bpp = [float(v) for v in budget_bpp]
        elif budget_bpp is not None:
            if not _positive(budget_bpp):
                raise ValueError(f"RefineConfig: budget_bpp must be a positive finite number, a sequence of them or None, got {budget_bpp!r}")
            budget_bpp = float(budget_bpp)
        if budget_rel is not None and not _positive(budget_rel):
            raise ValueError(f"RefineConfig: budget_rel must be a positive finite number or None, got {budget_rel!r}")
        if not _positive(budget_gain):
            raise ValueError(f"RefineConfig: budget_gain must be a positive finite number, got {budget_gain!r}")
        self.budget_bpp, self.budget_rel = budget_bpp, None if budget_rel is None else float(budget_rel)
        self.budget_gain = float(budget_gain)
        self.steps, self.lr, self.check_every, self.seed = steps, float(lr), check_every, seed
        self.pair_keys, self.lmbda = pair_keys, None if lmbda is None else float(lmbda)

    def keys_for(self, B):
        """The B pair keys of a call as a list."""
        if self.pair_keys is None:
            return list(range(B))
        if len(self.pair_keys) != B:
            raise ValueError(f"RefineConfig: {len(self.pair_keys)} pair keys for {B} pairs")
        return list(self.pair_keys)

    @property
    def has_budget(self):
        return self.budget_bpp is not None or self.budget_rel is not None

    def budget_bpp_for(self, B, who="RefineConfig"):
        """budget_bpp as a list of B values (None without one); ValueError for a sequence of another length."""
        if self.budget_bpp is None or not isinstance(self.budget_bpp, list):
            return None if self.budget_bpp is None else [self.budget_bpp] * B
        if len(self.budget_bpp) != B:
            raise ValueError(f"{who}: RefineConfig.budget_bpp holds {len(self.budget_bpp)} values for {B} pairs")
        return list(self.budget_bpp)

    def __repr__(self):
        return (f"RefineConfig(steps={self.steps}, lr={self.lr}, check_every={self.check_every}, seed={self.seed}, "
                f"pair_keys={self.pair_keys}, lmbda={self.lmbda}, budget_bpp={self.budget_bpp}, budget_rel={self.budget_rel}, "
                f"budget_gain={self.budget_gain})")


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _four(ts, name, like=None):
    """Four contiguous float32 device tensors [B, ...] -> (host pointer array, host array of elements per pair, B)."""
    ts = list(ts)
    if len(ts) != 4:
        raise RuntimeError(f"masic_amd.refine: {name} must be four tensors, got {len(ts)}")
    for k, t in enumerate(ts):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"masic_amd.refine: {name}[{k}] must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.numel() == 0:
            raise RuntimeError(f"masic_amd.refine: {name}[{k}] must be a non-empty contiguous float32 tensor [B, ...]")
    B = int(ts[0].shape[0])
    if not 1 <= B <= MAX_PAIRS or any(t.shape[0] != B for t in ts):
        raise RuntimeError(f"masic_amd.refine: {name}: one B in 1 .. {MAX_PAIRS} for the four tensors")
    if like is not None and [tuple(t.shape) for t in ts] != [tuple(t.shape) for t in like]:
        raise RuntimeError(f"masic_amd.refine: {name} must have the shapes of the first four tensors")
    ptr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])
    cnt = (ctypes.c_size_t * 4)(*[t.numel() // B for t in ts])
    return ptr, cnt, B


def _scalar(t, name, dtype, n=1):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f"masic_amd.refine: {name} must be a contiguous {dtype} device tensor of {n} element(s)")
    return t


def pair_keys_tensor(keys, device):
    """B integers 0 .. 2^32 - 1 -> the int32 device tensor that carries their 32 bits."""
    return torch.tensor([k - 2 ** 32 if k >= 2 ** 31 else k for k in keys], dtype=torch.int32, device=device)


def noise(outs, seed, pair_keys, step):
    """Fills the four tensors `outs` ([B, ...] each) with the noise of one step (masic_refine_noise): U[-1/2, 1/2) on a 2^-24 grid from
    Philox4x32-10, key (seed, pair_keys[b]), counter (element index within pair b's slice, tensor 0..3, step, 0).  pair_keys: int32 [B]
    device tensor (pair_keys_tensor); step: int32 device scalar.  One launch."""
    from . import ops
    ptr, cnt, B = _four(outs, "outs")
    _scalar(pair_keys, "pair_keys", torch.int32, B); _scalar(step, "step", torch.int32)
    _lib.check(_lib.lib.masic_refine_noise(ptr, cnt, B, int(seed) & 0xffffffff, ops._p(pair_keys), ops._p(step), ops._stream()), "refine_noise")
    return outs


def adam(params, grads, ms, vs, lr, step):
    """One bias-corrected Adam step on the four tensors in place (masic_refine_adam): betas 0.9 / 0.999, eps 1e-8, no decay, float32
    states ms / vs; step: int32 device scalar holding t >= 1.  One launch."""
    from . import ops
    p, cnt, B = _four(params, "params")
    g, _, _ = _four(grads, "grads", params)
    m, _, _ = _four(ms, "ms", params)
    v, _, _ = _four(vs, "vs", params)
    _scalar(step, "step", torch.int32)
    _lib.check(_lib.lib.masic_refine_adam(p, g, m, v, cnt, B, float(lr), ops._p(step), ops._stream()), "refine_adam")


def keep_best(cur, best, j_now, j_best):
    """For every pair b with j_now[b] < j_best[b]: pair b's slices of the four `cur` tensors are copied into `best` and j_best[b] =
    j_now[b] (masic_refine_keep_best).  j_now, j_best: float64 [B] on the device; the decision is the device's."""
    from . import ops
    c, cnt, B = _four(cur, "cur")
    b, _, _ = _four(best, "best", cur)
    _scalar(j_now, "j_now", torch.float64, B); _scalar(j_best, "j_best", torch.float64, B)
    _lib.check(_lib.lib.masic_refine_keep_best(c, b, cnt, B, ops._p(j_now), ops._p(j_best), ops._stream()), "refine_keep_best")


def _seed_args(who, x1_hat, x1, x2_hat, x2, liks, g, mu=None):
    """The checks and the host arrays rd_seeds and budget_seeds share -> (liks, B, g1, g2, gl, arr, out, cnt)."""
    liks = list(liks)
    if len(liks) > 4:
        raise RuntimeError(f"masic_amd.refine.{who}: at most 4 likelihood tensors, got {len(liks)}")
    for t in (x1_hat, x1, x2_hat, x2, *liks):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
            raise RuntimeError(f"masic_amd.refine.{who}: non-empty contiguous float32 device tensors only")
    if not (x1_hat.shape == x1.shape == x2_hat.shape == x2.shape) or x1.dim() < 1:
        raise RuntimeError(f"masic_amd.refine.{who}: the four pictures must have one shape [B, ...]")
    B = int(x1.shape[0])
    if not 1 <= B <= MAX_PAIRS or any(l.dim() < 1 or l.shape[0] != B for l in liks):
        raise RuntimeError(f"masic_amd.refine.{who}: one B in 1 .. {MAX_PAIRS} for every tensor")
    if g is not None:
        _scalar(g, "g", torch.float64, B)
    if mu is not None:
        _scalar(mu, "mu", torch.float64, B)
    g1, g2, gl = torch.empty_like(x1_hat), torch.empty_like(x2_hat), [torch.empty_like(l) for l in liks]
    n = max(len(liks), 1)
    arr = (ctypes.c_void_p * n)(*[l.data_ptr() for l in liks])
    out = (ctypes.c_void_p * n)(*[l.data_ptr() for l in gl])
    cnt = (ctypes.c_size_t * n)(*[l.numel() // B for l in liks])
    return liks, B, g1, g2, gl, arr, out, cnt


def rd_seeds(x1_hat, x1, x2_hat, x2, liks, lmbda, hw, g=None):
    """Backward of autograd.PairRateDistortionFn in one launch (masic_refine_rd_seeds) -> (g1, g2, [gl_k]):
    g1 = g[b] 2 lmbda 255^2 (x1_hat - x1) / n_pic, g2 likewise, gl_k = -g[b] / (ln 2 hw lik_k); g: float64 [B] or None for ones."""
    from . import ops
    liks, B, g1, g2, gl, arr, out, cnt = _seed_args("rd_seeds", x1_hat, x1, x2_hat, x2, liks, g)
    _lib.check(_lib.lib.masic_refine_rd_seeds(ops._p(x1_hat), ops._p(x1), ops._p(x2_hat), ops._p(x2), x1.numel() // B, arr, cnt, len(liks), B,
                                              float(lmbda), float(hw), ops._p(g), ops._p(g1), ops._p(g2), out, ops._stream()), "refine_rd_seeds")
    return g1, g2, gl


# ------------------------------------------------------------------------------------------------------------------ the budget's kernels
def budget_seeds(x1_hat, x1, x2_hat, x2, liks, lmbda, hw, g=None, mu=None):
    """Backward of autograd.PairBudgetFn in one launch (masic_budget_rd_seeds) -> (g1, g2, [gl_k]): rd_seeds with gl_k =
    -g[b] mu[b] / (ln 2 hw lik_k); g, mu: float64 [B] or None for ones.  With mu None or ones the results are rd_seeds' bit for bit."""
    from . import ops
    liks, B, g1, g2, gl, arr, out, cnt = _seed_args("budget_seeds", x1_hat, x1, x2_hat, x2, liks, g, mu)
    _lib.check(_lib.lib.masic_budget_rd_seeds(ops._p(x1_hat), ops._p(x1), ops._p(x2_hat), ops._p(x2), x1.numel() // B, arr, cnt, len(liks), B,
                                              float(lmbda), float(hw), ops._p(g), ops._p(mu), ops._p(g1), ops._p(g2), out, ops._stream()),
               "budget_rd_seeds")
    return g1, g2, gl


def budget_select(cur, best, r_now, d_now, target, r_best, d_best):
    """The constrained keep-best (masic_budget_select).  For every pair b whose candidate (r_now[b], d_now[b]) wins against the kept
    (r_best[b], d_best[b]) under the budget target[b] -- neither value NaN, and feasible (r <= target) against infeasible, or both
    feasible and a smaller d, or both infeasible and a smaller r; never on equality -- pair b's slices of the four `cur` tensors are
    copied into `best` and (r_best[b], d_best[b]) = (r_now[b], d_now[b]).  The five: float64 [B] on the device; the decision is the
    device's."""
    from . import ops
    c, cnt, B = _four(cur, "cur")
    b, _, _ = _four(best, "best", cur)
    for t, name in ((r_now, "r_now"), (d_now, "d_now"), (target, "target"), (r_best, "r_best"), (d_best, "d_best")):
        _scalar(t, name, torch.float64, B)
    _lib.check(_lib.lib.masic_budget_select(c, b, cnt, B, ops._p(r_now), ops._p(d_now), ops._p(target), ops._p(r_best), ops._p(d_best),
                                            ops._stream()), "budget_select")


def budget_mu(mu, r_now, target, gain, mu_min=MU_MIN, mu_max=MU_MAX):
    """mu[b] = min(max(mu[b] exp(gain (r_now[b] / target[b] - 1)), mu_min), mu_max) in place, float64 [B] on the device
    (masic_budget_mu); a NaN r_now[b] leaves mu[b].  gain, mu_min <= mu_max: positive finite numbers."""
    from . import ops
    if not isinstance(mu, torch.Tensor) or mu.dim() != 1 or not 1 <= mu.numel() <= MAX_PAIRS:
        raise RuntimeError(f"masic_amd.refine: mu must be a float64 device tensor [B], B in 1 .. {MAX_PAIRS}")
    B = mu.numel()
    _scalar(mu, "mu", torch.float64, B); _scalar(r_now, "r_now", torch.float64, B); _scalar(target, "target", torch.float64, B)
    if not (_positive(gain) and _positive(mu_min) and _positive(mu_max) and float(mu_min) <= float(mu_max)):
        raise RuntimeError(f"masic_amd.refine: budget_mu needs positive finite gain, mu_min <= mu_max, got {gain!r}, {mu_min!r}, {mu_max!r}")
    _lib.check(_lib.lib.masic_budget_mu(ops._p(mu), ops._p(r_now), ops._p(target), B, float(gain), float(mu_min), float(mu_max), ops._stream()),
               "budget_mu")


def bits_and_mse(rows, n_pic):
    """(R, D) float64 [B] from metrics.pair_rd's rows: R_b = -sum of the four log columns / ln 2 (the estimated bits of the pair), D_b =
    (squared error of view 1 + of view 2) / n_pic = MSE1_b + MSE2_b.  A few float64 torch operations on the device."""
    return rows[:, 2:].sum(dim=1) * (-1.0 / math.log(2.0)), (rows[:, 0] + rows[:, 1]) / float(n_pic)


# ------------------------------------------------------------------------------------------------------------------ the loop
class _Frozen:
    """requires_grad off on every parameter of the model for the duration (restored on exit, also after an error)."""

    def __init__(self, module):
        self._params = [p for _, p in module.named_parameters()]

    def __enter__(self):
        self._flags = [p.requires_grad for p in self._params]
        for p in self._params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p, f in zip(self._params, self._flags):
            p.requires_grad_(f)
        return False


def surrogate_grads(hsic, latents, x1, x2, m_fwd, m_back, noise, lmbda, gates=None, mu=None):
    """One gradient of the loop: (d sum_b J_b / d (y1, y2, z1, z2), J [B] float64) of the surrogate HSIC._forward_refine at `latents`
    under the noise tensors `noise`, the weights frozen for the call.  m_fwd / m_back: homography.warp_matrices of the pairs.
    mu (float64 [B] on the device; None: the objective as it is): J_b(mu) = mu_b bits_b / (H W) + lmbda 255^2 (MSE1_b + MSE2_b) of the
    budgeted loop (autograd.PairBudgetFn)."""
    from .autograd import PairBudgetFn, PairRateDistortionFn
    with _Frozen(hsic), torch.enable_grad():
        leaves = [t.detach().requires_grad_(True) for t in latents]
        out = hsic._forward_refine(*leaves, x1, x2, m_fwd, m_back, noise, gates=gates)
        L = out["likelihoods"]
        if mu is None:
            J = PairRateDistortionFn.apply(lmbda, x1, x2, out["x1_hat"], out["x2_hat"], L["y1"], L["y2"], L["z1"], L["z2"])
        else:
            J = PairBudgetFn.apply(lmbda, mu, x1, x2, out["x1_hat"], out["x2_hat"], L["y1"], L["y2"], L["z1"], L["z2"])
        grads = torch.autograd.grad(J.sum(), leaves)
    return [g.contiguous() for g in grads], J.detach()


def _check_call(hsic, x1, x2, h_matrix, lmbda, config, who):
    from . import nn as _mnn
    if not isinstance(config, RefineConfig):
        raise TypeError(f"{who}: config must be a RefineConfig, got {type(config).__name__}")
    if _mnn.get_precision() == "fp8":
        raise NotImplementedError(f"{who}: the latent refinement runs with bf16 or f32 operands; the fp8 mode has no backward")
    if hsic.training:
        raise RuntimeError(f"{who}: call .eval() first (the files are coded in eval mode)")
    if lmbda is None:
        lmbda = config.lmbda
    if lmbda is None or not (0.0 < float(lmbda) < float("inf")):
        raise ValueError(f"{who}: needs a positive lmbda (the argument, or RefineConfig(lmbda=...))")
    for t, name in ((x1, "x1"), (x2, "x2"), (h_matrix, "h_matrix")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
    if x1.dim() != 4 or x1.shape != x2.shape or x1.shape[1] != 3 or h_matrix.shape[0] != x1.shape[0]:
        raise ValueError(f"{who}: x1, x2 [B,3,H,W] of one shape and h_matrix [B,3,3]")
    hsic._codec_check(who, x1.shape[2], x1.shape[3])
    return float(lmbda)


def refine_latents(hsic, x1, x2, h_matrix, lmbda=None, config=None, trace=None):
    """-> Refined (RefinedToBudget when config sets a bit budget: the module's docstring).  hsic: an eval-mode MASIC.HSIC on the device; x1, x2: float32 [B,3,H,W] with H, W multiples of 64 (what compress
    codes); h_matrix [B,3,3]; lmbda: the rate-distortion weight the checkpoint was trained with (or config.lmbda); config: a
    RefineConfig.  Starts from exactly the latents compress computes (each pair on its own, as there).  After the call no parameter's
    .grad or requires_grad, no entry of the state dict, hsic.training and neither of torch's default generators has changed.
    trace (a list, for measurements): receives (step, float64 [B] device tensor) of every evaluation of the true objective -- device
    tensors, so the loop still reads nothing on the host; under a budget (step, R [B], D [B], mu [B]), mu after the check's
    update.  All of the above holds under a budget; steps = 0 then returns the encoder's latents with the bookkeeping filled."""
    who = "masic_amd.refine.refine_latents"
    config = RefineConfig() if config is None else config
    lmbda = _check_call(hsic, x1, x2, h_matrix, lmbda, config, who)
    from . import ops
    from .homography import warp_matrices
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, _, H, W = x1.shape
    dev = x1.device
    keys = pair_keys_tensor(config.keys_for(B), dev)
    config.budget_bpp_for(B, who)          # one budget per pair, before anything runs
    with torch.no_grad():
        mats = [warp_matrices(h_matrix[i:i + 1], (H, W), (H, W), want_inverse=True) for i in range(B)]
        m_fwd, m_back = torch.cat([m[0] for m in mats]).contiguous(), torch.cat([m[1] for m in mats]).contiguous()
        start = [[], [], [], []]
        for i in range(B):          # the latents of HSIC._compress_pairs, pair by pair as there
            a, b_ = x1[i:i + 1], x2[i:i + 1]
            y1 = hsic.encoder1.latent(a)
            y2 = hsic.encoder2.forward_views(ops.warp_perspective(a, mats[i][0], (H, W)), b_)
            for k, t in enumerate((y1, y2, hsic._h_a1(y1), hsic._h_a2(y2))):
                start[k].append(t)
        cur = [torch.cat(ts).contiguous() for ts in start]
        gates = hsic.mask2weights_unit(ops.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))).contiguous()

        if config.has_budget:
            return _refine_to_budget(hsic, x1, x2, m_fwd, m_back, gates, cur, keys, lmbda, config, trace)

        def true_cost():
            out = hsic._eval_from_latents(*cur, m_fwd, gates)
            L = out["likelihoods"]
            return metrics_cost(out["x1_hat"], out["x2_hat"], (L["y1"], L["y2"], L["z1"], L["z2"]))

        def metrics_cost(x1_hat, x2_hat, liks):
            from . import metrics
            return metrics.pair_objective(metrics.pair_rd(x1_hat.contiguous(), x1, x2_hat.contiguous(), x2, [l.contiguous() for l in liks]),
                                          lmbda, H * W, 3 * H * W)

        cost_start = true_cost()
        if trace is not None:
            trace.append((0, cost_start.clone()))
        if config.steps == 0:
            return Refined(*cur, cost_start, cost_start.clone())
        best = [t.clone() for t in cur]
        cost_best = cost_start.clone()
        ms, vs = [torch.zeros_like(t) for t in cur], [torch.zeros_like(t) for t in cur]
        us = [torch.empty_like(t) for t in cur]
        step = torch.zeros(1, dtype=torch.int32, device=dev)
    with _Frozen(hsic):
        for s in range(1, config.steps + 1):
            with torch.no_grad():
                step.add_(1)
                noise(us, config.seed, keys, step)
            grads, _ = surrogate_grads(hsic, cur, x1, x2, m_fwd, m_back, us, lmbda, gates=gates)
            with torch.no_grad():
                adam(cur, grads, ms, vs, config.lr, step)
                if s % config.check_every == 0 or s == config.steps:
                    now = true_cost()
                    if trace is not None:
                        trace.append((s, now))
                    keep_best(cur, best, now, cost_best)
    return Refined(*best, cost_start, cost_best)


def _refine_to_budget(hsic, x1, x2, m_fwd, m_back, gates, cur, keys, lmbda, config, trace):
    """The loop of refine_latents under a bit budget, from the encoder's latents `cur` (called under no_grad) -> RefinedToBudget."""
    from . import metrics
    B, _, H, W = x1.shape
    dev = x1.device

    def true_rd():
        out = hsic._eval_from_latents(*cur, m_fwd, gates)
        L = out["likelihoods"]
        rows = metrics.pair_rd(out["x1_hat"].contiguous(), x1, out["x2_hat"].contiguous(), x2,
                               [L[k].contiguous() for k in ("y1", "y2", "z1", "z2")])
        return bits_and_mse(rows, 3 * H * W)

    def cost(r, d):
        return r / float(H * W) + (lmbda * 255.0 ** 2) * d

    bpp = config.budget_bpp_for(B)
    r_start, d_start = true_rd()
    if bpp is not None:
        target = torch.tensor([v * H * W for v in bpp], dtype=torch.float64, device=dev)
    else:
        target = config.budget_rel * r_start
    mu = torch.ones(B, dtype=torch.float64, device=dev)
    budget_mu(mu, r_start, target, config.budget_gain)          # the start is a check like the others
    if trace is not None:
        trace.append((0, r_start.clone(), d_start.clone(), mu.clone()))
    if config.steps == 0:
        return RefinedToBudget(*cur, cost(r_start, d_start), cost(r_start, d_start), r_start, r_start.clone(), d_start, d_start.clone(),
                               target, mu)
    best = [t.clone() for t in cur]
    r_best, d_best = r_start.clone(), d_start.clone()
    ms, vs = [torch.zeros_like(t) for t in cur], [torch.zeros_like(t) for t in cur]
    us = [torch.empty_like(t) for t in cur]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    with _Frozen(hsic):
        for s in range(1, config.steps + 1):
            step.add_(1)
            noise(us, config.seed, keys, step)
            grads, _ = surrogate_grads(hsic, cur, x1, x2, m_fwd, m_back, us, lmbda, gates=gates, mu=mu)
            adam(cur, grads, ms, vs, config.lr, step)
            if s % config.check_every == 0 or s == config.steps:
                r_now, d_now = true_rd()
                budget_select(cur, best, r_now, d_now, target, r_best, d_best)
                budget_mu(mu, r_now, target, config.budget_gain)
                if trace is not None:
                    trace.append((s, r_now, d_now, mu.clone()))
    return RefinedToBudget(*best, cost(r_start, d_start), cost(r_best, d_best), r_start, r_best, d_start, d_best, target, mu)
