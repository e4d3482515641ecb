"""TEST INFRASTRUCTURE for the encoder-side latent refinement (masic_amd/refine.py): independent restatements on the CPU.

    philox_noise      numpy Philox4x32-10 with the keying of masic_refine_noise
    adam_step         float64 Adam (betas 0.9 / 0.999, eps 1e-8, bias-corrected, no decay)
    forward_from_latents / pair_costs   the graph of HSIC._forward_refine composed from oracle.hsic_oracle functions with torch
                      autograd ("mixed" quantisation: rounded values with an identity gradient wherever the decoder sees a rounded
                      value, noise where a likelihood is evaluated), and the per-pair objective
                      J_b = bits_b / (H W) + lmbda 255^2 (MSE1_b + MSE2_b)
    oracle_loop       the refinement loop on those: Adam on the latents, the true (eval-mode, no noise) objective every few steps,
                      best iterate kept
    tiny_case         the fixture of the gradient and loop tests: hsic_tiny weights, B pairs, given latents

oracle/ itself is not edited; this file only composes its functions.
"""
import math

import numpy as np
import torch

from oracle import hsic_oracle as O
from tests.util import load_npz

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011) on uint64 arrays holding 32-bit words -> the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return c0, c1, c2, c3


def philox_noise(n, tensor_id, step, seed, pair_key):
    """float32 [n]: the noise of one pair's slice of tensor `tensor_id` (0..3 = y1, y2, z1, z2) at `step`:
    key (seed, pair_key), counter (element index, tensor id, step, 0), value (word 0 >> 8) * 2^-24 - 1/2."""
    i = np.arange(n, dtype=np.uint64)
    w = philox4x32_10(i & _MASK, tensor_id, step, i >> np.uint64(32), seed, pair_key)[0]
    return ((w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)).astype(np.float32)


def step_noise(shapes, step, seed, pair_keys):
    """The four noise tensors of a step for B pairs: shapes = the four [B, ...] shapes -> list of float32 numpy arrays."""
    out = []
    for t, shp in enumerate(shapes):
        n = int(np.prod(shp[1:]))
        out.append(np.stack([philox_noise(n, t, step, seed, k) for k in pair_keys]).reshape(shp))
    return out


def adam_step(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    """float64 numpy arrays -> (p, m, v) after Adam step t >= 1."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)
    return p, m, v


def ste_round(x):
    """round forward, identity backward"""
    return x + (torch.round(x) - x).detach()


def _eb_noise_layout(u):
    C = u.shape[1]
    return u.permute(1, 2, 3, 0).contiguous().reshape(C, 1, -1)          # oracle.entropy_bottleneck's (C, 1, h w B) order


def forward_from_latents(sd, y1, y2, z1, z2, x1, h_matrix, noise, K):
    """The refinement graph from the four latents.  noise: (u_y1, u_y2, u_z1, u_z2) in the tensors' own [B, C, h, w] layout, or None --
    then the eval-mode path (likelihoods at the rounded values: the true objective).  -> dict with x1_hat, x2_hat, likelihoods and
    y1_warp (the unrounded warped latent, for the tie check)."""
    H, W = x1.shape[-2:]

    def bottleneck(z, p, u):
        med = sd[p + ".quantiles"][:, 0, 1].view(1, -1, 1, 1)
        z_r = ste_round(z - med) + med
        if u is None:
            lik = O.entropy_bottleneck(z, sd, p, training=False)[1]
        else:
            lik = O.entropy_bottleneck(z, sd, p, training=True, noise=_eb_noise_layout(u))[1]
        return z_r, lik

    u = noise if noise is not None else (None,) * 4
    at = lambda y, n: torch.round(y) if n is None else y + n
    y1_r, y2_r = ste_round(y1), ste_round(y2)
    z1_r, z1_lik = bottleneck(z1, "entropy_bottleneck1", u[2])
    params1 = O.hyper_synthesis_up(z1_r, sd, "h_s1_up")
    ctx1 = torch.nn.functional.conv2d(y1_r, O.masked_weight(sd["context_prediction1.weight"]), sd["context_prediction1.bias"], padding=2)
    s1, m1, w1 = O.gmm_params_y1(torch.cat((params1, ctx1), dim=1), sd, K)
    y1_lik = O.gmm_likelihood(at(y1, u[0]), s1, m1, w1, K)
    x1_hat = O.decoder1(y1_r, sd)

    z2_r, z2_lik = bottleneck(z2, "entropy_bottleneck2", u[3])
    params2 = O.hyper_synthesis_up(z2_r, sd, "h_s2_up")
    ctx2 = torch.nn.functional.conv2d(y2_r, O.masked_weight(sd["context_prediction2.weight"]), sd["context_prediction2.bias"], padding=2)
    with torch.no_grad():
        gates = O.mask2weights(O.mask(x1, h_matrix)[0], sd)
    x1_hat_warp = O.warp_perspective(x1_hat, h_matrix, (H, W))
    y1_warp = O.encoder1(x1_hat_warp, sd)
    cat2 = torch.cat((params2 * gates[:, 0:1], ctx2 * gates[:, 1:2], ste_round(y1_warp) * gates[:, 2:3]), dim=1)
    s2, m2, w2 = O.gmm_params_y2(cat2, sd, K)
    y2_lik = O.gmm_likelihood(at(y2, u[1]), s2, m2, w2, K)
    x2_hat = O.decoder2(y2_r, x1_hat_warp, sd)
    return {"x1_hat": x1_hat, "x2_hat": x2_hat, "y1_warp": y1_warp,
            "likelihoods": {"y1": y1_lik, "y2": y2_lik, "z1": z1_lik, "z2": z2_lik}}


def pair_costs(out, x1, x2, lmbda):
    """J_b [B] of a forward_from_latents result."""
    B, _, H, W = x1.shape
    bits = sum(-torch.log2(l).reshape(B, -1).sum(dim=1) for l in out["likelihoods"].values())
    mse = ((out["x1_hat"] - x1) ** 2).reshape(B, -1).mean(dim=1) + ((out["x2_hat"] - x2) ** 2).reshape(B, -1).mean(dim=1)
    return bits / (H * W) + lmbda * 255.0 ** 2 * mse


def latent_grads(sd, lat, x1, x2, h_matrix, noise, K, lmbda):
    """d sum_b J_b / d (y1, y2, z1, z2) and J [B] on the surrogate; tensors of sd's dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in lat]
    out = forward_from_latents(sd, *leaves, x1, h_matrix, noise, K)
    J = pair_costs(out, x1, x2, lmbda)
    return list(torch.autograd.grad(J.sum(), leaves)), J.detach(), out


def true_costs(sd, lat, x1, x2, h_matrix, K, lmbda):
    with torch.no_grad():
        return pair_costs(forward_from_latents(sd, *lat, x1, h_matrix, None, K), x1, x2, lmbda)


def oracle_loop(sd, lat, x1, x2, h_matrix, K, lmbda, steps, lr, check_every=5, seed=0, pair_keys=None):
    """-> (cost_start [B], cost_best [B], list of the checked costs) as float64 numpy; the loop of masic_amd.refine.refine_latents."""
    B = x1.shape[0]
    pair_keys = list(range(B)) if pair_keys is None else list(pair_keys)
    dt = x1.dtype
    cur = [t.detach().clone() for t in lat]
    ms, vs = [np.zeros(t.shape) for t in cur], [np.zeros(t.shape) for t in cur]
    start = true_costs(sd, cur, x1, x2, h_matrix, K, lmbda).double().numpy()
    best, trace = start.copy(), [start.copy()]
    for s in range(1, steps + 1):
        noise = [torch.from_numpy(u).to(dt) for u in step_noise([tuple(t.shape) for t in cur], s, seed, pair_keys)]
        grads, _, _ = latent_grads(sd, cur, x1, x2, h_matrix, noise, K, lmbda)
        for k in range(4):
            p, ms[k], vs[k] = adam_step(cur[k].double().numpy(), grads[k].double().numpy(), ms[k], vs[k], lr, s)
            cur[k] = torch.from_numpy(p).to(dt)
        if s % check_every == 0 or s == steps:
            now = true_costs(sd, cur, x1, x2, h_matrix, K, lmbda).double().numpy()
            trace.append(now.copy())
            best = np.where(now < best, now, best)
    return start, best, trace


# ------------------------------------------------------------------------------------------------------------------ the fixture
LATENT_SEED = 118                # chosen so that tests/test_cpu_refine.py::test_fixture_is_admissible holds (it checks this value)
NOISE_SEED, NOISE_STEP = 11, 1


def tiny_case(B=2, dtype=torch.float32, latent_seed=LATENT_SEED):
    """hsic_tiny weights (HSIC(16,24,3), lmbda 0.01), B pairs at 64 x 64 -- pair 0 the fixture's pictures, pair b > 0 the same two
    pictures with the views swapped and flipped b - 1 times more, one h_matrix -- and GIVEN latents drawn from `latent_seed`:
    y ~ 2 N(0,1), z ~ median + 1.5 N(0,1).  -> dict(sd, x1, x2, h_matrix, lat, N, M, K, lmbda) of CPU tensors of `dtype`."""
    import sys, os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (here, os.path.join(here, "coremasic", "mywork")):
        if p not in sys.path:
            sys.path.insert(0, p)
    fx = load_npz("hsic_tiny.npz")
    N, M, K = (int(v) for v in fx["NMK"])
    sd32 = {k[3:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("sd/")}
    a, b = torch.from_numpy(fx["x1"]), torch.from_numpy(fx["x2"])
    x1s, x2s = [a], [b]
    for i in range(1, B):
        x1s.append(torch.flip(b, dims=[3]) if i % 2 else torch.flip(a, dims=[2]))
        x2s.append(torch.flip(a, dims=[3]) if i % 2 else torch.flip(b, dims=[2]))
    x1, x2 = torch.cat(x1s), torch.cat(x2s)
    rng = np.random.RandomState(latent_seed)
    med = [sd32[f"entropy_bottleneck{v}.quantiles"][:, 0, 1].view(1, -1, 1, 1).numpy() for v in (1, 2)]
    y = [torch.from_numpy((2.0 * rng.standard_normal((B, M, 4, 4))).astype(np.float32)) for _ in range(2)]
    z = [torch.from_numpy((med[v] + 1.5 * rng.standard_normal((B, N, 1, 1))).astype(np.float32)) for v in range(2)]
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd32.items()}
    return dict(sd=sd, sd32=sd32, x1=x1.to(dtype), x2=x2.to(dtype), h_matrix=torch.from_numpy(fx["h_matrix"]).repeat(B, 1, 1).to(dtype),
                lat=[t.to(dtype) for t in (y[0], y[1], z[0], z[1])], N=N, M=M, K=K, lmbda=float(fx["lmbda"]))


def tie_distance(t):
    """min over elements of | frac(t) - 1/2 |: the distance of the nearest element from a rounding tie"""
    t = t.detach().double()
    return float(((t - torch.floor(t)) - 0.5).abs().min())
