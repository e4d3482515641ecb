"""Float64 restatement of the weight-free patch aligner and the synthetic pairs its tests run on.

The model is b(u) ~ a(W(u; delta)) with W the homography that takes the square s = (0,0), (P,0), (P,P), (0,P) to s + delta, sampled
bilinearly in pixel-index coordinates; a sample is valid iff 0 <= X <= n-1 and 0 <= Y <= n-1 and invalid pixels are masked out of
every sum.  Stage 1 is an integer translation search on the 32 x 32 level of a 2 x 2 box-mean pyramid, stage 2 a fixed number of
forward-additive Gauss-Newton steps per level on the eight free entries of the level's matrix.  Everything here is batched torch on
the CPU; `align` works in the dtype it is given (float64 by default) and mirrors masic_amd/csrc/align.hip step for step, but shares
no code with it.
"""
import numpy as np
import torch

LEVEL_SIZE = 32            # the pyramid stops here
ITERS = (30, 15, 10)       # coarse to fine; the last `levels` entries are used


# ---------------------------------------------------------------------------------------------------------------- geometry
def square(P, dtype=torch.float64):
    return torch.tensor([[0.0, 0.0], [P, 0.0], [P, P], [0.0, P]], dtype=dtype)


def h_from_delta(delta, P):
    """H [B,3,3], h33 = 1, with H(s_k) = s_k + delta_k: the closed form of the square-to-quadrilateral map (the solution of
    get_perspective_transform's 8 x 8 system).  A degenerate quadrilateral gives non-finite entries."""
    q = square(P, delta.dtype) + delta
    x0, y0, x1, y1, x2, y2, x3, y3 = (q[:, k // 2, k % 2] for k in range(8))
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    det = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / det
    h = (dx1 * sy - sx * dy1) / det
    rows = [(x1 - x0 + g * x1) / P, (x3 - x0 + h * x3) / P, x0, (y1 - y0 + g * y1) / P, (y3 - y0 + h * y3) / P, y0, g / P, h / P,
            torch.ones_like(g)]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def apply_h(H, pts):
    """H [B,3,3] applied to pts [K,2] -> [B,K,2]"""
    x, y = pts[:, 0], pts[:, 1]
    D = H[:, 2, 0, None] * x + H[:, 2, 1, None] * y + H[:, 2, 2, None]
    X = (H[:, 0, 0, None] * x + H[:, 0, 1, None] * y + H[:, 0, 2, None]) / D
    Y = (H[:, 1, 0, None] * x + H[:, 1, 1, None] * y + H[:, 1, 2, None]) / D
    return torch.stack((X, Y), -1)


def _T(level, dtype):
    s = float(2 ** level)
    t = (s - 1.0) / 2.0
    return torch.tensor([[s, 0.0, t], [0.0, s, t], [0.0, 0.0, 1.0]], dtype=dtype)


def to_level(H, level):
    """H_l = T_l^-1 H T_l, renormalised to h33 = 1 (coarse pixel i sits at fine coordinate 2^l i + (2^l - 1) / 2)"""
    T = _T(level, H.dtype)
    M = torch.linalg.inv(T) @ H @ T
    return M / M[:, 2:3, 2:3]


def from_level(Hl, level):
    T = _T(level, Hl.dtype)
    M = T @ Hl @ torch.linalg.inv(T)
    return M / M[:, 2:3, 2:3]


def pyramid(img):
    """[fine, ..., 32 x 32] of img [B,P,P] by 2 x 2 box means"""
    out = [img]
    while out[-1].shape[-1] > LEVEL_SIZE:
        f = out[-1]
        out.append(((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + (f[:, 1::2, 0::2] + f[:, 1::2, 1::2])) * 0.25)
    return out


# ---------------------------------------------------------------------------------------------------------------- sampling
def sample(a, X, Y):
    """bilinear sample of a [B,n,n] at X, Y [B,N] with its own gradient: (value, d/dX, d/dY, valid)"""
    B, n, _ = a.shape
    valid = (X >= 0) & (X <= n - 1) & (Y >= 0) & (Y <= n - 1)           # NaN compares false
    Xc, Yc = torch.where(valid, X, torch.zeros_like(X)), torch.where(valid, Y, torch.zeros_like(Y))
    x0, y0 = Xc.floor().clamp(0, n - 2), Yc.floor().clamp(0, n - 2)
    fx, fy = Xc - x0, Yc - y0
    idx = (y0 * n + x0).long()
    flat = a.reshape(B, n * n)
    a00, a10, a01, a11 = (flat.gather(1, idx + o) for o in (0, 1, n, n + 1))
    val = (1 - fy) * ((1 - fx) * a00 + fx * a10) + fy * ((1 - fx) * a01 + fx * a11)
    gx = (1 - fy) * (a10 - a00) + fy * (a11 - a01)
    gy = (1 - fx) * (a01 - a00) + fx * (a11 - a10)
    return val, gx, gy, valid


def _grid(n, dtype):
    y, x = torch.meshgrid(torch.arange(n, dtype=dtype), torch.arange(n, dtype=dtype), indexing="ij")
    return x.reshape(-1), y.reshape(-1)


def _warp_terms(a, b, H):
    n = a.shape[-1]
    x, y = _grid(n, a.dtype)
    h = H.reshape(-1, 9)
    D = h[:, 6:7] * x + h[:, 7:8] * y + 1.0
    X = (h[:, 0:1] * x + h[:, 1:2] * y + h[:, 2:3]) / D
    Y = (h[:, 3:4] * x + h[:, 4:5] * y + h[:, 5:6]) / D
    val, gx, gy, valid = sample(a, X, Y)
    m = valid.to(a.dtype)
    r = torch.where(valid, val - b.reshape(b.shape[0], -1), torch.zeros_like(val))
    return x, y, D, X, Y, gx, gy, m, r, valid


def masked_mse(a, b, H):
    """(masked MSE [B] (inf without a valid pixel), valid fraction [B]) of a(W(u)) - b(u)"""
    *_, m, r, _ = _warp_terms(a, b, H)
    cnt = m.sum(1)
    mse = torch.where(cnt > 0, (r * r).sum(1) / cnt.clamp(min=1), torch.full_like(cnt, float("inf")))
    return mse, cnt / m.shape[1]


def gauss_newton_step(a, b, H, damping):
    """One forward-additive step on the 8 free entries of H [B,3,3] (h33 = 1): (H_new, ok [B], valid fraction [B])"""
    x, y, D, X, Y, gx, gy, m, r, valid = _warp_terms(a, b, H)
    z = torch.zeros_like(gx)
    gx, gy = torch.where(valid, gx / D, z), torch.where(valid, gy / D, z)
    q = -(gx * torch.where(valid, X, z) + gy * torch.where(valid, Y, z))
    J = torch.stack((gx * x, gx * y, gx, gy * x, gy * y, gy, q * x, q * y), -1)            # [B,N,8]
    A = J.transpose(1, 2) @ J
    g = (J * r[..., None]).sum(1)
    A = A + damping * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
    frac = m.sum(1) / m.shape[1]
    finite = torch.isfinite(A).all(-1).all(-1) & torch.isfinite(g).all(-1)
    A = torch.where(finite[:, None, None], A, torch.eye(8, dtype=A.dtype).expand_as(A))
    L, bad = torch.linalg.cholesky_ex(A)                                                     # bad > 0: a non-positive pivot
    ok = finite & (bad == 0) & (frac >= 0.25)
    L = torch.where(ok[:, None, None], L, torch.eye(8, dtype=A.dtype).expand_as(L))
    dp = torch.cholesky_solve(torch.where(ok[:, None], g, torch.zeros_like(g))[..., None], L)[..., 0]
    h = H.reshape(-1, 9).clone()
    h[:, :8] -= dp
    return h.reshape(-1, 3, 3), ok, frac


# ---------------------------------------------------------------------------------------------------------------- stage 1
def search_costs(a, b, R):
    """Masked mean squared difference of a(u + d) and b(u) for every integer d in [-R, R]^2 on a level [B,n,n]: costs [B,(2R+1)^2]
    in scan order (dy outer, dx inner, ascending); +inf where the overlap is below a quarter of the level"""
    B, n, _ = a.shape
    out = torch.full((B, (2 * R + 1) ** 2), float("inf"), dtype=a.dtype)
    k = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ylo, yhi, xlo, xhi = max(0, -dy), min(n, n - dy), max(0, -dx), min(n, n - dx)
            cnt = max(0, yhi - ylo) * max(0, xhi - xlo)
            if cnt > 0 and 4 * cnt >= n * n:
                d = a[:, ylo + dy:yhi + dy, xlo + dx:xhi + dx] - b[:, ylo:yhi, xlo:xhi]
                out[:, k] = (d * d).sum((1, 2)) / cnt
            k += 1
    return out


def pick_shift(costs, R):
    """(dx, dy) [B] of the least cost; ties: smaller |dx| + |dy|, then scan order.  A NaN cost never wins; with none finite: (0, 0)"""
    B = costs.shape[0]
    best_c = torch.full((B,), float("inf"), dtype=costs.dtype)
    best = torch.zeros((B, 2), dtype=torch.long)
    k = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            c = costs[:, k]
            l1 = abs(dx) + abs(dy)
            take = (c < best_c) | ((c == best_c) & (l1 < best.abs().sum(1)))
            best_c = torch.where(take, c, best_c)
            best = torch.where(take[:, None], torch.tensor([dx, dy]), best)
            k += 1
    return best[:, 0], best[:, 1]


def search_margin(costs):
    """(second best - best) / second best of each item's search costs: the generator rejects cases below 1 %"""
    c = torch.where(torch.isfinite(costs), costs, torch.full_like(costs, float("inf"))).sort(1).values
    return (c[:, 1] - c[:, 0]) / c[:, 1]


# ---------------------------------------------------------------------------------------------------------------- the estimator
def align(a, b, delta0=None, search_radius=12, iters=ITERS, damping=1e-6, dtype=torch.float64):
    """a, b [B,1,P,P] (or [B,P,P]) -> (delta [B,4,2], info [B,4], costs [B,(2R+1)^2] or None), all in `dtype`.
    info = (masked MSE at the start value, masked MSE and valid fraction at the returned delta, status)."""
    a = a.reshape(-1, a.shape[-2], a.shape[-1]).to(dtype)
    b = b.reshape(-1, b.shape[-2], b.shape[-1]).to(dtype)
    B, P = a.shape[0], a.shape[-1]
    pa, pb = pyramid(a), pyramid(b)
    levels = len(pa)
    its = tuple(iters)[-levels:]
    start = torch.zeros((B, 4, 2), dtype=dtype) if delta0 is None else delta0.to(dtype).reshape(B, 4, 2)
    fail = ~(torch.isfinite(a).all(-1).all(-1) & torch.isfinite(b).all(-1).all(-1) & torch.isfinite(start).all(-1).all(-1))
    costs = None
    if delta0 is None:
        costs = search_costs(pa[-1], pb[-1], search_radius)
        dx, dy = pick_shift(costs, search_radius)
        H = torch.eye(3, dtype=dtype).repeat(B, 1, 1)
        H[:, 0, 2] = dx.to(dtype) * 2 ** (levels - 1)
        H[:, 1, 2] = dy.to(dtype) * 2 ** (levels - 1)
    else:
        H = h_from_delta(start, P)
    fail |= ~torch.isfinite(H).all(-1).all(-1)
    H = torch.where(fail[:, None, None], torch.eye(3, dtype=dtype).expand_as(H), H)
    sq = square(P, dtype)
    for level, n_it in zip(range(levels - 1, -1, -1), its):
        Hl = to_level(H, level)
        for _ in range(n_it):
            new, ok, _ = gauss_newton_step(pa[level], pb[level], Hl, damping)
            c = apply_h(from_level(new, level), sq)
            inside = ((c >= -P / 2) & (c <= 1.5 * P)).all(-1).all(-1)            # NaN compares false
            fail |= ~(ok & inside)
            Hl = torch.where(fail[:, None, None], Hl, new)
        H = from_level(Hl, level)
    Hs = torch.where(fail[:, None, None], torch.eye(3, dtype=dtype).expand_as(H), h_from_delta(start, P))
    mse0, frac0 = masked_mse(a, b, Hs)
    mse1, frac = masked_mse(a, b, H)
    fail |= frac < 0.25
    delta = apply_h(H, sq) - sq
    fail |= ~torch.isfinite(delta).all(-1).all(-1)
    status = torch.where(fail, 1, torch.where(mse1 > mse0, 2, 0)).to(dtype)
    delta = torch.where((status != 0)[:, None, None], start, delta)
    nan = torch.full_like(mse0, float("nan"))
    back = status == 2                                   # the start value is returned: its figures are the result's
    mse1, frac = torch.where(back, mse0, mse1), torch.where(back, frac0, frac)
    info = torch.stack((torch.where(fail, nan, mse0), torch.where(fail, nan, mse1), torch.where(fail, torch.zeros_like(frac), frac),
                        status), 1)
    return delta, info, costs


# ---------------------------------------------------------------------------------------------------------------- synthetic pairs
TEX, ORG = 384, 128


def texture(sigma, seed):
    """384 x 384 white Gaussian noise under a separable Gaussian of `sigma` px (wrapped at the border), scaled to unit variance"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((TEX, TEX))
    k = np.arange(TEX, dtype=np.float64)
    k = np.minimum(k, TEX - k)
    g = np.fft.fft(np.exp(-0.5 * (k / sigma) ** 2))
    t = np.real(np.fft.ifft(np.fft.ifft(np.fft.fft(np.fft.fft(w, axis=0) * g[:, None], axis=1) * g[None, :], axis=1), axis=0))
    return torch.from_numpy(t / t.std())


def render(tex, delta_true, P, noise, rng):
    """b(u) = bilinear sample of tex at ORG + W_true(u), plus N(0, noise^2)"""
    H = h_from_delta(delta_true.reshape(1, 4, 2).double(), P)
    x, y = _grid(P, torch.float64)
    w = apply_h(H, torch.stack((x, y), 1))[0] + ORG
    val, _, _, valid = sample(tex[None], w[None, :, 0], w[None, :, 1])
    assert bool(valid.all()), "the synthetic warp left the texture"
    return val.reshape(P, P) + noise * torch.from_numpy(rng.standard_normal((P, P)))


def make_case(P, sigma, tmax, jitter, seed, noise=0.02):
    """(a [P,P], b [P,P], delta_true [4,2]) float64: delta_true = t + jitter, t uniform in +-tmax on both axes, jitter uniform in
    +-jitter per coordinate"""
    rng = np.random.default_rng([seed, P, int(sigma * 10), int(tmax), int(jitter)])
    tex = texture(sigma, int(rng.integers(1 << 31)))
    t = rng.uniform(-tmax, tmax, size=2) if tmax else np.zeros(2)
    d = torch.from_numpy(t[None, :] + rng.uniform(-jitter, jitter, size=(4, 2)) if jitter else np.repeat(t[None, :], 4, 0))
    a = tex[ORG:ORG + P, ORG:ORG + P].clone()
    return a, render(tex, d, P, noise, rng), d


def make_set(P, sigmas, tmax, jitter, seeds, noise=0.02):
    """stacked cases: a, b [B,1,P,P] float32, delta_true [B,4,2] float64, sigma-major then seed"""
    cases = [make_case(P, s, tmax, jitter, seed, noise) for s in sigmas for seed in seeds]
    a = torch.stack([c[0] for c in cases])[:, None].float()
    b = torch.stack([c[1] for c in cases])[:, None].float()
    return a, b, torch.stack([c[2] for c in cases])


def corner_error(delta, delta_true):
    """mean over the four corners of the Euclidean error, per item"""
    return (delta.double() - delta_true.double()).norm(dim=-1).mean(-1)
