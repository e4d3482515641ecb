"""TEST INFRASTRUCTURE: plain-torch restatement of the UDH training step (the reference's udh/udh/model.py: Net with explicit
Dropout masks, and photometric_loss).  Imports nothing of masic_amd; works in float32 or float64 (the dtype of its inputs), on any
device torch runs on.

PARITY UNPINNED for the two kornia functions, exactly as oracle/udh_oracle.py and oracle/hsic_oracle.py declare: kornia 0.5.0 is
a pip dependency of the reference that is absent from its tree and from this environment.
  * get_perspective_transform: the 8 x 8 direct-linear-transform system of oracle/udh_oracle.py ([x y 1 0 0 0 -xu -yu] h = u,
    [0 0 0 x y 1 -xv -yv] h = v, h33 = 1), solved with torch.linalg.solve.
  * warp_perspective(src, M, dsize): normalize_homography -> inverse -> create_meshgrid(normalized) -> transform_points ->
    convert_points_from_homogeneous(eps = 1e-8) -> F.grid_sample(bilinear, zeros, align_corners=True), the operation order of
    oracle/hsic_oracle.py: warp_perspective.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

WIDTHS = (2, 64, 64, 128, 128)


class Net(nn.Module):
    """The reference's Net (same 20 state-dict tensors); forward(a, b, masks) with masks = (m1, m2) keep-bits or None (= eval)."""

    def __init__(self, patch_size=128):
        super().__init__()
        blocks = []
        for i in range(4):
            layers = [nn.Conv2d(WIDTHS[i], WIDTHS[i + 1], 3, padding=1), nn.ReLU(), nn.Conv2d(WIDTHS[i + 1], WIDTHS[i + 1], 3, padding=1), nn.ReLU()]
            if i < 3:
                layers.append(nn.MaxPool2d(2, 2))
            blk = nn.Module()
            blk.layers = nn.Sequential(*layers)
            blocks.append(blk)
        self.cnn = nn.Sequential(*blocks)
        side = patch_size // 8
        self.fc = nn.Sequential(nn.Identity(), nn.Identity(), nn.Linear(128 * side * side, 1024), nn.Identity(), nn.Identity(), nn.Linear(1024, 8))

    def forward(self, a, b, masks=None):
        x = torch.cat((a, b), dim=1)
        for blk in self.cnn:
            x = blk.layers(x)
        x = x.flatten(1)
        if masks is not None:
            x = x * (2.0 * masks[0].to(x.dtype))
        x = F.relu(self.fc[2](x))
        if masks is not None:
            x = x * (2.0 * masks[1].to(x.dtype))
        return self.fc[5](x).view(-1, 4, 2)


KINK_MARGIN = 4.0 * 2.0 ** -24


def kink_margin(net, a, b, masks=None):
    """How far the net's evaluation at (a, b) stays from its own kinks, in float64: the smallest |z| / A over every ReLU argument z
    (the eight convolutions and Linear 1), A = sum of the magnitudes of the terms of z (|w| . |x| + |b|), and the smallest
    (largest - second largest) / A over every max-pool window with a positive maximum.  A float32 evaluation of z differs from the
    exact value by about u A at most (u = 2^-24; rounding errors of a dot product add up like a random walk over terms whose
    magnitudes sum to A), so above KINK_MARGIN = 4 u every correct float32 evaluation takes the same ReLU branches and pool
    elements as float64; below it two of them may differ, and one differing branch moves a bias gradient by a whole summand --
    1e-2 of the peak was seen -- so parity of the gradients is undefined there, as at the loss's own kinks."""
    r = float("inf")
    with torch.no_grad():
        x = torch.cat((a, b), dim=1).double()
        for blk in net.cnn:
            for conv in (blk.layers[0], blk.layers[2]):
                w, bias = conv.weight.double(), conv.bias.double()
                z = F.conv2d(x, w, bias, padding=1)
                A = F.conv2d(x.abs(), w.abs(), bias.abs(), padding=1)
                r = min(r, float((z.abs() / A).min()))
                x = F.relu(z)
            if len(blk.layers) > 4:
                B, C, H, W = x.shape
                win = lambda t: t.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)  # noqa: E731
                top = win(x).sort(dim=-1, descending=True).values
                live = top[..., 0] > 0
                if bool(live.any()):
                    r = min(r, float(((top[..., 0] - top[..., 1]) / win(A).max(dim=-1).values)[live].min()))
                x = F.max_pool2d(x, 2, 2)
        x = x.flatten(1)
        if masks is not None:
            x = x * (2.0 * masks[0].double())
        w, bias = net.fc[2].weight.double(), net.fc[2].bias.double()
        r = min(r, float((F.linear(x, w, bias).abs() / F.linear(x.abs(), w.abs(), bias.abs())).min()))
    return r


def get_perspective_transform(src, dst):
    """[B,4,2] x 2 -> [B,3,3] with h33 = 1 (kornia's published algorithm as the exact 8 x 8 solve)."""
    x, y = src[..., 0], src[..., 1]
    u, v = dst[..., 0], dst[..., 1]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    rx = torch.stack((x, y, one, zero, zero, zero, -x * u, -y * u), dim=-1)
    ry = torch.stack((zero, zero, zero, x, y, one, -x * v, -y * v), dim=-1)
    A = torch.stack((rx, ry), dim=2).reshape(-1, 8, 8)                     # rows 2k, 2k + 1 for corner k
    rhs = torch.stack((u, v), dim=2).reshape(-1, 8, 1)
    h = torch.linalg.solve(A, rhs).squeeze(-1)
    return torch.cat((h, torch.ones_like(h[:, :1])), dim=1).view(-1, 3, 3)


def _normal_transform_pixel(h, w, dtype, device):
    m = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]], dtype=dtype, device=device)
    m[0, 0] = m[0, 0] * 2.0 / (1e-14 if w == 1 else w - 1.0)
    m[1, 1] = m[1, 1] * 2.0 / (1e-14 if h == 1 else h - 1.0)
    return m.unsqueeze(0)


def sampling_matrix(M, src_hw, dst_hw):
    """inverse(N_dst M N_src^-1) [B,3,3]: the matrix the normalised output grid is multiplied by."""
    n_src = _normal_transform_pixel(src_hw[0], src_hw[1], M.dtype, M.device)
    n_dst = _normal_transform_pixel(dst_hw[0], dst_hw[1], M.dtype, M.device)
    return torch.inverse(n_dst @ (M @ torch.inverse(n_src)))


def sampling_grid(S, h_out, w_out):
    """Normalised sampling grid [B,h,w,2] of the matrix S."""
    dt, dev = S.dtype, S.device
    xs = (torch.linspace(0, w_out - 1, w_out, dtype=dt, device=dev) / (w_out - 1) - 0.5) * 2
    ys = (torch.linspace(0, h_out - 1, h_out, dtype=dt, device=dev) / (h_out - 1) - 0.5) * 2
    gx = xs.view(1, 1, w_out).expand(1, h_out, w_out)
    gy = ys.view(1, h_out, 1).expand(1, h_out, w_out)
    B = S.shape[0]

    def row(r):
        return (gx * S[:, r, 0].view(B, 1, 1) + gy * S[:, r, 1].view(B, 1, 1)) + S[:, r, 2].view(B, 1, 1)

    X, Y, Z = row(0), row(1), row(2)
    eps = 1e-8
    scale = torch.where(Z.abs() > eps, 1.0 / (Z + eps), torch.ones_like(Z))
    return torch.stack((X * scale, Y * scale), dim=-1)


def warp_perspective(src, M, dsize, align_corners=True):
    grid = sampling_grid(sampling_matrix(M, src.shape[-2:], dsize), dsize[0], dsize[1])
    return F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=align_corners)


def photo_matrix(delta, corners, src_hw, dst_hw):
    """S of photometric_loss (what masic_udh_photo_matrix computes)."""
    corners_hat = corners + delta
    h = get_perspective_transform(corners - corners[:, 0].view(-1, 1, 2), corners_hat)
    return sampling_matrix(torch.inverse(h), src_hw, dst_hw)


def loss_from_matrix(S, img_a, patch_b, align_corners=True):
    grid = sampling_grid(S, patch_b.shape[-2], patch_b.shape[-1])
    return F.l1_loss(F.grid_sample(img_a, grid, mode="bilinear", padding_mode="zeros", align_corners=align_corners), patch_b)


def photometric_loss(delta, img_a, patch_b, corners, align_corners=True):
    """udh/udh/model.py:18-45."""
    corners_hat = corners + delta
    corners = corners - corners[:, 0].view(-1, 1, 2)
    h = get_perspective_transform(corners, corners_hat)
    h_inv = torch.inverse(h)
    patch_b_hat = warp_perspective(img_a, h_inv, (patch_b.shape[-2], patch_b.shape[-1]), align_corners)
    return F.l1_loss(patch_b_hat, patch_b)


def margins(delta, img_a, patch_b, corners, align_corners=True):
    """Float64 distances from the points where the loss is not differentiable: (the smallest distance of a sample's pixel
    coordinate from an integer, the smallest |diff|, the fraction of samples outside img_a)."""
    delta, img_a, patch_b, corners = (t.detach().double().cpu() for t in (delta, img_a, patch_b, corners))
    H, W = img_a.shape[-2:]
    S = photo_matrix(delta, corners, (H, W), patch_b.shape[-2:])
    grid = sampling_grid(S, patch_b.shape[-2], patch_b.shape[-1])
    if align_corners:
        fx, fy = (grid[..., 0] + 1) / 2 * (W - 1), (grid[..., 1] + 1) / 2 * (H - 1)
    else:
        fx, fy = ((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2
    frac = torch.minimum((fx - fx.round()).abs().min(), (fy - fy.round()).abs().min())
    diff = F.grid_sample(img_a, grid, mode="bilinear", padding_mode="zeros", align_corners=align_corners) - patch_b
    outside = ((fx < 0) | (fx > W - 1) | (fy < 0) | (fy > H - 1)).double().mean()
    return float(frac), float(diff.abs().min()), float(outside)


# ---- seeded inputs of the loss (numpy PCG64, as tests/udh_weights.py), one seed per pair
MARGIN_COORD, MARGIN_DIFF = 1e-4, 1e-5


def loss_pair(seed, img_hw, patch_hw, rho):
    """One pair from its seed: (img_a [1,H,W], patch_b [1,h,w], corners [4,2]) float32.  img_a is a sum of four plane waves plus
    noise; corners are those of an h x w window inside it (top-left, top-right, bottom-right, bottom-left), each moved by
    uniform(-rho, rho) pixels; patch_b is the flipped window of img_a at half weight plus noise (any patch_b makes a valid loss)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    H, W = img_hw
    h, w = patch_hw
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.3 * rng.standard_normal((H, W))
    for _ in range(4):
        fx, fy = rng.uniform(0.05, 0.5, 2)
        img += rng.uniform(0.2, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 6.28))
    x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
    corners = np.array([[x0, y0], [x0 + w - 1, y0], [x0 + w - 1, y0 + h - 1], [x0, y0 + h - 1]], dtype=np.float64)
    corners += rng.uniform(-rho, rho, (4, 2))
    pb = 0.5 * img[y0:y0 + h, x0:x0 + w][::-1, ::-1] + 0.7 * rng.standard_normal((h, w))
    f = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))  # noqa: E731
    return f(img[None]), f(pb[None]), f(corners)


def patch_batch(seeds, p):
    """(a, b) [B,1,p,p]: tests/udh_weights.py: patches(seed, 1, p) of each pair seed, stacked."""
    from tests import udh_weights as UW
    pairs = [UW.patches(int(s), 1, p) for s in seeds]
    return torch.cat([q[0] for q in pairs]), torch.cat([q[1] for q in pairs])


def loss_inputs(seeds, img_hw, patch_hw, rho):
    """(img_a [B,1,H,W], patch_b [B,1,h,w], corners [B,4,2]) for a list of pair seeds."""
    pairs = [loss_pair(int(s), img_hw, patch_hw, rho) for s in seeds]
    return tuple(torch.stack([p[i] for p in pairs]) for i in range(3))


def in_general_position(delta, img_a, patch_b, corners, align_corners=(True,)):
    """True if, in float64, every sample coordinate is > 1e-4 px from an integer and every |diff| >= 1e-5: away from the points
    where the loss is not differentiable (there two correct float32 evaluations may take different one-sided derivatives)."""
    for ac in align_corners:
        coord, diff, _ = margins(delta, img_a, patch_b, corners, ac)
        if not (coord > MARGIN_COORD and diff >= MARGIN_DIFF):        # (a NaN fails)
            return False
    return True


def find_pair_seeds(delta, img_hw, patch_hw, rho, first, align_corners=(True,), tries=20000):
    """For each row of delta [B,4,2], the first seed >= first + 100000 * row whose pair is in general position with that row."""
    seeds = []
    for n in range(delta.shape[0]):
        for s in range(first + 100000 * n, first + 100000 * n + tries):
            img, pb, c = loss_pair(s, img_hw, patch_hw, rho)
            if in_general_position(delta[n:n + 1], img[None], pb[None], c[None], align_corners):
                seeds.append(s)
                break
        else:
            raise RuntimeError(f"no pair seed in general position for row {n}")
    return seeds
