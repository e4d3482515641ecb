"""SSIM and MS-SSIM on the HIP path, behind the pytorch-msssim 0.2.1 API (`ssim`, `ms_ssim`, `SSIM`, `MS_SSIM`).

The reference drivers report MS-SSIM for every RD point and every CQE training step (coremasic/mywork/test3_real.py:102-103,
newtrain_cqe_real.py:93-95): `ms_ssim(x_hat, target, data_range=1, size_average=False)`.  Same definition as 0.2.1: an 11-tap
Gaussian window (float32 taps, sigma 1.5) applied as a valid separable filter, C1 = (K1 R)^2, C2 = (K2 R)^2, per-channel spatial
means of the SSIM and contrast-structure maps, a 2x2 average-pool pyramid (padding = side % 2, zeros counted), and
prod(relu(m_i) ** w_i) over the levels.  Forward and backward are HIP kernels (masic_amd/csrc/ssim.hip); autograd gives the
gradient for X and for Y, whichever requires it.

Supported: float32 4-D CUDA tensors, win_size 11, win None.  Everything else 0.2.1 accepts raises ValueError here.
"""
import torch

from . import _lib, ops

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM", "SsimFn", "MsSsimFn"]

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

_taps_cache = {}


def gaussian_taps(win_size=11, win_sigma=1.5):
    """The 1-D window as 0.2.1 builds it, on the CPU in float32: exp(-(k - size//2)^2 / (2 sigma^2)) / sum.  A tuple of floats."""
    key = (int(win_size), float(win_sigma))
    if key not in _taps_cache:
        coords = torch.arange(win_size).float()
        coords -= win_size // 2
        g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
        g /= g.sum()
        _taps_cache[key] = tuple(g.tolist())
    return _taps_cache[key]


def _check(X, Y, win_size, win, name):
    """0.2.1's argument checks, then the ones of this port."""
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if len(X.shape) not in (4, 5):
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    if not X.type() == Y.type():
        raise ValueError(f"Input images should have the same dtype, but got {X.type()} and {Y.type()}.")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    if len(X.shape) == 5:
        raise ValueError(f"{name}: 5-d (video) input is not supported by the HIP port; got {tuple(X.shape)}")
    if win is not None:
        raise ValueError(f"{name}: a custom `win` tensor is not supported by the HIP port (pass win_size / win_sigma)")
    if win_size != 11:
        raise ValueError(f"{name}: win_size {win_size} is not supported by the HIP port (the kernels are specialised for 11 taps)")
    if X.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {X.dtype} is not supported by the HIP port (float32 only)")
    for t, n in ((X, "X"), (Y, "Y")):       # CPU tensors: RuntimeError, as everywhere on the product path
        if not t.is_cuda:
            ops._dev(t, n)


def _constants(data_range, K):
    K1, K2 = K
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


class _Base(torch.autograd.Function):
    @staticmethod
    def _run(ctx, X, Y, taps, weights, C1, C2, flags):
        out, ws = ops.ssim_fwd(X, Y, taps, weights, C1, C2, flags)
        ctx.save_for_backward(X, Y, ws)
        ctx.args = (taps, weights, C1, C2, flags)
        return out

    @staticmethod
    def _grad(ctx, g):
        X, Y, ws = ctx.saved_tensors
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None
        taps, weights, C1, C2, flags = ctx.args
        return ops.ssim_bwd(X, Y, ws, g, taps, weights, C1, C2, flags, need_x=need_x, need_y=need_y)


class SsimFn(_Base):
    """ssim(X, Y) per image ([N]) or averaged ([]): apply(X, Y, taps, C1, C2, size_average, nonnegative_ssim)."""

    @staticmethod
    def forward(ctx, X, Y, taps, C1, C2, size_average, nonnegative_ssim):
        flags = (_lib.SSIM_SIZE_AVERAGE if size_average else 0) | (_lib.SSIM_NONNEG if nonnegative_ssim else 0)
        return _Base._run(ctx, X, Y, taps, None, C1, C2, flags)

    @staticmethod
    def backward(ctx, g):
        return _Base._grad(ctx, g) + (None,) * 5


class MsSsimFn(_Base):
    """ms_ssim(X, Y) per image ([N]) or averaged ([]): apply(X, Y, taps, weights, C1, C2, size_average)."""

    @staticmethod
    def forward(ctx, X, Y, taps, weights, C1, C2, size_average):
        flags = _lib.SSIM_MS | (_lib.SSIM_SIZE_AVERAGE if size_average else 0)
        return _Base._run(ctx, X, Y, taps, tuple(weights), C1, C2, flags)

    @staticmethod
    def backward(ctx, g):
        return _Base._grad(ctx, g) + (None,) * 5


def _levels_fit(H, W, levels):
    for _ in range(levels):
        if H < 11 or W < 11:
            return False
        H, W = (H + 1) // 2, (W + 1) // 2
    return True


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim (0.2.1): [N] per-image SSIM (size_average=False) or their mean."""
    _check(X, Y, win_size, win, "ssim")
    if min(X.shape[-2:]) < 11:
        raise ValueError(f"ssim: spatial size {tuple(X.shape[-2:])} is smaller than the 11-tap window; the HIP port filters both sides")
    C1, C2 = _constants(data_range, K)
    return SsimFn.apply(X.contiguous(), Y.contiguous(), gaussian_taps(win_size, win_sigma), C1, C2, bool(size_average),
                        bool(nonnegative_ssim))


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim (0.2.1): [N] per-image MS-SSIM (size_average=False) or their mean."""
    _check(X, Y, win_size, win, "ms_ssim")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((win_size - 1) * (2 ** 4))
    if weights is None:
        weights = DEFAULT_WEIGHTS
    weights = tuple(torch.tensor([float(w) for w in weights], dtype=torch.float32).tolist())    # 0.2.1 holds them in float32
    if not 1 <= len(weights) <= 8 or not _levels_fit(X.shape[-2], X.shape[-1], len(weights)):
        raise ValueError(f"ms_ssim: {len(weights)} levels on {tuple(X.shape[-2:])}: the HIP port needs 1 .. 8 levels of at least 11 x 11")
    C1, C2 = _constants(data_range, K)
    return MsSsimFn.apply(X.contiguous(), Y.contiguous(), gaussian_taps(win_size, win_sigma), weights, C1, C2, bool(size_average))


def _check_module(win_size, spatial_dims):
    if spatial_dims != 2:
        raise ValueError(f"spatial_dims {spatial_dims} is not supported by the HIP port (2-d images only)")
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")


class SSIM(torch.nn.Module):
    """pytorch_msssim.SSIM (0.2.1).  `channel` is accepted for compatibility (the window is shared by every channel)."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, K=(0.01, 0.03),
                 nonnegative_ssim=False):
        super().__init__()
        _check_module(win_size, spatial_dims)
        self.win_size = win_size
        self.win_sigma = win_sigma
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size, win_sigma=self.win_sigma,
                    K=self.K, nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    """pytorch_msssim.MS_SSIM (0.2.1)."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None,
                 K=(0.01, 0.03)):
        super().__init__()
        _check_module(win_size, spatial_dims)
        self.win_size = win_size
        self.win_sigma = win_sigma
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size, win_sigma=self.win_sigma,
                       weights=self.weights, K=self.K)
