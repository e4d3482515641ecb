"""CPU checks of the SSIM / MS-SSIM port (no GPU): the pytorch_msssim names and their 0.2.1 signatures, the argument errors raised
before any device work, and the float64 restatement of tests/test_gpu_ssim.py against closed forms."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_ssim import ref__ssim, ref_ms_ssim, ref_pool, ref_ssim, ref_window


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_pytorch_msssim_exposes_the_hip_port_with_0_2_1_signatures():
    import pytorch_msssim
    from masic_amd import ssim as S
    from pytorch_msssim import MS_SSIM, SSIM, ms_ssim, ssim
    assert (ssim, ms_ssim, SSIM, MS_SSIM) == (S.ssim, S.ms_ssim, S.SSIM, S.MS_SSIM)
    assert set(pytorch_msssim.__all__) == {"ssim", "ms_ssim", "SSIM", "MS_SSIM"}
    E = inspect.Parameter.empty
    assert _params(ssim) == [("X", E), ("Y", E), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                             ("win", None), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
    assert _params(ms_ssim) == [("X", E), ("Y", E), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                ("win", None), ("weights", None), ("K", (0.01, 0.03))]
    assert _params(SSIM.__init__) == [("self", E), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                      ("channel", 3), ("spatial_dims", 2), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
    assert _params(MS_SSIM.__init__) == [("self", E), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                         ("channel", 3), ("spatial_dims", 2), ("weights", None), ("K", (0.01, 0.03))]
    assert issubclass(SSIM, torch.nn.Module) and issubclass(MS_SSIM, torch.nn.Module)


def test_taps_are_the_float32_window():
    from masic_amd.ssim import gaussian_taps
    t = torch.tensor(gaussian_taps(11, 1.5), dtype=torch.float32)
    assert torch.equal(t, ref_window(11, 1.5).float())
    assert torch.equal(t, t.flip(0)) and abs(float(t.double().sum()) - 1.0) < 1e-6


def test_argument_errors_before_the_device():
    from masic_amd import ssim as S
    X = torch.rand(1, 3, 176, 176)
    with pytest.raises(ValueError):
        S.ms_ssim(X, X[:, :, :170])
    with pytest.raises(ValueError):
        S.ssim(X, X.double())
    with pytest.raises(ValueError):
        S.ssim(X[0], X[0])
    with pytest.raises(ValueError):
        S.ms_ssim(X, X, win_size=12)
    with pytest.raises(ValueError):
        S.ms_ssim(X.unsqueeze(2), X.unsqueeze(2))
    with pytest.raises(ValueError):
        S.ssim(X, X, win=torch.ones(3, 1, 1, 11))
    with pytest.raises(ValueError):
        S.ms_ssim(X, X, win_size=9)
    with pytest.raises(ValueError):
        S.ssim(X.half(), X.half())
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # CPU tensors: refused like every other op
        S.ssim(X, X)


@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.5, 0.5), (1.0, 0.0), (30.0, 200.0)])
def test_restatement_constant_images(a, b):
    R = 255.0 if max(a, b) > 1 else 1.0
    X = torch.full((2, 3, 40, 37), a, dtype=torch.float64)
    Y = torch.full((2, 3, 40, 37), b, dtype=torch.float64)
    C1 = (0.01 * R) ** 2
    g = ref_window()
    s, cs = ref__ssim(X, Y, R, g / g.sum())          # taps summing to 1 in float64: a constant filters to itself
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert torch.allclose(s, torch.full_like(s, want), rtol=0, atol=1e-12)
    assert torch.allclose(cs, torch.ones_like(cs), rtol=0, atol=1e-12)
    # with the float32 taps (sum 1 within 1e-7) as the contract has them
    assert torch.allclose(ref_ssim(X, Y, data_range=R, size_average=False), torch.full((2,), want, dtype=torch.float64), rtol=0, atol=1e-5)


def test_restatement_identity_and_pooled_sizes():
    X = torch.rand(1, 2, 181, 203, dtype=torch.float64)
    assert abs(float(ref_ms_ssim(X, X, data_range=1)) - 1.0) < 1e-9
    assert abs(float(ref_ssim(X, X, data_range=1)) - 1.0) < 1e-9
    h, w = 181, 203
    x = X
    for _ in range(4):
        x = ref_pool(x)
        h, w = (h + 1) // 2, (w + 1) // 2           # avg_pool2d(2, padding=side % 2): ceil(side / 2)
        assert tuple(x.shape[2:]) == (h, w)
    # the odd-size rule: the first window starts at -1 and averages one zero (count_include_pad)
    t = torch.arange(1.0, 10.0, dtype=torch.float64).view(1, 1, 3, 3)
    p = ref_pool(t)
    assert p.shape[2:] == (2, 2)
    assert float(p[0, 0, 0, 0]) == 1.0 / 4 and float(p[0, 0, 1, 1]) == (5 + 6 + 8 + 9) / 4
    assert torch.equal(p, F.avg_pool2d(t, 2, padding=1, count_include_pad=True, ceil_mode=False))
