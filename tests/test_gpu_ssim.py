"""SSIM / MS-SSIM on the HIP path (masic_amd/ssim.py, masic_amd/csrc/ssim.hip) against a float64 restatement of pytorch-msssim 0.2.1.

The restatement below (`ref_*`) is 0.2.1's op sequence in plain torch ops on the CPU in float64: the float32 window
(arange(11).float(), exp, normalise), the valid separable depthwise filter (H then W), _ssim's maps and spatial means,
the avg_pool2d(2, padding=side % 2) pyramid, relu and prod(m ** w).  tests/test_cpu_ssim.py checks it against closed forms."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


# ---------------------------------------------------------------- float64 restatement (CPU)
def ref_window(win_size=11, win_sigma=1.5):
    coords = torch.arange(win_size).float()
    coords -= win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g /= g.sum()
    return g.double()


def ref_filter(x, g):
    C = x.shape[1]
    out = F.conv2d(x, g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(out, g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)


def ref__ssim(X, Y, data_range, g, K=(0.01, 0.03)):
    C1 = (K[0] * data_range) ** 2
    C2 = (K[1] * data_range) ** 2
    mu1, mu2 = ref_filter(X, g), ref_filter(Y, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = ref_filter(X * X, g) - mu1_sq
    sigma2_sq = ref_filter(Y * Y, g) - mu2_sq
    sigma12 = ref_filter(X * Y, g) - mu1_mu2
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)


def ref_pool(x):
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def ref_ssim(X, Y, data_range=255, size_average=True, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    s, _ = ref__ssim(X, Y, data_range, ref_window(11, win_sigma), K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ref_ms_ssim(X, Y, data_range=255, size_average=True, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    g = ref_window(11, win_sigma)
    w = torch.tensor(WEIGHTS if weights is None else weights, dtype=torch.float32).double()
    mcs = []
    for i in range(len(w)):
        s, cs = ref__ssim(X, Y, data_range, g, K)
        if i < len(w) - 1:
            mcs.append(torch.relu(cs))
            X, Y = ref_pool(X), ref_pool(Y)
    s = torch.relu(s)
    val = torch.prod(torch.stack(mcs + [s], dim=0) ** w.view(-1, 1, 1), dim=0)
    return val.mean() if size_average else val.mean(1)


# ---------------------------------------------------------------- inputs
def smooth(N, C, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    lo = torch.rand(N, C, max(2, H // 16), max(2, W // 16), generator=gen)
    mid = torch.rand(N, C, max(2, H // 4), max(2, W // 4), generator=gen)
    y = 0.7 * F.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False) + \
        0.3 * F.interpolate(mid, size=(H, W), mode="bilinear", align_corners=False)
    return y.clamp(0, 1).contiguous()


def pair(shape, s, seed=0):
    Y = smooth(*shape, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    X = (Y + s * torch.randn(shape, generator=gen)).clamp(0, 1)
    return X.contiguous(), Y


def _ms():
    from masic_amd import ssim as S
    return S


def _rel(g, r):
    return float((g.double() - r).norm() / r.norm())


# ---------------------------------------------------------------- 1. values
SHAPES = [(8, 3, 512, 512), (1, 3, 1216, 2176), (2, 3, 181, 203)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_vs_float64(shape):
    S = _ms()
    cases = [(f"noise {s}", *pair(shape, s, seed=7)) for s in (0.01, 0.1, 0.5)]
    Yi = smooth(*shape, 7)
    cases.append(("1 - Y", (1 - Yi).contiguous(), Yi))
    worst = 0.0
    for name, X, Y in cases:
        Xd, Yd = X.cuda(), Y.cuda()
        X64, Y64 = X.double(), Y.double()
        for sa in (False, True):
            got = S.ms_ssim(Xd, Yd, data_range=1, size_average=sa)
            ref = ref_ms_ssim(X64, Y64, data_range=1, size_average=sa)
            assert got.dtype == torch.float32 and got.shape == ref.shape
            err = float((got.cpu().double() - ref).abs().max())
            worst = max(worst, err)
            assert err <= 5e-6, (name, "ms_ssim", sa, err)
            for nn_ in (False, True):
                got = S.ssim(Xd, Yd, data_range=1, size_average=sa, nonnegative_ssim=nn_)
                ref = ref_ssim(X64, Y64, data_range=1, size_average=sa, nonnegative_ssim=nn_)
                assert got.dtype == torch.float32 and got.shape == ref.shape
                err = float((got.cpu().double() - ref).abs().max())
                worst = max(worst, err)
                assert err <= 5e-6, (name, "ssim", sa, nn_, err)
        if name == "1 - Y":
            # cs < 0 at the finest level: the relu clip is taken, MS-SSIM is 0; plain SSIM is negative unless nonnegative_ssim
            _, cs = ref__ssim(X64, Y64, 1, ref_window())
            assert (cs < 0).all()
            assert (S.ms_ssim(Xd, Yd, data_range=1, size_average=False) == 0).all()
    # data_range 255 (the default) on 0..255 images
    X, Y = pair(shape, 0.1, seed=3)
    got = S.ms_ssim((255 * X).cuda(), (255 * Y).cuda(), size_average=False)
    ref = ref_ms_ssim(255 * X.double(), 255 * Y.double(), size_average=False)
    assert float((got.cpu().double() - ref).abs().max()) <= 5e-6
    print(f"{shape}: worst |HIP - float64| = {worst:.2e}")


# ---------------------------------------------------------------- 2. gradients
GSHAPES = [(2, 3, 256, 256), (2, 3, 181, 203)]


def _ref_grads(fn, X, Y):
    X64 = X.double().requires_grad_(True)
    Y64 = Y.double().requires_grad_(True)
    fn(X64, Y64).backward()
    return X64.grad, Y64.grad


def _hip_grads(fn, X, Y, need=(True, True)):
    Xd = X.cuda().requires_grad_(need[0])
    Yd = Y.cuda().requires_grad_(need[1])
    fn(Xd, Yd).backward()
    return (Xd.grad.cpu() if need[0] else None), (Yd.grad.cpu() if need[1] else None)


@pytest.mark.parametrize("shape", GSHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_vs_float64_autograd(shape):
    S = _ms()
    X, Y = pair(shape, 0.1, seed=11)
    losses = {
        "1 - ms_ssim": (lambda a, b: (1 - S.ms_ssim(a, b, data_range=1)).sum(),
                        lambda a, b: (1 - ref_ms_ssim(a, b, data_range=1)).sum()),
        "1 - ms_ssim per image": (lambda a, b: (1 - S.ms_ssim(a, b, data_range=1, size_average=False)).sum(),
                                  lambda a, b: (1 - ref_ms_ssim(a, b, data_range=1, size_average=False)).sum()),
        "ssim": (lambda a, b: S.ssim(a, b, data_range=1).sum(), lambda a, b: ref_ssim(a, b, data_range=1).sum()),
        "ssim per image": (lambda a, b: S.ssim(a, b, data_range=1, size_average=False).sum(),
                           lambda a, b: ref_ssim(a, b, data_range=1, size_average=False).sum()),
    }
    for name, (hip, ref) in losses.items():
        rx, ry = _ref_grads(ref, X, Y)
        gx, gy = _hip_grads(hip, X, Y)
        ex, ey = _rel(gx, rx), _rel(gy, ry)
        print(f"{shape} {name}: relative gradient error dX {ex:.1e} dY {ey:.1e}")
        assert ex <= 5e-4 and ey <= 5e-4, (name, ex, ey)
        # one side only (the training case: the target carries no gradient), and the other side only
        gx1, _ = _hip_grads(hip, X, Y, need=(True, False))
        _, gy1 = _hip_grads(hip, X, Y, need=(False, True))
        assert _rel(gx1, gx.double()) <= 1e-6 and _rel(gy1, gy.double()) <= 1e-6, name


def test_gradient_zero_through_relu_clipped_level():
    S = _ms()
    Y = smooth(2, 3, 181, 203, 5)
    X = (1 - Y).contiguous()
    gx, gy = _hip_grads(lambda a, b: (1 - S.ms_ssim(a, b, data_range=1)).sum(), X, Y)
    rx, ry = _ref_grads(lambda a, b: (1 - ref_ms_ssim(a, b, data_range=1)).sum(), X, Y)
    assert torch.isfinite(rx).all() and (rx == 0).all()          # what torch autograd gives through relu(cs) <= 0
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
    assert (gx == 0).all() and (gy == 0).all()


# ---------------------------------------------------------------- 3. identity, 4. determinism
def test_identity_is_exactly_one():
    S = _ms()
    for shape in [(2, 3, 181, 203), (1, 3, 256, 320)]:
        X = smooth(*shape, 2).cuda()
        assert (S.ms_ssim(X, X, data_range=1, size_average=False) == 1.0).all()
        assert (S.ssim(X, X, data_range=1, size_average=False) == 1.0).all()
        assert float(S.ms_ssim(X, X, data_range=1)) == 1.0 and float(S.ssim(X, X, data_range=1)) == 1.0


def test_bit_reproducible():
    S = _ms()
    X, Y = pair((2, 3, 181, 203), 0.1, seed=4)
    res = []
    for _ in range(2):
        Xd, Yd = X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
        v = S.ms_ssim(Xd, Yd, data_range=1, size_average=False)
        (1 - v).sum().backward()
        s = S.ssim(Xd.detach(), Yd.detach(), data_range=1, size_average=False)
        res.append((v.detach().cpu(), s.cpu(), Xd.grad.cpu(), Yd.grad.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 5. capture
def test_graph_capture_matches_eager():
    S = _ms()
    X, Y = pair((2, 3, 256, 256), 0.1, seed=9)
    Xs, Ys = X.cuda().requires_grad_(True), Y.cuda()

    def step():
        v = S.ms_ssim(Xs, Ys, data_range=1, size_average=False)
        gx, = torch.autograd.grad((1 - v).sum(), Xs)
        return v.detach(), gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ---------------------------------------------------------------- 6. drop-in on the CQE stage
class DistortionLossWithReport(nn.Module):
    """newtrain_cqe_real.py:69-96, kind=0, with its two ms_ssim report entries (they do not enter the loss)."""

    def __init__(self, lmbda=1e-2, report=True):
        super().__init__()
        self.mse = nn.MSELoss()
        self.lmbda = lmbda
        self.report = report

    def forward(self, output, target1, target2):
        from pytorch_msssim import ms_ssim
        out = {}
        out['mse_loss'] = self.mse(output['x1_hat'], target1) + self.mse(output['x2_hat'], target2)
        out['loss'] = self.lmbda * 255 ** 2 * out['mse_loss']
        if self.report:
            out['ms_ssim1'] = ms_ssim(output['x1_hat'], target1, data_range=1, size_average=False)[0]
            out['ms_ssim2'] = ms_ssim(output['x2_hat'], target2, data_range=1, size_average=False)[0]
            out['ms_ssim'] = (out['ms_ssim1'] + out['ms_ssim2']) / 2
        out['psnr1'] = 10 * math.log10(1 / self.mse(output['x1_hat'], target1))
        out['psnr2'] = 10 * math.log10(1 / self.mse(output['x2_hat'], target2))
        return out


def test_drop_in_import_and_cqe_driver_call():
    import pytorch_msssim
    from pytorch_msssim import MS_SSIM, SSIM, ms_ssim, ssim
    from masic_amd import ssim as S
    assert (ssim, ms_ssim, SSIM, MS_SSIM) == (S.ssim, S.ms_ssim, S.SSIM, S.MS_SSIM)
    assert pytorch_msssim.__name__ == "pytorch_msssim" and "masic_amd" in ms_ssim.__module__

    import MASIC
    from masic_amd import synth
    x1, x2, hm = synth.synth_inputs(1, 192, 256, seed=31)
    gen = torch.Generator().manual_seed(31)
    xh1 = (x1 + 0.02 * torch.randn(x1.shape, generator=gen)).clamp(0, 1)
    xh2 = (x2 + 0.02 * torch.randn(x2.shape, generator=gen)).clamp(0, 1)
    d1, d2, hm, xh1, xh2 = (t.to(DEV) for t in (x1, x2, hm, xh1, xh2))
    net2 = MASIC.Independent_EN()
    net2.load_state_dict(synth.synth_state_dict(net2.state_dict(), seed=31))
    net2 = net2.to(DEV).train()

    # the drivers' exact call on Independent_EN's train-mode outputs, grad enabled
    out = net2(xh1, xh2, hm)
    assert out['x1_hat'].requires_grad
    v = ms_ssim(out['x1_hat'], d1, data_range=1, size_average=False)[0]
    ref = ref_ms_ssim(out['x1_hat'].detach().cpu().double(), d1.cpu().double(), data_range=1, size_average=False)[0]
    assert v.dtype == torch.float32 and abs(float(v) - float(ref)) <= 5e-6, (float(v), float(ref))

    # one CQE step with and without the report entries: the same parameter gradients
    def grads(report):
        net2.zero_grad(set_to_none=True)
        o = net2(xh1, xh2, hm)
        crit = DistortionLossWithReport(report=report)(o, d1, d2)
        crit['loss'].backward()
        if report:
            assert 0.0 < float(crit['ms_ssim']) <= 1.0
        return {n: p.grad.detach().clone() for n, p in net2.named_parameters()}

    a, b, c = grads(False), grads(False), grads(True)
    assert len(a) == 86
    for n in a:
        noise = float((a[n] - b[n]).abs().max())
        diff = float((c[n] - a[n]).abs().max())
        assert diff <= 3 * noise, (n, diff, noise)


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors():
    S = _ms()
    X = torch.rand(1, 3, 176, 176, device=DEV)
    with pytest.raises(ValueError):
        S.ms_ssim(X, X[:, :, :170])                                   # shape mismatch
    with pytest.raises(ValueError):
        S.ssim(X, X.double())                                         # dtype mismatch
    with pytest.raises(ValueError):
        S.ssim(X[0], X[0])                                            # not 4-D
    with pytest.raises(ValueError):
        S.ms_ssim(X, X, win_size=10)                                  # even window
    with pytest.raises(ValueError):
        S.ssim(X.unsqueeze(2), X.unsqueeze(2))                        # 5-D: unsupported
    with pytest.raises(ValueError):
        S.ms_ssim(X, X, win=torch.ones(3, 1, 1, 11))                  # custom window: unsupported
    with pytest.raises(ValueError):
        S.ssim(X, X, win_size=7)                                      # win_size != 11: unsupported
    with pytest.raises(ValueError):
        S.ssim(X[:, :, :10], X[:, :, :10])                            # side < 11 in ssim
    with pytest.raises(ValueError):
        S.ssim(X.double(), X.double())                                # float64: unsupported
    with pytest.raises(AssertionError):
        S.ms_ssim(X[:, :, :160], X[:, :, :160])                       # min side <= 160
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ms_ssim(X.cpu(), X.cpu())
    with pytest.raises(ValueError):
        S.SSIM(win_size=4)
    with pytest.raises(ValueError):
        S.MS_SSIM(spatial_dims=3)
    # the modules match the functions
    Y = (X + 0.1 * torch.randn_like(X)).clamp(0, 1)
    assert torch.equal(S.MS_SSIM(data_range=1, size_average=False)(X, Y), S.ms_ssim(X, Y, data_range=1, size_average=False))
    assert torch.equal(S.SSIM(data_range=1, channel=3)(X, Y), S.ssim(X, Y, data_range=1))
