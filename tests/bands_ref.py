"""What the tests of the banded y bitstream share (tests/test_cpu_codec_bands.py, tests/test_gpu_codec_bands.py): the bands of a latent,
the live taps of the type-A 5x5 mask, and the float64 reference of the banded context model -- tests/gemm_ref.layer64 applied to each
band cut out as an image of its own.  Nothing here needs a GPU."""
import torch

from tests import gemm_ref as G

# (dy, dx) of the 12 live taps of the type-A 5x5 mask: rows -2 and -1 with five columns each, row 0 columns -2 and -1
LIVE_TAPS = [(dy, dx) for dy in (-2, -1) for dx in range(-2, 3)] + [(0, -2), (0, -1)]
SCHEDULE_CASES = [(8, 12, 1), (8, 12, 3), (8, 12, 4), (4, 4, 2), (76, 136, 8), (5, 7, 2)]          # (h, w, S)


def bands(h, S):
    """[(first row, one past the last row)] of the bands of S rows of a latent of h rows; the last one is shorter when S does not
    divide h.  S = 0 or S >= h: one band."""
    if S <= 0 or S >= h:
        return [(0, h)]
    return [(r, min(r + S, h)) for r in range(0, h, S)]


def expected_steps(h, w, S):
    return w + 3 * (min(S, h) - 1)


def banded_layer64(case, l, x, w, bias, S):
    """gemm_ref.layer64 of a context-model case with the band top: every band of x [B, Cin, H, W] as an image of its own, the results
    put back in place"""
    assert case.ctx
    return torch.cat([G.layer64(case, l, x[:, :, r0:r1], w, bias) for r0, r1 in bands(x.shape[2], S)], dim=2)


def hsic(N, M, K, seed, prec, dev="cuda"):
    """HSIC(N, M, K) with synthetic weights in eval mode on the device, the operand mode set (the caller restores "f32")"""
    import MASIC
    from masic_amd import nn as mnn, synth
    mnn.set_precision(prec)
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    net = net.to(dev).eval()
    net.update()
    return net
