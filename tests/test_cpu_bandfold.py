"""The band-aware entropy model without a GPU: include/masic_bandfold.h and its binding, the validation of HSIC.band_rows and
bands.model_band_rows, and the numpy references the GPU tests compare the kernels with (tests/bandfold_ref.py)."""
import os

import numpy as np
import pytest

from tests import bandfold_ref as BR
from tests import bands_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_BAND_ROWS = [True, False, 3.0, "3", -1, 256, None]


def test_the_pinned_headers_do_not_know_it():
    """the entry points are masic_bandfold.h's alone (a row of tests/test_cpu_side_headers.py)"""
    for pinned in ("masic_hip.h", "masic_bands.h"):
        with open(os.path.join(ROOT, "include", pinned)) as f:
            assert "bandfold" not in f.read()


def test_grid_cap_is_the_one_the_past_the_cap_cases_exceed():
    from masic_amd import bandfold
    assert bandfold.max_blocks() * 256 == BR.GRID_CAP_LANES
    for B, C, h, w, S in BR.PAST_CAP_CASES:
        v = 4 if (S * w) % 4 == 0 and (h * w) % 4 == 0 else 2 if (S * w) % 2 == 0 and (h * w) % 2 == 0 else 1
        assert B * BR.n_bands(h, S) * C * S * w // v > BR.GRID_CAP_LANES          # fold: one lane per vector of the folded tensor
        assert B * C * h * w // v > BR.GRID_CAP_LANES                              # unfold: one per vector of the latent
    assert {(S * w) % 2 for _, _, _, w, S in BR.PAST_CAP_CASES} == {0, 1}          # the vector path and the single-float path


@pytest.mark.parametrize("bad", BAD_BAND_ROWS, ids=repr)
def test_band_rows_validation(bad):
    import MASIC
    from masic_amd import bands
    net = MASIC.HSIC(16, 16, 2)
    assert net.band_rows == 0
    net.band_rows = 4
    with pytest.raises(ValueError, match="band_rows must be an integer in 0 .. 255"):
        net.band_rows = bad
    assert net.band_rows == 4                                # a refused value changes nothing
    with pytest.raises(ValueError, match="band_rows must be an integer in 0 .. 255"):
        with bands.model_band_rows(net, bad):
            raise AssertionError("the body must not run")
    assert net.band_rows == 4


def test_band_rows_is_a_plain_attribute():
    import inspect
    import MASIC
    from masic_amd import bands
    net = MASIC.HSIC(16, 16, 2)
    keys = set(net.state_dict())
    for ok in (0, 1, 255, np.int64(7)):
        net.band_rows = ok
        assert net.band_rows == int(ok) and type(net.band_rows) is int
    assert set(net.state_dict()) == keys and not any("band" in k for k in keys)
    assert "band_rows" not in inspect.signature(MASIC.HSIC.__init__).parameters
    assert isinstance(MASIC.HSIC.band_rows, property)
    with bands.model_band_rows(net, 3) as inside:
        assert inside is net and net.band_rows == 3
        with bands.model_band_rows(net, 0):
            assert net.band_rows == 0
        assert net.band_rows == 3
    assert net.band_rows == 7
    with pytest.raises(KeyError):
        with bands.model_band_rows(net, 5):
            raise KeyError("restored after an exception too")
    assert net.band_rows == 7
    # the coder's own argument keeps its default
    for fn in (MASIC.HSIC.compress, MASIC.HSIC.compress_batch):
        assert inspect.signature(fn).parameters["band_rows"].default == 0


@pytest.mark.parametrize("case", BR.CASES + [(2, 4, 9, 6, 4), (1, 2, 7, 3, 255)], ids=str)
def test_numpy_fold_agrees_with_the_bands_and_unfold_inverts_it(case):
    B, C, h, w, S = case
    x = BR.rand((B, C, h, w), seed=11)
    xb = BR.fold(x, S)
    T = BR.n_bands(h, S)
    spans = R.bands(h, S) if S < h else [(0, h)]
    assert len(spans) == T and xb.shape == (B * T, C, S, w)
    for b in range(B):
        for t, (r0, r1) in enumerate(spans):
            assert np.array_equal(xb[b * T + t, :, :r1 - r0], x[b, :, r0:r1])
            pad = xb[b * T + t, :, r1 - r0:]
            assert np.array_equal(pad.view(np.uint32), np.zeros(pad.shape, dtype=np.uint32))         # +0.0, not -0.0
    assert np.array_equal(BR.unfold(xb, B, h, S).view(np.uint32), x.view(np.uint32))


def test_numpy_fold_and_unfold_are_adjoint():
    B, C, h, w, S = 2, 3, 5, 7, 2
    x = BR.rand((B, C, h, w), seed=1).astype(np.float64)
    g = BR.rand((B * BR.n_bands(h, S), C, S, w), seed=2).astype(np.float64)
    assert abs(float((BR.fold(x, S) * g).sum()) - float((x * BR.unfold(g, B, h, S)).sum())) < 1e-9


def test_bf16_bits_is_round_to_nearest_even():
    import torch
    x = np.concatenate([BR.rand((4096,), seed=3), np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 3.0e38], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(BR.bf16_bits(x), want)


def test_f16k_records_layout():
    bits = np.arange(2 * 19 * 2 * 3, dtype=np.uint16).reshape(2, 19, 2, 3)
    rec = BR.f16k_records(bits, 32)
    assert rec.shape == (2, 2, 6, 16)
    assert rec[1, 1, 4, 2] == bits[1, 18, 1, 1] and rec[0, 0, 5, 15] == bits[0, 15, 1, 2]
    assert not rec[:, 1, :, 3:].any()                        # channels 19 .. 31 do not exist


@pytest.mark.parametrize("S", [3, 4])
def test_oracle_seed_of_the_gpu_model_tests_has_an_empty_tie_zone(S):
    """tests/test_gpu_bandfold.py compares the eval forward with the oracle under the tie-zone rule of tests/test_gpu_hsic.py; for its
    seed and picture size no oracle latent lies within 1e-4 of a rounding boundary (the nearest is 2e-4 away), so that rule leaves out
    nothing -- and the oracle with banded context models differs from the plain one in the y likelihoods only."""
    import torch
    import MASIC
    from masic_amd import synth
    from oracle import hsic_oracle as O
    from tests.util import tie_zone
    N, M, K, seed, H, W = 32, 48, 3, 360, 128, 192
    sd = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=seed)
    x1, x2, hm = synth.synth_inputs(1, H, W, seed=seed)
    with torch.no_grad():
        plain = O.hsic_forward(sd, x1, x2, hm, K=K, keep=True)
        with BR.oracle_with_bands(O, S):
            banded = O.hsic_forward(sd, x1, x2, hm, K=K, keep=True)
        again = O.hsic_forward(sd, x1, x2, hm, K=K, keep=True)
    aux = banded["_aux"]
    assert tuple(aux["y1"].shape) == (1, M, 8, 12)
    for k in ("y1", "y2", "y1_warp", "z1", "z2"):
        v = aux[k] if k[0] == "y" else aux[k] - sd[f"entropy_bottleneck{k[1]}.quantiles"][:, 0, 1].view(1, -1, 1, 1)
        assert int(tie_zone(v).sum()) == 0 and int(tie_zone(v, eps=2e-4).sum()) == 0, k
        assert torch.equal(aux[k], plain["_aux"][k])
    for k in ("x1_hat", "x2_hat", "y1_hat", "z1_hat"):
        assert torch.equal(banded[k], plain[k]), k
    for k in ("z1", "z2"):
        assert torch.equal(banded["likelihoods"][k], plain["likelihoods"][k])
    for k, name in (("y1", "ctx1"), ("y2", "ctx2")):
        a, b = aux[name], plain["_aux"][name]
        assert torch.equal(a[:, :, :S], b[:, :, :S]) and not torch.equal(a[:, :, S:S + 2], b[:, :, S:S + 2])       # band 0 is the latent's top
        assert not torch.equal(banded["likelihoods"][k], plain["likelihoods"][k])
        assert torch.equal(again["likelihoods"][k], plain["likelihoods"][k])                                     # the wrapping is undone
        # each band of the banded context is the plain context model of that band cut out
        w = O.masked_weight(sd[f"context_prediction{k[1]}.weight"])
        for r0, r1 in R.bands(8, S):
            cut = torch.nn.functional.conv2d(torch.round(aux[k][:, :, r0:r1]), w, sd[f"context_prediction{k[1]}.bias"], padding=2)
            assert torch.equal(a[:, :, r0:r1], cut)
