"""Encoder-side latent refinement (masic_amd/refine.py), the parts that need no GPU: RefineConfig's validation, the host-side argument
checks of the entry points of include/masic_refine.h (the header itself is a row of tests/test_cpu_side_headers.py), the CPU restatement
of the loop on the tiny fixture (tests/refine_ref.py on oracle/hsic_oracle.py) and the admissibility of the fixture the GPU gradient test
compares on."""
import ctypes

import numpy as np
import pytest
import torch

from tests import refine_ref as R


# ---------------------------------------------------------------------------------------------------------------- RefineConfig
def test_config_defaults_are_off():
    from masic_amd.refine import DEFAULT_LR, RefineConfig
    c = RefineConfig()
    assert (c.steps, c.lr, c.check_every, c.seed, c.pair_keys, c.lmbda) == (0, DEFAULT_LR, 5, 0, None, None)
    assert c.keys_for(3) == [0, 1, 2]
    assert RefineConfig(steps=7, pair_keys=[5, 2 ** 32 - 1]).keys_for(2) == [5, 2 ** 32 - 1]


@pytest.mark.parametrize("kw", [dict(steps=-1), dict(steps=1.5), dict(steps=True), dict(lr=0), dict(lr=-0.1), dict(lr=float("nan")),
                                dict(lr=float("inf")), dict(check_every=0), dict(check_every=2.0), dict(seed=-1), dict(seed=2 ** 32),
                                dict(pair_keys=[0, -1]), dict(pair_keys=[2 ** 32]), dict(pair_keys=[0.5]), dict(lmbda=0), dict(lmbda=-1.0)])
def test_config_refuses(kw):
    from masic_amd.refine import RefineConfig
    with pytest.raises(ValueError, match="RefineConfig"):
        RefineConfig(**kw)


def test_config_pair_keys_must_match_the_batch():
    from masic_amd.refine import RefineConfig
    with pytest.raises(ValueError, match="pair keys"):
        RefineConfig(pair_keys=[1, 2]).keys_for(3)


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_bad_arguments_launch_nothing():
    """the argument checks are host code: a null pointer array, B out of range"""
    from masic_amd import _lib
    lib = _lib.lib
    four = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    n = (ctypes.c_size_t * 4)(1, 1, 1, 1)
    assert lib.masic_refine_noise(None, n, 1, 0, None, None, None) != 0
    assert lib.masic_refine_noise(four, n, 0, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None) != 0
    assert lib.masic_refine_noise(four, n, 70000, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None) != 0
    assert lib.masic_refine_adam(four, four, four, None, n, 1, 0.1, ctypes.c_void_p(16), None) != 0
    assert lib.masic_refine_keep_best(four, four, n, 1, None, None, None) != 0
    assert b"refine_keep_best" in lib.masic_last_error()


# ---------------------------------------------------------------------------------------------------------------- the restatements
def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32-10 (kat_vectors: zero, all-ones and the pi digits)"""
    got = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(w) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    got = R.philox4x32_10(f, f, f, f, f, f)
    assert [int(w) for w in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = R.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(w) for w in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_philox_noise_range_and_keying():
    u = R.philox_noise(4096, 0, 1, 0, 0)
    assert u.dtype == np.float32 and u.min() >= -0.5 and u.max() < 0.5 and abs(float(u.mean())) < 0.02
    assert abs(float(u.var()) - 1.0 / 12.0) < 0.01
    for other in (R.philox_noise(4096, 1, 1, 0, 0), R.philox_noise(4096, 0, 2, 0, 0), R.philox_noise(4096, 0, 1, 1, 0),
                  R.philox_noise(4096, 0, 1, 0, 1)):
        assert abs(float(np.corrcoef(u, other)[0, 1])) < 0.06                     # tensor id, step, seed and pair key each give another stream
    assert np.array_equal(R.philox_noise(100, 2, 3, 4, 5), R.philox_noise(4096, 2, 3, 4, 5)[:100])     # an element's value is its index's


def _encoder_latents(c):
    from oracle import hsic_oracle as O
    sd = c["sd"]
    H, W = c["x1"].shape[-2:]
    with torch.no_grad():
        y1 = O.encoder1(c["x1"], sd)
        y2 = O.encoder2(O.warp_perspective(c["x1"], c["h_matrix"], (H, W)), c["x2"], sd)
        return [y1, y2, O.hyper_analysis(y1, sd, "_h_a1"), O.hyper_analysis(y2, sd, "_h_a2")]


def test_oracle_loop_lowers_the_true_objective():
    """The loop of refine_latents restated on the CPU oracle, hsic_tiny (HSIC(16,24,3), 1 x 3 x 64 x 64, lmbda 0.01), Philox noise,
    Adam lr 0.1, 100 steps, the true objective every 5: it ends below its start.  Recorded here: cost_best / cost_start = 0.9622
    (0.962 was seen with torch's CPU noise), and the true objective fell at each of the 20 checks."""
    torch.manual_seed(0)
    c = R.tiny_case(B=1)
    start, best, trace = R.oracle_loop(c["sd"], _encoder_latents(c), c["x1"], c["x2"], c["h_matrix"], c["K"], c["lmbda"], steps=100, lr=0.1,
                                       check_every=5)
    ratio = float(best[0] / start[0])
    print(f"oracle loop: cost_start {start[0]:.4f}  cost_best {best[0]:.4f}  ratio {ratio:.4f}  checks {len(trace) - 1}")
    assert len(trace) == 21 and np.isfinite(trace).all()
    assert best[0] < start[0]
    assert best[0] == min(float(t[0]) for t in trace)


def test_fixture_is_admissible():
    """The fixture of the GPU gradient test (refine_ref.tiny_case at LATENT_SEED, B = 2): every y, every z - median and the oracle's
    y1_warp is at least 1e-3 from a rounding tie, and the oracle's float32 and float64 roundings agree -- so the float32 kernels and
    the float64 oracle differentiate the same piecewise-smooth function."""
    c32, c64 = R.tiny_case(2, torch.float32), R.tiny_case(2, torch.float64)
    outs = []
    for c in (c32, c64):
        with torch.no_grad():
            outs.append(R.forward_from_latents(c["sd"], *c["lat"], c["x1"], c["h_matrix"], None, c["K"]))
    med = [c64["sd"][f"entropy_bottleneck{v}.quantiles"][:, 0, 1].view(1, -1, 1, 1) for v in (1, 2)]
    y1, y2, z1, z2 = c64["lat"]
    for name, t in (("y1", y1), ("y2", y2), ("z1 - median", z1 - med[0]), ("z2 - median", z2 - med[1]), ("y1_warp", outs[1]["y1_warp"]),
                    ("y1_warp (float32)", outs[0]["y1_warp"])):
        assert R.tie_distance(t) >= 1e-3, f"{name}: {R.tie_distance(t):.2e} from a tie at LATENT_SEED {R.LATENT_SEED}"
    assert torch.equal(torch.round(outs[0]["y1_warp"]).double(), torch.round(outs[1]["y1_warp"]))
    for k in range(4):
        assert torch.equal(torch.round(c32["lat"][k]).double(), torch.round(c64["lat"][k]))
    for v in (0, 1):
        assert torch.equal(torch.round(c32["lat"][2 + v] - med[v].float()).double(), torch.round(c64["lat"][2 + v] - med[v]))


def test_surrogate_gradient_is_the_objectives():
    """the float64 oracle graph against central differences of its own surrogate in a few coordinates (round is flat between ties, so
    the identity-gradient terms are taken out: the likelihood points y + u, z + u and nothing else are moved)"""
    c = R.tiny_case(2, torch.float64)
    shapes = [tuple(t.shape) for t in c["lat"]]
    noise = [torch.from_numpy(u).double() for u in R.step_noise(shapes, R.NOISE_STEP, R.NOISE_SEED, [0, 1])]
    grads, J, _ = R.latent_grads(c["sd"], c["lat"], c["x1"], c["x2"], c["h_matrix"], noise, c["K"], c["lmbda"])
    assert J.shape == (2,) and bool(torch.isfinite(J).all())
    for g, t in zip(grads, c["lat"]):
        assert g.shape == t.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # moving the noise by eps moves only the likelihood point: d J / d u_k is the likelihood part of d J / d latent_k; for z nothing else
    # of z's gradient is smooth-and-nonzero except the identity-gradient path, so compare the likelihood part through a second graph
    # float64 J ~ 5e2: the rounding of the difference quotient is ~ 5e2 * 2^-52 / eps = 1e-9 at eps = 1e-4, its truncation ~ eps^2
    eps = 1e-4
    for k, idx in ((0, (1, 3, 2, 1)), (1, (0, 7, 0, 3)), (2, (1, 3, 0, 0))):
        def cost(delta):
            n2 = [u.clone() for u in noise]
            n2[k][idx] += delta
            with torch.no_grad():
                return float(R.pair_costs(R.forward_from_latents(c["sd"], *c["lat"], c["x1"], c["h_matrix"], n2, c["K"]), c["x1"], c["x2"],
                                          c["lmbda"]).sum())
        fd = (cost(eps) - cost(-eps)) / (2 * eps)
        leaves = [u.clone().requires_grad_(True) for u in noise]
        out = R.forward_from_latents(c["sd"], *c["lat"], c["x1"], c["h_matrix"], leaves, c["K"])
        an = float(torch.autograd.grad(R.pair_costs(out, c["x1"], c["x2"], c["lmbda"]).sum(), leaves[k])[0][idx])
        assert abs(fd - an) <= 1e-4 * abs(an) + 1e-7, (k, fd, an)
