"""GPU tests (-m gpu) of the encoder-side latent refinement (masic_amd/refine.py, masic_amd/csrc/refine.hip, HSIC._forward_refine,
HSIC.compress(latents=), StereoCodec(refine=)) against the CPU restatements of tests/refine_ref.py."""
import os

import numpy as np
import pytest
import torch

from tests import refine_ref as R
from tests.util import GOLDEN, assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1025)
_CACHE = {}


def _others(n):
    """the per-pair lengths of the four tensors of one launch: n and three more of the list, so that one launch mixes lengths"""
    i = LENGTHS.index(n)
    return [LENGTHS[(i + d) % len(LENGTHS)] for d in (0, 1, 3, 6)]


def _tensor(B, n, shift, fill=None):
    """contiguous float32 [B, n] on the device whose first element sits `shift` floats past a 16-byte boundary"""
    buf = torch.zeros(B * n + 8, dtype=torch.float32, device=DEV)
    base = (buf.data_ptr() // 4) % 4
    off = (shift - base) % 4
    t = buf[off:off + B * n].view(B, n)
    assert (t.data_ptr() // 4) % 4 == shift and t.is_contiguous()
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)).view(B, n))
    return t


def _step(value):
    return torch.tensor([value], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. the elementwise kernels
@pytest.mark.parametrize("n", LENGTHS)
def test_noise_is_the_numpy_philox(n):
    from masic_amd import refine
    seed, step, keys = 0x9E3779B9, 7, [5, 2 ** 32 - 1, 123456789]
    ns = _others(n)
    got = {}
    for B in (1, 3):
        outs =[_tensor(B, m, shift) for m, shift in zip(ns, (0, 1, 2, 3))]
        refine.noise(outs, seed, refine.pair_keys_tensor(keys[:B], DEV), _step(step))
        got[B] = [o.cpu().numpy() for o in outs]
        for t, (o, m) in enumerate(zip(got[B], ns)):
            want = np.stack([R.philox_noise(m, t, step, seed, k) for k in keys[:B]])
            assert o.dtype == np.float32 and np.array_equal(o, want), (B, t, m)
            assert o.min() >= -0.5 and o.max() < 0.5
    for t in range(4):
        assert np.array_equal(got[1][t][0], got[3][t][0])               # pair 0 under the same key: the same noise at B = 1 and B = 3
    # a pair's noise follows its key, not its position
    outs = [_tensor(1, m, 0) for m in ns]
    refine.noise(outs, seed, refine.pair_keys_tensor(keys[2:3], DEV), _step(step))
    for t in range(4):
        assert np.array_equal(outs[t].cpu().numpy()[0], got[3][t][2])


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_adam_three_steps(n, B):
    """three steps against the float64 restatement: 1e-6 of the tensor's magnitude -- a few float32 roundings per element and step"""
    from masic_amd import refine
    rng = np.random.RandomState(1000 * B + n)
    ns = _others(n)
    lr = 0.1
    # tensors 0, 1: the four arrays aligned alike (vector path); 2, 3: aligned differently (the scalar path throughout)
    shifts = [(0, 0, 0, 0), (3, 3, 3, 3), (0, 1, 0, 0), (2, 2, 2, 1)]
    p0 = [rng.standard_normal((B, m)) * 3 for m in ns]
    p = [_tensor(B, m, s[0], a) for m, s, a in zip(ns, shifts, p0)]
    m_ = [_tensor(B, m, s[2]) for m, s in zip(ns, shifts)]
    v_ = [_tensor(B, m, s[3]) for m, s in zip(ns, shifts)]
    ref = [(a.astype(np.float32).astype(np.float64), np.zeros((B, m)), np.zeros((B, m))) for a, m in zip(p0, ns)]
    step = _step(0)
    for t in (1, 2, 3):
        g0 = [rng.standard_normal((B, m)) * 10.0 ** rng.randint(-3, 2) for m in ns]
        g = [_tensor(B, m, s[1], a) for m, s, a in zip(ns, shifts, g0)]
        step.add_(1)
        refine.adam(p, g, m_, v_, lr, step)
        ref = [R.adam_step(r[0], a.astype(np.float32).astype(np.float64), r[1], r[2], lr, t) for r, a in zip(ref, g0)]
    for k in range(4):
        for name, got, want in (("p", p[k], ref[k][0]), ("m", m_[k], ref[k][1]), ("v", v_[k], ref[k][2])):
            e = rel_err(got.cpu(), torch.from_numpy(want))
            assert e <= 1e-6, (name, k, ns[k], e)


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_keep_best_is_exact(n, B):
    from masic_amd import refine
    rng = np.random.RandomState(7 * B + n)
    ns = _others(n)
    cur0 = [rng.standard_normal((B, m)).astype(np.float32) for m in ns]
    best0 = [rng.standard_normal((B, m)).astype(np.float32) for m in ns]
    cases = [("none improves", np.full(B, 2.0), np.full(B, 1.0)), ("equal is no improvement", np.full(B, 1.0), np.full(B, 1.0)),
             ("nan never wins", np.full(B, np.nan), np.full(B, 1.0)), ("all improve", np.full(B, 0.5), np.full(B, 1.0))]
    if B == 3:
        cases.append(("the middle pair only", np.array([2.0, 0.25, 1.0]), np.array([1.0, 1.0, 1.0])))
        cases.append(("the outer pairs", np.array([0.5, 3.0, -1.0]), np.array([1.0, 1.0, 1.0])))
    for what, now, jb in cases:
        cur = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 2, 3), cur0)]
        best = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 0, 3), best0)]          # tensor 2: cur and best aligned differently
        j_now, j_best = torch.from_numpy(now).to(DEV), torch.from_numpy(jb.copy()).to(DEV)
        refine.keep_best(cur, best, j_now, j_best)
        take = now < jb
        assert np.array_equal(j_best.cpu().numpy(), np.where(take, now, jb)), what
        for k in range(4):
            want = np.where(take[:, None], cur0[k], best0[k])
            assert np.array_equal(best[k].cpu().numpy(), want), (what, k)
            assert np.array_equal(cur[k].cpu().numpy(), cur0[k]), (what, k)


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_rd_seeds_closed_forms(n, B):
    from masic_amd import refine
    rng = np.random.RandomState(31 * B + n)
    ns = _others(n)
    lmbda, hw = 0.0125, 37.0
    pics = [rng.uniform(0, 1, (B, n)).astype(np.float32) for _ in range(4)]
    liks = [rng.uniform(1e-6, 1.0, (B, m)).astype(np.float32) for m in ns]
    for g in (None, rng.uniform(0.5, 2.0, B)):
        tp = [_tensor(B, n, s, a) for s, a in zip((1, 1, 0, 0), pics)]
        tl = [_tensor(B, m, s, a) for m, s, a in zip(ns, (0, 1, 2, 3), liks)]
        g1, g2, gl = refine.rd_seeds(tp[0], tp[1], tp[2], tp[3], tl, lmbda, hw, None if g is None else torch.from_numpy(g).to(DEV))
        gg = np.ones(B) if g is None else g
        pd = [a.astype(np.float64) for a in pics]
        want1 = gg[:, None] * 2 * lmbda * 255.0 ** 2 * (pd[0] - pd[1]) / n
        want2 = gg[:, None] * 2 * lmbda * 255.0 ** 2 * (pd[2] - pd[3]) / n
        assert rel_err(g1.cpu(), torch.from_numpy(want1)) <= 1e-6 and rel_err(g2.cpu(), torch.from_numpy(want2)) <= 1e-6
        for k in range(4):
            want = -gg[:, None] / (np.log(2.0) * hw * liks[k].astype(np.float64))
            err = float(np.max(np.abs(gl[k].cpu().numpy().astype(np.float64) - want) / np.abs(want)))       # every element to 1e-6 of itself
            assert err <= 1e-6, (k, err)


def test_kernel_wrappers_refuse():
    from masic_amd import refine
    t = [torch.zeros(2, 5, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="four tensors"):
        refine.noise(t[:3], 0, refine.pair_keys_tensor([0, 1], DEV), _step(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.noise([x.cpu() for x in t], 0, refine.pair_keys_tensor([0, 1], DEV), _step(1))
    with pytest.raises(RuntimeError, match="pair_keys"):
        refine.noise(t, 0, refine.pair_keys_tensor([0], DEV), _step(1))
    with pytest.raises(RuntimeError, match="shapes"):
        refine.adam(t, t[:3] + [torch.zeros(2, 6, device=DEV)], t, t, 0.1, _step(1))
    with pytest.raises(RuntimeError, match="j_now"):
        refine.keep_best(t, t, torch.zeros(2, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ the tiny model
def _tiny_net(prec):
    import MASIC
    from masic_amd import nn as mnn
    from tests.util import golden_state_dict, load_npz
    mnn.set_precision(prec)
    fx = load_npz("hsic_tiny.npz")
    N, M, K = (int(v) for v in fx["NMK"])
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(golden_state_dict(fx, net.state_dict()))
    net = net.to(DEV).eval()
    net.update()
    return net


def _snapshot(net):
    # (every forward of a context model first zeroes its masked taps in place, as the reference does: taken after that)
    net.context_prediction1.zero_masked_taps()
    net.context_prediction2.zero_masked_taps()
    return ({k: v.detach().clone() for k, v in net.state_dict().items()}, [p.requires_grad for _, p in net.named_parameters()],
            net.training, torch.get_rng_state().clone(), torch.cuda.get_rng_state(0).clone())


def _assert_untouched(net, snap):
    sd, flags, training, cpu_rng, dev_rng = snap
    for name, p in net.named_parameters():
        assert p.grad is None, name
    assert [p.requires_grad for _, p in net.named_parameters()] == flags
    assert net.training == training
    now = net.state_dict()
    assert set(now) == set(sd)
    for k, v in sd.items():
        assert torch.equal(now[k], v), k
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(0), dev_rng)


# ------------------------------------------------------------------------------------------------ 2. gradient parity
def test_gradient_parity_with_the_float64_oracle():
    """d sum_b J_b / d (y1, y2, z1, z2) of HSIC._forward_refine (f32 operands) against the float64 oracle graph of tests/refine_ref.py:
    HSIC(16,24,3), B = 2, 64 x 64, hsic_tiny weights, given latents (admissible: tests/test_cpu_refine.py), given Philox noise."""
    from masic_amd import nn as mnn, refine
    from masic_amd.homography import warp_matrices
    try:
        net = _tiny_net("f32")
        next(iter(net.parameters())).requires_grad_(False)          # a flag that differs from the default must come back as it was
        c = R.tiny_case(2, torch.float64)
        shapes = [tuple(t.shape) for t in c["lat"]]
        noise_np = R.step_noise(shapes, R.NOISE_STEP, R.NOISE_SEED, [0, 1])
        want, J_want, _ = R.latent_grads(c["sd"], c["lat"], c["x1"], c["x2"], c["h_matrix"], [torch.from_numpy(u).double() for u in noise_np],
                                        c["K"], c["lmbda"])
        x1, x2, hm = (c[k].float().to(DEV) for k in ("x1", "x2", "h_matrix"))
        lat = [t.float().to(DEV).contiguous() for t in c["lat"]]
        noise = [torch.empty_like(t) for t in lat]
        refine.noise(noise, R.NOISE_SEED, refine.pair_keys_tensor([0, 1], DEV), _step(R.NOISE_STEP))
        for u, w in zip(noise, noise_np):
            assert np.array_equal(u.cpu().numpy(), w)
        m_fwd, m_back = warp_matrices(hm, (64, 64), (64, 64), want_inverse=True)
        snap = _snapshot(net)
        grads, J = refine.surrogate_grads(net, lat, x1, x2, m_fwd, m_back, noise, c["lmbda"])
        torch.cuda.synchronize()
        _assert_untouched(net, snap)
        print("J", J.cpu().numpy(), "oracle", J_want.numpy())
        assert_close(J.cpu(), J_want, "J")
        for name, g, w in zip(("y1", "y2", "z1", "z2"), grads, want):
            e = assert_close(g.cpu(), w, f"d J / d {name}")
            print(f"d J / d {name}: relative error {e:.2e}, magnitude {float(w.abs().max()):.3e}")
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------------ 3. the loop
def _loop_case():
    """refine_latents on the tiny fixture, B = 2, lr 0.1, 100 steps (run twice), and the oracle loop from the same start with the same
    noise: computed once for the tests below"""
    if "loop" not in _CACHE:
        from masic_amd import nn as mnn, refine
        try:
            net = _tiny_net("f32")
            c = R.tiny_case(2, torch.float32)
            x1, x2, hm = (c[k].to(DEV) for k in ("x1", "x2", "h_matrix"))
            snap = _snapshot(net)
            cfg = refine.RefineConfig(steps=100, lr=0.1, check_every=5, seed=3)
            start = refine.refine_latents(net, x1, x2, hm, c["lmbda"], refine.RefineConfig())
            a = refine.refine_latents(net, x1, x2, hm, c["lmbda"], cfg)
            b = refine.refine_latents(net, x1, x2, hm, c["lmbda"], cfg)
            torch.cuda.synchronize()
            _assert_untouched(net, snap)
            o_start, o_best, _ = R.oracle_loop(c["sd"], [t.cpu() for t in start[:4]], c["x1"], c["x2"], c["h_matrix"], c["K"], c["lmbda"],
                                               steps=100, lr=0.1, check_every=5, seed=3)
            _CACHE["loop"] = dict(net=net, c=c, start=start, a=a, b=b, o_start=o_start, o_best=o_best, x=(x1, x2, hm))
        finally:
            mnn.set_precision("f32")
    return _CACHE["loop"]


def test_loop_lowers_every_pairs_objective():
    L = _loop_case()
    cs, cb = L["a"].cost_start.cpu().numpy(), L["a"].cost_best.cpu().numpy()
    gain, o_gain = 1.0 - cb / cs, 1.0 - L["o_best"] / L["o_start"]
    print("cost_start", cs, "cost_best", cb, "relative decrease", gain, "| oracle start", L["o_start"], "best", L["o_best"], "decrease", o_gain)
    assert cs.dtype == np.float64 and cs.shape == (2,)
    assert_close(torch.from_numpy(cs), torch.from_numpy(L["o_start"]), "cost_start against the oracle's true objective")
    assert np.array_equal(cs, L["start"].cost_start.cpu().numpy())
    assert (cb <= cs).all()
    assert (cb < cs).all()
    assert (gain >= 0.5 * o_gain).all()                    # half: round-with-identity-gradient lets the two trajectories part at a tie


def test_steps_zero_returns_the_encoders_latents():
    L = _loop_case()
    net, (x1, x2, hm) = L["net"], L["x"]
    with torch.no_grad():
        y1, y2, z1, z2 = net.latents(x1[:1], x2[:1], hm[:1])
    for got, want in zip(L["start"][:4], (y1, y2, z1, z2)):
        assert torch.equal(got[:1], want)
    assert torch.equal(L["start"].cost_start, L["start"].cost_best)


def test_two_identical_calls_are_bit_equal():
    L = _loop_case()
    for k, name in enumerate(("y1", "y2", "z1", "z2", "cost_start", "cost_best")):
        assert torch.equal(L["a"][k], L["b"][k]), name
    assert not torch.equal(L["a"].y1, L["start"].y1)


def test_refine_refuses():
    from masic_amd import nn as mnn, refine
    L = _loop_case()
    net, (x1, x2, hm) = L["net"], L["x"]
    with pytest.raises(ValueError, match="lmbda"):
        refine.refine_latents(net, x1, x2, hm, None, refine.RefineConfig(steps=1))
    with pytest.raises(TypeError, match="RefineConfig"):
        refine.refine_latents(net, x1, x2, hm, 0.01, {"steps": 1})
    with pytest.raises(ValueError, match="multiple of 64"):
        refine.refine_latents(net, x1[..., :48], x2[..., :48], hm, 0.01, refine.RefineConfig(steps=1))
    net.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            refine.refine_latents(net, x1, x2, hm, 0.01, refine.RefineConfig(steps=1))
    finally:
        net.eval()
    try:
        mnn.set_precision("fp8")
        with pytest.raises(NotImplementedError, match="fp8"):
            refine.refine_latents(net, x1, x2, hm, 0.01, refine.RefineConfig(steps=1))
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------------ 4. files
FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")


def _files(path, name):
    return tuple(open(os.path.join(str(path), name + ext), "rb").read() for ext in (".npz", ".bin"))


def test_files_steps_zero_are_todays_files(tmp_path):
    from masic_amd import refine
    L = _loop_case()
    net, (x1, x2, hm) = L["net"], L["x"]
    with torch.no_grad():
        for i in range(2):
            s = (slice(i, i + 1),)
            plain = net.compress(x1[s], x2[s], hm[s], f"plain{i}", str(tmp_path))
            lat = refine.refine_latents(net, x1[s], x2[s], hm[s], 0.01, refine.RefineConfig(steps=0))
            given = net.compress(x1[s], x2[s], hm[s], f"given{i}", str(tmp_path), latents=lat)
            assert _files(tmp_path, f"plain{i}") == _files(tmp_path, f"given{i}")
            for k in FIELDS:
                assert torch.equal(plain[k], given[k]), k
        net.compress_batch(x1, x2, hm, ["bp0", "bp1"], str(tmp_path))
        net.compress_batch(x1, x2, hm, ["bg0", "bg1"], str(tmp_path), latents=tuple(L["start"][:4]))
        for i in range(2):
            assert _files(tmp_path, f"bp{i}") == _files(tmp_path, f"bg{i}") == _files(tmp_path, f"plain{i}")
        with pytest.raises(ValueError, match="latents"):
            net.compress(x1[:1], x2[:1], hm[:1], "bad", str(tmp_path), latents=tuple(L["start"][:3]))
        with pytest.raises(ValueError, match="shape"):
            net.compress(x1[:1], x2[:1], hm[:1], "bad", str(tmp_path), latents=tuple(L["start"][:4]))          # B = 2 latents, one pair


def test_files_from_refined_latents_round_trip(tmp_path):
    """steps = 20: the file decodes with today's decompress, to the pictures compress returned, bit for bit; the same through
    compress_batch at B = 2"""
    from masic_amd import refine
    L = _loop_case()
    net, (x1, x2, hm) = L["net"], L["x"]
    cfg = refine.RefineConfig(steps=20, lr=0.1)
    with torch.no_grad():
        one = refine.refine_latents(net, x1[:1], x2[:1], hm[:1], 0.01, cfg)
        assert not torch.equal(one.y1, L["start"].y1[:1])
        enc = net.compress(x1[:1], x2[:1], hm[:1], "r", str(tmp_path), latents=one)
        dec = net.decompress(None, None, hm[:1], "r", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
        assert torch.equal(enc["y1_hat"], torch.round(one.y1)) and torch.equal(enc["y2_hat"], torch.round(one.y2))
        two = refine.refine_latents(net, x1, x2, hm, 0.01, cfg)
        encb = net.compress_batch(x1, x2, hm, ["r0", "r1"], str(tmp_path), latents=two)
        decb = net.decompress_batch(["r0", "r1"], hm, str(tmp_path))
        for k in FIELDS:
            assert torch.equal(encb[k], decb[k]), k
        d1 = net.decompress(None, None, hm[1:2], "r1", str(tmp_path))
        assert torch.equal(d1["x1_hat"], encb["x1_hat"][1:2]) and torch.equal(d1["x2_hat"], encb["x2_hat"][1:2])


def test_full_width_bf16_never_worse_and_exact_round_trip(tmp_path):
    """once at HSIC(128,192,5), 2 x 128 x 128, bf16 operands: the F16K kernel families (AnalysisFn, SynthesisFn, GmmHeadsFn with frozen
    weights); never worse than the start, and the files of the refined latents decode exactly"""
    import MASIC
    from masic_amd import nn as mnn, refine, synth
    try:
        mnn.set_precision("bf16")
        net = MASIC.HSIC(128, 192, 5)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=21))
        net = net.to(DEV).eval()
        net.update()
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(2, 128, 128, seed=21))
        snap = _snapshot(net)
        out = refine.refine_latents(net, x1, x2, hm, 0.01, refine.RefineConfig(steps=10, lr=0.1, check_every=5))
        torch.cuda.synchronize()
        _assert_untouched(net, snap)
        cs, cb = out.cost_start.cpu().numpy(), out.cost_best.cpu().numpy()
        print("bf16 full width: cost_start", cs, "cost_best", cb)
        assert np.isfinite(cs).all() and np.isfinite(cb).all() and (cb <= cs).all()
        with torch.no_grad():
            enc = net.compress_batch(x1, x2, hm, ["a", "b"], str(tmp_path), latents=out)
            dec = net.decompress_batch(["a", "b"], hm, str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------------ 5. StereoCodec
def test_stereo_codec_refine(tmp_path):
    """StereoCodec(refine=RefineConfig(steps=10)): encode writes .msf files the unmodified decode reads; refine=None (and steps=0) writes
    the files of a codec built without the argument, byte for byte"""
    from masic_amd import StereoCodec, nn as mnn, refine
    from masic_amd.align import PatchAligner
    from masic_amd import synth
    try:
        net = _tiny_net("f32")
        udh = PatchAligner().to(DEV).eval()
        a, b, _ = synth.synth_inputs(2, 72, 100, seed=5)
        u8 = lambda x: torch.from_numpy(np.ascontiguousarray(np.rint(x.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).to(DEV)
        left, right = u8(a), u8(b)
        plain, none, zero, ref = (tmp_path / n for n in ("plain", "none", "zero", "ref"))
        for d in (plain, none, zero, ref):
            d.mkdir()
        names = ["p", "q"]
        StereoCodec(net, udh).encode(left, right, names, str(plain))
        StereoCodec(net, udh, refine=None).encode(left, right, names, str(none))
        StereoCodec(net, udh, refine=refine.RefineConfig(steps=0)).encode(left, right, names, str(zero))
        msf = lambda d, n: open(os.path.join(str(d), n + ".msf"), "rb").read()
        for n in names:
            assert msf(plain, n) == msf(none, n) == msf(zero, n)
        enc = StereoCodec(net, udh, refine=refine.RefineConfig(steps=10, lmbda=0.01)).encode(left, right, names, str(ref))
        dec = StereoCodec(net).decode(names, str(ref))
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert torch.equal(dec["x1_hat"], enc["x1_hat"]) and torch.equal(dec["x2_hat"], enc["x2_hat"])
        assert any(msf(ref, n) != msf(plain, n) for n in names)
        with pytest.raises(ValueError, match="lmbda"):
            StereoCodec(net, udh, refine=refine.RefineConfig(steps=3))
        with pytest.raises(TypeError, match="RefineConfig"):
            StereoCodec(net, udh, refine=10)
    finally:
        mnn.set_precision("f32")
