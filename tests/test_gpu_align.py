"""GPU tests (-m gpu) of the weight-free patch aligner (masic_amd/align.py, masic_amd/csrc/align.hip): the one-launch kernel against
the float64 restatement of tests/align_ref.py and against ground truth, its determinism, its guards, and a .msf file encoded with it.

TOL is 4 x the largest |delta_gpu - delta_f64| measured on the MI355X over the case list of test_kernel_matches_the_restatement
(DESIGN.md section 8.8); it has to stay below 1/128 px, half the 1/64 px step in which the file format stores the offsets."""
import gc
import os

import numpy as np
import pytest
import torch

from tests import align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 0.05                        # px, mean corner error against ground truth
TOL = 9.2e-5                      # px: 4 x the 2.28e-5 px measured (P = 128, translation 40, jitter 8); see the module docstring
_CACHE = {}

# (P, sigma, tmax, jitter, seeds): B = 3 and B = 1 at every patch size
SEARCH_CASES = [(128, 2.5, 40, 8, (0, 1, 2)), (128, 4.0, 16, 4, (3,)), (64, 2.5, 16, 3, (0, 1, 2)), (64, 4.0, 20, 0, (3,)),
                (32, 2.5, 8, 2, (0, 1, 2)), (32, 2.5, 10, 0, (3,))]
START_CASES = [(128, 4.0, 0, 8, (0, 1, 2)), (64, 2.5, 0, 4, (3,)), (32, 2.5, 0, 2, (0, 1, 2))]      # stage 2 alone from delta0 = 0


@pytest.fixture(scope="module", autouse=True)
def _leave_the_device_as_found():
    """After the module: drop the cached cases and return to the driver the device memory these tests leave in torch's caching
    allocator (patches holding NaN and Inf, the captured graph's pool, blocks of the side stream)."""
    yield
    _CACHE.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _align():
    from masic_amd import align
    return align


def _set(P, sigma, tmax, jitter, seeds, search):
    """(a, b, truth, delta_f64, info_f64) of one case; with the search, the items whose best and second-best search costs differ by
    less than 1 % are rejected here, on the CPU"""
    key = (P, sigma, tmax, jitter, seeds, search)
    if key not in _CACHE:
        a, b, truth = R.make_set(P, (sigma,), tmax, jitter, seeds)
        delta, info, costs = R.align(a, b, None if search else torch.zeros_like(truth))
        if search:
            keep = R.search_margin(costs) >= 0.01
            assert bool(keep.any()), f"every item of {key} has a near-tie in its search"
            a, b, truth, delta, info = a[keep], b[keep], truth[keep], delta[keep], info[keep]
        _CACHE[key] = (a, b, truth, delta, info)
    return _CACHE[key]


def _run(a, b, delta0=None, **kw):
    delta, info = _align().align_patches(a.to(DEV), b.to(DEV), None if delta0 is None else delta0.float().to(DEV), **kw)
    return delta.cpu(), info.cpu()


# ------------------------------------------------------------------------------------------ 1. kernel against restatement
def test_kernel_matches_the_restatement():
    worst = 0.0
    for search, cases in ((True, SEARCH_CASES), (False, START_CASES)):
        for case in cases:
            a, b, truth, want, winfo = _set(*case, search)
            got, info = _run(a, b, None if search else torch.zeros_like(truth))
            d = float((got.double() - want).abs().max())
            print(f"P {case[0]} sigma {case[1]} tmax {case[2]} jitter {case[3]} B {a.shape[0]} search {search}: max |delta_gpu - delta_f64| "
                  f"{d:.3e} px, status {info[:, 3].tolist()} (f64 {winfo[:, 3].tolist()})")
            assert torch.equal(info[:, 3].double(), winfo[:, 3]) and winfo[:, 3].eq(0).all()
            # the figures of info: a pixel on the border of validity may fall either way in float32 (two of them: 2 / P^2 of the
            # fraction, and with them a percent of a mean over a thousand pixels)
            assert torch.allclose(info[:, :2].double(), winfo[:, :2], rtol=1e-2, atol=1e-9)
            assert float((info[:, 2].double() - winfo[:, 2]).abs().max()) <= 2.0 / case[0] ** 2
            worst = max(worst, d)
    print(f"worst {worst:.3e} px; TOL {TOL:.3e} px")
    assert TOL <= 1.0 / 128
    assert worst <= TOL


# ------------------------------------------------------------------------------------------ 2. ground truth, photometric loss
@pytest.mark.parametrize("tmax,jitter", [(16, 4), (32, 4), (40, 8), (45, 0), (0, 8)])
def test_ground_truth_and_photometric_loss(tmax, jitter):
    from masic_amd import ops
    a, b, truth = R.make_set(128, (2.5, 4.0), tmax, jitter, (0, 1))
    start = None if tmax else torch.zeros_like(truth)                    # the +-8 set is stage 2 alone, as on the CPU
    delta, info = _run(a, b, start)
    err = R.corner_error(delta, truth)
    print(f"tmax {tmax} jitter {jitter}: mean corner error per case", [f"{e:.4f}" for e in err.tolist()])
    assert info[:, 3].eq(0).all() and float(err.max()) <= CAP
    if tmax:                                                             # the translation sets: the loss the net is trained on
        s = R.square(128, torch.float32).to(DEV)[None]
        for i in range(a.shape[0]):
            ai, bi = a[i:i + 1].to(DEV), b[i:i + 1].to(DEV)
            at = [float(ops.udh_photo_loss(ai, ops.udh_photo_matrix(s, d.contiguous(), (128, 128), (128, 128)), bi))
                  for d in (delta[i:i + 1].to(DEV), torch.zeros((1, 4, 2), device=DEV))]
            print(f"  item {i}: photometric loss {at[0]:.4f} at the result, {at[1]:.4f} at delta = 0")
            assert at[0] < at[1]


# ------------------------------------------------------------------------------------------ 3. determinism
def _mixed_batch(P):
    """five pairs: three that align (status 0), a constant one and one with a NaN (status 1)"""
    a, b, _, _, _ = _set(P, 2.5, P // 4, 2, (0, 1, 2), True)
    assert a.shape[0] == 3
    flat = torch.full_like(a[:1], 0.5)
    bad = a[:1].clone()
    bad[0, 0, P // 2, 3] = float("nan")
    return torch.cat((a[:1], flat, a[1:2], bad, a[2:])), torch.cat((b[:1], flat, b[1:2], b[:1], b[2:]))


@pytest.mark.parametrize("P", [32, 64, 128])
def test_bits_depend_on_neither_the_call_nor_the_batch(P):
    a, b = _mixed_batch(P)
    d5, i5 = _run(a, b)
    again = _run(a, b)
    assert i5[:, 3].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
    assert torch.equal(d5, again[0]) and torch.equal(i5.view(torch.int32), again[1].view(torch.int32))
    for i in range(5):
        d1, i1 = _run(a[i:i + 1], b[i:i + 1])
        assert torch.equal(d1[0], d5[i]) and torch.equal(i1.view(torch.int32)[0], i5.view(torch.int32)[i]), i
    order = [4, 0, 3]
    d3, _ = _run(a[order], b[order])
    assert torch.equal(d3, d5[order])


def test_one_captured_graph_replayed_on_new_inputs_gives_the_eager_bits():
    align = _align()
    a1, b1 = _mixed_batch(128)
    order = [3, 4, 0, 2, 1]
    a2, b2 = a1[order].contiguous(), b1[order[::-1]].contiguous()      # other pairs, related or not, in the same buffers
    sa, sb = a1.to(DEV), b1.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        align.align_patches(sa, sb)                       # the LDS opt-in and the allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        delta, info = align.align_patches(sa, sb)
    for a, b in ((a1, b1), (a2, b2)):
        sa.copy_(a)
        sb.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        want, winfo = _run(a, b)
        assert torch.equal(delta.cpu(), want) and torch.equal(info.cpu().view(torch.int32), winfo.view(torch.int32))


# ------------------------------------------------------------------------------------------ 4. guards
@pytest.mark.parametrize("P", [32, 128])
def test_guards(P):
    a, b, truth, _, _ = _set(P, 2.5, P // 4, 2, (0, 1, 2), True)
    flat = torch.full_like(a, -0.75)
    delta, info = _run(flat, flat)
    assert info[:, 3].eq(1).all() and delta.eq(0).all()
    delta, info = _run(a, a)
    assert info[:, 3].eq(0).all() and float(delta.abs().max()) <= 1e-4
    bad = a.clone()
    bad[1, 0, P - 1, P - 1] = float("nan")
    bad[2, 0, 0, 0] = float("inf")
    d0 = truth.float() + 0.25
    delta, info = _run(bad, b, d0)
    assert info[:, 3].tolist() == [0.0, 1.0, 1.0] and torch.equal(delta[1:], d0[1:]) and not torch.equal(delta[0], d0[0])
    delta, info = _run(bad, b)
    assert info[:, 3].tolist() == [0.0, 1.0, 1.0] and delta[1:].eq(0).all()
    d0[2, 0, 0] = float("nan")                                          # a NaN start value comes back as it is
    delta, info = _run(a, b, d0)
    assert info[:, 3].tolist() == [0.0, 0.0, 1.0] and torch.equal(delta[2].view(torch.int32), d0[2].view(torch.int32))


def test_a_start_two_pixels_off_converges():
    a, b, truth = R.make_set(128, (2.5, 4.0), 24, 4, (0, 1))
    delta, info = _run(a, b, truth + 2.0)
    err = R.corner_error(delta, truth)
    print("start = truth + 2 px: mean corner error per case", [f"{e:.4f}" for e in err.tolist()])
    assert info[:, 3].eq(0).all() and float(err.max()) <= CAP


def test_the_module_is_the_function_and_init_supplies_the_start_value():
    align = _align()
    a, b, truth = R.make_set(64, (2.5,), 12, 3, (0, 1))
    a, b, start = a.to(DEV), b.to(DEV), (truth + 1.5).float().to(DEV)

    class Start(torch.nn.Module):
        def forward(self, pa, pb):
            return start.reshape(-1, 8)                                  # the net's own output shape

    plain = align.PatchAligner().eval()
    want, winfo = align.align_patches(a, b)
    assert torch.equal(plain(a, b), want) and torch.equal(plain.last_info, winfo) and len(plain.state_dict()) == 0
    refined = align.PatchAligner(init=Start(), iters=(0, 8, 6)).eval()
    assert len(refined.state_dict()) == 0 and not list(refined.children())      # init is called, not owned
    want, winfo = align.align_patches(a, b, start, iters=(0, 8, 6))
    got = refined(a, b)
    assert torch.equal(got, want) and torch.equal(refined.last_info, winfo) and winfo[:, 3].eq(0).all()
    assert float(R.corner_error(got.cpu(), truth).max()) <= CAP
    with pytest.raises(ValueError, match="P in"):
        align.align_patches(a[:, :, :48, :48].contiguous(), b[:, :, :48, :48].contiguous())
    with pytest.raises(ValueError, match="delta0"):
        align.align_patches(a, b, start[:1])


@pytest.mark.parametrize("shift,frac", [((70.0, 0.0), 58 / 128), ((0.0, -66.0), 62 / 128), ((66.0, 66.0), (62 / 128) ** 2)])
def test_corner_and_valid_fraction_guards_return_the_start_value(shift, frac):
    """A start value that is a translation of the 128-pixel patch.  By 70 px along x (or 66 along y) the start has corners past 3P/2 =
    192 (below -P/2 = -64) with 45 % (48 %) of the pixels valid, so only the corner guard can fire, on the first step's candidate; by
    (66, 66) the valid fraction at the start is (62/128)^2 = 0.235 < 1/4, so the fraction guard fires on the first step whatever
    the candidate is.  Either way: status 1, the start value back exactly, NaN MSEs, fraction 0 -- as in the restatement."""
    a, b, _, _, _ = _set(128, 2.5, 32, 2, (0, 1, 2), True)
    d0 = torch.tensor(shift).expand(3, 4, 2).contiguous()
    assert abs(float(R.masked_mse(a.double()[:, 0], b.double()[:, 0], R.h_from_delta(d0.double(), 128))[1][0]) - frac) < 1e-12
    _, winfo, _ = R.align(a, b, d0)
    assert winfo[:, 3].eq(1).all()
    delta, info = _run(a, b, d0)
    assert info[:, 3].eq(1).all() and torch.equal(delta, d0)
    assert bool(torch.isnan(info[:, :2]).all()) and info[:, 2].eq(0).all()


def _check_start_or_better(delta, info, start):
    """every item: finite offsets; status 1 returns the start value exactly with NaN MSEs and a zero fraction; status 0 or 2 has finite
    figures and an MSE no worse than the start's"""
    seen = set()
    for i in range(delta.shape[0]):
        status = float(info[i, 3])
        seen.add(status)
        assert bool(torch.isfinite(delta[i]).all()), i
        if status == 1.0:
            assert torch.equal(delta[i], start[i]), i
            assert bool(torch.isnan(info[i, :2]).all()) and float(info[i, 2]) == 0.0, (i, info[i].tolist())
        else:
            assert status in (0.0, 2.0), (i, status)
            assert bool(torch.isfinite(info[i]).all()) and float(info[i, 1]) <= float(info[i, 0]), (i, info[i].tolist())
            if status == 2.0:
                assert torch.equal(delta[i], start[i]), i
    return seen


def test_unrelated_textures_end_at_the_start_value_or_better():
    """Six pairs of unrelated textures, all of them launched.  Under the guards of the contract such a pair does not always end with
    status 0 or 2: Gauss-Newton on unrelated content can push a corner out of [-P/2, 3P/2] or the overlap below a quarter, which is
    status 1 (3 of the 6 in the float64 restatement).  These are the inputs that reach those two guards; both outcomes must occur."""
    a = R.make_set(128, (2.5,), 0, 0, range(6))[0]
    b = R.make_set(128, (4.0,), 0, 0, range(10, 16))[1]
    _, winfo, _ = R.align(a, b)
    delta, info = _run(a, b)
    print("unrelated textures: info", info.tolist(), "restatement", winfo.tolist())
    seen = _check_start_or_better(delta, info, torch.zeros_like(delta))
    assert 1.0 in seen and seen - {1.0}, seen
    start = torch.full((6, 4, 2), 0.75)                                  # no search: a guard returns THIS value, not zeros
    delta, info = _run(a, b, start)
    print("unrelated textures from delta0 = 0.75: info", info.tolist())
    _check_start_or_better(delta, info, start)


# ------------------------------------------------------------------------------------------ 5. end to end
def test_msf_files_encoded_with_the_aligner(tmp_path):
    """Two 100 x 150 pairs cut from one texture with a known shift: the files decode with the weights alone, bit for bit, each file is
    the one its pair gives alone, and the coded offsets are the shift in the 256 x 256 resized picture."""
    import MASIC
    from masic_amd import PatchAligner, StereoCodec, stereofile, synth
    net = MASIC.HSIC(32, 48, 3)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31))
    net = net.to(DEV).eval()
    net.update()
    H0, W0 = 100, 150
    shifts = [(6, 2), (-9, 3)]                                          # (x, y) picture pixels: right(u) = left(u + shift)
    tex = R.texture(4.0, 77).numpy()
    u8 = lambda t: np.repeat(np.clip(np.rint(128 + 48 * t), 0, 255).astype(np.uint8)[..., None], 3, axis=-1)
    left = torch.from_numpy(np.stack([u8(tex[100 + 120 * i:100 + 120 * i + H0, 100:100 + W0]) for i in range(2)])).to(DEV)
    right = torch.from_numpy(np.stack([u8(tex[100 + 120 * i + sy:100 + 120 * i + sy + H0, 100 + sx:100 + sx + W0])
                                       for i, (sx, sy) in enumerate(shifts)])).to(DEV)
    sc = StereoCodec(net, PatchAligner().eval())
    both = tmp_path / "both"
    both.mkdir()
    enc = sc.encode(left, right, ["p0", "p1"], str(both))
    dec = StereoCodec(net).decode(["p0", "p1"], str(both))
    assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
    assert torch.equal(dec["h_matrix"], enc["h_matrix"])
    for i, name in enumerate(("p0", "p1")):
        alone = tmp_path / name
        alone.mkdir()
        sc.encode(left[i], right[i], name, str(alone))
        with open(os.path.join(both, name + ".msf"), "rb") as f, open(os.path.join(alone, name + ".msf"), "rb") as g:
            assert f.read() == g.read(), name
    coded = stereofile.dequantise(enc["delta_q"].numpy()).reshape(2, 4, 2)
    want = np.array([[sx * 256.0 / W0, sy * 256.0 / H0] for sx, sy in shifts])[:, None, :]
    print("coded offsets", coded.tolist(), "shift in the resized picture", want.tolist())
    assert np.abs(coded - want).max() <= 0.5
