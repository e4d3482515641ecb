"""GPU tests (-m gpu) of the two kernels of masic_amd/csrc/codec.hip at the edges of their lane arithmetic: gmm_cdf_kernel<K> (one
coding table per latent element) over the alphabet sizes on its chunk = ceil(L / 64) transitions, every K instantiation and the
parameter regimes where a table degenerates, and rans_decode_step_kernel at the boundary of its register form, on every stride of its
general form and with padding anywhere in a step list.  The references are plain (tests/codec_ref.py: the float64 table recipe, a
Python-integer rANS decoder, the code length the tables assign), latents are tiny: a table row is one wavefront, so the row count
alone covers the lane logic.  Every test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

from tests import codec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 0.11
M, CHAN = 8, (1, 4, 7)                                                         # 8 latent channels, 3 of them coded


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _cur():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scatter(rows, K, h, w, pix, chan, rs, fill):
    """[npix * nch][K] per-row values (row i * nch + c = pixel pix[i], channel chan[c]) -> the head-output layout [1][K * M][h][w];
    the other elements hold `fill` values no table may depend on"""
    t = fill(rs, (K, M, h * w)).astype(np.float32)
    nch = len(chan)
    v = rows.reshape(len(pix), nch, K)
    for c, m in enumerate(chan):
        t[:, m, pix] = v[:, c, :].T
    return torch.from_numpy(t.reshape(1, K * M, h, w))


def _check_tables(sigma_r, mu_r, logits_r, K, minmax, h, w, pix, rs, what):
    """sigma_r, mu_r, logits_r: [npix * 3][K] parameters of the rows (pix[i], CHAN[c]).  Builds the tables on the device and applies
    every assertion of this file's table tests; -> (worst deviation outside the mode, worst deviation of a mode)."""
    from masic_amd import codec
    L, nch, npix = 2 * minmax + 1, len(CHAN), len(pix)
    n = npix * nch
    sigma = _scatter(sigma_r, K, h, w, pix, CHAN, rs, lambda g, s: g.uniform(0.0, 6.0, s)).to(DEV)
    mu = _scatter(mu_r, K, h, w, pix, CHAN, rs, lambda g, s: g.uniform(-minmax, minmax, s)).to(DEV)
    logits = _scatter(logits_r, K, h, w, pix, CHAN, rs, lambda g, s: g.standard_normal(s)).to(DEV)
    pix_d = torch.from_numpy(pix.astype(np.int32)).to(DEV)
    chan_d = torch.tensor(CHAN, dtype=torch.int32)
    rows = np.arange(n)
    st0 = None
    for place in ("low", "high", "zero", "random"):
        y = np.full((M, h * w), 9999.0, dtype=np.float32)                      # uncoded elements: outside every alphabet, never read
        val = {"low": -minmax, "high": minmax, "zero": 0}.get(place)
        sym_v = rs.randint(-minmax, minmax + 1, size=(npix, nch)) if val is None else np.full((npix, nch), val)
        for c, m in enumerate(CHAN):
            y[m, pix] = sym_v[:, c]
        y_hat = torch.from_numpy(y.reshape(1, M, h, w)).to(DEV)
        starts, sf, err = codec.gmm_tables(sigma, mu, logits, M, K, pix_d, chan_d, minmax, BOUND, y_hat=y_hat)
        assert int(err.item()) == 0, (what, place)
        st = starts.cpu().numpy().view(np.uint16).astype(np.int64)
        assert st.shape == (n, L)
        if st0 is None:
            st0 = st
            assert (st[:, 0] == 0).all(), what
            freq = np.diff(np.concatenate([st, np.full((n, 1), R.TOTAL)], axis=1), axis=1)
            assert (freq >= 1).all(), (what, int(freq.min()))                 # total exactly 2^16, strictly increasing starts
        else:
            assert np.array_equal(st, st0), (what, place)                      # the tables do not depend on the symbols
        sym = (sym_v.reshape(-1) + minmax).astype(np.int64)
        sfh = sf.cpu().numpy()
        assert np.array_equal(sfh[:, 0], st0[rows, sym]) and np.array_equal(sfh[:, 1], freq[rows, sym]), (what, place)
        none, sf2, err2 = codec.gmm_tables(sigma, mu, logits, M, K, pix_d, chan_d, minmax, BOUND, y_hat=y_hat, want_starts=False)
        assert none is None and int(err2.item()) == 0 and np.array_equal(sf2.cpu().numpy(), sfh), (what, place)
    want, raw = R.table_counts_f64(sigma_r, mu_r, logits_r, minmax, BOUND)
    worst, worst_mode = R.check_counts(freq, want, raw)
    print(f"{what}: worst count deviation {worst} (condition: <= 1), at the mode {worst_mode}")
    assert worst <= 1
    return worst, worst_mode


def _rows_for(regimes, n, K, minmax, rs):
    parts = [R.regime_params(g, -(-n // len(regimes)), K, minmax, rs) for g in regimes]
    return tuple(np.concatenate([p[i] for p in parts])[:n] for i in range(3))


@pytest.mark.parametrize("minmax", [1, 2, 31, 32, 63, 64, 127, 128, 511])
def test_tables_over_alphabet_sizes(minmax):
    """K = 3 at the alphabets on the transitions of chunk = ceil(L / 64) -- L = 3 and 5 (idle lanes), 63 | 65, 127 | 129, 255 | 257 --
    and the largest the kernels hold (1023); random parameters and sharp modes at the ends of the alphabet and of lanes' runs."""
    h, w, K = 5, 7, 3
    rs = np.random.RandomState(1000 + minmax)
    pix = rs.permutation(h * w)
    _check_tables(*_rows_for(("random", "mode"), pix.size * len(CHAN), K, minmax, rs), K, minmax, h, w, pix, rs, f"minmax={minmax} K={K}")


@pytest.mark.parametrize("minmax", [37, 32])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_tables_over_every_mixture_size(K, minmax):
    """every instantiation of cdf_launch's switch"""
    h, w = 3, 5
    rs = np.random.RandomState(2000 + 10 * minmax + K)
    pix = rs.permutation(h * w)
    _check_tables(*_rows_for(("random", "mode"), pix.size * len(CHAN), K, minmax, rs), K, minmax, h, w, pix, rs, f"minmax={minmax} K={K}")


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("minmax", [5, 32, 511])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_tables_in_parameter_regimes(regime, minmax, K):
    """codec_ref.regime_params: sigma at or under the bound with mu on integers, half-integers and outside the alphabet; flat tables;
    equal, spread and underflowing mixture weights; a sharp mode at the alphabet's ends and across a lane boundary; random."""
    h, w = 4, 6
    rs = np.random.RandomState(3000 + 10 * minmax + K)
    pix = rs.permutation(h * w)
    _check_tables(*R.regime_params(regime, pix.size * len(CHAN), K, minmax, rs), K, minmax, h, w, pix, rs,
                  f"regime {regime} minmax={minmax} K={K}")


# ---- descriptor errors, through the C ABI with a two-pair stream table
def _two_pair_launch(sigma, mu, logits, K, HW, chans, minmaxes, y_hat, poison=0x5A5A):
    """masic_gmm_cdf_rows_batch over both pairs' pixels (all of them, raster order), into poisoned buffers -> (starts u16 per pair,
    start_freq rows per pair, err [2])"""
    from masic_amd import codec
    from masic_amd._lib import check, lib
    desc, n, nstarts, nrows = codec._stream_table(chans, minmaxes, HW, DEV)
    pix = torch.arange(2 * HW, dtype=torch.int32, device=DEV)
    starts = torch.full((nstarts,), poison, dtype=torch.int16, device=DEV)
    sf = torch.full((nrows, 2), -12345, dtype=torch.int32, device=DEV)
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    check(lib.masic_gmm_cdf_rows_batch(_P(sigma), _P(mu), _P(logits), M, K, HW, _P(pix), None, 2 * HW, HW, _P(desc), n, BOUND,
                                       _P(y_hat), _P(starts), _P(sf), _P(err), _cur()), "gmm_cdf_rows_batch")
    torch.cuda.synchronize()
    st, sfh = starts.cpu().numpy().view(np.uint16), sf.cpu().numpy()
    s0, r0 = HW * len(chans[0]) * (2 * minmaxes[0] + 1), HW * len(chans[0])
    return (st[:s0], st[s0:]), (sfh[:r0], sfh[r0:]), err.cpu().tolist()


def _two_pair_inputs(K, h, w, seed):
    rs = np.random.RandomState(seed)
    shape = (2, K * M, h, w)
    sigma = torch.from_numpy(rs.uniform(0.0, 3.0, shape).astype(np.float32)).to(DEV)
    mu = torch.from_numpy((np.round(rs.uniform(-3.0, 3.0, shape) * 256) / 256).astype(np.float32)).to(DEV)
    logits = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(DEV)
    return rs, sigma, mu, logits


@pytest.mark.parametrize("bad_pair", [0, 1])
@pytest.mark.parametrize("bad_minmax", [0, 512])
def test_a_descriptor_the_tables_cannot_hold_flags_its_own_pair_and_writes_nothing(bad_minmax, bad_pair):
    from masic_amd import codec
    K, h, w = 3, 3, 5
    HW, good = h * w, 1 - bad_pair
    rs, sigma, mu, logits = _two_pair_inputs(K, h, w, 40 + bad_minmax + bad_pair)
    chans = [[0, 3], [2, 5, 6]]
    minmaxes = [4, 4]
    minmaxes[bad_pair] = bad_minmax
    y_hat = torch.from_numpy(rs.randint(-4, 5, (2, M, h, w)).astype(np.float32)).to(DEV)
    starts, sf, err = _two_pair_launch(sigma, mu, logits, K, HW, chans, minmaxes, y_hat)
    assert err[bad_pair] == 1 and err[good] == 0, err
    assert (starts[bad_pair] == 0x5A5A).all() and (sf[bad_pair] == -12345).all()          # nothing written for the refused pair
    one_st, one_sf, one_err = codec.gmm_tables(sigma[good:good + 1], mu[good:good + 1], logits[good:good + 1], M, K,
                                               torch.arange(HW, dtype=torch.int32, device=DEV), torch.tensor(chans[good], dtype=torch.int32),
                                               minmaxes[good], BOUND, y_hat=y_hat[good:good + 1])
    assert int(one_err.item()) == 0
    assert np.array_equal(starts[good], one_st.cpu().numpy().view(np.uint16).reshape(-1))  # the other pair: complete, as on its own
    assert np.array_equal(sf[good], one_sf.cpu().numpy())
    assert sf[good][:, 1].min() >= 1


def test_a_symbol_outside_the_alphabet_flags_its_own_pair_only():
    K, h, w = 2, 3, 5
    HW = h * w
    rs, sigma, mu, logits = _two_pair_inputs(K, h, w, 50)
    chans, minmaxes = [[0, 3], [2, 5, 6]], [5, 3]
    y = rs.randint(-3, 4, (2, M, h, w)).astype(np.float32)
    clean = torch.from_numpy(y).to(DEV)
    _, sf_clean, err = _two_pair_launch(sigma, mu, logits, K, HW, chans, minmaxes, clean)
    assert err == [0, 0]
    for b, m, v in ((1, 5, 4.0), (1, 2, -4.0), (0, 3, 6.0)):
        y2 = y.copy()
        y2[b, m, 1, 2] = v
        _, sf, err = _two_pair_launch(sigma, mu, logits, K, HW, chans, minmaxes, torch.from_numpy(y2).to(DEV))
        assert err[b] == 2 and err[1 - b] == 0, (b, m, v, err)
        assert np.array_equal(sf[1 - b], sf_clean[1 - b])
        assert (sf[b] != sf_clean[b]).any(axis=1).sum() == 1                   # only the offending symbol's row (left unwritten)
    y2 = y.copy()
    y2[0, 1, 0, 0] = 99.0                                                      # not a coded channel: never read
    _, sf, err = _two_pair_launch(sigma, mu, logits, K, HW, chans, minmaxes, torch.from_numpy(y2).to(DEV))
    assert err == [0, 0] and all(np.array_equal(a, b) for a, b in zip(sf, sf_clean))


# ---- the decode-step kernel
def _step_lists(h, w, layout, rs):
    """-> [(pixels of the step, their positions in the step's h-entry list)].  "wavefront": the coder's own steps, padding at the
    tail; "full": every step holds h pixels (all rows of the kernel live); "scattered": the wavefront steps with their pixels at random
    positions of the list, padding entries at the front and in the middle."""
    from masic_amd import codec
    if layout == "full":
        assert (h * w) % h == 0
        return [(p.astype(np.int32), np.arange(h)) for p in rs.permutation(h * w).reshape(w, h)]
    steps = codec.wavefront_steps(h, w)
    if layout == "wavefront":
        return [(p, np.arange(p.size)) for p in steps]
    out = []
    for t, p in enumerate(steps):
        pos = np.sort(rs.choice(np.arange(1, h), size=p.size, replace=False)) if p.size < h else np.arange(h)   # entry 0: padding
        out.append((p, pos))
    assert any(np.any(np.diff(pos) > 1) for _, pos in out)                     # padding in the middle too
    return out


DECODE_CASES = [(8, 8, 3, 31, "wavefront"), (64, 2, 2, 31, "wavefront"), (65, 2, 2, 3, "wavefront"), (6, 6, 3, 32, "wavefront"),
                (6, 6, 2, 63, "wavefront"), (6, 6, 2, 64, "wavefront"), (4, 6, 2, 511, "wavefront"),
                (64, 2, 2, 31, "full"), (65, 2, 2, 3, "full"),
                (8, 8, 3, 31, "scattered"), (6, 6, 3, 32, "scattered")]


@pytest.mark.parametrize("kind", ["edge", "random"])
@pytest.mark.parametrize("h,w,nch,minmax,layout", DECODE_CASES)
def test_device_decode_steps_at_the_edges_of_both_forms(h, w, nch, minmax, layout, kind):
    """masic_rans_decode_step_batch in the form of test_gpu_codec.test_device_rans_decode_steps_equal_the_host_decoder.
    (8, 8, 3, 31): register form with L = 63, lane 63 holds the 0x10000 sentinel; (64, 2, 2, 31): register form with 64 rows;
    (65, 2, 2, 3): general form because of the row count alone, 7-entry alphabet; (6, 6, 3, 32): L = 65, the second stride holds one
    entry; minmax 63 / 64: L = 127 / 129; (4, 6, 2, 511): L = 1023, 16 strides.  Tables: one symbol of freq 65536 - (L - 1) and
    freq == 1 everywhere else ("edge"), or random small counts with freq == 1 symbols ("random").  layout: see _step_lists -- a padding
    entry may stand anywhere in a step list (include/masic_hip.h: "-1 = padding: its rows are skipped"; both kernels test every
    entry)."""
    from masic_amd import codec, ops
    from masic_amd._lib import check, lib
    rs = np.random.RandomState(h * 1000 + w * 100 + nch + minmax)
    Mq, L, HW = nch + 3, 2 * minmax + 1, h * w
    chan = np.sort(rs.choice(Mq, size=nch, replace=False)).astype(np.int32)
    steps = _step_lists(h, w, layout, rs)
    order = np.concatenate([p for p, _ in steps])
    npix = order.size
    assert npix == HW
    n = npix * nch
    f = R.edge_tables(rs, n, L, kind)
    st = R.starts_of(f)
    sym = rs.randint(L, size=n)
    forced = [s for s in (0, L - 1, 62, 63, 64, 65) if s < L]
    for k, s in enumerate(forced):                                              # every channel codes 0, L - 1 and the lane-boundary symbols
        sym[k * nch:(k + 1) * nch] = s
    for r in range(len(forced) * nch, min(n, (len(forced) + 6) * nch)):         # ... freq == 1 symbols and the near-2^16 one
        sym[r] = rs.choice(np.flatnonzero(f[r] == 1)) if r % 2 else int(f[r].argmax())
    rows = np.arange(n)
    sf = np.stack([st[rows, sym], f[rows, sym]], axis=1).astype(np.int32)
    assert (sf[:, 1] == 1).any() and (sym == f.argmax(axis=1)).any()
    streams, _ = codec.split_channels(codec.encode_channels(sf, npix, nch))
    words = np.frombuffer(b"".join(streams), dtype=np.uint32)
    cnt = np.array([len(s) // 4 for s in streams], dtype=np.uint32)
    off = np.concatenate(([0], np.cumsum(cnt)[:-1])).astype(np.uint32)
    state0 = words[off].astype(np.uint64) | (words[off + 1].astype(np.uint64) << np.uint64(32))
    pix_all = np.full((len(steps), h), -1, dtype=np.int32)
    for t, (p, pos) in enumerate(steps):
        pix_all[t, pos] = p
    d32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)
    words_d, pix_d = d32(words), d32(pix_all.reshape(-1))
    desc, nd, nstarts, _ = codec._stream_table([chan.tolist()], [minmax], h, DEV, words=[(off, cnt)])
    assert nd == nch and nstarts == h * nch * L
    state_d = torch.from_numpy(state0.view(np.int64)).to(DEV)
    pos_d = torch.full((nch,), 2, dtype=torch.int32, device=DEV)
    step_d, done_d, err = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
    y_hat = torch.full((Mq, HW), -777.0, dtype=torch.float32, device=DEV)
    starts_d = torch.empty((h, nch, L), dtype=torch.int16, device=DEV)
    y16 = torch.zeros(((Mq + 15) // 16) * HW * 16, dtype=torch.int16, device=DEV)
    row0 = 0
    for t, (p, pos) in enumerate(steps):
        block = np.full((h, nch, L), 0xFFFF, dtype=np.uint16)                  # rows of padding entries: never read
        block[pos] = st[row0 * nch:(row0 + p.size) * nch].astype(np.uint16).reshape(p.size, nch, L)
        starts_d.copy_(torch.from_numpy(block.view(np.int16)))
        check(lib.masic_rans_decode_step_batch(_P(words_d), _P(desc), nd, _P(state_d), _P(pos_d), _P(starts_d), _P(pix_d), h, _P(step_d), h, Mq,
                                               _P(y_hat), _P(y16), HW, _P(err), _P(done_d), _cur()), "rans_decode_step_batch")
        row0 += p.size
    check(lib.masic_rans_decode_finish_batch(_P(desc), nd, _P(state_d), _P(pos_d), _P(err), _cur()), "rans_decode_finish_batch")
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and int(step_d.item()) == len(steps) and int(done_d.item()) == 0
    assert pos_d.cpu().tolist() == cnt.tolist()
    got = y_hat.cpu().numpy()
    want = np.full((Mq, HW), -777.0, dtype=np.float32)
    want[chan[None, :], order[:, None]] = (sym.reshape(npix, nch) - minmax).astype(np.float32)
    assert np.array_equal(got, want)                                           # the symbols, and the poison everywhere else
    y32 = ops.f16k_to_nchw(y16, 1, Mq, h, w).cpu().numpy().reshape(Mq, HW)
    exact = np.abs(want[chan]) <= 256                                          # the F16K copy is bf16: exact for |value| <= 256
    assert np.array_equal(y32[chan][exact], want[chan][exact])
    untouched = np.setdiff1d(np.arange(Mq), chan)
    assert not y32[untouched].any()
    for c, data in enumerate(streams):                                         # the plain decoder on the same streams and tables
        ref, finished = R.rans_decode_py(data, st[np.arange(npix) * nch + c])
        assert finished and ref == sym[np.arange(npix) * nch + c].tolist(), c
        lo, hi = R.code_length_slack(len(data), sf[np.arange(npix) * nch + c, 1])
        assert lo >= 0 and hi >= 0


# ---- both kernels together
@pytest.mark.parametrize("use_graph", [True, False])
def test_round_trip_of_three_alphabets_in_one_launch_and_the_streams_code_length(use_graph):
    """codec.encode_views / decode_views on fixed entropy parameters: pairs with minmax 31 (register form), 32 and 511 (general form,
    2 and 16 strides) in one launch, the parameter regimes sharp / flat / logits / random mixed across the pixels.  The latents come
    back, a pair's bytes equal those of the pair alone, and every channel stream is as long as its own tables say
    (codec_ref.code_length_slack, freq from gmm_tables on the same rows)."""
    from masic_amd import codec
    B, K, h, w = 3, 5, 6, 7
    HW = h * w
    rs = np.random.RandomState(77)
    minmaxes = [31, 32, 511]
    chans = [[1, 4, 7], [0, 4, 5], [2, 3, 6]]
    sigma, mu, logits = (np.zeros((B, K, M, HW), dtype=np.float32) for _ in range(3))
    y = np.zeros((B, M, HW), dtype=np.float32)
    for b in range(B):
        for m in range(M):
            s_, m_, l_ = _rows_for(("sharp", "flat", "logits", "random"), HW, K, minmaxes[b], rs)
            perm = rs.permutation(HW)
            sigma[b, :, m], mu[b, :, m], logits[b, :, m] = s_[perm].T, m_[perm].T, l_[perm].T
        for m in chans[b]:
            y[b, m] = rs.randint(-minmaxes[b], minmaxes[b] + 1, HW)
            y[b, m, rs.choice(HW, 3, replace=False)] = (-minmaxes[b], 0, minmaxes[b])
    sigma, mu, logits = (torch.from_numpy(a.reshape(B, K * M, h, w)).to(DEV) for a in (sigma, mu, logits))
    y_hat = torch.from_numpy(y.reshape(B, M, h, w)).to(DEV)

    class Fixed:
        """the entropy parameters as given: no layers to run"""
        skinny = True

        def __init__(self):
            self.sigma, self.mu, self.logits = sigma, mu, logits
            self.y16 = torch.zeros(B * 16 * HW, dtype=torch.int16, device=DEV)

        def set_latent(self, y):
            pass

        def run(self, *a):
            pass

    blobs = codec.encode_views(Fixed(), y_hat, M, K, chans, minmaxes, BOUND)
    order = torch.from_numpy(np.concatenate(codec.wavefront_steps(h, w))).to(DEV)
    tightest = np.inf
    for b in range(B):
        single, = codec.encode_views(lambda _y, b=b: (sigma[b:b + 1], mu[b:b + 1], logits[b:b + 1]), y_hat[b:b + 1], M, K,
                                     [chans[b]], [minmaxes[b]], BOUND)
        assert blobs[b] == single, b
        _, sf, err = codec.gmm_tables(sigma[b:b + 1], mu[b:b + 1], logits[b:b + 1], M, K, order, torch.tensor(chans[b], dtype=torch.int32),
                                      minmaxes[b], BOUND, y_hat=y_hat[b:b + 1], want_starts=False)
        assert int(err.item()) == 0
        freq = sf.cpu().numpy()[:, 1].reshape(HW, len(chans[b]))
        streams, _ = codec.split_channels(blobs[b])
        assert len(streams) == len(chans[b])
        for c, data in enumerate(streams):
            lo, hi = R.code_length_slack(len(data), freq[:, c])
            print(f"pair {b} (minmax {minmaxes[b]}) channel {chans[b][c]}: {8 * len(data)} bits, ideal {R.ideal_bits(freq[:, c]):.1f}, "
                  f"{lo:.1f} above the lower bound, {hi:.1f} under the upper")
            assert lo >= 0 and hi >= 0, (b, c)
            tightest = min(tightest, lo, hi)
    print(f"tightest code-length slack: {tightest:.2f} bits")
    got = codec.decode_views(Fixed(), blobs, (h, w), M, K, chans, minmaxes, BOUND, DEV, use_graph=use_graph)
    assert torch.equal(got, y_hat)
