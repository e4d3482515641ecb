"""The plain references of tests/codec_ref.py against the host coder of rans.hip (no GPU): the Python-integer decoder returns what
codec.AdaptiveDecoder returns, every channel stream of masic_rans_encode_channels is as short as its own tables say, and the float32
restatement of the table recipe stays within one count of the float64 recipe in every parameter regime of the GPU tests."""
import numpy as np
import pytest

from tests import codec_ref as R


def _coded_case(L, kind, seed, npix=150, nch=3):
    """tables, symbols and the (start, freq) rows of npix x nch symbols; the symbols include 0, L - 1, freq == 1 ones and the big one"""
    rs = np.random.RandomState(seed)
    n = npix * nch
    f = R.edge_tables(rs, n, L, kind)
    st = R.starts_of(f)
    sym = rs.randint(L, size=n)
    sym[:nch] = 0
    sym[nch:2 * nch] = L - 1
    sym[2 * nch:4 * nch] = f[2 * nch:4 * nch].argmax(axis=1)                 # the near-2^16 symbol
    for r in range(4 * nch, 8 * nch):                                         # a freq == 1 symbol for sure
        sym[r] = rs.choice(np.flatnonzero(f[r] == 1))
    rows = np.arange(n)
    sf = np.stack([st[rows, sym], f[rows, sym]], axis=1).astype(np.int32)
    assert (f[rows, sym] == 1).sum() >= 4 * nch
    return f, st, sym, sf


@pytest.mark.parametrize("kind", ["edge", "random"])
@pytest.mark.parametrize("L", [3, 63, 65, 129, 1023])
def test_python_decoder_equals_host_decoder_and_streams_meet_their_code_length(L, kind):
    from masic_amd import codec
    npix, nch = 150, 3
    f, st, sym, sf = _coded_case(L, kind, 100 + L, npix, nch)
    streams, used = codec.split_channels(codec.encode_channels(sf, npix, nch))
    assert len(streams) == nch
    worst_lo, worst_hi = np.inf, np.inf
    for c, data in enumerate(streams):
        rows = np.arange(npix) * nch + c
        dec = codec.AdaptiveDecoder(data)
        host = dec.decode_rows(st[rows].astype(np.uint16))
        assert dec.finished()
        dec.close()
        got, finished = R.rans_decode_py(data, st[rows])
        assert finished
        assert got == host.tolist() == sym[rows].tolist(), c
        lo, hi = R.code_length_slack(len(data), sf[rows, 1])
        worst_lo, worst_hi = min(worst_lo, lo), min(worst_hi, hi)
        assert lo >= 0 and hi >= 0, (c, len(data), R.ideal_bits(sf[rows, 1]))
    print(f"L={L} {kind}: bits above ideal - 1: {worst_lo:.2f}, bits left under ideal + 96 + 1e-4 n: {worst_hi:.2f}")


def test_python_decoder_on_an_empty_and_on_a_damaged_stream():
    from masic_amd import codec
    streams, _ = codec.split_channels(codec.encode_channels(np.zeros((0, 2), dtype=np.int32), 0, 1))
    assert len(streams[0]) == 8
    assert R.rans_decode_py(streams[0], []) == ([], True)                      # the flushed initial state alone
    f, st, sym, sf = _coded_case(65, "random", 5, 40, 1)
    data, = codec.split_channels(codec.encode_channels(sf, 40, 1))[0]
    assert R.rans_decode_py(data, st) == (sym.tolist(), True)
    assert R.rans_decode_py(data, st[:-1])[1] is False                         # one symbol short of the end: not the final state
    with pytest.raises(ValueError):
        R.rans_decode_py(data[:8], st)                                         # runs dry
    flipped = bytearray(data)
    flipped[9] ^= 0x10
    got, finished = R.rans_decode_py(bytes(flipped), st)
    assert got != sym.tolist() or not finished


def test_code_length_bound_holds_for_long_and_for_skewed_streams():
    """the 1e-4 n term: 20000 symbols of one channel, all on near-certain symbols (the coder's loss per step is largest relative to
    the payload there), and 20000 random ones"""
    from masic_amd import codec
    rs = np.random.RandomState(9)
    n, L = 20000, 65
    for kind, pick in (("edge", "big"), ("random", "any")):
        f = R.edge_tables(rs, n, L, kind)
        st = R.starts_of(f)
        sym = f.argmax(axis=1) if pick == "big" else rs.randint(L, size=n)
        sf = np.stack([st[np.arange(n), sym], f[np.arange(n), sym]], axis=1).astype(np.int32)
        data, = codec.split_channels(codec.encode_channels(sf, n, 1))[0]
        lo, hi = R.code_length_slack(len(data), sf[:, 1])
        print(f"{kind}/{pick}: {8 * len(data)} bits, ideal {R.ideal_bits(sf[:, 1]):.1f}, slack {lo:.2f} / {hi:.2f}")
        assert lo >= 0 and hi >= 0


@pytest.mark.parametrize("regime", R.REGIMES)
def test_float32_restatement_of_the_table_recipe_meets_the_count_condition(regime):
    """table_counts_f32 (the kernel's operation order in numpy float32) against table_counts_f64 on the inputs of every regime of
    tests/test_gpu_codec_edges.py: float32 arithmetic alone stays inside codec_ref.check_counts, the condition the kernel's tables are
    held to, so a failure there is the kernel's.  (regime_params says which inputs were chosen for this to hold.)"""
    for minmax in (1, 5, 32, 37, 511):
        if regime == "flat" and minmax < 5:
            continue
        for K in (1, 3, 5, 8):
            rs = np.random.RandomState(minmax * 10 + K)
            sigma, mu, logits = R.regime_params(regime, 72, K, minmax, rs)
            want, raw = R.table_counts_f64(sigma, mu, logits, minmax, 0.11)
            got, _ = R.table_counts_f32(sigma, mu, logits, minmax, 0.11)
            assert (got.sum(axis=1) == 65536).all() and got.min() >= 1
            worst, worst_mode = R.check_counts(got, want, raw)
            print(f"{regime} minmax={minmax} K={K}: worst deviation {worst}, at the mode {worst_mode}")
            assert worst <= 1
