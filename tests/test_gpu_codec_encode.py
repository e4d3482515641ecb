"""GPU tests (-m gpu) of the device rANS encoder: masic_rans_encode_channels_batch / masic_rans_pack_pairs_batch (masic_amd/csrc/codec.hip)
behind codec.encode_channels_device and codec.encode_views(coder="device").  The host coder (codec.encode_channels, rans.hip) is the
checker: every comparison is byte for byte, there is no tolerance in this feature.  The Python-integer decoder of tests/codec_ref.py,
which shares no code with either coder, reads a sample of the device streams back."""
import os

import numpy as np
import pytest
import torch

from tests import codec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 0.11
TOTAL = 65536
PRIMES = np.array([3, 65535, 2, 5, 7, 251, 257, 4093, 32749, 65521])


def _rows(regime, n, rs):
    """n (start, freq) rows, int32 [n][2]: "random" valid intervals; "ones": freq = 1 (16 bits per symbol: a word every second symbol,
    the closest a stream gets to its npix + 2 words); "full": (0, 65536), no word is ever emitted; "primes": freq in {3, 65535, primes}
    with start at either end of its range; "mixed": every row from one of the four."""
    if regime == "random":
        freq = rs.randint(1, TOTAL + 1, size=n)
        start = (rs.rand(n) * (TOTAL - freq + 1)).astype(np.int64)
    elif regime == "ones":
        freq, start = np.ones(n, dtype=np.int64), rs.randint(0, TOTAL, size=n)
    elif regime == "full":
        freq, start = np.full(n, TOTAL), np.zeros(n, dtype=np.int64)
    elif regime == "primes":
        freq = PRIMES[rs.randint(PRIMES.size, size=n)]
        start = np.where(rs.rand(n) < 0.5, 0, TOTAL - freq)
    else:
        parts = np.stack([_rows(g, n, rs) for g in ("random", "ones", "full", "primes")])
        return parts[rs.randint(4, size=n), np.arange(n)]
    sf = np.stack([start, freq], axis=1).astype(np.int32)
    assert (sf[:, 0] >= 0).all() and (sf[:, 1] >= 1).all() and (sf.sum(axis=1) <= TOTAL).all()
    return sf


def _device_blobs(rows_per_pair, nchs, npix):
    """the pairs' rows through ONE call of the two kernels -> (blobs, flags)"""
    from masic_amd import codec
    B = len(nchs)
    desc, n, _, nrows = codec._stream_table([list(range(c)) for c in nchs], [1] * B, npix, DEV)
    assert n == sum(nchs) and nrows == npix * n
    sf = np.concatenate(rows_per_pair + [np.zeros((0, 2), dtype=np.int32)])
    sf_d = torch.from_numpy(np.ascontiguousarray(sf) if sf.size else np.zeros((1, 2), dtype=np.int32)).to(DEV)
    first = [0] + np.cumsum(nchs).tolist()
    return codec.encode_channels_device(sf_d, desc, n, npix, B, first)


def _table_row(start, freq):
    """a strictly increasing row of interval starts that holds [start, start + freq), and the interval's index in it"""
    row = sorted({0, int(start), int(start) + int(freq)} - {TOTAL})
    return row, row.index(int(start))


# pairs of ONE call: a single lane; one lane past a wave; a pair WITHOUT streams between pairs with streams; three full waves; and two
# more so that every regime has a pair of its own.  Lanes are streams in table order, so the pairs also start at lanes 0, 1, 2 (66 % 64),
# 2 (258 % 64) and 9 of their waves.
NCHS = (1, 65, 0, 192, 7, 66)
REGIMES = ("ones", "random", None, "primes", "full", "mixed")


@pytest.mark.parametrize("npix", [1, 2, 37, 1024])
def test_kernels_equal_the_host_coder_byte_for_byte(npix):
    """npix: one symbol; two; 37 = one whole and one partial tile of the kernel's 32-pixel staging; 1024 = 32 whole tiles."""
    from masic_amd import codec
    rs = np.random.RandomState(4000 + npix)
    rows = [_rows(g, npix * c, rs) if c else np.zeros((0, 2), dtype=np.int32) for g, c in zip(REGIMES, NCHS)]
    want = [codec.encode_channels(r, npix if c else 0, c) for r, c in zip(rows, NCHS)]
    assert want[2] == np.zeros(1, dtype=np.uint32).tobytes()
    blobs, flags = _device_blobs(rows, NCHS, npix)
    assert flags == [0] * len(NCHS)
    for b, (got, ref) in enumerate(zip(blobs, want)):
        assert got == ref, (b, REGIMES[b], len(got), len(ref))
    again, flags2 = _device_blobs(rows, NCHS, npix)
    assert again == blobs and flags2 == flags                                  # the same bytes every run
    for b, c in ((0, 0), (1, 64), (3, 191), (4, 3), (5, 65)):                  # one stream per regime through the independent decoder
        streams, used = codec.split_channels(blobs[b])
        assert used == len(blobs[b]) and len(streams) == NCHS[b]
        assert all(len(s) >= 8 and len(s) % 4 == 0 and len(s) <= 4 * (npix + 2) for s in streams)
        mine = rows[b][np.arange(npix) * NCHS[b] + c]
        tables = [_table_row(st, fr) for st, fr in mine]
        sym, finished = R.rans_decode_py(streams[c], [t for t, _ in tables])
        assert finished and sym == [s for _, s in tables], (b, c)
    full, _ = codec.split_channels(blobs[4])
    assert all(s == (1 << 31).to_bytes(8, "little") for s in full)             # (0, 65536) rows: the 8 bytes of the initial state
    ones, _ = codec.split_channels(blobs[0])
    assert len(ones[0]) == 4 * (2 + npix // 2)                                 # freq = 1: 16 bits per symbol, a word every second one
    print(f"npix={npix}: {[len(b) for b in blobs]} bytes per pair")


def test_bad_rows_are_flagged_not_coded():
    """Pair 1 holds a freq = 0 row and a start + freq = 65537 row (the host coder's argument error): err bit 4 for pair 1 alone, pair
    0's bytes untouched; pair 1's blob is still framed and codes the other rows (the host coder on the rows without the bad ones)."""
    from masic_amd import codec
    npix, nchs = 37, (5, 3)
    rs = np.random.RandomState(51)
    rows = [_rows("mixed", npix * c, rs) for c in nchs]
    good = rows[1].copy()
    rows[1][4 * 3 + 1] = (17, 0)                                               # pixel 4, channel 1
    rows[1][30 * 3 + 2] = (65535, 2)                                           # pixel 30, channel 2
    blobs, flags = _device_blobs(rows, nchs, npix)
    assert flags == [0, 16]
    assert blobs[0] == codec.encode_channels(rows[0], npix, nchs[0])
    with pytest.raises(RuntimeError):
        codec.encode_channels(rows[1], npix, nchs[1])
    streams, used = codec.split_channels(blobs[1])
    assert used == len(blobs[1]) and len(streams) == 3
    keep = good.reshape(npix, 3, 2)
    assert streams[0] == codec.encode_freqs(keep[:, 0])
    assert streams[1] == codec.encode_freqs(np.delete(keep[:, 1], 4, axis=0))
    assert streams[2] == codec.encode_freqs(np.delete(keep[:, 2], 30, axis=0))


def _fixed_params(B, M, K, h, w, minmaxes, chans, seed):
    HW = h * w
    rs = np.random.RandomState(seed)
    sigma, mu, logits = (np.zeros((B, K, M, HW), dtype=np.float32) for _ in range(3))
    y = np.zeros((B, M, HW), dtype=np.float32)
    for b in range(B):
        for m in range(M):
            parts = [R.regime_params(g, -(-HW // 4), K, minmaxes[b], rs) for g in ("sharp", "flat", "logits", "random")]
            s_, m_, l_ = (np.concatenate([p[i] for p in parts])[:HW] for i in range(3))
            perm = rs.permutation(HW)
            sigma[b, :, m], mu[b, :, m], logits[b, :, m] = s_[perm].T, m_[perm].T, l_[perm].T
        for m in chans[b]:
            y[b, m] = rs.randint(-minmaxes[b], minmaxes[b] + 1, HW)
            y[b, m, rs.choice(HW, 3, replace=False)] = (-minmaxes[b], 0, minmaxes[b])
    sigma, mu, logits = (torch.from_numpy(a.reshape(B, K * M, h, w)).to(DEV) for a in (sigma, mu, logits))
    return sigma, mu, logits, torch.from_numpy(y.reshape(B, M, h, w)).to(DEV)


def _fixed(sigma, mu, logits):
    class Fixed:
        """the entropy parameters as given: no layers to run (the pixel-list stand-in of tests/test_gpu_codec_edges.py)"""
        skinny = True

        def __init__(self):
            self.sigma, self.mu, self.logits = sigma, mu, logits

        def set_latent(self, y):
            pass

        def run(self, *a):
            pass
    return Fixed()


def test_encode_views_device_equals_host_on_fixed_parameters():
    """B = 3 pairs on a 4 x 6 latent, minmax 31 / 32 / 511, different channel sets, one of them empty: the device coder's blobs equal
    the host coder's, a pair alone equals the pair in the batch, and the device table never went through encode_channels."""
    from masic_amd import codec
    B, M, K, h, w = 3, 8, 5, 4, 6
    minmaxes, chans = [31, 32, 511], [[1, 4, 7], [], [0, 2, 3, 6]]
    sigma, mu, logits, y_hat = _fixed_params(B, M, K, h, w, minmaxes, chans, 91)
    dev = codec.encode_views(_fixed(sigma, mu, logits), y_hat, M, K, chans, minmaxes, BOUND, coder="device")
    host = codec.encode_views(_fixed(sigma, mu, logits), y_hat, M, K, chans, minmaxes, BOUND, coder="host")
    default = codec.encode_views(_fixed(sigma, mu, logits), y_hat, M, K, chans, minmaxes, BOUND)
    assert isinstance(dev, list) and len(dev) == B and all(isinstance(b, bytes) for b in dev)
    assert dev == host and default == host
    assert dev[1] == np.zeros(1, dtype=np.uint32).tobytes()
    for b in range(B):
        for coder in ("device", "host"):
            single, = codec.encode_views(lambda _y, b=b: (sigma[b:b + 1], mu[b:b + 1], logits[b:b + 1]), y_hat[b:b + 1], M, K,
                                         [chans[b]], [minmaxes[b]], BOUND, coder=coder)
            assert single == dev[b], (b, coder)
    with pytest.raises(ValueError):
        codec.encode_views(_fixed(sigma, mu, logits), y_hat, M, K, chans, minmaxes, BOUND, coder="gpu")


def test_a_flagged_pair_surfaces_from_encode_views_with_its_index(monkeypatch):
    """err bit 4 through encode_views: the table kernel's rows of pair 1 are replaced by one the coder cannot take before the device
    coder runs -> PairStreamError naming pair 1, raised before any blob is copied."""
    from masic_amd import codec
    B, M, K, h, w = 2, 8, 3, 4, 6
    minmaxes, chans = [5, 5], [[1, 4], [0, 2, 3]]
    sigma, mu, logits, y_hat = _fixed_params(B, M, K, h, w, minmaxes, chans, 92)
    orig = codec._encode_device

    def spoiled(sf, *a, **k):
        sf[h * w * len(chans[0]) + 7, 1] = 0                                   # a row of pair 1: freq = 0
        return orig(sf, *a, **k)
    monkeypatch.setattr(codec, "_encode_device", spoiled)
    with pytest.raises(codec.PairStreamError, match="symbol interval outside") as e:
        codec.encode_views(_fixed(sigma, mu, logits), y_hat, M, K, chans, minmaxes, BOUND)
    assert e.value.pair == 1


# ---- through the model
def _net(N, M, K, seed, prec):
    import MASIC
    from masic_amd import nn as mnn
    from masic_amd import synth
    mnn.set_precision(prec)
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    net = net.to(DEV).eval()
    net.update()
    return net


def _files(path, name):
    return tuple(open(os.path.join(str(path), name + ext), "rb").read() for ext in (".npz", ".bin"))


def _count_calls(monkeypatch, mod, name):
    calls = []
    orig = getattr(mod, name)

    def wrapped(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(mod, name, wrapped)
    return calls


def _device_against_host_files(net, x1, x2, hm, names, tmp_path, monkeypatch):
    """compress_batch with the device coder (the default: no host-coder call at all) and with encode_views forced to coder="host" ->
    the same files; -> (the device run's result, its directory)"""
    from masic_amd import codec
    d_dev, d_host = tmp_path / "device", tmp_path / "host"
    d_dev.mkdir()
    d_host.mkdir()
    with torch.no_grad():
        with monkeypatch.context() as mp:
            host_calls = _count_calls(mp, codec, "encode_channels")
            enc = net.compress_batch(x1, x2, hm, names, str(d_dev))
            assert len(host_calls) == 0
        with monkeypatch.context() as mp:
            orig = codec.encode_views
            mp.setattr(codec, "encode_views", lambda *a, **k: orig(*a, **dict(k, coder="host")))
            host_calls = _count_calls(mp, codec, "encode_channels")
            net.compress_batch(x1, x2, hm, names, str(d_host))
            assert len(host_calls) == 2 * len(names)                          # the checker did run: every view of every pair
    for n in names:
        assert _files(d_dev, n) == _files(d_host, n), n
    return enc, d_dev


@pytest.mark.parametrize("N,M,K,H,W,B,prec", [(32, 48, 3, 128, 192, 3, "f32"), (32, 48, 3, 128, 192, 3, "bf16"),
                                              (128, 192, 5, 256, 320, 2, "bf16")])
def test_model_files_of_the_device_coder_equal_the_host_coders(tmp_path, monkeypatch, N, M, K, H, W, B, prec):
    from masic_amd import nn as mnn, synth
    try:
        net = _net(N, M, K, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=21))
        names = [f"pair{i}" for i in range(B)]
        enc, d_dev = _device_against_host_files(net, x1, x2, hm, names, tmp_path, monkeypatch)
        with torch.no_grad():
            dec = net.decompress_batch(names, hm, str(d_dev))
        for k in ("y1_hat", "y2_hat"):
            assert torch.equal(enc[k], dec[k]), k
    finally:
        mnn.set_precision("f32")


def test_fp8_mode_files_of_the_device_coder_equal_the_host_coders(tmp_path, monkeypatch):
    from masic_amd import fp8, nn as mnn, synth
    try:
        net = _net(128, 192, 5, 23, "fp8")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=23))
        fp8.calibrate(net, [(x1, x2, hm)])
        _device_against_host_files(net, x1, x2, hm, ["pair8"], tmp_path, monkeypatch)
    finally:
        mnn.set_precision("f32")
