"""GPU tests (-m gpu) of the decoder's integrity checks: HSIC.decompress / decompress_batch refuse damaged or mismatched files instead of
returning pictures decoded from garbage.  The device check (masic_rans_decode_finish_batch, masic_amd/csrc/codec.hip) rests on the rANS
invariant that a stream read with the encoder's tables ends with all its words consumed and the coder at 2^31; the container checks
(codec.split_views, HSIC._read_pair) run on the host before any kernel.  All damage is passed in as file bytes, and every damaged length
is one the host parser rejects: no kernel is asked to read outside its buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")


def _net(N, M, K, seed, prec):
    import MASIC
    from masic_amd import nn as mnn, synth
    mnn.set_precision(prec)
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    net = net.to(DEV).eval()
    net.update()
    return net


def _read(path, name, ext):
    with open(os.path.join(path, name + ext), "rb") as f:
        return f.read()


def _write(path, name, ext, data):
    with open(os.path.join(path, name + ext), "wb") as f:
        f.write(data)


def _bin_layout(raw):
    """Byte (offset, length) of every channel stream of an f32 / bf16 .bin (8 header bytes, no fp8 table), per view."""
    assert raw[:4] == b"MSR2" and not raw[5] & 1
    off, views = 8, []
    for _ in range(2):
        n = int(np.frombuffer(raw[off:off + 4], dtype=np.uint32)[0])
        lengths = np.frombuffer(raw[off + 4:off + 4 + 4 * n], dtype=np.uint32)
        off += 4 + 4 * n
        streams = []
        for ln in lengths:
            streams.append((off, int(ln)))
            off += int(ln)
        views.append(streams)
    assert off == len(raw)
    return views


def _flip(raw, byte_off, bit):
    out = bytearray(raw)
    out[byte_off + bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def _flip_up(raw, word_off):
    """Flips the lowest CLEAR bit of the little-endian 32-bit word at word_off: the coder's state rises by 2^k where it takes the word
    in.  (A flip that lowers the state can leave the last state just below 2^31, where the decoder asks for one more word: that is
    reported by the older "ended before its last symbol" flag, which takes precedence.)"""
    word = int(np.frombuffer(raw[word_off:word_off + 4], dtype=np.uint32)[0])
    assert word != 0xffffffff
    k = next(b for b in range(32) if not (word >> b) & 1)
    return _flip(raw, word_off, k)


def _longest(streams):
    return max(streams, key=lambda s: s[1])


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_clean_streams_still_decode(tmp_path, prec):
    """No false positive: the pixel-list path (bf16 operands) and the full-latent path (float32) round-trip with the check on."""
    from masic_amd import nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=21))
        with torch.no_grad():
            enc = net.compress(x1, x2, hm, "p", str(tmp_path))
            dec = net.decompress(None, None, hm, "p", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_bit_flips_are_caught(tmp_path, prec):
    """One flipped bit of p.bin -- in the first stream word of view 1 (a state word), in a word in the middle of a view-1 channel stream,
    in the last word of the last channel stream of view 2 -- raises CorruptStreamError (a ValueError and a PairStreamError); a position
    where the damaged coder happens to run out of words first gives the older "ended before its last symbol" PairStreamError.  Before
    the final-state check the second and third case returned pictures."""
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=21))
        with torch.no_grad():
            net.compress(x1, x2, hm, "p", str(tmp_path))
        raw = _read(tmp_path, "p", ".bin")
        v1, v2 = _bin_layout(raw)
        assert v1 and v2
        mid_off, mid_len = _longest(v1)
        assert mid_len >= 16                                             # two state words and at least two more
        last_off, last_len = v2[-1]
        cases = {
            "first stream word of view 1": _flip(raw, v1[0][0], 3),
            "middle word of a view-1 stream": _flip(raw, mid_off + (mid_len // 8) * 4, 17),
            "last word of the last stream of view 2": _flip_up(raw, last_off + last_len - 4),
        }
        for what, data in cases.items():
            assert len(data) == len(raw) and data != raw
            _write(tmp_path, "p", ".bin", data)
            with pytest.raises(codec.PairStreamError) as ei, torch.no_grad():
                net.decompress(None, None, hm, "p", str(tmp_path))
            print(f"{prec}, flip in the {what}: {type(ei.value).__name__}: {ei.value}")
            if isinstance(ei.value, codec.CorruptStreamError):
                assert isinstance(ei.value, ValueError) and "final state" in str(ei.value), what
            else:
                assert "ended before its last symbol" in str(ei.value), what
            assert ei.value.pair == 0
        _write(tmp_path, "p", ".bin", raw)
        with torch.no_grad():
            net.decompress(None, None, hm, "p", str(tmp_path))           # the undamaged file still decodes
    finally:
        mnn.set_precision("f32")


def test_header_of_another_pair_is_caught(tmp_path):
    """Pair A's .bin beside pair B's .npz (same size, other content): the z strings, channel flags and minmax are B's, so the tables are
    not the encoder's -> CorruptStreamError, or the ValueError of the stream count when the pairs code different channel sets."""
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, "bf16")
        hms = {}
        with torch.no_grad():
            for name, seed in (("a", 5), ("b", 6)):
                x1, x2, hms[name] = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=seed))
                net.compress(x1, x2, hms[name], name, str(tmp_path))
        assert _read(tmp_path, "a", ".npz") != _read(tmp_path, "b", ".npz")
        _write(tmp_path, "a", ".npz", _read(tmp_path, "b", ".npz"))
        with pytest.raises(ValueError) as ei, torch.no_grad():
            net.decompress(None, None, hms["a"], "a", str(tmp_path))
        print(f"another pair's header: {type(ei.value).__name__}: {ei.value}")
        assert isinstance(ei.value, codec.CorruptStreamError) or "one rANS stream per coded channel" in str(ei.value)
    finally:
        mnn.set_precision("f32")


def test_container_damage_is_refused_before_any_kernel(tmp_path, monkeypatch):
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, "bf16")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=21))
        with torch.no_grad():
            net.compress(x1, x2, hm, "p", str(tmp_path))
        raw_bin, raw_npz = _read(tmp_path, "p", ".bin"), _read(tmp_path, "p", ".npz")
        calls = []
        monkeypatch.setattr(codec, "decode_views", lambda *a, **k: calls.append(1))
        monkeypatch.setattr(net.entropy_bottleneck1, "decompress", lambda *a, **k: calls.append(1))
        for what, ext, data in (("4 bytes appended to p.bin", ".bin", raw_bin + b"\0\0\0\0"),
                                ("the last 4 bytes of p.bin removed", ".bin", raw_bin[:-4]),
                                ("p.npz cut in half", ".npz", raw_npz[:len(raw_npz) // 2]),
                                ("a byte appended to p.npz", ".npz", raw_npz + b"\0"),
                                ("p.bin cut inside its header", ".bin", raw_bin[:6])):
            _write(tmp_path, "p", ".bin", raw_bin)
            _write(tmp_path, "p", ".npz", raw_npz)
            _write(tmp_path, "p", ext, data)
            with pytest.raises(ValueError, match="HSIC.decompress") as ei:
                net.decompress(None, None, hm, "p", str(tmp_path))
            print(f"{what}: {ei.value}")
            assert not isinstance(ei.value, codec.PairStreamError) and not calls, what
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_batch_names_the_damaged_pair(tmp_path, prec):
    """Three pairs, pair 1's .bin with one bit flipped in the last word of a view-2 channel stream: decompress_batch raises
    CorruptStreamError for pair 1 and names it; with the clean files every slice equals decompress of that pair alone."""
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(3, 128, 192, seed=21))
        names = ["left", "middle", "right"]
        with torch.no_grad():
            net.compress_batch(x1, x2, hm, names, str(tmp_path))
            dec = net.decompress_batch(names, hm, str(tmp_path))
            for i, n in enumerate(names):
                one = net.decompress(None, None, hm[i:i + 1], n, str(tmp_path))
                for k in FIELDS:
                    assert torch.equal(one[k], dec[k][i:i + 1]), (n, k)
        raw = _read(tmp_path, "middle", ".bin")
        off, ln = _longest(_bin_layout(raw)[1])
        assert ln > 8                                                    # its last word is a renormalisation word
        _write(tmp_path, "middle", ".bin", _flip_up(raw, off + ln - 4))
        with pytest.raises(codec.CorruptStreamError) as ei, torch.no_grad():
            net.decompress_batch(names, hm, str(tmp_path))
        print(f"{prec}, batch: {ei.value}")
        assert ei.value.pair == 1 and "middle" in str(ei.value) and "left" not in str(ei.value) and "right" not in str(ei.value)
    finally:
        mnn.set_precision("f32")


def test_other_weights_do_not_decode(tmp_path):
    """A valid file and a model of other weights: the z coder or the y check raises; the call must not return pictures."""
    from masic_amd import nn as mnn, synth
    try:
        net = _net(32, 48, 3, 21, "bf16")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 128, 192, seed=21))
        with torch.no_grad():
            net.compress(x1, x2, hm, "p", str(tmp_path))
        other = _net(32, 48, 3, 22, "bf16")
        with pytest.raises((ValueError, RuntimeError)) as ei, torch.no_grad():
            other.decompress(None, None, hm, "p", str(tmp_path))
        print(f"other weights: {type(ei.value).__name__}: {ei.value}")
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("h,w,nch,minmax", [(8, 8, 5, 3), (32, 32, 40, 20)])
def test_device_finish_check(h, w, nch, minmax):
    """masic_rans_decode_finish_batch on the state the decode kernel leaves (synthetic tables, two pairs holding the same streams, set up
    as in test_device_rans_decode_steps_equal_the_host_decoder): after all coding steps no flag; after all but the last, bit 3 and only
    bit 3 for both pairs (every channel has a symbol on the last wavefront); with one stream of pair 1 given a trailing word (present in
    the buffer, counted in word_cnt, never consumed), bit 3 for pair 1 only."""
    from masic_amd import codec
    from masic_amd._lib import lib, check
    B = 2
    rs = np.random.RandomState(h * 1000 + nch + 7)
    M, L, HW = nch + 3, 2 * minmax + 1, h * w
    chan = np.sort(rs.choice(M, size=nch, replace=False)).astype(np.int32)
    steps = codec.wavefront_steps(h, w)
    npix = HW
    f = rs.randint(1, 60, size=(npix * nch, L)).astype(np.int64)
    f[np.arange(npix * nch), rs.randint(L, size=npix * nch)] += 65536 - f.sum(axis=1)
    assert f.min() >= 1
    st = np.concatenate([np.zeros((npix * nch, 1), dtype=np.int64), np.cumsum(f, axis=1)[:, :-1]], axis=1)
    sym = rs.randint(L, size=npix * nch)
    sf = np.stack([st[np.arange(npix * nch), sym], f[np.arange(npix * nch), sym]], axis=1).astype(np.int32)
    streams, _ = codec.split_channels(codec.encode_channels(sf, npix, nch))
    pix_all = np.full((len(steps), B, h), -1, dtype=np.int32)
    for t, p in enumerate(steps):
        for b in range(B):
            pix_all[t, b, :p.size] = b * HW + p
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    d32 = lambda a: torch.from_numpy(np.array(a).view(np.int32)).to(DEV)

    def run(nsteps, trailing_word_on=None):
        blobs, wo, wc, base = [], [], [], 0
        for b in range(B):
            mine = list(streams)
            if trailing_word_on is not None and trailing_word_on[0] == b:
                mine[trailing_word_on[1]] = mine[trailing_word_on[1]] + b"\0\0\0\0"
            cnt = np.array([len(s) // 4 for s in mine], dtype=np.int64)
            wo.append(base + np.cumsum(cnt) - cnt)
            wc.append(cnt)
            base += int(cnt.sum())
            blobs.extend(mine)
        words = np.frombuffer(b"".join(blobs), dtype=np.uint32)
        assert words.size == base and all(int((o + c).max()) <= base for o, c in zip(wo, wc))        # every stream inside the buffer
        off = np.concatenate(wo)
        state0 = words[off].astype(np.uint64) | (words[off + 1].astype(np.uint64) << np.uint64(32))
        desc, n, nstarts, _ = codec._stream_table([chan.tolist()] * B, [minmax] * B, h, DEV, words=list(zip(wo, wc)))
        assert n == B * nch and nstarts == B * h * nch * L
        words_d, pix_d = d32(words), d32(pix_all.reshape(-1))
        state_d = torch.from_numpy(state0.view(np.int64)).to(DEV)
        pos_d = torch.full((n,), 2, dtype=torch.int32, device=DEV)
        step_d, done_d = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
        err = torch.zeros(B, dtype=torch.int32, device=DEV)
        y_hat = torch.zeros((B, M, HW), dtype=torch.float32, device=DEV)
        starts_d = torch.zeros((B, h * nch, L), dtype=torch.int16, device=DEV)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        row0 = 0
        for p in steps[:nsteps]:
            rows = st[row0 * nch:(row0 + p.size) * nch].astype(np.uint16)
            starts_d[:, :p.size * nch].copy_(torch.from_numpy(rows.view(np.int16)))
            check(lib.masic_rans_decode_step_batch(P(words_d), P(desc), n, P(state_d), P(pos_d), P(starts_d), P(pix_d), B * h, P(step_d), h, M,
                                                   P(y_hat), None, HW, P(err), P(done_d), stream), "rans_decode_step_batch")
            row0 += p.size
        check(lib.masic_rans_decode_finish_batch(P(desc), n, P(state_d), P(pos_d), P(err), stream), "rans_decode_finish_batch")
        torch.cuda.synchronize()
        assert int(step_d.item()) == nsteps
        return err.cpu().tolist(), y_hat.cpu().numpy()

    order = np.concatenate(steps)
    want = np.zeros((M, HW), dtype=np.float32)
    want[chan[None, :], order[:, None]] = (sym.reshape(npix, nch) - minmax).astype(np.float32)
    flags, got = run(len(steps))
    assert flags == [0, 0]
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    flags, _ = run(len(steps) - 1)
    assert flags == [8, 8]
    flags, got = run(len(steps), trailing_word_on=(1, nch // 2))
    assert flags == [0, 8]
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)          # the symbols themselves are all there
    # no streams (a pair whose latent is all zero): no launch, no flag
    desc, n, _, _ = codec._stream_table([chan.tolist()], [minmax], h, DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    state_d, pos_d = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    check(lib.masic_rans_decode_finish_batch(P(desc), 0, P(state_d), P(pos_d), P(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "rans_decode_finish_batch")
    torch.cuda.synchronize()
    assert int(err.item()) == 0
