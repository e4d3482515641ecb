"""CPU tests of what makes HSIC.decompress reject damaged files (no GPU needed): the final-state invariant of the rANS coder on the host
decoder (masic_rans_decoder_finished, the host form of the device check masic_rans_decode_finish_batch), the strict container parser
codec.split_views, and fp8.stream_scales validating an untrusted calibration table before it touches a module."""
import json

import numpy as np
import pytest
import torch

from masic_amd import codec, fp8


def _tables(rs, nrows, L):
    """Random strictly increasing interval starts [nrows][L] (counts >= 1 totalling 2^16), a symbol per row and its (start, freq)."""
    f = rs.randint(1, 200, size=(nrows, L)).astype(np.int64)
    f[np.arange(nrows), rs.randint(L, size=nrows)] += 65536 - f.sum(axis=1)
    assert f.min() >= 1
    starts = np.concatenate([np.zeros((nrows, 1), dtype=np.int64), np.cumsum(f, axis=1)[:, :-1]], axis=1)
    sym = rs.randint(L, size=nrows)
    sf = np.stack([starts[np.arange(nrows), sym], f[np.arange(nrows), sym]], axis=1).astype(np.int32)
    return starts.astype(np.uint16), sym, sf


def _flip_last_word(data, bit):
    raw = bytearray(data)
    raw[len(raw) - 4 + bit // 8] ^= 1 << (bit % 8)
    return bytes(raw)


def _decodes_unfinished(data, rows):
    """A damaged stream: the host decoder raises on the way, or ends outside the final state."""
    dec = codec.AdaptiveDecoder(data)
    try:
        dec.decode_rows(rows)
        return not dec.finished()
    except RuntimeError:
        return True
    finally:
        dec.close()


def test_host_decoder_ends_in_the_final_state_exactly_after_the_last_symbol():
    rs = np.random.RandomState(41)
    npix, nch, L = 211, 6, 33
    starts, sym, sf = _tables(rs, npix * nch, L)
    streams, _ = codec.split_channels(codec.encode_channels(sf, npix, nch))
    for c, data in enumerate(streams):
        rows = np.arange(npix) * nch + c
        dec = codec.AdaptiveDecoder(data)
        got = dec.decode_rows(starts[rows[:-1]])
        assert not dec.finished(), c                                     # one symbol still to come
        got = np.concatenate([got, dec.decode_rows(starts[rows[-1:]])])
        assert np.array_equal(got, sym[rows]) and dec.finished(), c
        dec.close()
        assert len(data) > 8                                             # the last word is a renormalisation word, not the state
        for bit in (0, 13, 31):
            assert _decodes_unfinished(_flip_last_word(data, bit), starts[rows]), (c, bit)


def test_host_decoder_final_state_of_a_single_stream():
    rs = np.random.RandomState(42)
    for n, L in ((1, 2), (50, 7), (3000, 81)):
        starts, sym, sf = _tables(rs, n, L)
        data = codec.encode_freqs(sf)
        dec = codec.AdaptiveDecoder(data)
        if n > 1:
            dec.decode_rows(starts[:-1])
            assert not dec.finished(), n
            got = dec.decode_rows(starts[-1:])
            assert got[0] == sym[-1]
        else:
            assert not dec.finished()                                    # nothing decoded yet
            assert dec.decode_rows(starts)[0] == sym[0]
        assert dec.finished(), n
        dec.close()
        if len(data) > 8:
            assert _decodes_unfinished(_flip_last_word(data, 5), starts), n


def _two_views(rs):
    blobs = []
    for npix, nch, L in ((37, 5, 9), (37, 3, 21)):
        _, _, sf = _tables(rs, npix * nch, L)
        blobs.append(codec.encode_channels(sf, npix, nch))
    return blobs


def test_split_views_parses_what_split_channels_parses():
    rs = np.random.RandomState(43)
    v1, v2 = _two_views(rs)
    views = codec.split_views(v1 + v2, 2)
    assert views == [v1, v2]
    s1, used1 = codec.split_channels(v1 + v2)
    s2, used2 = codec.split_channels((v1 + v2)[used1:])
    assert used1 + used2 == len(v1 + v2)
    assert [codec.split_channels(v)[0] for v in views] == [s1, s2]
    assert [codec.split_channels(v)[1] for v in views] == [len(v1), len(v2)]
    # a view without coded channels is a bare zero count
    empty = codec.encode_channels(np.zeros((0, 2), dtype=np.int32), 0, 0)
    assert codec.split_views(v1 + empty, 2) == [v1, empty] and codec.split_views(empty + empty, 2) == [empty, empty]


def _with_u32(blob, off, value):
    return blob[:off] + np.array([value], dtype=np.uint32).tobytes() + blob[off + 4:]


def test_split_views_rejects_malformed_containers():
    rs = np.random.RandomState(44)
    v1, v2 = _two_views(rs)
    blob = v1 + v2
    len0 = int(np.frombuffer(v1[4:8], dtype=np.uint32)[0])
    last_len_off = len(v1) + 4 + 4 * 2                                   # the length field of view 2's last stream (3 streams)
    last_len = int(np.frombuffer(blob[last_len_off:last_len_off + 4], dtype=np.uint32)[0])
    bad = {
        "first length raised by 4": _with_u32(blob, 4, len0 + 4),
        "last length raised by 4": _with_u32(blob, last_len_off, last_len + 4),
        "last word dropped": blob[:-4],
        "bytes appended": blob + b"\0\0\0\0",
        "one byte appended": blob + b"\0",
        "count larger than the buffer": _with_u32(blob, 0, len(blob)),
        "count of view 2 larger than the buffer": _with_u32(blob, len(v1), 1 << 31),
        "length below 8": _with_u32(blob, 4, 4),
        "length not a multiple of 4": _with_u32(blob, 4, len0 + 2),
        "second view missing": v1,
        "empty": b"",
        "cut inside the length fields": blob[:10],
    }
    for what, data in bad.items():
        with pytest.raises(ValueError):
            codec.split_views(data, 2)
            print("accepted:", what)
    assert codec.split_views(blob, 2) == [v1, v2]


def test_corrupt_stream_error_is_a_pair_stream_error_and_a_value_error():
    assert issubclass(codec.CorruptStreamError, codec.PairStreamError) and issubclass(codec.CorruptStreamError, ValueError)
    names = ["a", "b", "c"]
    with pytest.raises(codec.CorruptStreamError, match="final state") as ei:
        codec.check_errs(torch.tensor([0, 8, 8], dtype=torch.int32), "decode", names)
    assert ei.value.pair == 1 and "1 (b)" in str(ei.value)
    for cause in ("corrupt", "header", "weights", "operand mode"):
        assert cause in str(ei.value), cause
    # the earlier flags keep their precedence, message and type
    for flag, text in ((1 | 8, "normalised"), (2 | 8, "outside the alphabet"), (4 | 8, "ended before its last symbol")):
        with pytest.raises(codec.PairStreamError, match=text) as ei:
            codec.check_errs(torch.tensor([flag], dtype=torch.int32), "decode")
        assert not isinstance(ei.value, codec.CorruptStreamError) and ei.value.pair == 0
    codec.check_errs(torch.zeros(3, dtype=torch.int32), "decode", names)


class _Leaf(torch.nn.Module):
    pass


def _scaled_tree():
    net = torch.nn.Module()
    net.encoder1, net.decoder1 = _Leaf(), _Leaf()
    net.decoder1.inner = _Leaf()
    net.encoder1.__dict__["_fp8_scale"] = {"a": 0.1, "b": 2.5e-3}
    net.decoder1.inner.__dict__["_fp8_scale"] = {"x": 7.0}
    return net


def test_stream_scales_validates_the_table_before_touching_the_model():
    net = _scaled_tree()
    own = fp8.export_scales(net)
    assert own == {"encoder1": {"a": 0.1, "b": 2.5e-3}, "decoder1.inner": {"x": 7.0}}
    bad = {
        "garbage bytes": b"\xff\xfe\x00{{{",
        "not JSON": b"{'encoder1': 1}",
        "top level not a dict": b"[1, 2]",
        "unknown module": json.dumps({"encoder1": {"a": 1.0}, "nowhere": {"a": 1.0}}).encode(),
        "non-numeric value": json.dumps({"encoder1": {"a": "1.0"}}).encode(),
        "scales not a dict": json.dumps({"encoder1": 3.0}).encode(),
        "non-finite value": b'{"encoder1": {"a": NaN}}',
        "infinite value": b'{"encoder1": {"a": Infinity}}',
        "boolean value": b'{"encoder1": {"a": true}}',
        "integer beyond the float range": b'{"encoder1": {"a": 1' + b"0" * 400 + b"}}",
    }
    for what, raw in bad.items():
        entered = False
        with pytest.raises(ValueError, match="foreign fp8 table"):
            with fp8.stream_scales(net, raw):
                entered = True
        assert not entered, what
        assert fp8.export_scales(net) == own, what                       # bit-equal: the same floats under the same names
        assert net.encoder1.__dict__["_fp8_scale"] == {"a": 0.1, "b": 2.5e-3}
    # a good table is in place inside the context and gone afterwards
    theirs = {"encoder1": {"a": 0.5}, "decoder1": {"y": 3.0}}
    with fp8.stream_scales(net, json.dumps(theirs).encode()):
        assert fp8.export_scales(net) == theirs
    assert fp8.export_scales(net) == own
    with fp8.stream_scales(net, None):
        assert fp8.export_scales(net) == own
