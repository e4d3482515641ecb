"""Host side of the self-contained stereo files (masic_amd/stereofile.py): the .msf container, the quantisation of the corner
offsets, and the refusals that need no device."""
import struct
import zlib

import numpy as np
import pytest
import torch

from masic_amd import codec, stereofile as SF

Q = np.array([-32768, -65, -1, 0, 1, 63, 4097, 32767], dtype=np.int16)
HEADER = struct.pack("<HH", 128, 192) + bytes(range(1, 40))          # stands for a .npz: the padded size, then anything
STREAMS = codec.MAGIC + bytes([1, 0, 0, 0]) + bytes(range(200, 256))  # stands for a .bin
FIELDS = (("magic", 0, 4), ("version", 4, 1), ("flags", 5, 1), ("H0", 6, 2), ("W0", 8, 2), *((f"offset {i}", 10 + 2 * i, 2) for i in range(8)),
          ("header length", 26, 4), ("stream length", 30, 4), ("crc", 34, 4))


def _file():
    return SF.pack(100, 150, Q, HEADER, STREAMS)


def test_corrupt_stream_error_is_the_value_error_decompress_raises():
    assert issubclass(codec.CorruptStreamError, ValueError)


def test_pack_and_parse_return_every_field():
    data = _file()
    assert SF.HEADER_BYTES == 38
    assert len(data) == 38 + len(HEADER) + len(STREAMS)
    assert data[:4] == b"MSF1" and data[4] == 1 and data[5] == 0
    assert struct.unpack_from("<I", data, 34)[0] == zlib.crc32(data[:34])
    f = SF.parse(data, "test")
    assert (f.H0, f.W0) == (100, 150)
    assert f.delta_q.dtype == np.int16 and np.array_equal(f.delta_q, Q)
    assert f.header == HEADER and f.streams == STREAMS
    assert struct.unpack_from("<8h", data, 10) == tuple(int(v) for v in Q)       # little-endian, the order of delta.reshape(8)
    assert struct.unpack_from("<II", data, 26) == (len(HEADER), len(STREAMS))
    # the sections may be empty of streams; sizes that need no padding keep their own size in the inner header
    g = SF.parse(SF.pack(64, 128, Q.reshape(4, 2), struct.pack("<HH", 64, 128), b""), "test")
    assert (g.H0, g.W0, g.header, g.streams) == (64, 128, struct.pack("<HH", 64, 128), b"")


def test_pack_refuses_what_the_header_cannot_hold():
    for H0, W0 in ((0, 64), (64, 0), (65536, 64), (65535, 64)):        # 65535 pads to 65536
        with pytest.raises(ValueError):
            SF.pack(H0, W0, Q, HEADER, STREAMS)
    with pytest.raises(ValueError):
        SF.pack(100, 150, Q[:7], HEADER, STREAMS)
    with pytest.raises(ValueError):
        SF.pack(100, 150, Q.astype(np.float32), HEADER, STREAMS)
    with pytest.raises(ValueError):
        SF.pack(100, 150, Q.astype(np.int64) * 2, HEADER, STREAMS)


def test_offset_quantisation():
    rng = np.random.default_rng(5)
    d = rng.uniform(-500, 500, (1000, 4, 2)).astype(np.float32)
    q = SF.quantise(d)
    assert q.dtype == np.int16 and q.shape == d.shape
    back = SF.dequantise(q)
    assert back.dtype == np.float32
    assert np.abs(back.astype(np.float64) - d.astype(np.float64)).max() <= 1.0 / 128
    assert np.array_equal(SF.quantise(back), q)                                   # quantising twice = quantising once
    assert np.array_equal(SF.dequantise(Q).astype(np.float64) * 64, Q.astype(np.float64))        # q / 64 is exact
    edge = np.array([511.99, 512.0, 600.0, 1e30, np.inf, -512.0, -512.01, -1e30, -np.inf], dtype=np.float32)
    assert SF.quantise(edge).tolist() == [32767] * 5 + [-32768] * 4
    assert SF.quantise(np.array([np.nan], dtype=np.float32)).tolist() == [0]
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5], dtype=np.float32) / np.float32(64)     # rint: ties to even
    assert SF.quantise(ties).tolist() == [0, 2, 2, 0, -2, -2, 4]


@pytest.mark.parametrize("field,offset,size", FIELDS, ids=[f[0] for f in FIELDS])
def test_a_flipped_bit_in_any_header_field_is_detected(field, offset, size):
    good = _file()
    for bit in (0, 8 * size - 1):
        bad = bytearray(good)
        bad[offset + bit // 8] ^= 1 << (bit % 8)
        with pytest.raises(codec.CorruptStreamError, match="test"):
            SF.parse(bytes(bad), "test")


def test_fields_that_pass_the_checksum_are_still_checked():
    """A writer that recomputes the CRC over a foreign version, set flags, an empty picture or wrong lengths is refused field by field."""
    def forged(**kw):
        v = dict(magic=b"MSF1", version=1, flags=0, H0=100, W0=150, n1=len(HEADER), n2=len(STREAMS))
        v.update(kw)
        head = struct.pack("<4sBBHH8hII", v["magic"], v["version"], v["flags"], v["H0"], v["W0"], *(int(x) for x in Q), v["n1"], v["n2"])
        return head + struct.pack("<I", zlib.crc32(head)) + HEADER + STREAMS

    assert SF.parse(forged(), "test").header == HEADER
    for kw, what in ((dict(magic=b"MSF2"), "magic"), (dict(version=2), "version"), (dict(version=0), "version"), (dict(flags=1), "flags"),
                     (dict(flags=128), "flags"), (dict(H0=0), "empty"), (dict(W0=0), "empty"), (dict(n1=len(HEADER) + 1), "sections"),
                     (dict(n2=len(STREAMS) - 1), "sections"), (dict(n1=0, n2=len(HEADER) + len(STREAMS)), "header section")):
        with pytest.raises(codec.CorruptStreamError, match=what):
            SF.parse(forged(**kw), "test")


def test_truncation_and_trailing_bytes():
    good = _file()
    for cut in (0, 3, 37, 38, 38 + len(HEADER), len(good) - 1):          # inside and at every section boundary, one byte short of the end
        with pytest.raises(codec.CorruptStreamError):
            SF.parse(good[:cut], "test")
    with pytest.raises(codec.CorruptStreamError, match="sections"):
        SF.parse(good + b"\0", "test")
    assert SF.parse(good, "test").streams == STREAMS


@pytest.mark.parametrize("hw", [(100, 150), (128, 256), (192, 192), (64, 192)])
def test_an_inner_header_of_another_size_is_refused(hw):
    """H0 x W0 = 100 x 150 is coded as 128 x 192 and as nothing else -- not the unpadded size, not a larger multiple of 64."""
    with pytest.raises(codec.CorruptStreamError, match="inner header"):
        SF.parse(SF.pack(100, 150, Q, struct.pack("<HH", *hw) + HEADER[4:], STREAMS), "test")


def test_parse_errors_carry_the_callers_tag_and_pair_index():
    with pytest.raises(codec.CorruptStreamError, match=r"decode: pair 2 \(c\)") as e:
        SF.parse(_file()[:-1], "decode: pair 2 (c)", 2)
    assert e.value.pair == 2


def test_a_codec_built_for_decoding_refuses_to_encode_and_other_refusals():
    import MASIC
    import masic_amd
    assert masic_amd.StereoCodec is SF.StereoCodec
    hsic = MASIC.HSIC(16, 24, 3).eval()
    pic = torch.zeros((100, 150, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="udh=None"):
        SF.StereoCodec(hsic).encode(pic, pic, "a")
    with pytest.raises(RuntimeError, match="cqe=None"):
        SF.StereoCodec(hsic).decode("a", enhance=True)
    hsic.train()
    with pytest.raises(RuntimeError, match="training mode"):
        SF.StereoCodec(hsic).decode("a")
    hsic.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # the modules live on the host here
        SF.StereoCodec(hsic).decode("a")
