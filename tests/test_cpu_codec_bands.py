"""The banded y bitstream without a device: the coding schedule codec.wavefront_steps(h, w, band_rows), the argument check of the entry
point of include/masic_bands.h (the header itself is a row of tests/test_cpu_side_headers.py), the "MSR3" container header through
HSIC._read_pair on files written by hand, and the refusal of a band_rows that is no integer in 0 .. 255 before any device work."""
import os
import types

import numpy as np
import pytest

from tests import bands_ref as BR


# ------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("h,w,S", BR.SCHEDULE_CASES)
def test_schedule(h, w, S):
    from masic_amd import codec
    steps = codec.wavefront_steps(h, w, S)
    assert len(steps) == BR.expected_steps(h, w, S) == w + 3 * (min(S, h) - 1)
    step_of = np.full(h * w, -1, dtype=np.int64)
    for t, p in enumerate(steps):
        assert p.dtype == np.int32
        rows = p // w
        assert (np.diff(rows) > 0).all(), f"step {t}: rows ascend, at most one pixel per row"
        assert (step_of[p] == -1).all(), f"step {t}: a pixel coded twice"
        step_of[p] = t
        assert ((p % w) + 3 * (rows % S) == t).all()
    assert (step_of >= 0).all(), "every pixel is coded"
    for i in range(h):
        top = (i // S) * S
        for j in range(w):
            for dy, dx in BR.LIVE_TAPS:
                r, c = i + dy, j + dx
                if top <= r and 0 <= c < w:               # inside the latent and inside the pixel's band (r <= i < h always)
                    assert step_of[r * w + c] < step_of[i * w + j], ((i, j), (dy, dx))


@pytest.mark.parametrize("h,w", [(8, 12), (5, 7), (76, 136)])
def test_one_band_is_the_unbanded_schedule(h, w):
    from masic_amd import codec
    plain = codec.wavefront_steps(h, w)
    assert len(plain) == w + 3 * (h - 1)
    for S in (0, h, h + 5):
        got = codec.wavefront_steps(h, w, S)
        assert len(got) == len(plain) and all(np.array_equal(a, b) for a, b in zip(got, plain)), S
    ii = np.arange(h)
    for t, p in enumerate(plain):                      # the lists of the two-argument call are what they were: t = j + 3 i
        j = t - 3 * ii
        keep = (j >= 0) & (j < w)
        assert np.array_equal(p, (ii[keep] * w + j[keep]).astype(np.int32))


# ------------------------------------------------------------------------------------------ entry point
def test_band_rows_below_one_is_an_argument_error_of_the_entry_point():
    """before any pointer is looked at: no device needed"""
    from masic_amd import _lib
    for bad in (0, -3):
        rc = _lib.lib.masic_bands_skinny_ctx_fwd_batch(None, None, None, 0, 1, 1, 4, 4, None, 0, 0, bad, None)
        assert rc == _lib.CONSTANTS["ERR_ARG"], bad
        assert "band_rows" in _lib.lib.masic_last_error().decode()


# ------------------------------------------------------------------------------------------ container
M = 48


def _write(tmp_path, name, bin_head, bin_rest=bytes(8)):
    """a pair's two files by hand: 64 x 128, no coded channel in either view (n = 0 streams), empty z strings"""
    npz = np.array([64, 128], dtype=np.uint16).tobytes()
    for _ in range(2):
        npz += np.array([0, 1], dtype=np.uint16).tobytes() + bytes(M // 8)
    (tmp_path / (name + ".npz")).write_bytes(npz)
    (tmp_path / (name + ".bin")).write_bytes(bin_head + bin_rest)


def _read(tmp_path, name):
    import MASIC
    return MASIC.HSIC._read_pair(types.SimpleNamespace(M=M), str(tmp_path), name, "test")


def test_read_pair_takes_band_rows_from_an_msr3_header(tmp_path):
    _write(tmp_path, "plain", b"MSR2" + bytes([0, 0, 0, 0]))
    _write(tmp_path, "bands", b"MSR3" + bytes([0, 0, 5, 0]))
    _write(tmp_path, "most", b"MSR3" + bytes([0, 0, 255, 0]))
    for name, want in (("plain", 0), ("bands", 5), ("most", 255)):
        H, W, views, streams, fp8_table, band_rows = _read(tmp_path, name)
        assert (H, W, fp8_table, band_rows) == (64, 128, None, want), name
        assert [v[2] for v in views] == [[], []] and streams == [bytes(4), bytes(4)]


def test_read_pair_refuses_msr3_without_band_rows(tmp_path):
    _write(tmp_path, "zero", b"MSR3" + bytes([0, 0, 0, 0]))
    with pytest.raises(ValueError, match="band_rows"):
        _read(tmp_path, "zero")


@pytest.mark.parametrize("magic", [b"MSR2", b"MSR3"])
def test_read_pair_refuses_a_truncated_header(tmp_path, magic):
    for n in (4, 6, 7):
        _write(tmp_path, "cut", (magic + bytes([0, 0, 4, 0]))[:n], b"")
        with pytest.raises(ValueError, match="truncated"):
            _read(tmp_path, "cut")


def test_read_pair_ignores_bytes_6_and_7_of_an_msr2_file(tmp_path):
    _write(tmp_path, "old", b"MSR2" + bytes([0, 0, 9, 7]))
    assert _read(tmp_path, "old")[5] == 0


def test_read_pair_refuses_another_magic(tmp_path):
    _write(tmp_path, "other", b"MSR4" + bytes([0, 0, 4, 0]))
    with pytest.raises(ValueError, match="not a stream of this library"):
        _read(tmp_path, "other")


# ------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize("bad", [-1, 256, 2.5, "4"])
def test_band_rows_must_be_an_integer_of_one_byte(tmp_path, bad):
    """raised before the pictures are looked at: they live on the CPU here, where nothing of the codec could run"""
    import torch
    import MASIC
    from masic_amd import StereoCodec
    net = MASIC.HSIC(32, M, 3).eval()
    x, hm = torch.zeros(1, 3, 64, 64), torch.eye(3)[None]
    with pytest.raises(ValueError, match="band_rows"):
        net.compress(x, x, hm, "pair", str(tmp_path), band_rows=bad)
    with pytest.raises(ValueError, match="band_rows"):
        net.compress_batch(x, x, hm, ["pair"], str(tmp_path), band_rows=bad)
    with pytest.raises(ValueError, match="band_rows"):
        StereoCodec(net, band_rows=bad)
    assert not os.listdir(tmp_path)
