"""CPU tests of the weight-free patch aligner: the float64 restatement (tests/align_ref.py) against ground truth, the parser's messages for
a side header, the library's host-side answers, and the refusals of the Python surface."""
import ctypes

import pytest
import torch

from tests import align_ref as R

SIGMAS = (2.5, 4.0)
SEEDS = tuple(range(8))
CAP = 0.05                       # px, mean corner error


# ------------------------------------------------------------------------------------------ 1. restatement against ground truth
@pytest.mark.parametrize("tmax,jitter", [(16, 4), (32, 4), (40, 8), (45, 0)])
def test_restatement_recovers_translation_plus_jitter(tmax, jitter):
    a, b, truth = R.make_set(128, SIGMAS, tmax, jitter, SEEDS)
    delta, info, _ = R.align(a, b)
    err = R.corner_error(delta, truth)
    print(f"tmax {tmax} jitter {jitter}: mean corner error per case", [f"{e:.4f}" for e in err.tolist()])
    assert info[:, 3].eq(0).all(), info[:, 3]
    assert float(err.max()) <= CAP
    assert bool((info[:, 1] < info[:, 0]).all()) and bool((info[:, 2] >= 0.25).all())


def test_restatement_stage_two_alone_recovers_independent_corner_offsets():
    a, b, truth = R.make_set(128, SIGMAS, 0, 8, SEEDS)
    delta, info, costs = R.align(a, b, delta0=torch.zeros_like(truth))
    err = R.corner_error(delta, truth)
    print("jitter 8, no search: mean corner error per case", [f"{e:.4f}" for e in err.tolist()])
    assert costs is None and info[:, 3].eq(0).all()
    assert float(err.max()) <= CAP


def test_restatement_geometry():
    """h_from_delta is the homography of the four corner pairs; the level matrices map coarse pixel centres as the fine one does."""
    g = torch.Generator().manual_seed(3)
    delta = (torch.rand((5, 4, 2), generator=g, dtype=torch.float64) - 0.5) * 40
    for P in (32, 64, 128):
        H = R.h_from_delta(delta, P)
        assert torch.allclose(R.apply_h(H, R.square(P)), R.square(P) + delta, atol=1e-9)
        pts = torch.rand((7, 2), generator=g, dtype=torch.float64) * 31
        for level in (1, 2):
            s, t = 2.0 ** level, (2.0 ** level - 1) / 2
            fine = R.apply_h(H, pts * s + t)
            assert torch.allclose(R.apply_h(R.to_level(H, level), pts) * s + t, fine, atol=1e-9)
            assert torch.allclose(R.from_level(R.to_level(H, level), level), H, atol=1e-12)


def test_restatement_guards():
    a, b, _ = R.make_set(32, (2.5,), 4, 1, (0, 1, 2))
    flat = torch.full_like(a, 0.25)
    delta, info, _ = R.align(flat, flat)
    assert info[:, 3].eq(1).all() and delta.eq(0).all()
    delta, info, _ = R.align(a, a)
    assert info[:, 3].eq(0).all() and float(delta.abs().max()) <= 1e-4
    bad = a.clone()
    bad[1, 0, 5, 7] = float("nan")
    d0 = torch.full((3, 4, 2), 0.5, dtype=torch.float64)
    delta, info, _ = R.align(bad, b, delta0=d0)
    assert info[:, 3].tolist() == [0.0, 1.0, 0.0] and torch.equal(delta[1], d0[1])


# ------------------------------------------------------------------------------------------ 2. binding
def test_the_parser_names_the_header_it_was_given():
    """(what include/masic_align.h declares and how it is bound: tests/test_cpu_side_headers.py)"""
    from masic_amd import _lib
    assert not [n for n in _lib.SIGNATURES if n.startswith("masic_align")]
    with pytest.raises(ValueError, match=r"^masic_align\.h: unknown type"):
        _lib.parse_header("int masic_align_x(foo a);", header="masic_align.h")
    with pytest.raises(ValueError, match=r"^masic_hip\.h: unknown type"):
        _lib.parse_header("int masic_align_x(foo a);")
    assert _lib.lib.masic_version() == 1


def test_workspace_bytes_and_host_side_refusals():
    from masic_amd import _lib, align          # noqa: F401 (importing align binds masic_align.h: size_t for the workspace query)
    ws = _lib.lib.masic_align_workspace_bytes
    assert ws(1, 32) == 0 and ws(3, 64) == 3 * 2 * 32 * 32 * 4 and ws(65535, 128) == 65535 * 2 * (64 * 64 + 32 * 32) * 4
    assert ws(1, 256) == 0 and ws(0, 128) == 0 and ws(65536, 128) == 0
    call = _lib.lib.masic_align_patches
    x = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused before the launch
    for B, P, radius, its, damping, word in ((1, 256, 12, (30, 15, 10), 1e-6, "P = 256"), (65536, 128, 12, (30, 15, 10), 1e-6, "B = 65536"),
                                             (0, 128, 12, (30, 15, 10), 1e-6, "B = 0"), (1, 128, 16, (30, 15, 10), 1e-6, "search_radius"),
                                             (1, 128, 12, (30, -1, 10), 1e-6, "iteration"), (1, 128, 12, (30, 15, 10), float("nan"), "damping")):
        assert call(x, x, None, x, x, x, B, P, radius, *its, damping, None) != 0
        assert word in _lib.lib.masic_last_error().decode()
    assert call(x, x, None, x, x, None, 1, 128, 12, 30, 15, 10, 1e-6, None) != 0 and b"workspace" in _lib.lib.masic_last_error()
    assert call(None, x, None, x, x, x, 1, 128, 12, 30, 15, 10, 1e-6, None) != 0 and b"null" in _lib.lib.masic_last_error()


# ------------------------------------------------------------------------------------------ 3. refusals
def test_cpu_tensors_raise_and_the_aligner_holds_no_state():
    import MASIC
    import masic_amd
    from masic_amd import align
    from masic_amd.stereofile import StereoCodec
    assert masic_amd.PatchAligner is align.PatchAligner
    a = torch.zeros((1, 1, 128, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.align_patches(a, a)
    aligner = align.PatchAligner().eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner(a, a)
    assert len(aligner.state_dict()) == 0 and not list(aligner.parameters()) and not list(aligner.buffers())
    assert len(align.PatchAligner(init=torch.nn.Linear(2, 2)).state_dict()) == 0      # init is called, not owned
    hsic = MASIC.HSIC(16, 24, 3).eval()
    pic = torch.zeros((100, 150, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # reached past the "udh=None" refusal
        StereoCodec(hsic, aligner).encode(pic, pic, "a")
    with pytest.raises(RuntimeError, match="training mode"):
        StereoCodec(hsic, align.PatchAligner()).encode(pic, pic, "a")
