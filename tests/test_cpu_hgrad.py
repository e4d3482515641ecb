"""CPU tests of the h_matrix gradient path: the C ABI declares and exports its entry points, and the admission rule of
tests/hgrad_cases.py -- a case is compared only where the CPU oracle's float32 and float64 matrix gradients agree to 1e-4 --
admits every named case the GPU tests compare."""
import os
import re

import pytest
import torch

from tests import hgrad_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HGRAD_SYMBOLS = ["masic_warp_perspective_bwd_matrix", "masic_warp_matrix_bwd", "masic_homography_from_corners_bwd", "masic_warp_matrix_slots"]


def test_header_declares_and_library_exports_the_matrix_gradient_entry_points():
    from masic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "masic_hip.h")).read()
    for name in HGRAD_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), f"{name} is not declared in include/masic_hip.h"
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), f"{name} is not exported by the library"
    from masic_amd import autograd, homography, ops
    for fn in ("warp_perspective_bwd_matrix", "warp_matrix_bwd", "homography_from_corners_bwd"):
        assert callable(getattr(ops, fn))
    assert callable(homography.h_matrix_from_corners)
    for node in ("WarpFn", "WarpOnesFn", "WarpMatricesFn", "HomographyFromCornersFn"):
        assert issubclass(getattr(autograd, node), torch.autograd.Function)


def test_slots_cover_the_destination():
    from masic_amd import _lib
    slots = _lib.lib.masic_warp_matrix_slots
    assert slots(17, 23) == 1 and slots(32, 32) == 1 and slots(32, 33) == 2 and slots(48, 64) == 3 and slots(512, 512) == 256
    assert slots(0, 5) == 0 and slots(5, -1) == 0 and slots(1 << 16, 1 << 16) == 0


@pytest.mark.parametrize("case", HC.operator_cases() + HC.ones_cases(), ids=lambda c: c.name)
def test_every_named_case_is_admitted(case):
    e32, g64 = case.admission()
    print(f"{case.name}: e32 {e32:.2e}, |g64| {float(g64.norm()):.3e}")
    assert bool(torch.isfinite(g64).all())
    if case.ones and case.kind == "magnify1.5":
        assert float(g64.abs().max()) == 0.0        # every sample in range: the mask is 1 whatever the matrix
        return
    assert e32 <= HC.ADMIT, (case.name, e32)


@pytest.mark.parametrize("case", HC.rejected_cases(), ids=lambda c: c.name)
def test_rejected_kinds_sit_on_cell_boundaries(case):
    """identity, 0.6 x about the centre: samples on integer coordinates, where the one-sided derivative taken depends on the last bit of
    the coordinate -- float32 and float64 oracle disagree by a multiple of the gradient itself, so no tolerance-based comparison exists
    there (the GPU tests check finiteness and reproducibility only)."""
    e32, g64 = case.admission()
    print(f"{case.name}: e32 {e32:.2e}")
    assert bool(torch.isfinite(g64).all())
    assert e32 > HC.ADMIT
