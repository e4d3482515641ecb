"""include/masic_latent.h, the fourth side header of libmasic_hip.so (masic_amd/latent.py, masic_amd/csrc/conv_s2_latent.hip): the checks
tests/test_cpu_side_headers.py makes for masic_align.h, masic_deconv.h and masic_conv_s2.h -- prototypes only, every name an entry point of
its own under the header's prefix, the signatures, each bound on the library with the types the header states, the kernel's source in the
build -- and what the module answers without a GPU."""
import ctypes
import os
import re

import pytest

from tests.test_cpu_side_headers import ROOT, C, F, I, P, S, _parsed       # noqa: F401 (F: the header has no float argument by value)

HEADER, PREFIX, SOURCE = "masic_latent.h", "masic_latent_", "conv_s2_latent.hip"
WANT = {
    "masic_latent_s2_f16k_supported": (I, [I] * 3),
    "masic_latent_s2_f16k_preferred": (I, [I] * 3),
    "masic_latent_s2_f16k_fwd": (I, [P] * 8 + [I] * 7 + [P]),
    "masic_latent_s2_f16k_kernel_name": (I, [I] * 3 + [C, S]),
}


def test_header_parses_to_prototypes_only():
    signatures, constants, structs = _parsed(HEADER)
    assert not constants and not structs
    assert set(signatures) == set(WANT)


def test_names_are_its_own():
    from masic_amd import _lib
    for name in _parsed(HEADER)[0]:
        assert name.startswith(PREFIX) and name not in _lib.SIGNATURES, name


def test_signatures():
    sig = _parsed(HEADER)[0]
    for name, (res, args) in WANT.items():
        assert sig[name] == (res, args), name


def test_bound_on_the_library():
    from masic_amd import _lib, latent
    assert latent.HEADER_PATH == os.path.join(ROOT, "include", HEADER)
    assert set(latent.SIGNATURES) == set(_parsed(HEADER)[0])
    for name, (res, args) in latent.SIGNATURES.items():
        fn = getattr(_lib.lib, name)                        # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == list(args)


def test_kernel_source_is_built():
    with open(os.path.join(ROOT, "masic_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), flags=re.M).group(1).split()
    assert SOURCE in srcs and os.path.exists(os.path.join(ROOT, "masic_amd", "csrc", SOURCE))


def test_shape_queries_need_no_gpu():
    """supported / preferred / kernel_name are host arithmetic: the shape limit, and the rule of `preferred` -- a threshold on the
    workgroup count (tiles of 4 x 32 output pixels, times B) that says 0 at two workgroups and 1 at the 64 of the benchmark shape"""
    from masic_amd import _lib, latent
    lib = _lib.lib
    assert lib.masic_latent_s2_f16k_supported(1, 5, 7) == 1 and lib.masic_latent_s2_f16k_supported(8, 64, 64) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 2048, 2048)):
        assert lib.masic_latent_s2_f16k_supported(*bad) == 0 and lib.masic_latent_s2_f16k_preferred(*bad) == 0, bad
    assert latent.kernel_name(8, 64, 64) == latent.kernel_name(1, 5, 7) == "conv_s2_latent_f16k"
    with pytest.raises(RuntimeError, match="bad arguments"):
        latent.kernel_name(0, 8, 8)
    assert lib.masic_latent_s2_f16k_kernel_name(1, 5, 7, ctypes.create_string_buffer(8), 8) != 0       # a buffer too small
    assert not latent.preferred(None, 2, 8, 16) and latent.preferred(None, 8, 64, 64)
    took = [bool(lib.masic_latent_s2_f16k_preferred(8, 8 * k, 2)) for k in range(1, 33)]                 # 8 k workgroups
    assert took == sorted(took) and took[-1], "one threshold on the workgroup count"
    assert (latent.IN_CHANNELS, latent.OUT_CHANNELS, latent.PACKED_BYTES) == (128, 192, 2 * 8 * 5 * 20480)
    assert latent.out_hw(5, 7) == (3, 4) and latent.out_hw(33, 130) == (17, 65)
