"""include/masic_deconv.h: a header of libmasic_hip.so beside the pinned include/masic_hip.h (tests/test_cpu_abi.py, which this leaves as
it is) -- prototypes only, every name a masic_deconv_* entry point of its own, each exported by the library, and the kernel file in the
build."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "masic_deconv.h")


def _parsed():
    from masic_amd import _lib
    with open(HEADER) as f:
        return _lib.parse_header(f.read(), header="masic_deconv.h")


def test_header_parses_to_prototypes_only():
    signatures, constants, structs = _parsed()
    assert not constants and not structs
    assert set(signatures) == {"masic_deconv_igdn_f16k_supported", "masic_deconv_igdn_f16k_fwd", "masic_deconv_igdn_f16k_kernel_name"}


def test_names_are_its_own():
    from masic_amd import _lib
    for name in _parsed()[0]:
        assert name.startswith("masic_deconv_") and name not in _lib.SIGNATURES, name


def test_signatures():
    import ctypes
    sig = _parsed()[0]
    assert sig["masic_deconv_igdn_f16k_supported"] == (ctypes.c_int, [ctypes.c_int] * 3)
    assert sig["masic_deconv_igdn_f16k_fwd"] == (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p])
    assert sig["masic_deconv_igdn_f16k_kernel_name"] == (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_char_p, ctypes.c_size_t])


def test_bound_on_the_library():
    from masic_amd import _lib, deconv
    assert set(deconv.SIGNATURES) == set(_parsed()[0])
    for name, (res, args) in deconv.SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)


def test_shape_answers_need_no_device():
    """host code only: which shapes run, and which kernel each takes"""
    from masic_amd import _lib, deconv
    assert _lib.lib.masic_deconv_igdn_f16k_supported(8, 128, 128) == 1
    assert _lib.lib.masic_deconv_igdn_f16k_supported(0, 128, 128) == 0
    assert _lib.lib.masic_deconv_igdn_f16k_supported(1, 4096, 4096) == 0
    assert deconv.kernel_name(8, 128, 128) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 64, 64) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 32, 32) == "deconv_igdn_f16k<8, 1, 5>"
    assert deconv.kernel_name(8, 32, 32, tile=1) == "deconv_igdn_f16k<8, 2, 5>"


def test_kernel_source_is_built():
    with open(os.path.join(ROOT, "masic_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), flags=re.M).group(1).split()
    assert "deconv_igdn.hip" in srcs and os.path.exists(os.path.join(ROOT, "masic_amd", "csrc", "deconv_igdn.hip"))
