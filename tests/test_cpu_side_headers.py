"""The side headers of libmasic_hip.so -- the ten files of HEADERS beside the pinned include/masic_hip.h (tests/test_cpu_abi.py, which this
leaves as it is): each holds prototypes only, every name an entry point of its own under the header's prefix, each bound on the library
by _lib.bind_header with the types the header states, and the kernels' sources are in the build.  Then bind_header's refusals, on
headers written for the test."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, P, F, S, C, D, U32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_double, ctypes.c_uint32
# module of masic_amd -> (header, prefix, {name: (restype, argtypes)}, kernel source or None)
HEADERS = {
    "align": ("masic_align.h", "masic_align_", {
        "masic_align_workspace_bytes": (S, [I, I]),
        "masic_align_patches": (I, [P] * 6 + [I] * 6 + [F, P])}, None),
    "deconv": ("masic_deconv.h", "masic_deconv_", {
        "masic_deconv_igdn_f16k_supported": (I, [I] * 3),
        "masic_deconv_igdn_f16k_fwd": (I, [P] * 5 + [I] * 5 + [P]),
        "masic_deconv_igdn_f16k_kernel_name": (I, [I] * 5 + [C, S])}, "deconv_igdn.hip"),
    "conv_s2": ("masic_conv_s2.h", "masic_conv_s2_", {
        "masic_conv_s2_gdn_f16k_supported": (I, [I] * 3),
        "masic_conv_s2_gdn_f16k_fwd": (I, [P] * 5 + [I] * 3 + [P]),
        "masic_conv_s2_gdn_f16k_kernel_name": (I, [I] * 3 + [C, S])}, "conv_s2_gdn.hip"),
    "latent": ("masic_latent.h", "masic_latent_", {
        "masic_latent_s2_f16k_supported": (I, [I] * 3),
        "masic_latent_s2_f16k_preferred": (I, [I] * 3),
        "masic_latent_s2_f16k_fwd": (I, [P] * 8 + [I] * 7 + [P]),
        "masic_latent_s2_f16k_kernel_name": (I, [I] * 3 + [C, S])}, "conv_s2_latent.hip"),
    "d2s_layer": ("masic_d2s.h", "masic_d2s_", {
        "masic_d2s_layer_f16k_supported": (I, [I] * 3),
        "masic_d2s_layer_f16k_preferred": (I, [I] * 3),
        "masic_d2s_layer_f16k_fwd": (I, [P] * 4 + [I] * 7 + [P]),
        "masic_d2s_layer_f16k_kernel_name": (I, [I] * 3 + [C, S])}, "d2s_layer.hip"),
    "metrics": ("masic_metrics.h", "masic_metrics_", {
        "masic_metrics_pair_rd_workspace_bytes": (S, [I]),
        "masic_metrics_pair_rd": (I, [P] * 4 + [S, P, P, I, I, P, P, P]),
        "masic_metrics_u8_sse_workspace_bytes": (S, [I]),
        "masic_metrics_u8_sse": (I, [P, P, S, I, P, P, P])}, "metrics.hip"),
    "bands": ("masic_bands.h", "masic_bands_", {
        "masic_bands_skinny_ctx_fwd_batch": (I, [P] * 3 + [I] * 5 + [P] + [I] * 3 + [P])}, "skinny.hip"),
    "bandfold": ("masic_bandfold.h", "masic_bandfold_", {
        "masic_bandfold_fold": (I, [P, P] + [I] * 5 + [P]),
        "masic_bandfold_unfold": (I, [P, P] + [I] * 7 + [P, I, I, P]),
        "masic_bandfold_unfold_f16k": (I, [P, P] + [I] * 7 + [P, I, I, P]),
        "masic_bandfold_max_blocks": (I, [])}, "band_fold.hip"),
    "refine": ("masic_refine.h", "masic_refine_", {
        "masic_refine_noise": (I, [P, P, I, U32, P, P, P]),
        "masic_refine_adam": (I, [P, P, P, P, P, I, D, P, P]),
        "masic_refine_keep_best": (I, [P, P, P, I, P, P, P]),
        "masic_refine_rd_seeds": (I, [P] * 4 + [S, P, P, I, I, D, D] + [P] * 5)}, "refine.hip"),
    "refine_budget": ("masic_budget.h", "masic_budget_", {
        "masic_budget_rd_seeds": (I, [P] * 4 + [S, P, P, I, I, D, D] + [P] * 6),
        "masic_budget_select": (I, [P, P, P, I] + [P] * 6),
        "masic_budget_mu": (I, [P, P, P, I, D, D, D, P])}, "refine_budget.hip"),
}
BOUND_AS = {"refine_budget": ("refine", "BUDGET_")}     # row -> (module, prefix of its HEADER_PATH / SIGNATURES) where not (row, "")
MODULES = sorted(HEADERS)


def _parsed(header):
    from masic_amd import _lib
    with open(os.path.join(ROOT, "include", header)) as f:
        return _lib.parse_header(f.read(), header=header)


@pytest.mark.parametrize("module", MODULES)
def test_header_parses_to_prototypes_only(module):
    header, _, want, _ = HEADERS[module]
    signatures, constants, structs = _parsed(header)
    assert not constants and not structs
    assert set(signatures) == set(want)


@pytest.mark.parametrize("module", MODULES)
def test_names_are_its_own(module):
    """under the header's prefix, and in no other header: neither the pinned one nor another row's"""
    from masic_amd import _lib
    header, prefix, _, _ = HEADERS[module]
    elsewhere = set(_lib.SIGNATURES).union(*(HEADERS[m][2] for m in MODULES if m != module))
    for name in _parsed(header)[0]:
        assert name.startswith(prefix) and name not in elsewhere, name


@pytest.mark.parametrize("module", MODULES)
def test_signatures(module):
    header, _, want, _ = HEADERS[module]
    sig = _parsed(header)[0]
    for name, (res, args) in want.items():
        assert sig[name] == (res, args), name


@pytest.mark.parametrize("module", MODULES)
def test_bound_on_the_library(module):
    from masic_amd import _lib
    header, _, want, _ = HEADERS[module]
    name, attr = BOUND_AS.get(module, (module, ""))
    mod = importlib.import_module("masic_amd." + name)
    assert getattr(mod, attr + "HEADER_PATH") == os.path.join(ROOT, "include", header)
    signatures = getattr(mod, attr + "SIGNATURES")
    assert signatures == _parsed(header)[0] == want
    for name, (res, args) in signatures.items():
        fn = getattr(_lib.lib, name)                        # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == list(args)


@pytest.mark.parametrize("module", [m for m in MODULES if HEADERS[m][3]])
def test_kernel_source_is_built(module):
    source = HEADERS[module][3]
    with open(os.path.join(ROOT, "masic_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), flags=re.M).group(1).split()
    assert source in srcs and os.path.exists(os.path.join(ROOT, "masic_amd", "csrc", source))


# ------------------------------------------------------------------------------------------ bind_header's refusals
def _bind(tmp_path, text, prefix="masic_side_"):
    from masic_amd import _lib
    path = tmp_path / "masic_side.h"
    if text is not None:
        path.write_text(text)
    return _lib.bind_header(str(path), prefix)


def test_bind_header_missing_file(tmp_path):
    with pytest.raises(ImportError, match=r"^masic_amd\.side: .*masic_side\.h is missing: the binding is derived from it"):
        _bind(tmp_path, None)


def test_bind_header_refuses_a_constant(tmp_path):
    with pytest.raises(ValueError, match=r"^masic_side\.h: declares constants or structs"):
        _bind(tmp_path, "#define MASIC_X 1\nint masic_side_f(int a);\n")


def test_bind_header_refuses_a_name_outside_the_prefix(tmp_path):
    with pytest.raises(ValueError, match=r"^masic_side\.h: masic_other_f is not a masic_side_\* entry point of its own"):
        _bind(tmp_path, "int masic_other_f(int a);\n")


def test_bind_header_refuses_a_name_of_the_pinned_header(tmp_path):
    from masic_amd import _lib
    assert "masic_version" in _lib.SIGNATURES
    before = (_lib.lib.masic_version.restype, _lib.lib.masic_version.argtypes)
    with pytest.raises(ValueError, match=r"^masic_side\.h: masic_version is not a masic_\* entry point of its own"):
        _bind(tmp_path, "int masic_version(int a);\n", prefix="masic_")
    assert (_lib.lib.masic_version.restype, _lib.lib.masic_version.argtypes) == before and _lib.lib.masic_version() == 1


def test_bind_header_symbol_not_exported(tmp_path):
    with pytest.raises(AttributeError, match="masic_side_nosuch"):
        _bind(tmp_path, "int masic_side_nosuch(int a);\n")
