"""The ctypes binding (masic_amd/_lib.py) is derived from include/masic_hip.h; tests/golden/abi.json holds what the C compiler says of
the header's structs and constants and the derived signatures (tests/golden/make_abi_golden.py).  No GPU and no compiler needed."""
import ctypes
import importlib.util
import json
import os
import re

import pytest
import torch  # noqa: F401  (before masic_amd._lib, as everywhere: libmasic_hip.so must bind to the HIP runtime torch has loaded)

from masic_amd import _lib, ops
from masic_amd._lib import ConvDesc, GemmGroup, lib, parse_header

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_abi_golden", os.path.join(HERE, "golden", "make_abi_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(G.OUT) as _f:
    ABI = json.load(_f)
P = ctypes.c_void_p


def test_signatures_are_the_recorded_ones():
    assert G.signature_strings(_lib.SIGNATURES) == ABI["signatures"]


def test_every_function_carries_its_signature():
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_every_prototype_of_the_header_is_bound():
    with open(_lib.HEADER_PATH) as f:
        code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    declared = set(re.findall(r"(masic_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SIGNATURES) and len(declared) == len(_lib.SIGNATURES) == len(ABI["signatures"])


def test_structs_have_the_compilers_layout():
    assert set(_lib.STRUCTS) == set(ABI["structs"])
    for name, want in ABI["structs"].items():
        cls = _lib.STRUCTS[name]
        assert issubclass(cls, ctypes.Structure) and ctypes.sizeof(cls) == want["size"], name
        got = [[f, getattr(cls, f).offset, getattr(cls, f).size] for f, _ in cls._fields_]
        assert got == want["fields"], name
    for alias, name in (("ConvDesc", "masic_conv_desc_t"), ("CodeStream", "masic_code_stream_t"), ("GemmGroup", "masic_gemm_group_t"),
                        ("F16kMultiOut", "masic_f16k_multi_out_t")):
        assert getattr(_lib, alias) is _lib.STRUCTS[name]
    d = ConvDesc(B=2, prec=_lib.PREC_BF16)              # keyword construction, and an instance __dict__ (ops._desc_query keeps a memo there)
    d.__dict__["_memo"] = {}
    assert (d.B, d.prec, d.Cin) == (2, 1, 0)


def test_numpy_records_have_the_compilers_layout():
    for dtype, fields, name in ((ops._view_desc_dtype(), ops.VIEW_DESC_FIELDS, "masic_view_desc_t"),
                                (ops._udh_view_desc_dtype(), ops.UDH_VIEW_DESC_FIELDS, "masic_udh_view_desc_t")):
        want = ABI["structs"][name]
        assert dtype.itemsize == want["size"] and dtype.names == fields == tuple(f for f, _, _ in want["fields"])
        assert [[f, dtype.fields[f][1], dtype.fields[f][0].itemsize] for f in fields] == want["fields"]
        assert all(dtype.fields[f][0].kind in "iu" for f in fields)


def test_constants_have_the_compilers_values():
    assert _lib.CONSTANTS == ABI["constants"]
    for name, value in ABI["constants"].items():
        assert getattr(_lib, name) == value and type(getattr(_lib, name)) is int, name
    used = ("ACT_NONE ACT_RELU ACT_LEAKY ACT_SOFTMAX_C INOP_NONE INOP_ABS INOP_ROUND PREC_F32 PREC_BF16 PREC_FP8 F16K_GDN F16K_NOSPLIT "
            "F16K_MULTI WGRAD_DET WGRAD_IN16 WGRAD_CLEAN CONV_GATE CONV_RES1 CONV_RES2 CONV_F16K_OUT SSIM_MS SSIM_SIZE_AVERAGE SSIM_NONNEG "
            "EB_PARAMS_PER_CHANNEL")
    assert set(used.split()) <= set(ABI["constants"])


@pytest.mark.parametrize("snippet, offender", [
    ("int masic_a(const float* x, long n);", "masic_a"),                                      # a scalar outside the closed map
    ("int masic_a(foo_t* x);", "masic_a"),                                                    # ... also behind a pointer
    ("short masic_a(void);", "masic_a"),
    ("typedef struct { int32_t a; wchar_t b; } masic_s_t;", "masic_s_t"),                     # unknown type in a struct field
    ("typedef struct { int32_t a[4]; } masic_s_t;", "masic_s_t"),
    ("int masic_a(int n);\nint masic_b(void (*cb)(int), int n);\nint masic_c(void);", "masic_b"),   # a parameter list that does not split
    ("int masic_a(int n, int);", "masic_a"),
    ("int masic_a(masic_conv_desc_t d);", "masic_a"),
    ("#define MASIC_X (1 << 3)", "MASIC_X"),
    ("enum { MASIC_A = 1, OTHER = 2 };", "OTHER"),
    ("int masic_a(int n)\nint masic_b(int n);", "masic_a"),                                   # a missing semicolon
    ("int masic_b(int n);\nint masic_a(int n)", "masic_a"),
    ("int masic_a(int n);\nstatic int x = 3;", "static int x = 3"),                           # something that is no prototype
])
def test_parser_refuses_what_it_does_not_understand(snippet, offender):
    with pytest.raises(ValueError, match=rf"\b{offender}\b"):
        parse_header("typedef struct { int32_t B; } masic_conv_desc_t;\n" + snippet)


def test_parser_accepts_the_forms_the_header_uses():
    S, C, T = parse_header("""
        /* masic_ghost(int) in a comment; and a semicolon */
        #ifndef MASIC_HIP_H
        #define MASIC_HIP_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define MASIC_FLAG 4     /* masic_ghost2( */
        enum { MASIC_ZERO = 0, MASIC_NEG = -3,
               MASIC_NEXT /* unnumbered */ };
        typedef struct masic_gemm_group { const void* x; float s; int32_t a, b;   // masic_ghost3(
        } masic_gemm_group_t;
        typedef struct { uint64_t offset; uint32_t w; } masic_view_desc_t;
        int masic_multi(const float* x,
                        const masic_gemm_group_t* g, size_t n,
                        double d, float f, void* stream);
        int masic_none(void);
        const char* masic_text(void);
        void masic_void(char* buf, const float* const* liks, const unsigned char* m, int32_t* out, const masic_view_desc_t* dev, void** h);
        #ifdef __cplusplus
        }
        #endif
        #endif
        """)
    g = T["masic_gemm_group_t"]
    assert list(T) == ["masic_gemm_group_t", "masic_view_desc_t"]
    assert g._fields_ == [("x", P), ("s", ctypes.c_float), ("a", ctypes.c_int32), ("b", ctypes.c_int32)]
    assert T["masic_view_desc_t"]._fields_ == [("offset", ctypes.c_uint64), ("w", ctypes.c_uint32)]
    assert C == {"FLAG": 4, "ZERO": 0, "NEG": -3, "NEXT": -2}
    assert S == {"masic_multi": (ctypes.c_int, [P, ctypes.POINTER(g), ctypes.c_size_t, ctypes.c_double, ctypes.c_float, P]),
                 "masic_none": (ctypes.c_int, []),
                 "masic_text": (ctypes.c_char_p, []),
                 "masic_void": (None, [ctypes.c_char_p, P, P, P, P, P])}       # a device-resident struct's pointer stays void*


def test_call_sites_arguments_pass_the_argtypes():
    """from_param of every argument form the callers build for a parameter whose type is no longer the hand-written one"""
    def accepts(name, index, value):
        _lib.SIGNATURES[name][1][index].from_param(value)

    desc = {"masic_conv_f16k_supported": 0, "masic_conv_f16k_kernel_name": 0, "masic_conv_f16k_plan_name": 0, "masic_conv_f16k_packed_bytes": 0,
            "masic_conv_f16k_pack_weight": 2, "masic_conv_f16k_fwd": 6, "masic_conv_f16k_gdn_fwd": 8, "masic_conv_f16k_d2s_fwd": 7}
    for name, i in desc.items():
        assert _lib.SIGNATURES[name][1][i] is ctypes.POINTER(ConvDesc), name
        accepts(name, i, ctypes.byref(ConvDesc()))
    accepts("masic_skinny_group_fwd_batch", 0, (GemmGroup * 3)())
    accepts("masic_gemm_f16k_group_fwd", 0, (GemmGroup * 3)())
    accepts("masic_conv_f16k_multi_fwd", 3, ctypes.byref(_lib.F16kMultiOut()))
    for i in (0, 1):
        accepts("masic_gemm_f16k_pack_weights", i, (ctypes.c_void_p * 4)())
    for i in (2, 3, 4):
        accepts("masic_gemm_f16k_pack_weights", i, (ctypes.c_int * 4)())
    accepts("masic_rans_decoder_finished", 1, ctypes.byref(ctypes.c_int()))
    accepts("masic_eb_table_split", 3, (ctypes.c_int * 14)())
    for i in (1, 2):
        accepts("masic_lpips_finish", i, (ctypes.c_int * 5)())
    accepts("masic_rans_decoder_open", 2, ctypes.byref(ctypes.c_void_p()))
    device = ctypes.c_void_p(1 << 40)                       # c_void_p(tensor.data_ptr()): records that live in device memory
    for name, i in (("masic_gmm_cdf_rows_batch", 10), ("masic_rans_decode_step_batch", 1), ("masic_rans_decode_finish_batch", 0),
                    ("masic_rans_encode_channels_batch", 1), ("masic_rans_pack_pairs_batch", 2), ("masic_views_prep", 2),
                    ("masic_udh_views_prep", 4)):
        assert _lib.SIGNATURES[name][1][i] is ctypes.c_void_p, name
        accepts(name, i, device)
        accepts(name, i, 1 << 40)
    with pytest.raises(TypeError):
        accepts("masic_conv_f16k_fwd", 6, device)           # a host struct's parameter is typed
