"""include/masic_d2s.h, a side header of libmasic_hip.so (masic_amd/d2s_layer.py, masic_amd/csrc/d2s_layer.hip): the checks
tests/test_cpu_latent_header.py makes for masic_latent.h -- prototypes only, every name an entry point of its own under the header's
prefix, the signatures, each bound on the library with the types the header states, the kernel's source in the build -- and what the
module answers and refuses without a GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests.test_cpu_side_headers import ROOT, C, F, I, P, S, _parsed       # noqa: F401 (F: the header has no float argument by value)

HEADER, PREFIX, SOURCE = "masic_d2s.h", "masic_d2s_", "d2s_layer.hip"
WANT = {
    "masic_d2s_layer_f16k_supported": (I, [I] * 3),
    "masic_d2s_layer_f16k_preferred": (I, [I] * 3),
    "masic_d2s_layer_f16k_fwd": (I, [P] * 4 + [I] * 7 + [P]),
    "masic_d2s_layer_f16k_kernel_name": (I, [I] * 3 + [C, S]),
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
    from masic_amd import _lib, d2s_layer
    assert d2s_layer.HEADER_PATH == os.path.join(ROOT, "include", HEADER)
    assert set(d2s_layer.SIGNATURES) == set(_parsed(HEADER)[0])
    for name, (res, args) in d2s_layer.SIGNATURES.items():
        fn = getattr(_lib.lib, name)                        # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == list(args)


def test_kernel_source_is_built():
    with open(os.path.join(ROOT, "masic_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), flags=re.M).group(1).split()
    assert SOURCE in srcs and os.path.exists(os.path.join(ROOT, "masic_amd", "csrc", SOURCE))


def test_shape_queries_need_no_gpu():
    """supported / preferred / kernel_name are host arithmetic: the shape limit, and the rule of `preferred` -- never a shape that
    conv_f16k runs on another row than the one whose stream and sum order the kernel shares, and one threshold on that row's tile count"""
    from masic_amd import _lib, d2s_layer
    lib = _lib.lib
    assert lib.masic_d2s_layer_f16k_supported(1, 5, 7) == 1 and lib.masic_d2s_layer_f16k_supported(8, 256, 256) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 4096, 4096)):
        assert lib.masic_d2s_layer_f16k_supported(*bad) == 0 and lib.masic_d2s_layer_f16k_preferred(*bad) == 0, bad
    assert d2s_layer.kernel_name(8, 256, 256) == d2s_layer.kernel_name(1, 5, 7) == "d2s_layer_f16k"
    with pytest.raises(RuntimeError, match="bad arguments"):
        d2s_layer.kernel_name(0, 8, 8)
    assert lib.masic_d2s_layer_f16k_kernel_name(1, 5, 7, ctypes.create_string_buffer(8), 8) != 0       # a buffer too small
    shapes = [(8, 256, 256), (8, 128, 128), (1, 256, 256), (57, 65, 65), (88, 33, 65), (512, 32, 32), (511, 32, 32), (4096, 16, 31),
              (8, 255, 225), (8, 256, 224), (16, 192, 160), (2, 512, 512), (1, 5, 7)]
    for s in shapes:
        if d2s_layer.preferred(None, *s):
            assert d2s_layer.takes_row(*s), s
    assert d2s_layer.takes_row(8, 256, 256) and d2s_layer.takes_row(57, 65, 65) and d2s_layer.takes_row(88, 33, 65)
    assert not d2s_layer.takes_row(8, 128, 128) and not d2s_layer.preferred(None, 8, 128, 128) and not d2s_layer.preferred(None, 1, 256, 256)
    took = [bool(lib.masic_d2s_layer_f16k_preferred(8 * k, 32, 32)) for k in range(1, 129)]             # 8 k tiles of conv_f16k
    assert took == sorted(took), "one threshold on the tile count"
    assert (d2s_layer.IN_CHANNELS, d2s_layer.MAX_OUT_CHANNELS, d2s_layer.PACKED_BYTES) == (128, 8, 8 * 5 * 2 * 4096)


def _layer(**kw):
    d = dict(transposed_conv=True, masked_conv=False, in_channels=128, out_channels=3, _geometry=lambda: (5, 5, 2, 2),
             d2s_supported=lambda B, Hi, Wi: True)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_supported_and_launch_refuse_other_forms():
    from masic_amd import _lib, d2s_layer
    B, H, W = 8, 256, 256
    assert d2s_layer.supported(_layer(), B, H, W)
    assert not d2s_layer.supported(_layer(), 8, 128, 128)                                # conv_f16k's 32-channel-chunk row: another stream
    assert not d2s_layer.supported(_layer(), B, H, W, in_ctot=160, in_coff=16)           # a channel view of the input
    assert not d2s_layer.supported(_layer(), B, H, W, in_ctot=160)
    assert not d2s_layer.supported(_layer(in_channels=96), B, H, W)                      # other widths
    assert not d2s_layer.supported(_layer(out_channels=9), B, H, W)
    assert not d2s_layer.supported(_layer(transposed_conv=False), B, H, W)
    assert not d2s_layer.supported(_layer(_geometry=lambda: (3, 3, 2, 1)), B, H, W)
    assert not d2s_layer.supported(_layer(), B, H, W, prec=_lib.PREC_FP8)
    assert not d2s_layer.supported(_layer(), B, H, W, prec=_lib.PREC_F32)
    assert not d2s_layer.supported(_layer(d2s_supported=lambda B, Hi, Wi: False), B, H, W)
    # launch: the checks that come before anything touches a device
    x = torch.empty(1 * 128 * 5 * 7, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="CUDA buffer"):
        d2s_layer.launch(x, torch.empty(d2s_layer.PACKED_BYTES // 2, dtype=torch.int16), None, 1, 5, 7, 3)
    meta = torch.device("meta")
    xm = types.SimpleNamespace(dtype=torch.int16, is_cuda=True, numel=lambda: 128 * 5 * 7, device=meta)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: d2s_layer.PACKED_BYTES // 2 - 1, device=meta)
    with pytest.raises(RuntimeError, match="slab stream"):                               # a wrong pack size
        d2s_layer.launch(xm, pm, None, 1, 5, 7, 3)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: d2s_layer.PACKED_BYTES // 2, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="slab stream"):                               # a pack on another device
        d2s_layer.launch(xm, pm, None, 1, 5, 7, 3)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: d2s_layer.PACKED_BYTES // 2, device=meta)
    with pytest.raises(RuntimeError, match="bias must be a CUDA"):                       # a bias on another device
        d2s_layer.launch(xm, pm, torch.zeros(32), 1, 5, 7, 3)
