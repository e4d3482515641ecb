"""CPU tests of the deterministic mode (masic_amd/determinism.py): the C ABI declares and exports every `_det` entry point, the Python
switch and its tie to torch.use_deterministic_algorithms, and the slab workspace sizes at the training shapes."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_SYMBOLS = [
    "masic_conv2d_wgrad_det_workspace_bytes", "masic_conv2d_wgrad_det", "masic_conv2d_wgrad_bf16in_det",
    "masic_conv3x3_wgrad_f16k_det_workspace_bytes", "masic_conv3x3_wgrad_f16k_det",
    "masic_conv5x5_wgrad_f16k_det_workspace_bytes", "masic_conv5x5_wgrad_f16k_det",
    "masic_gemm_wgrad_bias_f16k_det_workspace_bytes", "masic_gemm_wgrad_bias_f16k_det",
    "masic_warp_perspective_bwd_gather_det_workspace_bytes", "masic_warp_perspective_bwd_gather_det",
]
CAP = 64 << 20


def test_header_declares_and_library_exports_every_det_entry_point():
    from masic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "masic_hip.h")).read()
    for name in DET_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), f"{name} is not declared in include/masic_hip.h"
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), f"{name} is not exported by the library"
    assert _lib.lib.masic_version() == 1


def test_switch_context_manager_and_torch_flag():
    from masic_amd import determinism as D
    assert not torch.are_deterministic_algorithms_enabled()
    prev = D._ON
    try:
        D.set_deterministic(False)
        assert not D.is_deterministic()
        D.set_deterministic(True)
        assert D.is_deterministic()
        with D.deterministic(False):
            assert not D.is_deterministic()
            with D.deterministic():
                assert D.is_deterministic()
            assert not D.is_deterministic()
        assert D.is_deterministic()
        D.set_deterministic(False)
        with pytest.raises(ValueError):
            with D.deterministic(True):
                assert D.is_deterministic()
                raise ValueError("boom")
        assert not D.is_deterministic(), "the context manager restores the previous value after an exception"
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            assert D.is_deterministic(), "torch.use_deterministic_algorithms turns the mode on"
            with D.deterministic(False):
                assert D.is_deterministic(), "the effective mode is the module flag OR torch's switch"
        finally:
            torch.use_deterministic_algorithms(False)
        assert not D.is_deterministic()
    finally:
        D.set_deterministic(prev)


def _hsic_layers(B, H, W, N=128, M=192):
    """(Cin, Cout, k, s, transposed, Hi, Wi) of HSIC(128,192,5)'s strided / 1x1 layers on a B x 3 x H x W batch"""
    h4, w4 = H // 16, W // 16
    out = []
    for i, (ci, co) in enumerate([(3, N), (N, N), (N, N), (N, M)]):          # g_a
        out.append((ci, co, 5, 2, False, H >> i, W >> i))
    for i, (ci, co) in enumerate([(M, N), (N, N), (N, N), (N, 3)]):          # g_s
        out.append((ci, co, 5, 2, True, h4 << i, w4 << i))
    out += [(M, N, 3, 1, False, h4, w4), (N, N, 5, 2, False, h4, w4), (N, N, 5, 2, False, h4 // 2, w4 // 2)]      # h_a
    out += [(N, M, 5, 2, True, h4 // 4, w4 // 4), (M, M * 3 // 2, 5, 2, True, h4 // 2, w4 // 2), (M * 3 // 2, 2 * M, 3, 1, False, h4, w4)]
    out += [(M, 2 * M, 5, 1, False, h4, w4)]                                   # context model (masked 5x5)
    out += [(4 * M, 4 * M, 1, 1, False, h4, w4), (2 * M * 10 // 3, 2 * M * 8 // 3, 1, 1, False, h4, w4)]   # entropy-parameter 1x1
    out += [(6, 3, 5, 1, False, H, W), (6, 3, 5, 1, True, H, W)]              # pre_conv / after_conv
    return out


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_conv2d_wgrad_det_workspace_sizes_at_training_shapes(prec):
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16, PREC_F32
    B, H, W = 8, 512, 512
    for (Cin, Cout, k, s, tr, Hi, Wi) in _hsic_layers(B, H, W):
        d = ops.make_conv_desc(B, Cin, Hi, Wi, Cout, k, k, s, k // 2, transposed=tr, prec=PREC_BF16 if prec == "bf16" else PREC_F32)
        n = ops._desc_query("masic_conv2d_wgrad_det_workspace_bytes", d)
        wb = Cin * Cout * k * k * 4
        assert n > 0 and n % wb == 0, (Cin, Cout, k, s, tr, n, wb)
        assert n <= max(CAP, wb), (Cin, Cout, k, s, tr, n)


def test_f16k_det_workspace_sizes_at_training_shapes():
    from masic_amd import ops
    B, H, W = 8, 512, 512
    # Independent_EN: 3x3 stride-1 layers at full resolution (CQE stage); the hyper / context 5x5 and 3x3 layers at latent resolution
    for (ks, Cin, Cout, h, w) in [(3, 3 * 2, 96, H, W), (3, 96, 96, H, W), (3, 96, 64, H, W), (3, 64, 32, H, W), (3, 32, 32, H, W),
                                  (3, 192, 288, H // 16, W // 16), (5, 192, 384, H // 16, W // 16), (5, 128, 128, H // 16, W // 16)]:
        if Cin % 32 or Cout % 32:
            continue
        n = ops._int_query(f"masic_conv{ks}x{ks}_wgrad_f16k_det_workspace_bytes", B, Cin, Cout, h, w)
        wb = ks * ks * Cin * Cout * 4
        assert n > 0 and n % wb == 0 and n <= CAP, (ks, Cin, Cout, n)
    for (bias_of, CA, CQ, hw) in [(0, 1152, 768, 32 * 32), (1, 768, 768, 32 * 32), (2, 640, 512, 32 * 32), (1, 96, 160, 63)]:
        n = ops._int_query("masic_gemm_wgrad_bias_f16k_det_workspace_bytes", bias_of, B, CA, CQ, hw)
        assert n > 0 and n % (CA * CQ * 4) == 0 and n <= CAP + CA * CQ * 4, (bias_of, CA, CQ, n)
    assert ops._int_query("masic_conv3x3_wgrad_f16k_det_workspace_bytes", 0, 32, 32, 8, 8) == 0

