"""conv_s2_gdn_f16k's host-only answers, and the kernel's compile-time patch geometry against what the library's plan gives for the
layer.  (What include/masic_conv_s2.h declares and how it is bound: tests/test_cpu_side_headers.py.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_answers_need_no_device():
    """host code only: which shapes run, and which kernel each takes"""
    from masic_amd import _lib, conv_s2
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(8, 256, 256) == 1
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(1, 5, 7) == 1
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(0, 128, 128) == 0
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(70000, 128, 128) == 0
    assert _lib.lib.masic_conv_s2_gdn_f16k_supported(1, 4096, 4096) == 0
    assert conv_s2.kernel_name(8, 256, 256) == "conv_s2_gdn_f16k"
    assert conv_s2.kernel_name(8, 128, 128) == "conv_s2_gdn_f16k"
    assert conv_s2.out_hw(5, 7) == (3, 4) and conv_s2.out_hw(33, 130) == (17, 65)


def _constants():
    """the constexpr integers of conv_s2_gdn.hip, evaluated (they are products and sums of literals and of each other)"""
    with open(os.path.join(ROOT, "masic_amd", "csrc", "conv_s2_gdn.hip")) as f:
        text = f.read()
    env = {}
    for line in re.findall(r"^constexpr int (CS_[^;]*);", text, flags=re.M):
        for name, expr in re.findall(r"(CS_\w+)\s*=\s*([^,]+)", line):
            env[name] = eval(expr.replace("/", "//"), {}, env)          # noqa: S307 (the repository's own source)
    return env


def test_geometry_is_the_plan_of_conv_f16k():
    """The tile, patch and stream constants the kernel is compiled with are what conv_f16k's plan line gives for the layer where it picks
    the 8 x 32 tile (its kernel, ring, chunks, steps per chunk, patch row length, records per k-half plane, LDS beside the tap table and
    the sink), and the packed stream is 8 x 5 x 20480 bytes; the tap offsets are those of its tap table."""
    import ctypes
    from masic_amd import _lib, conv_s2
    from tests import f16k_ref as R
    k = _constants()
    c = R.case_of((8, 128, 256, 256, 128, 5, 2, 0, 0), flags=R.F16K_GDN)
    d = R.desc_of(c)
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.lib.masic_conv_f16k_plan_name(ctypes.byref(d), R.F16K_GDN, buf, 512), "conv_f16k_plan_name")
    name, grid, block, lds, ints = [s.strip() for s in buf.value.decode().split("|")]
    assert name == "conv_f16k<1, 5, 2, 6, 1, true, 4, 1, false>" and int(block) == 512
    TW, TH, NP, KS, T, D, L, msplit, ntiles, tiles_w, nphase, ncb, nchunks, spc, PW, PWh, NPIXp, xcd = map(int, ints.split())
    assert (TW, TH, NP, KS, T, D, L, msplit, nphase, ncb) == (k["CS_TW"], k["CS_TH"], 1, 1, k["CS_T"], k["CS_D"], 1, 1, 1, 1)
    assert (nchunks, spc, nchunks * spc) == (k["CS_CHUNKS"], 5, k["CS_STEPS"])
    assert (PW, PWh, NPIXp) == (k["CS_PW"], k["CS_PWH"], k["CS_NPIX"]) == (67, 34, 1312)
    assert k["CS_PH"] == 19 and k["CS_HALF"] == 19 * 34 and k["CS_NINSTR"] == 41 and k["CS_PSP"] == 6 and k["CS_NWS"] == 3
    assert [int(v) for v in grid.split(",")] == [ntiles, 1, 8] and ntiles == 16 * 4 and tiles_w == 4 and xcd == 1
    # conv_f16k: ring + patch buffers + 1 KiB sink + tap table; here: ring + patch buffers + beta^ + bias
    assert int(lds) - 1024 - 256 == k["CS_LDS"] - 1024 == k["CS_NWS"] * k["CS_WST"] + 2 * k["CS_PB"]
    assert k["CS_LDS"] <= 160 * 1024
    assert _lib.lib.masic_conv_f16k_packed_bytes(ctypes.byref(d)) == conv_s2.PACKED_BYTES == k["CS_STEPS"] * k["CS_WST"]
    # tap (ti, tj): record ((tj & 1) PH + ti) PWh + (tj >> 1) of the patch image -- the table conv_f16k writes for a stride-2 layer with
    # patch origin (-pad, -pad) -- as the kernel forms it: cs_tap(tj) + ti * PWh records
    with open(os.path.join(ROOT, "masic_amd", "csrc", "conv_s2_gdn.hip")) as f:
        assert "return ((tj & 1) * CS_HALF + (tj >> 1)) * 16;" in f.read()
    for ti in range(5):
        for tj in range(5):
            assert ((tj & 1) * k["CS_HALF"] + (tj >> 1)) + ti * k["CS_PWH"] == ((tj & 1) * 19 + ti) * 34 + (tj >> 1)
    # every record a tile's 256 output pixels read lies inside the 2 x 19 x 34 records a chunk's DMA fills
    top = max(((tj & 1) * 19 + ti + 2 * r) * 34 + (tj >> 1) + col for ti in range(5) for tj in range(5) for r in range(8) for col in range(32))
    assert top < 2 * k["CS_HALF"] <= k["CS_NPIX"]
