"""One hard case for every kernel instantiation of CONV_ROWS (masic_amd/csrc/conv.hip), and per tile shape a transposed and a
gate / residual / view case: the tables below, and the search that wrote them.

    python -m tests.conv_row_cases            # runs the search (host plan query only, no GPU) and prints the three tables

What makes a case hard (properties(), read from the integers of the plan line; tests/test_cpu_conv_rows.py asserts them per case):
  batch     B >= 2
  ragged_h  the phase plane's height is no multiple of the tile height TH          (more than one tile along the axis: `tiles`)
  ragged_w  ... its width no multiple of the tile width TW; a VEC4 column needs Wi % 4 == 0, so its width is 32 t + 4, all others 32 t + 1
  cout      Cout is no multiple of the block's channels BM: 24 / 72 / 40 / 120 under the 32 / 96 / 64 / 128-wide tiles (the last within
            choose_cfg's 10 % padding rule)
  k_chunks  Cin > KC and Cin % KC != 0: more than one K chunk, the last one partial.  The search takes Cin = 2 KC + 1 with KC the chunk
            the geometry allows once Cin no longer limits it: two whole chunks (both LDS buffers of the float32 kernel are reused) and a
            last chunk of one channel (odd: the float32 MFMA contracts channel pairs).
A case is the smallest output (B * Ho * Wo at the Cout above) among B in {2, 3}, heights (n - 1) TH + 1 and widths (m - 1) 32 + 1 (or + 4)
with n, m >= 2 that selects its instantiation with every property; among the layer kinds that do so at that size the first of KINDS[in_op].
Where choose_cfg allows no such case the search gives up k_chunks (largest Cin that keeps the column) or a property its caller names,
and the entry's last field holds the property given up and the rule that forces it.  No row case needed that: a bf16 PF column, which
needs PH * PW * KC / 8 <= 1024, is reached at KC = 32 by a 1x1 layer on the 256-pixel tiles and by a 3x3 on the smaller ones.
The five kernels without a K chunk or a tile in the plan line have the analogous properties (see properties()).
"""
import collections
import ctypes
import re
import sys

from tests.conv_ref import F16K_OUT, GATE, RES1, RES2, Case, case_of, desc_of

ACT_RELU, ACT_LEAKY = 1, 2
F32, BF16 = 0, 1

# (kernel, (B, Cin, H, W, Cout, k, stride, transposed, masked, prec, in_op), {property given up: the rule that forces it})
ROW_CASES = [
    ("conv_igemm_f32<1, 1, 2, 0, false>", (2, 17, 9, 33, 24, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<1, 1, 2, 0, true>", (2, 33, 9, 36, 24, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<1, 1, 2, 1, false>", (2, 9, 17, 65, 24, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<1, 1, 2, 2, false>", (2, 9, 17, 65, 24, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<1, 3, 2, 0, false>", (2, 17, 9, 33, 72, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<1, 3, 2, 0, true>", (2, 33, 9, 36, 72, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<1, 3, 2, 1, false>", (2, 9, 17, 65, 72, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<1, 3, 2, 2, false>", (2, 5, 17, 65, 72, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<2, 1, 1, 0, false>", (2, 17, 3, 33, 40, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 1, 0, true>", (2, 65, 3, 36, 40, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 1, 1, false>", (2, 17, 5, 65, 40, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<2, 1, 1, 2, false>", (2, 9, 5, 65, 40, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<2, 1, 2, 0, false>", (3, 17, 225, 65, 40, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 2, 0, true>", (3, 65, 225, 68, 40, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 2, 1, false>", (3, 17, 449, 129, 40, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<2, 1, 2, 2, false>", (3, 9, 449, 129, 40, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<2, 1, 4, 0, false>", (3, 17, 505, 97, 40, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 4, 0, true>", (3, 33, 505, 100, 40, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 4, 1, false>", (3, 9, 1009, 193, 40, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<2, 1, 4, 2, false>", (3, 5, 1009, 193, 40, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<2, 2, 2, 0, false>", (3, 9, 225, 65, 120, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 2, 0, true>", (3, 33, 225, 68, 120, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 2, 1, false>", (3, 9, 449, 129, 120, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<2, 2, 2, 2, false>", (3, 5, 449, 129, 120, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_f32<2, 2, 4, 0, false>", (3, 9, 449, 65, 120, 3, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 4, 0, true>", (3, 33, 449, 68, 120, 1, 1, 0, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 4, 1, false>", (3, 9, 897, 129, 120, 3, 2, 0, 0, 0, 1), {}),
    ("conv_igemm_f32<2, 2, 4, 2, false>", (3, 5, 897, 129, 120, 5, 2, 0, 0, 0, 2), {}),
    ("conv_igemm_bf16<1, 1, 2, 0, false>", (2, 65, 9, 33, 24, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<1, 1, 2, 0, true>", (2, 65, 9, 33, 24, 1, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<1, 1, 2, 1, false>", (2, 33, 17, 65, 24, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<1, 1, 2, 1, true>", (2, 65, 9, 33, 24, 1, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<1, 1, 2, 2, false>", (2, 33, 17, 65, 24, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<1, 1, 2, 2, true>", (2, 65, 9, 33, 24, 1, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<1, 3, 2, 0, false>", (2, 65, 9, 33, 72, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<1, 3, 2, 0, true>", (2, 65, 9, 33, 72, 1, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<1, 3, 2, 1, false>", (2, 33, 17, 65, 72, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<1, 3, 2, 1, true>", (2, 65, 9, 33, 72, 1, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<1, 3, 2, 2, false>", (2, 33, 17, 65, 72, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<1, 3, 2, 2, true>", (2, 65, 9, 33, 72, 1, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 1, 0, false>", (2, 65, 5, 65, 40, 3, 2, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 1, 0, true>", (2, 65, 3, 33, 40, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 1, 1, false>", (2, 65, 5, 65, 40, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 1, 1, true>", (2, 65, 3, 33, 40, 5, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 1, 2, false>", (2, 65, 5, 65, 40, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 1, 2, true>", (2, 65, 3, 33, 40, 3, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 2, 0, false>", (3, 65, 449, 129, 40, 3, 2, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 2, 0, true>", (3, 65, 225, 65, 40, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 2, 1, false>", (3, 65, 449, 129, 40, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 2, 1, true>", (3, 65, 225, 65, 40, 3, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 2, 2, false>", (3, 65, 449, 129, 40, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 2, 2, true>", (3, 65, 225, 65, 40, 3, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 4, 0, false>", (3, 65, 505, 97, 40, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 4, 0, true>", (3, 65, 505, 97, 40, 1, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 4, 1, false>", (3, 33, 1009, 193, 40, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 4, 1, true>", (3, 65, 505, 97, 40, 1, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 1, 4, 2, false>", (3, 33, 1009, 193, 40, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 1, 4, 2, true>", (3, 65, 505, 97, 40, 1, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 2, 2, 0, false>", (3, 65, 449, 129, 120, 3, 2, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 2, 0, true>", (3, 65, 225, 65, 120, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 2, 1, false>", (3, 65, 449, 129, 120, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 2, 2, 1, true>", (3, 65, 225, 65, 120, 3, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 2, 2, 2, false>", (3, 65, 449, 129, 120, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 2, 2, 2, true>", (3, 65, 225, 65, 120, 3, 1, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 2, 4, 0, false>", (3, 65, 449, 65, 120, 3, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 4, 0, true>", (3, 65, 249, 33, 120, 1, 1, 0, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 4, 1, false>", (3, 33, 897, 129, 120, 3, 2, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 2, 4, 1, true>", (3, 65, 249, 33, 120, 1, 1, 0, 0, 1, 1), {}),
    ("conv_igemm_bf16<2, 2, 4, 2, false>", (3, 33, 897, 129, 120, 5, 2, 0, 0, 1, 2), {}),
    ("conv_igemm_bf16<2, 2, 4, 2, true>", (3, 65, 249, 33, 120, 1, 1, 0, 0, 1, 2), {}),
    ("conv_direct_f32<3>", (2, 5, 33, 37, 2, 3, 2, 0, 0, 0, 1), {}),
    ("conv_direct_f32<8>", (2, 5, 17, 19, 6, 3, 1, 0, 0, 0, 2), {}),
    ("deconv5s2_small_cout", (2, 20, 17, 18, 3, 5, 2, 1, 0, 0, 0), {}),
    ("conv5s1_small<4>", (2, 7, 17, 19, 3, 5, 1, 0, 0, 0, 0), {}),
    ("conv5s1_small<8>", (2, 7, 17, 19, 6, 5, 1, 0, 0, 0, 0), {}),
]
# per tile shape: ConvTranspose2d 5x5 stride 2 (four phases), ragged phase planes
TRANSPOSED_CASES = [
    ("conv_igemm_f32<1, 1, 2, 0, false>", (2, 17, 9, 33, 24, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<1, 3, 2, 0, false>", (2, 17, 9, 33, 72, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 1, 0, false>", (2, 17, 3, 33, 40, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 2, 0, false>", (2, 17, 125, 33, 40, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 1, 4, 0, false>", (3, 17, 249, 33, 40, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 2, 0, false>", (2, 9, 125, 33, 120, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_f32<2, 2, 4, 0, false>", (2, 9, 249, 33, 120, 5, 2, 1, 0, 0, 0), {}),
    ("conv_igemm_bf16<1, 1, 2, 0, false>", (2, 65, 9, 33, 24, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<1, 3, 2, 0, false>", (2, 65, 9, 33, 72, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 1, 0, true>", (2, 65, 3, 33, 40, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 2, 0, true>", (2, 65, 125, 33, 40, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 1, 4, 0, false>", (3, 65, 249, 33, 40, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 2, 0, true>", (2, 65, 125, 33, 120, 5, 2, 1, 0, 1, 0), {}),
    ("conv_igemm_bf16<2, 2, 4, 0, false>", (2, 65, 249, 33, 120, 5, 2, 1, 0, 1, 0), {}),
]
# per tile shape: gate + two residuals + activation + channel views on both sides: (kernel, shape, act, (in_ctot, in_coff, out_ctot, out_coff), waived).
# The bf16 ones run a second time as F16K output (no gate, no residual) into the same wider buffer: that form needs Cout % 32 == 0 and a
# 16-aligned view, so 32 / 96 / 128 fill their blocks and only 160 under the 64-wide tiles is ragged.
F16K_COUT = "the F16K-output form needs Cout % 32 == 0: the only such Cout this tile shape takes is a whole block"
FORM_CASES = [
    ("conv_igemm_f32<1, 1, 2, 0, false>", (2, 17, 9, 33, 24, 5, 1, 0, 1, 0, 0), 2, (22, 3, 31, 4), {}),
    ("conv_igemm_f32<1, 3, 2, 0, false>", (2, 9, 9, 33, 72, 5, 1, 0, 1, 0, 0), 2, (14, 3, 79, 4), {}),
    ("conv_igemm_f32<2, 1, 1, 0, false>", (2, 17, 3, 33, 40, 5, 1, 0, 1, 0, 0), 2, (22, 3, 47, 4), {}),
    ("conv_igemm_f32<2, 1, 2, 0, false>", (3, 17, 225, 65, 40, 5, 1, 0, 1, 0, 0), 2, (22, 3, 47, 4), {}),
    ("conv_igemm_f32<2, 1, 4, 0, false>", (3, 17, 505, 97, 40, 5, 1, 0, 1, 0, 0), 2, (22, 3, 47, 4), {}),
    ("conv_igemm_f32<2, 2, 2, 0, false>", (3, 9, 225, 65, 120, 5, 1, 0, 1, 0, 0), 2, (14, 3, 127, 4), {}),
    ("conv_igemm_f32<2, 2, 4, 0, false>", (3, 9, 449, 65, 120, 5, 1, 0, 1, 0, 0), 2, (14, 3, 127, 4), {}),
    ("conv_igemm_bf16<1, 1, 2, 0, false>", (2, 65, 9, 33, 32, 3, 1, 0, 0, 1, 0), 1, (73, 5, 80, 16), {"cout": F16K_COUT}),
    ("conv_igemm_bf16<1, 3, 2, 0, false>", (2, 65, 9, 33, 96, 3, 1, 0, 0, 1, 0), 1, (73, 5, 144, 16), {"cout": F16K_COUT}),
    ("conv_igemm_bf16<2, 1, 1, 0, true>", (2, 65, 3, 33, 160, 3, 1, 0, 0, 1, 0), 1, (73, 5, 208, 16), {}),
    ("conv_igemm_bf16<2, 1, 2, 0, true>", (2, 65, 169, 33, 160, 3, 1, 0, 0, 1, 0), 1, (73, 5, 208, 16), {}),
    ("conv_igemm_bf16<2, 1, 4, 0, false>", (2, 65, 505, 33, 160, 3, 1, 0, 0, 1, 0), 1, (73, 5, 208, 16), {}),
    ("conv_igemm_bf16<2, 2, 2, 0, true>", (3, 65, 225, 65, 128, 3, 1, 0, 0, 1, 0), 1, (73, 5, 176, 16), {"cout": F16K_COUT}),
    ("conv_igemm_bf16<2, 2, 4, 0, false>", (3, 65, 449, 65, 128, 3, 1, 0, 0, 1, 0), 1, (73, 5, 176, 16), {"cout": F16K_COUT}),
]


# ------------------------------------------------------------------------------------------------ the plan line
def plan(c, form=None):
    """(kernel, (gx, gy, gz), {name: integer}) of the launch, or None where the launcher refuses the call"""
    from masic_amd import _lib
    buf = ctypes.create_string_buffer(256)
    d = desc_of(c)
    if _lib.lib.masic_conv_plan_name(ctypes.byref(d), c.form if form is None else form, buf, 256) != 0 or not buf.value:
        return None
    name, grid, _, _, ints = buf.value.decode().strip().split(" | ")
    ints = [int(v) for v in ints.split()]
    keys = {12: "Cin_pad Cout_pad KC TW TH SR PH PW PSZ buf_sz vec4 nphase", 2: "Cin_pad tiles_w", 1: "tiles_w"}[len(ints)].split()
    if name.startswith("conv_direct"):
        keys = ["nphase"]
    return name, tuple(int(v) for v in grid.split(",")), dict(zip(keys, ints))


def table_names():
    from masic_amd import _lib
    out, buf = [], ctypes.create_string_buffer(96)
    row = 0
    while any(_lib.lib.masic_conv_row_name(row, op, f, buf, 96) == 0 for op in range(3) for f in range(2)):
        out += [buf.value.decode() for op in range(3) for f in range(2) if _lib.lib.masic_conv_row_name(row, op, f, buf, 96) == 0]
        row += 1
    return out


def properties(c, p=None):
    """the properties of the module docstring as {name: bool}; keys a kernel family has no notion of are absent"""
    name, grid, v = p or plan(c)
    Hp, Wp = (c.H, c.W) if c.transposed or c.stride == 1 else ((c.H + 2 * (c.k // 2) - c.k) // 2 + 1, (c.W + 2 * (c.k // 2) - c.k) // 2 + 1)
    out = {"batch": c.B >= 2}
    if name.startswith("conv_igemm"):
        out.update(ragged_h=Hp % v["TH"] != 0, ragged_w=Wp % v["TW"] != 0, tiles=Hp > v["TH"] and Wp > v["TW"],
                   cout=c.Cout % (v["Cout_pad"] // grid[1]) != 0, k_chunks=c.Cin > v["KC"] and c.Cin % v["KC"] != 0)
        if name.endswith("true>") and "f32" in name:
            assert c.W % 4 == 0
    elif name.startswith("conv_direct"):        # 256 pixels of a phase plane per workgroup, CO channels in registers
        out.update(ragged_h=(Hp * Wp) % 256 != 0, ragged_w=Wp % 16 != 0, tiles=grid[0] > v["nphase"], cout=c.Cout % int(name[-2]) != 0)
    else:                                       # conv5s1_small<CO> / deconv5s2_small_cout: 16 x 16 tiles of the input plane
        out.update(ragged_h=c.H % 16 != 0, ragged_w=c.W % 16 != 0, tiles=c.H > 16 and c.W > 16, cout=c.Cout % (8 if name.endswith("<8>") else 4) != 0)
        if name.startswith("deconv"):
            out["k_chunks"] = c.Cin > 8 and c.Cin % 8 != 0      # channels are staged in groups of 8 (Cin_pad)
    return out


def row_cases():
    return [(k, case_of(t), w) for k, t, w in ROW_CASES]


def transposed_cases():
    return [(k, case_of(t), w) for k, t, w in TRANSPOSED_CASES]


def form_cases():
    return [(k, case_of(t, GATE | RES1 | RES2, act, view), w) for k, t, act, view, w in FORM_CASES]


def digest_form_cases():
    """the eleven FORM_CASES of tests/golden/make_conv_fwd_digest.py with the seeds of the digest's own inputs"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_conv_fwd_digest", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_conv_fwd_digest.py"))
    dig = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dig)
    return [(name, c["kernel"], case_of(c["shape"], c["form"], c["act"], c["view"]), 4000 + i)
            for i, c in enumerate(dig.cases()) if (name := c["name"]) in dig.FORM_CASES]


# waived: {property given up: rule}, None for a case whose shape is given; integers: tests/conv_ref.py, inputs()
Entry = collections.namedtuple("Entry", "id kernel case seed waived integers")


def all_cases():
    out = []
    for kind, cases in (("row", row_cases()), ("transposed", transposed_cases()), ("form", form_cases())):
        for k, c, w in cases:
            out.append(Entry(f"{kind} {k}", k, c, 7000 + len(out), w, False))
            if kind == "form" and c.prec == BF16:
                out.append(Entry(f"f16k-out {k}", k, c._replace(form=F16K_OUT), 7000 + len(out), w, True))
    out += [Entry("digest: " + name, k, c, seed, None, False) for name, k, c, seed in digest_form_cases()]
    return out


# ------------------------------------------------------------------------------------------------ the search
COUT = {(1, 1, 2): 24, (1, 3, 2): 72, (2, 1, 1): 40, (2, 1, 2): 40, (2, 1, 4): 40, (2, 2, 2): 120, (2, 2, 4): 120}
COUT_F16K = {(1, 1, 2): 32, (1, 3, 2): 96, (2, 1, 1): 160, (2, 1, 2): 160, (2, 1, 4): 160, (2, 2, 2): 128, (2, 2, 4): 128}
TILES = list(COUT)
# (k, stride), by in_op: kernels with a halo first and 1x1 last, a different first choice per column so that the table has every kind
KINDS = {0: [(3, 1), (3, 2), (5, 2), (5, 1), (1, 1)], 1: [(3, 2), (5, 1), (3, 1), (5, 2), (1, 1)], 2: [(5, 2), (3, 1), (3, 2), (5, 1), (1, 1)]}
CIN_PROBE = 200


def _sizes(tile, vec4):
    """(B, nth, ntw) by B * Ho * Wo with Ho = (nth - 1) TH + 1, Wo = (ntw - 1) 32 + 1 (4 for VEC4): phase-plane sizes, tile width 32"""
    TH = (4 // tile[0]) * tile[2]
    out = [(B * ((nth - 1) * TH + 1) * ((ntw - 1) * 32 + (4 if vec4 else 1)), B, (nth - 1) * TH + 1, (ntw - 1) * 32 + (4 if vec4 else 1))
           for B in (2, 3) for nth in range(2, 72) for ntw in range(2, 26)]
    return [t[1:] for t in sorted(out)]


def _shape(B, Cin, Hp, Wp, Cout, k, s, tr, masked, prec, op):
    if s == 2 and not tr:
        Hp, Wp = 2 * Hp - 1, 2 * Wp - 1          # the last window ends in the padding
    return (B, Cin, Hp, Wp, Cout, k, s, tr, masked, prec, op)


def _find(tile, prec, op, col, kinds, Cout, tr=0, masked=0, form=0, act=0, view=None, want_col=True, give_up=()):
    """smallest size at which some kind selects (tile, op, col) with every property; else with every property but k_chunks and the
    largest Cin that keeps the column"""
    fam = "conv_igemm_bf16" if prec == BF16 else "conv_igemm_f32"
    head = f"{fam}<{tile[0]}, {tile[1]}, {tile[2]}, {op}, "
    vec4 = prec == F32 and col and want_col

    def mk(B, Cin, Hp, Wp, k, s):
        v = (view[0] + Cin, view[1], view[2] + Cout, view[3]) if view else None
        return case_of(_shape(B, Cin, Hp, Wp, Cout, k, s, tr, masked, prec, op), form, act, v)

    for strict in (True, False):
        for B, Hp, Wp in _sizes(tile, vec4):
            for k, s in kinds:
                p = plan(mk(B, CIN_PROBE, Hp, Wp, k, s))
                if p is None or not p[0].startswith(head):
                    continue
                KC = p[2]["KC"]
                cins = [2 * KC + 1] if strict else range(64, 1, -1)
                for Cin in cins:
                    c = mk(B, Cin, Hp, Wp, k, s)
                    p = plan(c)
                    if p is None or not p[0].startswith(head) or (want_col and p[0] != head + ("true>" if col else "false>")):
                        continue
                    pr = properties(c, p)
                    if all(v for n, v in pr.items() if n not in give_up and (strict or n != "k_chunks")):
                        return p[0], c, {n: _REASONS[n] for n, v in pr.items() if not v}
    raise RuntimeError(f"no case for {head}{col}")


_REASONS = {"cout": F16K_COUT}           # the only property the search had to give up anywhere
_REASON_NAMES = {"cout": "F16K_COUT"}

SMALL = [      # the kernels choose_cfg picks by channel counts and kind alone: 2 x 2 ragged tiles (16 x 16; 256 pixels for conv_direct_f32)
    ("conv_direct_f32<3>", (2, 5, 33, 37, 2, 3, 2, 0, 0, F32, 1)),
    ("conv_direct_f32<8>", (2, 5, 17, 19, 6, 3, 1, 0, 0, F32, 2)),
    ("deconv5s2_small_cout", (2, 20, 17, 18, 3, 5, 2, 1, 0, F32, 0)),
    ("conv5s1_small<4>", (2, 7, 17, 19, 3, 5, 1, 0, 0, F32, 0)),
    ("conv5s1_small<8>", (2, 7, 17, 19, 6, 5, 1, 0, 0, F32, 0)),
]


def search():
    rows, trans, forms = [], [], []
    for name in table_names():
        m = re.match(r"conv_igemm_(f32|bf16)<(\d), (\d), (\d), (\d), (true|false)>", name)
        if not m:
            t = dict(SMALL)[name]
            assert plan(case_of(t))[0] == name
            rows.append((name, t, {}))
            continue
        prec, tile, op, col = BF16 if m.group(1) == "bf16" else F32, tuple(int(m.group(i)) for i in (2, 3, 4)), int(m.group(5)), m.group(6) == "true"
        kinds = [(1, 1)] if (prec == F32 and col) else KINDS[op]
        got, c, lost = _find(tile, prec, op, col, kinds, COUT[tile])
        assert got == name
        rows.append((name, tuple(c[:11]), lost))
    for prec in (F32, BF16):
        for tile in TILES:
            got, c, lost = _find(tile, prec, 0, 0, [(5, 2)], COUT[tile], tr=1, want_col=False)
            trans.append((got, tuple(c[:11]), lost))
            if prec == F32:      # the masked 5x5 of the context model, leaky
                got, c, lost = _find(tile, prec, 0, 0, [(5, 1)], COUT[tile], masked=1, form=GATE | RES1 | RES2, act=ACT_LEAKY, view=(5, 3, 7, 4), want_col=False)
            else:
                got, c, lost = _find(tile, prec, 0, 0, [(3, 1)], COUT_F16K[tile], form=GATE | RES1 | RES2, act=ACT_RELU, view=(8, 5, 48, 16), want_col=False,
                                     give_up=() if tile[:2] == (2, 1) else ("cout",))
                assert plan(c, F16K_OUT)[0] == got
            forms.append((got, tuple(c[:11]), c.act, c.view, lost))
    return rows, trans, forms


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coremasic", "mywork"))
    rows, trans, forms = search()
    for title, table in (("ROW_CASES", rows), ("TRANSPOSED_CASES", trans), ("FORM_CASES", forms)):
        print(f"{title} = [")
        for e in table:
            lost = "{" + ", ".join(f'"{n}": {_REASON_NAMES[n]}' for n in e[-1]) + "}"
            print("    (" + ", ".join(repr(f).replace("'", '"') for f in e[:-1]) + ", " + lost + "),")
        print("]")
