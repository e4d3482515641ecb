"""Shapes that drive every persistent-workgroup kernel past its grid cap, and the properties that make them hard -- read from the
launchers' own plan lines (masic_*_plan_name, include/masic_hip.h), never restated here: the cap of a family is whatever grid its plan
prints.  tests/test_cpu_tile_loops.py holds every case to its kernel and properties without a GPU; tests/test_gpu_tile_loops.py runs
them against float64.

The five families loop `for (tile = first; tile < ntiles; tile += stride)` with software-pipeline state carried from one iteration to
the next: patch buffers fetched one or two tiles ahead behind counted waits (conv_a, pic_wgrad, resident), LDS tiles and accumulators
reused per tile (gdn_bwd), or nothing (gdn_fwd).  Properties (properties(): per case):
  rounds   some workgroup runs its loop body at least rounds_min + 1 times and another one time fewer: items >= rounds_min * units + 1
           and items % units != 0, units = the work items taken per round by the whole grid.  rounds_min: conv_a 2 (the prologue
           fetches two tiles: the first in-loop fetch is for a workgroup's third), gdn_bwd 2, pic_wgrad 3 (the P ring of three wraps on
           the fourth chunk), gdn_fwd 1; resident: an XCD share whose workgroups run NBUF + 1 tiles (the patch ring wraps).
  ragged   the last tile is partial: conv_a Ho % 8 and Wo % 32 nonzero; gdn_bwd H W % 32 != 0 (32-pixel runs cross images) and a partial
           last tile; pic_wgrad Hc Wc % 64 != 0 and Wc % 64 != 0; resident ntiles % 8 != 0: its tiles are always whole
           (masic_conv3x3_resident_supported: H % (512 / Cout) == 0, W % 32 == 0), what is ragged is the split into eight XCD shares.
  batch    B >= 2 and the first two tiles of every workgroup that runs two lie in different images.
Where a launcher rule forbids a property the entry names the property and the rule (as ROW_CASES of tests/f16k_row_cases.py)."""
import collections
import ctypes

PREC_F32, PREC_BF16 = 0, 1
GDN_FWD_WHOLE = "masic_gdn_fwd_ex takes the 128-channel kernels for H W % 64 == 0 (gdn_mfma_c128) / % 32 == 0 (gdn_bf16x3_c128) only: every tile is whole"

# family, kernel, shape, form arguments of the plan query, {property given up: rule}
Case = collections.namedtuple("Case", "family kernel shape form given_up")

CONV_A_FORMS = [      # kernel, Wi, (gdn, products, out)
    ("conv_a_gdn_f16k_w", 68, (1, 1, 0)),
    ("conv_a_gdn_f16k<false, 0>", 66, (1, 1, 0)),
    ("conv_a_gdn_f16k<false, 1>", 66, (1, 1, 1)),
    ("conv_a_gdn_f16k<false, 2>", 66, (1, 1, 2)),
    ("conv_a_gdn_f16k<false, 3>", 66, (0, 1, 0)),
    ("conv_a_gdn_f16k<true, 0>", 66, (1, 3, 0)),
    ("conv_a_gdn_f16k<true, 1>", 66, (1, 3, 1)),
    ("conv_a_gdn_f16k<true, 2>", 66, (1, 3, 2)),
]
GDN_BWD_KERNELS = {(0, 0): "gdn_bwd_c128<false, false>", (1, 0): "gdn_bwd_c128<true, false>", (0, 1): "gdn_bwd_c128<false, true>", (1, 1): "gdn_bwd_c128_wn<2>"}
C3_PAIRS = [(16, 32), (32, 32), (16, 64), (32, 64), (64, 64)]

CASES = (
    # x: (29, 6 channels, in_coff 3, 130, Wi): Ho x Wo = 65 x 33 | 34, 9 x 2 tiles per image, 522 in all
    [Case("conv_a", k, (29, 130, wi), form, {}) for k, wi, form in CONV_A_FORMS]
    # 65 709 pixels, 514 tiles; form = (x F16K, g F16K, want_sum)
    + [Case("gdn_bwd", GDN_BWD_KERNELS[(xf, gf)], (3, 128, 149, 147), (xf, gf, 1), {}) for xf, gf in ((0, 0), (1, 0), (0, 1), (1, 1))]
    # 309 chunks per image, 1545 in all
    + [Case("pic_wgrad", "wgrad_pic_f16k", (5, 139, 142), (), {})]
    # W = 64, H = 5 tile heights, 10 tiles per image, 770 in all; form = (ex, sum_of)
    + [Case("resident", f"conv3x3_resident_f16k<{ci}, {c}, {'true' if ex else 'false'}>", (77, ci, c, 5 * (512 // c), 64), (ex, ex), {})
       for ci, c in C3_PAIRS for ex in (0, 1)]
    # 65 600 pixels: 1025 tiles of gdn_mfma_c128, 2050 strips of gdn_bf16x3_c128; form = (prec, out_f16k)
    + [Case("gdn_fwd", "gdn_mfma_c128", (5, 128, 80, 164), (PREC_F32, 0), {"ragged": GDN_FWD_WHOLE}),
       Case("gdn_fwd", "gdn_bf16x3_c128", (5, 128, 80, 164), (PREC_BF16, 0), {"ragged": GDN_FWD_WHOLE}),
       Case("gdn_fwd", "gdn_bf16x3_c128", (5, 128, 80, 164), (PREC_BF16, 1), {"ragged": GDN_FWD_WHOLE})]
)

QUERY = {"conv_a": "masic_conv_a_plan_name", "gdn_bwd": "masic_gdn_bwd_fused_plan_name", "pic_wgrad": "masic_pic_wgrad_f16k_plan_name",
         "resident": "masic_conv3x3_resident_plan_name", "gdn_fwd": "masic_gdn_fwd_plan_name"}
KEYS = {"conv_a": "ntiles tiles_w tiles_per_image Ho Wo", "gdn_bwd": "ntiles npix HW", "pic_wgrad": "ntiles tiles_per_image",
        "resident": "ntiles tiles_w tiles_per_image nbuf", "gdn_fwd": "ntiles per_wg tile_px tiles_per_image"}
ROUNDS_MIN = {"conv_a": 2, "gdn_bwd": 2, "pic_wgrad": 3, "gdn_fwd": 1}


def case_id(c):
    return f"{c.family} {c.kernel} {'x'.join(str(v) for v in c.shape)}" + (f" form {','.join(str(v) for v in c.form)}" if c.form else "")


def query_args(c, x_aligned16=1):
    """the integer arguments of the family's plan query in front of (buf, n)"""
    if c.family == "conv_a":
        return tuple(c.shape) + (x_aligned16,) + tuple(c.form)
    return tuple(c.shape) + tuple(c.form)


def plan_text(family, args, n=512):
    """(return code, text) of the family's plan query"""
    from masic_amd import _lib
    buf = ctypes.create_string_buffer(b"?" * (n - 1), n)
    rc = getattr(_lib.lib, QUERY[family])(*(int(v) for v in args), buf, n)
    return rc, buf.value.decode()


Launch = collections.namedtuple("Launch", "kernel grid block lds ints")


def parse(text):
    """[Launch] of a plan text, one per line"""
    out = []
    for line in text.strip().split("\n"):
        f = line.split(" | ")
        assert len(f) in (4, 5), line
        out.append(Launch(f[0], tuple(int(g) for g in f[1].split(",")), int(f[2]), int(f[3]), [int(v) for v in f[4].split()] if len(f) == 5 else []))
    return out


def plan(c, x_aligned16=1):
    """(the persistent kernel's Launch, {name: integer} of its line, every Launch of the call)"""
    rc, text = plan_text(c.family, query_args(c, x_aligned16))
    assert rc == 0 and text, (case_id(c), rc)
    launches = parse(text)
    main = [l for l in launches if l.ints]
    assert len(main) == 1, text
    keys = KEYS[c.family].split()
    assert len(main[0].ints) == len(keys), text
    return main[0], dict(zip(keys, main[0].ints)), launches


def tiles_of(c, wg):
    """the tile indices workgroup `wg` visits, in order (gdn_fwd's bf16x3 form: those of its wave 0), as its kernel computes them"""
    m, v, _ = plan(c)
    grid, nt = m.grid[0], v["ntiles"]
    if c.family == "resident":
        xcd, slot, nslot, per = wg & 7, wg >> 3, grid >> 3, (nt + 7) >> 3
        return list(range(xcd * per + slot, min((xcd + 1) * per, nt), nslot))
    per_wg = v.get("per_wg", 1)
    return list(range(wg * per_wg, nt, grid * per_wg))


def image_of(c, v, tile):
    if c.family == "gdn_bwd":
        return tile * 128 // v["HW"]
    return tile // v["tiles_per_image"]


def properties(c):
    """{property: bool} of the module docstring, from the plan line"""
    m, v, _ = plan(c)
    grid, nt, B = m.grid[0], v["ntiles"], c.shape[0]
    p = {}
    if c.family == "resident":
        per = -(-nt // 8)
        p["rounds"] = -(-per // (grid // 8)) >= v["nbuf"] + 1 and nt % grid != 0
        p["ragged"] = nt % 8 != 0
    else:
        units = grid * v.get("per_wg", 1)
        p["rounds"] = nt >= ROUNDS_MIN[c.family] * units + 1 and nt % units != 0
    if c.family == "conv_a":
        p["ragged"] = v["Ho"] % 8 != 0 and v["Wo"] % 32 != 0
    elif c.family == "gdn_bwd":
        p["ragged"] = v["HW"] % 32 != 0 and v["npix"] % 128 != 0
    elif c.family == "pic_wgrad":
        Hc, Wc = c.shape[1:]
        p["ragged"] = (Hc * Wc) % 64 != 0 and Wc % 64 != 0
    elif c.family == "gdn_fwd":
        p["ragged"] = False
    first_two = [t[:2] for t in (tiles_of(c, wg) for wg in range(grid)) if len(t) >= 2]
    p["batch"] = B >= 2 and len(first_two) > 0 and all(image_of(c, v, t[0]) != image_of(c, v, t[1]) for t in first_two)
    return p


def selective_tiles(c):
    """the tile set of the selective-support runs: the first tile of the second round (index grid), the first of the last round, the
    ragged last tile"""
    m, v, _ = plan(c)
    grid, nt = m.grid[0], v["ntiles"]
    return sorted({grid, (nt - 1) // grid * grid, nt - 1})
