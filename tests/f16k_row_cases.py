"""One hard case for every kernel instantiation of F16K_ROWS (masic_amd/csrc/conv_f16k.hip), a short list of geometry cases the row
table does not force, and the epilogue-form cases: the tables below, and the search that wrote the first.

    python -m tests.f16k_row_cases            # runs the search (host plan query only, no GPU) and prints ROW_CASES

What makes a row case hard (properties(): read from the integers of masic_conv_f16k_plan_name's line; tests/test_cpu_f16k_rows.py
asserts them per case):
  batch     B >= 2
  tiles     more than one tile along each axis of the phase plane
  ragged_h  the phase plane's height is no multiple of the tile height TH (the last tile row is partial)
  ragged_w  ... its width no multiple of the tile width TW
  ring      at least L + 2 K chunks: the L + 1 patch buffers are all reused
  pad_taps  a phase whose tap count is no multiple of T: the zero-weight padding taps of its last step are read
  cout      Cout is 160 or 192: the last 128-channel co-block is partly empty
  past      under msplit > 1 (the plan line says so; a row's msplit is 4 / NM): a sub-block that starts past the last channel, whose
            workgroups leave at once
A case is the cheapest shape (multiply-adds of its float64 reference) with every property among the candidates of search(): phase
planes 33 wide and (n - 1) 8 + 1 high, B, Cin and Cout from short lists, every layer kind the family runs.  Where a rule of
choose_f16k / plan_f16k forbids a property for the row, the search gives it up and the entry names the property and the rule.
"""
import collections
import ctypes
import re
import sys
import zlib

from tests.f16k_ref import (ACT_LEAKY, ACT_RELU, F16K_GDN, F16K_MULTI, F16K_NOSPLIT, PREC_BF16, PREC_FP8, Case, case_of, desc_of, macs,  # noqa: F401
                            out_hw, phase_taps)

T5 = "T = 5 is chosen only where every phase has 25 taps (choose_f16k: min_taps == max_taps == 25), which five taps per step divide"
GDN128 = "the fused GDN contracts one 128-channel block: plan_f16k refuses Cout != 128"
LITE = "the lite rows hold exactly Cout / 32 accumulator tiles and choose_f16k takes them for 33 <= Cout <= 96 only: Cout is 64 or 96"
NP4 = "choose_f16k takes the 1024-pixel tiles for Cout <= 32 only, and Cout % 32 == 0: Cout is 32"
_REASON_NAMES = {T5: "T5", GDN128: "GDN128", LITE: "LITE", NP4: "NP4"}

# (kernel, (B, Cin, H, W, Cout, k, stride, transposed, masked), prec, flags, {property given up: the rule that forces it})
ROW_CASES = [
    ("conv_f16k<1, 5, 2, 6, 1, true, 4, 1, false>", (2, 48, 17, 65, 128, 5, 2, 0, 0), PREC_BF16, 1, {"cout": GDN128, "pad_taps": T5}),
    ("conv_f16k<1, 5, 2, 6, 1, false, 1, 1, false>", (2, 48, 17, 65, 160, 5, 2, 0, 0), PREC_BF16, 0, {"pad_taps": T5}),
    ("conv_f16k<1, 5, 2, 6, 1, false, 2, 1, false>", (9, 48, 17, 65, 160, 5, 2, 0, 0), PREC_BF16, 0, {"pad_taps": T5}),
    ("conv_f16k<1, 5, 2, 6, 1, false, 4, 1, false>", (16, 48, 33, 65, 160, 5, 2, 0, 0), PREC_BF16, 0, {"pad_taps": T5}),
    ("conv_f16k_multi<1>", (2, 48, 17, 65, 160, 5, 2, 0, 0), PREC_BF16, 4, {"pad_taps": T5}),
    ("conv_f16k_multi<2>", (9, 48, 17, 65, 160, 5, 2, 0, 0), PREC_BF16, 4, {"pad_taps": T5}),
    ("conv_f16k_multi<4>", (16, 48, 33, 65, 160, 5, 2, 0, 0), PREC_BF16, 4, {"pad_taps": T5}),
    ("conv_f16k<1, 4, 3, 6, 1, true, 4, 1, false>", (2, 48, 17, 65, 128, 3, 2, 0, 0), PREC_BF16, 1, {"cout": GDN128}),
    ("conv_f16k<1, 4, 3, 6, 1, false, 1, 1, false>", (2, 48, 17, 65, 160, 3, 2, 0, 0), PREC_BF16, 0, {}),
    ("conv_f16k<1, 4, 3, 6, 1, false, 2, 1, false>", (9, 48, 17, 65, 160, 3, 2, 0, 0), PREC_BF16, 0, {}),
    ("conv_f16k<1, 4, 3, 6, 1, false, 4, 1, false>", (16, 48, 33, 65, 160, 3, 2, 0, 0), PREC_BF16, 0, {}),
    ("conv_f16k<2, 2, 3, 4, 2, true, 4, 1, false>", (2, 128, 9, 33, 128, 3, 1, 0, 0), PREC_BF16, 1, {"cout": GDN128}),
    ("conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 160, 3, 1, 0, 0), PREC_BF16, 0, {}),
    ("conv_f16k<2, 2, 3, 4, 2, false, 2, 1, false>", (3, 128, 9, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, {}),
    ("conv_f16k<2, 2, 3, 4, 2, false, 4, 1, false>", (8, 128, 9, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, {}),
    ("conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false>", (16, 64, 97, 33, 32, 5, 2, 1, 0), PREC_BF16, 0, {"cout": NP4}),
    ("conv_f16k<1, 2, 3, 3, 2, true, 4, 2, false>", (16, 80, 49, 33, 128, 5, 2, 1, 0), PREC_BF16, 1, {"cout": GDN128}),
    ("conv_f16k<1, 2, 3, 3, 2, false, 4, 2, false>", (16, 80, 17, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, {}),
    ("conv_f16k<2, 2, 2, 5, 1, true, 4, 2, false>", (16, 96, 49, 33, 128, 5, 2, 1, 0), PREC_BF16, 1, {"cout": GDN128}),
    ("conv_f16k<2, 2, 2, 5, 1, false, 4, 2, false>", (16, 96, 17, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, {}),
    ("conv_f16k<2, 2, 1, 3, 1, false, 2, 1, false>", (16, 96, 49, 33, 64, 5, 2, 1, 0), PREC_BF16, 0, {"cout": LITE}),
    ("conv_f16k<2, 2, 1, 3, 1, false, 3, 1, false>", (16, 96, 49, 33, 96, 5, 2, 1, 0), PREC_BF16, 0, {"cout": LITE}),
    ("conv_f16k<1, 4, 3, 6, 1, true, 4, 1, true>", (2, 96, 17, 65, 128, 3, 2, 0, 0), PREC_FP8, 1, {"cout": GDN128}),
    ("conv_f16k<1, 4, 3, 6, 1, false, 4, 1, true>", (2, 96, 17, 65, 160, 3, 2, 0, 0), PREC_FP8, 0, {}),
    ("conv_f16k<2, 2, 3, 4, 2, true, 4, 1, true>", (2, 256, 9, 33, 128, 3, 1, 0, 0), PREC_FP8, 1, {"cout": GDN128}),
    ("conv_f16k<2, 2, 3, 4, 2, false, 4, 1, true>", (2, 256, 9, 33, 160, 3, 1, 0, 0), PREC_FP8, 0, {}),
]

# geometry the row table does not force: (what, kernel, shape, prec, flags, (in_ctot, in_coff) or None)
GEOMETRY_CASES = [
    ("block map of B % 8 == 0", "conv_f16k<1, 5, 2, 6, 1, false, 2, 1, false>", (8, 48, 33, 65, 160, 5, 2, 0, 0), PREC_BF16, 0, None),
    ("block map of B % 8 != 0", "conv_f16k<1, 5, 2, 6, 1, false, 2, 1, false>", (11, 48, 33, 65, 160, 5, 2, 0, 0), PREC_BF16, 0, None),
    ("block map of B % 8 == 0, four phases", "conv_f16k<2, 2, 3, 4, 2, false, 4, 1, false>", (8, 128, 9, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, None),
    ("block map of B % 8 != 0, 512-pixel tiles", "conv_f16k<2, 2, 2, 5, 1, false, 4, 2, false>", (17, 96, 113, 33, 160, 3, 1, 0, 0), PREC_BF16, 0, None),
    ("TW = 8", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 33, 7, 160, 3, 1, 0, 0), PREC_BF16, 0, None),
    ("TW = 16", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 17, 13, 160, 3, 1, 0, 0), PREC_BF16, 0, None),
    ("TW = 8, strided", "conv_f16k<1, 5, 2, 6, 1, false, 1, 1, false>", (2, 48, 65, 13, 160, 5, 2, 0, 0), PREC_BF16, 0, None),
    ("TW = 16, strided", "conv_f16k<1, 4, 3, 6, 1, false, 1, 1, false>", (2, 48, 33, 25, 160, 3, 2, 0, 0), PREC_BF16, 0, None),
    ("transposed 5x5 stride 2: phases of 9 / 6 / 6 / 4 taps", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 160, 5, 2, 1, 0), PREC_BF16, 0, None),
    ("transposed 5x5 stride 2, fp8", "conv_f16k<2, 2, 3, 4, 2, false, 4, 1, true>", (2, 256, 9, 33, 160, 5, 2, 1, 0), PREC_FP8, 0, None),
    ("masked 5x5", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 160, 5, 1, 0, 1), PREC_BF16, 0, None),
    ("input channel view", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 160, 3, 1, 0, 0), PREC_BF16, 0, (176, 32)),
    ("input channel view, strided, fp8", "conv_f16k<1, 4, 3, 6, 1, false, 4, 1, true>", (2, 96, 17, 65, 160, 3, 2, 0, 0), PREC_FP8, 0, (160, 32)),
]

# the epilogue forms, each at a two-by-two-tile shape of a row that serves it: (form, kernel, shape, act, flags)
FORM_CASES = [
    ("res_ex relu: mask, y_pre, two residuals, res_ctot 80", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 64, 9, 33, 64, 3, 1, 0, 0), ACT_RELU, 0),
    ("res_ex leaky: mask slope 0.01, y_pre, two residuals, res_ctot 80", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 64, 9, 33, 64, 3, 1, 0, 0), ACT_LEAKY, 0),
    ("few channels C = 3 + res32", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 96, 9, 33, 32, 3, 1, 0, 0), ACT_RELU, F16K_NOSPLIT),
    ("depth-to-space C = 3 into a channel view", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 32, 3, 1, 0, 0), 0, F16K_NOSPLIT),
    ("gdn_dual into a wider buffer", "conv_f16k<1, 5, 2, 6, 1, true, 4, 1, false>", (2, 48, 17, 65, 128, 5, 2, 0, 0), 0, F16K_GDN),
    ("gated F16K output into a wider buffer", "conv_f16k<1, 4, 3, 6, 1, false, 1, 1, false>", (2, 48, 17, 65, 160, 3, 2, 0, 0), ACT_RELU, 0),
    ("gated float32 view", "conv_f16k<2, 2, 3, 4, 2, false, 1, 1, false>", (2, 128, 9, 33, 160, 3, 1, 0, 0), ACT_RELU, 0),
    ("fp8 output", "conv_f16k<1, 5, 2, 6, 1, false, 4, 1, false>", (2, 48, 17, 65, 160, 5, 2, 0, 0), 0, F16K_NOSPLIT),
    ("multi: four layouts, gated round16 view", "conv_f16k_multi<1>", (2, 48, 17, 65, 192, 5, 2, 0, 0), 0, F16K_MULTI),
]

KEYS = "TW TH NP KS T D L msplit ntiles tiles_w nphase ncb nchunks".split()
TAIL = "PW PWh NPIXp xcd_images".split()


# ------------------------------------------------------------------------------------------------ the plan line
def plan_line(c, flags=None, n=256):
    """(return code, the line) of masic_conv_f16k_plan_name"""
    from masic_amd import _lib
    buf = ctypes.create_string_buffer(b"?" * (n - 1), n)
    rc = _lib.lib.masic_conv_f16k_plan_name(ctypes.byref(desc_of(c)), c.flags if flags is None else flags, buf, n)
    return rc, buf.value.decode()


def parse(line):
    name, grid, block, lds, ints = line.strip().split(" | ")
    ints = [int(v) for v in ints.split()]
    v = dict(zip(KEYS, ints))
    v["spc"] = ints[len(KEYS):len(KEYS) + v["nphase"]]
    assert len(ints) == len(KEYS) + v["nphase"] + len(TAIL), line
    v.update(zip(TAIL, ints[len(KEYS) + v["nphase"]:]))
    v["block"], v["lds"] = int(block), int(lds)
    return name, tuple(int(g) for g in grid.split(",")), v


def plan(c, flags=None):
    """(kernel, (gx, gy, gz), {name: integer, "spc": [steps per chunk of each phase]}), or None where the launcher refuses the call"""
    rc, line = plan_line(c, flags)
    return parse(line) if rc == 0 and line else None


def table_names():
    from masic_amd import _lib
    out, buf = [], ctypes.create_string_buffer(96)
    while _lib.lib.masic_conv_f16k_row_name(len(out), buf, 96) == 0:
        out.append(buf.value.decode())
    return out


def row_params(name):
    """{KS, T, D, PSP, L, GDN, NM, NP, F8, MULTI} of a row's name"""
    m = re.fullmatch(r"conv_f16k_multi<(\d)>", name)
    if m:
        return dict(KS=1, T=5, D=2, PSP=6, L=1, GDN=False, NM=int(m.group(1)), NP=1, F8=False, MULTI=True)
    m = re.fullmatch(r"conv_f16k<(\d), (\d), (\d), (\d), (\d), (true|false), (\d), (\d), (true|false)>", name)
    g = m.groups()
    return dict(KS=int(g[0]), T=int(g[1]), D=int(g[2]), PSP=int(g[3]), L=int(g[4]), GDN=g[5] == "true", NM=int(g[6]), NP=int(g[7]), F8=g[8] == "true",
                MULTI=False)


def plane(c):
    """(Hp, Wp) of phase 0: the plane the tiles cover"""
    if c.transposed:
        return c.H, c.W
    return out_hw(c)


def properties(c, p=None):
    """the properties of the module docstring as {name: bool}; `past` only where the plan line says msplit > 1"""
    name, grid, v = p or plan(c)
    Hp, Wp = plane(c)
    NM = row_params(name)["NM"]
    rem = c.Cout % 128
    out = {"batch": c.B >= 2,
           "tiles": v["tiles_w"] > 1 and v["ntiles"] // v["tiles_w"] > 1,
           "ragged_h": Hp % v["TH"] != 0, "ragged_w": Wp % v["TW"] != 0,
           "ring": v["nchunks"] >= v["L"] + 2,
           "pad_taps": any(t % v["T"] != 0 for t in phase_taps(c)),
           "cout": c.Cout in (160, 192) and v["ncb"] == 2}
    if v["msplit"] > 1:
        out["past"] = rem != 0 and rem <= 128 - NM * 32
    return out


def waivable(name):
    """{property: rule} a row's own parameters force away"""
    r = row_params(name)
    out = {}
    if r["T"] == 5:
        out["pad_taps"] = T5
    if r["GDN"]:
        out["cout"] = GDN128
    elif r["D"] == 1:
        out["cout"] = LITE
    elif r["NP"] == 4:
        out["cout"] = NP4
    return out


Entry = collections.namedtuple("Entry", "id kernel case waived")


def row_cases():
    return [Entry("row " + k, k, case_of(t, prec, 0, flags), w) for k, t, prec, flags, w in ROW_CASES]


def geometry_cases():
    return [Entry("geometry " + what, k, case_of(t, prec, 0, flags, view), None) for what, k, t, prec, flags, view in GEOMETRY_CASES]


def form_cases():
    return [Entry("form " + what, k, case_of(t, PREC_BF16, act, flags), None) for what, k, t, act, flags in FORM_CASES]


def seed_of(entry):
    """the seed of a case's operands: a function of its id alone, so that a new case leaves every other case's operands alone"""
    return 9000 + zlib.crc32(entry.id.encode()) % 100000


# ------------------------------------------------------------------------------------------------ the search
KINDS = [(5, 2, 0, 0), (3, 2, 0, 0), (3, 1, 0, 0), (5, 1, 0, 0), (5, 1, 0, 1), (5, 2, 1, 0)]      # (k, stride, transposed, masked)
BATCHES = (2, 3, 8, 9, 16)
CINS = (48, 64, 80, 96, 128, 256)
COUTS = (32, 64, 96, 128, 160)
NTH = range(2, 62)


def _candidates(prec, flags):
    for k, s, tr, m in KINDS:
        for B in BATCHES:
            for Cin in CINS:
                if Cin % (32 if prec == PREC_FP8 else 16):
                    continue
                for Cout in ((128,) if flags & F16K_GDN else COUTS):
                    for n in NTH:
                        Hp, Wp = (n - 1) * 8 + 1, 33
                        H, W = (2 * Hp - 1, 2 * Wp - 1) if s == 2 and not tr else (Hp, Wp)
                        yield case_of((B, Cin, H, W, Cout, k, s, tr, m), prec, 0, flags)


def search():
    """ROW_CASES: per row the cheapest candidate with every property the row's own parameters do not forbid"""
    names = table_names()
    best = {}
    for prec in (PREC_BF16, PREC_FP8):
        for flags in (0, F16K_GDN, F16K_MULTI):
            if prec == PREC_FP8 and flags == F16K_MULTI:
                continue
            for c in _candidates(prec, flags):
                key = (macs(c), tuple(c))
                p = plan(c)
                if p is None or (p[0] in best and best[p[0]][0] <= key):
                    continue
                lost = {n for n, ok in properties(c, p).items() if not ok}
                if lost <= set(waivable(p[0])):
                    best[p[0]] = (key, c, lost)
    out = []
    for name in names:
        _, c, lost = best[name]
        w = waivable(name)
        out.append((name, tuple(c[:9]), c.prec, c.flags, {n: w[n] for n in sorted(lost)}))
    return out


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coremasic", "mywork"))
    print("ROW_CASES = [")
    for name, t, prec, flags, lost in search():
        why = "{" + ", ".join(f'"{n}": {_REASON_NAMES[r]}' for n, r in lost.items()) + "}"
        print(f'    ("{name}", {t}, {("PREC_BF16", "PREC_FP8")[prec - 1]}, {flags}, {why}),')
    print("]")
