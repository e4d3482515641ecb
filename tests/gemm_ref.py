"""A plain torch-on-CPU float64 reference of one entropy-parameter layer -- y = act(W x + b), or the type-A masked 5x5 context
convolution, optionally times a per-pixel gate -- and the case tables the six kernels that compute such layers are held to
(tests/test_cpu_gemm_rows.py, tests/test_gpu_gemm_rows.py).  Nothing here needs a GPU or the compiled library.

Which kernel a call runs follows from the kinds of its arguments, not from a name the caller passes:
    masic_gemm_f16k_group_fwd (gemm_f16k.hip)   wscale set -> gemm_f16k<4, true>;  else any fp8 output -> gemm_f16k<2>;  else gemm_f16k2
    masic_gemm1x1_bf16_fwd (gemm_bf16.hip)      gemm1x1_bf16_kernel
    masic_skinny_group_fwd_batch (skinny.hip)   ctx -> skinny_f16k<8, true>;  else skinny_f16k<4, false>
so a case's `kernel` column is a statement about its layers' operand precision and output kinds, which kernel_of() re-derives.

The layer and its bias are float64 (layer64) on the operands the kernel sees (bf16 values, or values e4m3 holds exactly); the
epilogue is float32 in the kernel's order (expected: act32, then * gate), with one round-to-nearest-even to bf16 for an F16K output
and f16k_ref.fp8_out_ref for an F8K output.  Operands are drawn by f16k_ref.inputs; the layouts, the prefill and the fp8 operand
lists are f16k_ref's as well.

The constants of the kernels that the case tables lean on are restated below, each with the line of the source it restates: a change
of tile shape or chunk depth has to revisit the tables, and tests/test_cpu_gemm_rows.py asserts what every case forces from them."""
import collections
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import hsic_oracle as O
from tests import conv_ref as C
from tests import f16k_ref as R
from tests.f16k_ref import ACT_LEAKY, ACT_NONE, ACT_RELU, PREC_BF16, PREC_FP8

G2, G16, G8, RS, S1, SC = ("gemm_f16k2", "gemm_f16k<2>", "gemm_f16k<4, true>", "gemm1x1_bf16_kernel", "skinny_f16k<4, false>",
                           "skinny_f16k<8, true>")
KERNELS = (G2, G16, G8, RS, S1, SC)

# ---- the kernels' constants, restated
CO_TILE, PX_TILE = 128, 256       # gemm_f16k.hip: "tile 128 co x 256 px" (p0 = ... * 256, m0 = cblk * 128, in all three kernels); gemm_bf16.hip: "block = 4 waves (2 x 2): 128 co x 256 pixels"
PAD_BLOCKS = 4                    # gemm_f16k.hip: `nchunks = round_up(ceil_div(Cin, 16), 4)` (pack) and `nkb = round_up(cin_b, 4)` (launch): channel blocks padded to a multiple of 4
BLOCK_CH = {G2: 16, G16: 16, G8: 32, RS: 16}      # gemm_f16k.hip: `const int cblk = f8 ? 32 : 16;` -- channels of one k block
CHUNK_BLOCKS = {G2: 4, G16: 2, G8: 4}             # gemm_f16k.hip: `const int kc = f8 ? 4 : (f8_out ? 2 : G2_KC);`, `constexpr int G2_KC = 4`: 64-, 32- and 128-channel chunks
RING = 3                          # gemm_f16k.hip: `G2_NS = 3` and, in gemm_f16k, `NS = 3`: weight (and activation) stages in flight
WAVE_PX = {G2: 64, G16: 32, G8: 32, RS: 128}      # gemm_f16k.hip: `p0 + wave * 64 + q * 32 + j` (gemm_f16k2), `p0 + wave * 32 + j` (gemm_f16k); gemm_bf16.hip: `p0 = blockIdx.x * 256 + wn * 128`
RS_WAVE_CO = 64                   # gemm_bf16.hip: `m0 = blockIdx.y * 128 + wm * 64`
XCD = 8                           # gemm_f16k.hip: `b = B >= 8 ? (n & 7) + 8 * ((n >> 3) / tiles_per_img) : n / tiles_per_img; if (b >= B) return;`
SK_NW = {S1: 4, SC: 8}            # skinny.hip: `hipLaunchKernelGGL((skinny_f16k<8, true>), grid, dim3(512)` / `(skinny_f16k<4, false>), grid, dim3(256)`: waves that split the K loop
SK_CH = 8                         # skinny.hip: `constexpr int SK_CH = 8;` k-steps per load batch and wave
SK_TAPS = 12                      # skinny.hip: `ctx ? 12 * cin16 : round_up(cin16, 4)` -- k-steps of a launch: the live taps of the type-A 5x5 mask
SK_PX = 32                        # skinny.hip: `const int pi = blockIdx.y * 32 + j;` pixels of a workgroup

# One layer of a launch.  out: "nchw" (float32), "f16k" (bf16), "f8k" (e4m3 of y / out_scale) or "f8k-sat" (the same with an out_scale
# under which some outputs pass +-448); view: (out_ctot, out_coff) or None for a whole buffer of Cout channels
Layer = collections.namedtuple("Layer", "Cin Cout act bias out transposed view")
# One launch: B images (nimg for the pixel-list kernels) of H x W, operand precision, its layers (a group launch has up to three), and
# for the context model ctx = True and gate = (gate_ctot, gate_c) or None.  forces: what the case is in the table for, as
# {property of properties(): value}
Case = collections.namedtuple("Case", "id kernel B H W prec layers ctx gate forces")


def L(Cin, Cout, act=ACT_NONE, bias=True, out="nchw", transposed=False, view=None):
    return Layer(Cin, Cout, act, bias, out, transposed, view)


def _case(id, kernel, B, hw, layers, prec=PREC_BF16, ctx=False, gate=None, **forces):
    layers = tuple(layers) if isinstance(layers, (list, tuple)) and not isinstance(layers, Layer) else (layers,)
    return Case(id, kernel, B, hw[0], hw[1], prec, layers, ctx, gate, forces)


SMALL, TWO_TILES, XCD_HW = (5, 7), (9, 33), (13, 21)      # HW = 35; 297 = 256 + 41; 273 = 256 + 17
GROUP3 = (L(176, 160, ACT_RELU, out="f16k"), L(64, 96, ACT_LEAKY), L(256, 288, ACT_NONE, out="f16k"))

FULL_CASES = [
    _case("g2-tiny", G2, 2, SMALL, L(16, 32, bias=False),
          nchunks=(1,), pad_blocks=(3,), co_blocks=(1,), last_co=(32,), px_tiles=1, last_px=35, subtile1_live=3),
    _case("g2-odd", G2, 3, TWO_TILES, L(176, 160, ACT_LEAKY, out="f16k", transposed=True),
          nchunks=(3,), tail_body=(True,), pad_blocks=(1,), co_blocks=(2,), last_co=(32,), px_tiles=2, last_px=41, dead_waves=3, xcd_order=False),
    _case("g2-even", G2, 2, TWO_TILES, L(256, 96, ACT_RELU, view=(136, 8)),
          nchunks=(4,), tail_body=(False,), ring_wraps=(True,), pad_blocks=(0,), last_co=(96,)),
    _case("g2-deep", G2, 2, TWO_TILES, L(1152, 160, ACT_LEAKY), nchunks=(18,), ring_wraps=(True,)),
    _case("g2-xcd8", G2, 8, XCD_HW, L(64, 160, ACT_RELU, out="f16k"), xcd_order=True, dead_workgroups=0, px_tiles=2, co_blocks=(2,)),
    _case("g2-xcd11", G2, 11, XCD_HW, L(64, 160, ACT_RELU), xcd_order=True, dead_workgroups=20, workgroups=64),
    _case("g2-view16", G2, 2, SMALL, L(64, 160, out="f16k", view=(256, 48)), view_align=(16,)),
    _case("g2-group3", G2, 3, TWO_TILES, GROUP3, cb_end=(2, 3, 6), nchunks=(3, 1, 4)),
    _case("g16-f8out", G16, 2, TWO_TILES, L(48, 160, ACT_RELU, out="f8k-sat"), nchunks=(2,), pad_blocks=(1,), chunk_channels=32),
    _case("g16-mixed", G16, 9, SMALL, (L(176, 160, ACT_LEAKY, out="f16k"), L(64, 96, ACT_NONE), L(176, 160, ACT_RELU, out="f8k")),
          nchunks=(6, 2, 6), cb_end=(2, 3, 5), grid_z=9),
    _case("g8-one", G8, 2, SMALL, L(32, 32), prec=PREC_FP8, nchunks=(1,), pad_blocks=(3,), chunk_channels=128),
    _case("g8-two", G8, 2, TWO_TILES, L(160, 160, ACT_LEAKY, out="f16k"), prec=PREC_FP8, nchunks=(2,), last_co=(32,)),
    _case("g8-ring", G8, 3, TWO_TILES, L(416, 96, ACT_RELU, out="f8k"), prec=PREC_FP8, nchunks=(4,), ring_wraps=(True,)),
    _case("r-odd", RS, 3, SMALL, L(100, 50, ACT_LEAKY, view=(60, 7)), cin_pad=(112,), cout_pad=(128,), clamped_px=128 - 35),
    _case("r-tiles", RS, 2, TWO_TILES, L(176, 160, ACT_RELU, out="f16k", transposed=True), co_blocks=(2,), px_tiles=2, wave_tiles=(2, 2)),
]

LIST_CASES = [
    _case("s1-k1", S1, 1, SMALL, L(16, 32), nsteps=(4,), nper=(1,)),
    _case("s1-k8", S1, 1, SMALL, L(512, 32, out="f16k"), nper=(8,), batches=(1,), last_batch=(8,)),
    _case("s1-k9", S1, 3, SMALL, L(528, 160, ACT_RELU, out="f16k", view=(256, 48)), nper=(9,), batches=(2,), last_batch=(1,), k16=(33,), nsteps=(36,)),
    _case("s1-k17", S1, 1, SMALL, L(1040, 32, ACT_LEAKY), nper=(17,), batches=(3,)),
    _case("s1-k18", S1, 3, TWO_TILES, L(1152, 160, ACT_LEAKY, view=(200, 24)), nper=(18,)),
    _case("s1-group3", S1, 3, TWO_TILES, GROUP3, tile_end=(5, 8, 17)),
    _case("sc-k2", SC, 1, SMALL, L(16, 32, bias=False, out="f16k"), ctx=True, nsteps=(12,), nper=(2,), idle_slots=(4,)),
    _case("sc-ragged", SC, 3, SMALL, L(80, 160, ACT_LEAKY, out="f16k", view=(400, 160)), ctx=True, gate=(3, 1), nsteps=(60,), nper=(8,), idle_slots=(4,)),
    _case("sc-wide", SC, 2, TWO_TILES, L(192, 384, out="f16k", view=(960, 384)), ctx=True, gate=(2, 1), nsteps=(144,), nper=(18,), idle_slots=(0,)),
]
CASES = FULL_CASES + LIST_CASES


def by_id(name):
    return next(c for c in CASES if c.id == name)


def seed_of(case, i=0):
    return zlib.crc32(case.id.encode()) % 100000 + 17 * i


def kernel_of(case):
    """the kernel the entry points' dispatch picks for the case's argument kinds (module docstring); the register-streamed kernel has an
    entry point of its own and is taken at its word"""
    if case.kernel in (S1, SC):
        return SC if case.ctx else S1
    if case.kernel == RS:
        return RS
    if case.prec == PREC_FP8:
        return G8
    return G16 if any(l.out.startswith("f8k") for l in case.layers) else G2


def _ceil(a, b):
    return -(-a // b)


def properties(case):
    """what the case's integers make the kernel do, from the constants above: per layer tuples, and launch-wide scalars"""
    k, HW, p = case.kernel, case.H * case.W, {}
    ls = case.layers
    if k in (S1, SC):
        nw = SK_NW[k]
        k16 = [l.Cin // 16 for l in ls]
        nsteps = [SK_TAPS * n if case.ctx else _ceil(n, PAD_BLOCKS) * PAD_BLOCKS for n in k16]
        nper = [_ceil(n, nw) for n in nsteps]
        p.update(k16=tuple(k16), nsteps=tuple(nsteps), nper=tuple(nper), batches=tuple(_ceil(n, SK_CH) for n in nper),
                 last_batch=tuple(n - (_ceil(n, SK_CH) - 1) * SK_CH for n in nper),
                 idle_slots=tuple(nw * a - b for a, b in zip(nper, nsteps)))           # k-steps past the end, whose loads read nothing
        ends, t = [], 0
        for l in ls:
            t += l.Cout // 32
            ends.append(t)
        p["tile_end"] = tuple(ends)
        return p
    bch = BLOCK_CH[k]
    blocks = [_ceil(l.Cin, bch) for l in ls]
    co_blocks = [_ceil(l.Cout, CO_TILE) for l in ls]
    p.update(co_blocks=tuple(co_blocks), last_co=tuple(l.Cout - (n - 1) * CO_TILE for l, n in zip(ls, co_blocks)),
             px_tiles=_ceil(HW, PX_TILE), last_px=HW - (_ceil(HW, PX_TILE) - 1) * PX_TILE,
             view_align=tuple(16 if l.view and l.view[1] % 32 else 32 for l in ls))
    ends, t = [], 0
    for n in co_blocks:
        t += n
        ends.append(t)
    p["cb_end"] = tuple(ends)
    p["dead_waves"] = PX_TILE // WAVE_PX[k] - _ceil(p["last_px"], WAVE_PX[k])        # waves of the last pixel tile with no live pixel
    if k == RS:
        p.update(cin_pad=tuple(n * 16 for n in blocks), cout_pad=tuple(n * CO_TILE for n in co_blocks),
                 clamped_px=max(0, WAVE_PX[RS] - p["last_px"]),                       # pixels of the last live wave tile clamped to HW - 1
                 wave_tiles=(CO_TILE // RS_WAVE_CO, PX_TILE // WAVE_PX[RS]))
        return p
    padded = [_ceil(n, PAD_BLOCKS) * PAD_BLOCKS for n in blocks]
    nchunks = [n // CHUNK_BLOCKS[k] for n in padded]
    p.update(nchunks=tuple(nchunks), pad_blocks=tuple(a - b for a, b in zip(padded, blocks)), chunk_channels=CHUNK_BLOCKS[k] * bch,
             ring_wraps=tuple(n > RING for n in nchunks), tail_body=tuple(n % 2 == 1 for n in nchunks), grid_z=case.B)
    if k == G2:
        tiles = p["px_tiles"] * ends[-1]
        p["subtile1_live"] = max(0, min(32, p["last_px"] - 32))                       # live lanes of wave 0's second 32-pixel sub-tile, last tile
        p["xcd_order"] = case.B >= XCD
        p["workgroups"] = XCD * tiles * _ceil(case.B, XCD) if case.B >= XCD else case.B * tiles
        p["dead_workgroups"] = p["workgroups"] - case.B * tiles
    return p


# ------------------------------------------------------------------------------------------------ operands
def _rcase(case, l):
    k = 5 if case.ctx else 1
    return R.case_of((case.B, l.Cin, case.H, case.W, l.Cout, k, 1, int(l.transposed), int(case.ctx)), case.prec, l.act)


def operands(case, i, integers=False, seed_shift=0):
    """(x, w, bias or None) of layer i, drawn as f16k_ref.inputs draws them: float32 CPU tensors, x [B, Cin, H, W] and w exact in the
    operand format; w is [Cout, Cin, k, k], or [Cin, Cout, 1, 1] for a transposed layer"""
    l = case.layers[i]
    x, w, bias = R.inputs(_rcase(case, l), seed_of(case, i) + seed_shift, integers=integers)
    return x, w, (bias if l.bias else None)


def gate_plane(case, seed_shift=0):
    """the gate tensor [B, gate_ctot, H, W] of a context-model case (float32 in [0, 1)), or None"""
    if case.gate is None:
        return None
    g = torch.Generator().manual_seed(seed_of(case, 7) + seed_shift)
    return torch.rand((case.B, case.gate[0], case.H, case.W), generator=g)


def exact_bound(case, l, x, w, bias):
    """max|x| max|w| K + max|bias| with K = Cin for a 1x1 layer and 12 Cin for the masked 5x5: below 2^24 every partial sum is a
    float32 integer in any order"""
    K = l.Cin * (SK_TAPS if case.ctx else 1)
    return float(x.abs().max()) * float(w.abs().max()) * K + (0.0 if bias is None else float(bias.abs().max()))


# ------------------------------------------------------------------------------------------------ the layer
def layer64(case, l, x, w, bias):
    """W x + b in float64, [B, Cout, H, W]: F.conv2d on the [Cout, Cin, 1, 1] view (a transposed layer's weight is [Cin, Cout, 1, 1],
    the ConvTranspose2d(k = 1) orientation), or on the type-A masked 5x5 weight with padding 2"""
    b = None if bias is None else bias.double()
    if case.ctx:
        return F.conv2d(x.double(), O.masked_weight(w.double()), b, padding=2)
    w2 = w.reshape(w.shape[0], w.shape[1])
    if l.transposed:
        w2 = w2.t()
    return F.conv2d(x.double(), w2.double().reshape(l.Cout, l.Cin, 1, 1), b)


def f8_scale(v32, saturate=False):
    """the power of two under which the peak of v lands in (224, 448] -- or, saturate, in (448, 896]: some outputs pass +-448"""
    e = int(math.ceil(math.log2(float(v32.abs().max()) / 448.0)))
    return 2.0 ** (e - 1 if saturate else e)


def expected(l, v64, gate=None, out_scale=None):
    """what the layer stores, from W x + b in float64: the float32 epilogue in the kernel's order -- act32(v), then * gate (float32
    [B, 1, H, W]) -- as float32 (NCHW), rounded once to bf16 (F16K), or through f16k_ref.fp8_out_ref (F8K: decoded, times out_scale)"""
    v = R.act32(v64.float(), l.act)
    if gate is not None:
        v = v * gate
    if l.out == "nchw":
        return v
    if l.out == "f16k":
        return v.bfloat16()
    return R.fp8_out_ref(v, out_scale)


def prefill_of(l, scale=1.0, listed=False):
    """what an output buffer holds before the call: bf16 0.5 (f16k_ref.PREFILL_BITS) for F16K, e4m3 1.0 for F8K; float32 0.5 for the
    full-latent kernels and NaN for the pixel-list kernels"""
    if l.out == "nchw":
        return float("nan") if listed else R.PREFILL
    return R.PREFILL if l.out == "f16k" else 1.0 * scale


def whole_buffer(l, y, prefill):
    """y as channels out_coff .. of the layer's output buffer"""
    ctot, coff = l.view or (l.Cout, 0)
    return R.in_view(y, ctot, coff, prefill)


def scatter_ref(full, pix_list, nimg, HW, prefill):
    """the full-latent result `full` [nimg, C, H, W] kept at the pixels the list names -- a valid entry is q with 0 <= q < nimg * HW,
    image q // HW, pixel q % HW -- and `prefill` everywhere else"""
    assert full.shape[0] == nimg and full.shape[2] * full.shape[3] == HW
    out = torch.full(full.shape, prefill, dtype=full.dtype)
    src, dst = full.reshape(nimg, full.shape[1], HW), out.view(nimg, full.shape[1], HW)
    for q in pix_list.tolist() if torch.is_tensor(pix_list) else pix_list:
        if 0 <= q < nimg * HW:
            dst[q // HW, :, q % HW] = src[q // HW, :, q % HW]
    return out


def gate_for(l):
    """the project's gate for a run on real operands, of the reference's peak (tests/conv_ref.gate_of; tests/test_gpu_f16k_rows run (b)):
    2e-5 for a float32 NCHW output, 2^-8 for an F16K output against the reference rounded to bf16; None for an F8K output, whose
    comparison with the reference is the whole-number run"""
    if l.out.startswith("f8k"):
        return None
    return C.gate_of(C.case_of((0,) * 9 + (C.PREC_BF16, 0), form=C.F16K_OUT if l.out == "f16k" else 0))


# ------------------------------------------------------------------------------------------------ pixel lists
PixList = collections.namedtuple("PixList", "name pix step list_stride npix named")     # named: the entries the launch reads (valid or not)


def pixel_lists(case):
    """the four lists every pixel-list case runs with (flat int32 tensors):
    all     every pixel of every image, in order;
    shuffle a seeded shuffle of about 60 % of the pixels with -1 entries, entries >= nimg * HW and one whole 32-entry block of -1 among
            them, of a length that is no multiple of 32;
    steps   the decoder's form, [steps][list_stride] padded with -1, read at the row a device step counter (1) names;
    one     one pixel alone"""
    HW = case.H * case.W
    N = case.B * HW
    g = torch.Generator().manual_seed(seed_of(case, 3))
    perm = torch.randperm(N, generator=g).tolist()
    some = perm[:round(0.6 * N)]
    for at, v in ((3, -1), (7, N + 5), (11, -1), (13, N)):
        some.insert(at, v)
    at = SK_PX if len(some) >= 2 * SK_PX else 0
    some[at:at] = [-1] * SK_PX
    if len(some) % SK_PX == 0:
        some.append(-1)
    stride, rows = 40, 3
    live = min(37, N // rows)
    grid = torch.full((rows, stride), -1, dtype=torch.int32)
    for r in range(rows):
        grid[r, :live] = torch.tensor(perm[r * live:(r + 1) * live], dtype=torch.int32)
    one = (case.B - 1) * HW + HW // 2
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return [PixList("all", torch.arange(N, dtype=torch.int32), None, 0, N, list(range(N))),
            PixList("shuffle", i32(some), None, 0, len(some), some),
            PixList("steps", grid.reshape(-1), 1, stride, stride, grid[1].tolist()),
            PixList("one", i32([one]), None, 0, 1, [one])]
