"""Cases, launcher rules, float64 references and derived error bounds for the kernels the training graph runs BETWEEN its contractions:
the non-contraction kernels of masic_amd/csrc/backward.hip, the helpers of misc.hip, quantize / symbols / softmax_k of entropy.hip, the
shared vector plane copy of common.h and the three elementwise / sum kernels of f16k_ops.hip.  Importable without a GPU:
tests/test_cpu_small_kernels.py holds every case to the branch it is filed under and every reference to torch float64 autograd of the
defining expression; tests/test_gpu_small_kernels.py runs the kernels.

References take the float32 values the kernel sees (bf16-rounded values for the F16K kernels), cast to float64, and evaluate the one
operation plainly.

Bounds are derived, never fitted.  With u = 2^-24 (one float32 rounding to nearest: |fl(v) - v| <= u |v|), a result that is a sum of terms,
each a product / quotient that has passed through at most m roundings, added up through at most a additions, is off by at most
    k u (sum of the magnitudes of the terms),  k = m + a,
to first order in u (k u < 2e-4 everywhere here).  Every k below is computed from the case's shape by a function that says which
roundings it counts.  Operations with one rounding or none must equal the float32 evaluation (numpy float32: IEEE, no fused
multiply-add) bit for bit, the sign of zero included.  sqrtf and / are correctly rounded under hipcc's defaults: one rounding each.
expf / logf: the per-call counts EXPF_ROUNDINGS / LOGF_ROUNDINGS below were measured on the device (see there)."""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ launcher rules, restated
CAP_EW = 8192          # backward.hip:17 grid_for(total, cap = 8192); entropy.hip:207-210; misc.hip:170,176,185 (lower_bound, copy_view)
CAP_MUL = 4096         # misc.hip:164  mul_inplace
CAP_RD_BWD = 4096      # misc.hip:251  rd_loss_bwd
CAP_RED = 1024         # misc.hip:23   RED_BLOCKS: sum_log, sse, rd_loss
CAP_GDN_SMALL = 2048   # backward.hip:994 grid_for(total, 2048)
CAP_F16K_ACT = 8192    # f16k_ops.hip:235
CAP_PLANE = 8192       # common.h:121  about 8192 workgroups across planes
MAX_PLANES = 65535     # common.h:118  gridDim.y
CS_SPLIT = 64          # backward.hip:59
CS_CHUNK = 4096        # backward.hip:67  pixels per (image, chunk) work item
CS_ONE_BLOCK_PIXELS, CS_ONE_BLOCK_CHANNELS = 16384, 128      # backward.hip:909
F16K_CS_CHUNKS = 32    # f16k_ops.hip:240
GDN_FINISH_ROWS = 512  # backward.hip:260  partial rows per pass of gdn_bwd_small_finish
PED = 2.0 ** -36       # backward.hip:991 reparametrisation pedestal


def cdiv(a, b):
    return -(-a // b)


def grid_for(total, cap):
    """backward.hip:17-20 / misc.hip:155-158: workgroups of 256 threads, capped"""
    return min(max(cdiv(total, 256), 1), cap)


def past_cap_uneven(items, cap):
    """the grid-stride loop runs more than once and some threads once more than others"""
    return items > cap * 256 and items % (cap * 256) != 0


def n_past(cap):
    return cap * 256 + 257


def plane_copy_plan(B, C, HW, aligned=True):
    """common.h:116-130 masic_plane_copy: None where it refuses (the caller's scalar kernel runs), else its grid"""
    if HW % 4 != 0 or B * C > MAX_PLANES or B * C == 0 or not aligned:
        return None
    HW4 = HW // 4
    gx = cdiv(HW4, 4 * 256)
    gx = max(1, min(gx, cdiv(CAP_PLANE, B * C)))
    passes = cdiv(HW4, 4 * gx * 256)
    return dict(gx=gx, planes=B * C, passes=passes, lane_loop=passes > 1, k3=HW4 > 3 * gx * 256)


def channel_sum_plan(B, C, HW, aligned=True):
    """backward.hip:904-916 masic_channel_sum and :61-93 channel_sum_stage1"""
    one_block = B * HW <= CS_ONE_BLOCK_PIXELS and C >= CS_ONE_BLOCK_CHANNELS
    splits = 1 if one_block else CS_SPLIT
    vec = HW % 4 == 0 and aligned
    chunks = cdiv(HW, CS_CHUNK)
    work = B * chunks
    per_chunk = cdiv(min(HW, CS_CHUNK), 1024 if vec else 256)       # additions into one float32 accumulator per work item
    n_acc = cdiv(work, splits) * per_chunk
    # n_acc float32 additions, the float64 tree (far below u: one unit covers it), the final rounding to float32
    return dict(one_block=one_block, vec=vec, chunks=chunks, work=work, splits=splits, ragged=HW % CS_CHUNK != 0,
                stage2_partial=(not one_block) and C % 64 != 0, k=n_acc + 2)


def f16k_sum_plan(B, C, HW):
    """f16k_ops.hip:147-169, :187-226: 32 pixel chunks per (image, 16-channel block), 128 pixel lanes per chunk"""
    per = cdiv(HW, F16K_CS_CHUNKS)
    last = HW - (cdiv(HW, per) - 1) * per                            # pixels of the last non-empty chunk
    sizes = {per, last}
    two_load = any(s > 128 for s in sizes)                           # some lane has px + 128 < hi
    single_tail = any(s % 256 != 0 for s in sizes)                   # some lane's last trip has no partner 128 pixels on
    # per-thread additions, 128 LDS additions, the float64 stage (one unit) and the final rounding
    return dict(per=per, empty_chunks=cdiv(HW, per) < F16K_CS_CHUNKS, two_load=two_load, single_tail=single_tail,
                k=cdiv(per, 128) + 128 + 2)


def gdn_small_plan(B, C, H, W):
    """backward.hip:986-1006"""
    total = B * H * W
    nb = grid_for(total, CAP_GDN_SMALL)
    return dict(nb=nb, per_thread=cdiv(total, nb * 256), finish_passes=cdiv(nb, GDN_FINISH_ROWS))


# ------------------------------------------------------------------------------------------------ helpers
def rng(seed):
    return np.random.RandomState(seed)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    return f32(a).view(np.int32)


def bit_equal(got, want):
    return np.array_equal(bits(got), bits(want))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; elements with a zero bound must be equal"""
    got, ref, bound = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, ref, np.broadcast_to(bound, np.shape(ref))))
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - ref)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def misaligned(t_numel, torch_device, shift=1):
    """contiguous float32 buffer on the device whose first element sits `shift` floats past a 16-byte line (tests/test_gpu_refine.py::_tensor)"""
    buf = torch.zeros(t_numel + 8, dtype=torch.float32, device=torch_device)
    off = (shift - (buf.data_ptr() // 4) % 4) % 4
    t = buf[off:off + t_numel]
    assert (t.data_ptr() // 4) % 4 == shift and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------ elementwise (backward.hip:23-54)
EW_OPS = ("ACT_BWD", "ABS_BWD", "SQUARE", "ABS", "AXPY", "RECIP_SCALE", "DIFF_SCALE", "MUL", "REPARAM", "REPARAM_BWD", "ADD")
EW_SIZES = (1, 255, 256, 257, n_past(CAP_EW))
EW_EXACT = ("ACT_BWD", "ABS_BWD", "ABS", "SQUARE", "MUL", "ADD", "DIFF_SCALE", "REPARAM_BWD")
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
REPARAM_BOUND = float(np.float32(math.sqrt(1e-6 + PED)))       # the beta bound of a GDN: a float32 value


def ew_inputs(op, n, seed, act=ACT_LEAKY, with_b=True):
    """(a, b or None, s0, s1): float32 arrays and float32-exact scalars, the edge values of the op in the first elements"""
    r = rng(seed)
    a, b = f32(r.standard_normal(n)), f32(r.standard_normal(n))
    s0, s1 = 0.0, 0.0
    if op == "ACT_BWD":
        s0 = float(act)
        b[: min(n, 4)] = f32([0.0, -0.0, 1.0, -1.0])[: min(n, 4)]
    elif op == "ABS_BWD":
        b[: min(n, 2)] = f32([0.0, -0.0])[: min(n, 2)]
    elif op == "AXPY":
        s0, s1 = float(np.float32(0.7)), float(np.float32(-1.3))
        if not with_b:
            b = None
    elif op == "RECIP_SCALE":
        a = f32(np.abs(a) + 0.1) * f32(np.where(r.rand(n) < 0.5, -1, 1))
        s0, b = float(np.float32(-0.37)), None
    elif op == "DIFF_SCALE":
        s0 = float(np.float32(2.0 / 3.0))
    elif op == "REPARAM":
        # stored parameters below, at and above the bound
        a = f32(np.abs(a) * 0.01)
        a[: min(n, 3)] = f32([REPARAM_BOUND, REPARAM_BOUND * 0.5, 0.0])[: min(n, 3)]
        s0, s1, b = REPARAM_BOUND, PED, None
    elif op == "REPARAM_BWD":
        # b = stored parameter below / at / above the bound, a = gradient of both signs: all six combinations lead
        b = f32(np.abs(b) * 0.002)
        edge_p = f32([REPARAM_BOUND * 0.5, REPARAM_BOUND * 0.5, REPARAM_BOUND, REPARAM_BOUND, 0.5, 0.5])
        edge_g = f32([1.5, -1.5, 1.5, -1.5, 1.5, -1.5])
        b[: min(n, 6)], a[: min(n, 6)] = edge_p[: min(n, 6)], edge_g[: min(n, 6)]
        s0 = REPARAM_BOUND
    elif op in ("SQUARE", "ABS"):
        b = None
    return a, b, s0, s1


def ew_ref32(op, a, b, s0, s1):
    """the float32 evaluation, operation for operation (numpy float32: IEEE, unfused)"""
    s0f, s1f = np.float32(s0), np.float32(s1)
    zero = np.float32(0.0)
    if op == "ACT_BWD":
        act = int(s0)
        if act == ACT_RELU:
            return f32(np.where(b > 0, a, zero))
        if act == ACT_LEAKY:
            return f32(np.where(b > 0, a, np.float32(0.01) * a))
        return f32(a)
    if op == "ABS_BWD":
        return f32(np.where(b > 0, a, np.where(b < 0, -a, zero)))
    if op == "SQUARE":
        return f32(a * a)
    if op == "ABS":
        return f32(np.abs(a))
    if op == "AXPY":
        return f32(s0f * a + (s1f * b if b is not None else zero))
    if op == "RECIP_SCALE":
        return f32(s0f / a)
    if op == "DIFF_SCALE":
        return f32(s0f * (a - b))
    if op == "MUL":
        return f32(a * b)
    if op == "REPARAM":
        v = np.maximum(a, s0f)
        return f32(v * v - s1f)
    if op == "REPARAM_BWD":
        g = f32(a * np.float32(2.0) * np.maximum(b, s0f))
        return f32(np.where((b >= s0f) | (g < 0), g, zero))
    return f32(a + b)


def ew_ref64(op, a, b, s0, s1):
    """(float64 reference, bound) of the ops that are not held bit for bit"""
    a64 = a.astype(np.float64)
    b64 = None if b is None else b.astype(np.float64)
    if op == "AXPY":        # may be contracted to one FMA: 2^-23 (|term1| + |term2|)
        t1, t2 = s0 * a64, (s1 * b64 if b is not None else np.zeros_like(a64))
        return t1 + t2, 2 * U * (np.abs(t1) + np.abs(t2))
    if op == "REPARAM":
        v = np.maximum(a64, s0)
        return v * v - s1, 2 * U * (v * v + abs(s1))
    if op == "RECIP_SCALE":  # one correctly rounded division
        return s0 / a64, U * np.abs(s0 / a64)
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ channel_sum (backward.hip:56-101, :904-916)
SumCase = namedtuple("SumCase", "id B C HW ctot coff aligned one_block vec k")


def _sum_case(id, B, C, HW, ctot=None, coff=0, aligned=True):
    p = channel_sum_plan(B, C, HW, aligned)
    return SumCase(id, B, C, HW, ctot or C, coff, aligned, p["one_block"], p["vec"], p["k"])


# k = ceil(B * chunks / splits) * ceil(min(HW, 4096) / (1024 float4 | 256 scalar)) + 2, written out by channel_sum_plan:
CHANNEL_SUM_CASES = [
    _sum_case("one_block_float4_two_chunks", 2, 128, 8192),               # k = 4 * 4 + 2 = 18
    _sum_case("one_block_scalar", 3, 130, 35),                            # k = 3 * 1 + 2 = 5
    _sum_case("one_block_at_16384", 1, 128, 16384),                       # k = 4 * 4 + 2 = 18
    _sum_case("two_stage_at_16385", 1, 128, 16385),                       # k = 1 * 16 + 2 = 18 (scalar, 5 work items over 64 splits)
    _sum_case("two_stage_68_items_ragged", 2, 3, 4096 * 33 + 4),          # k = 2 * 4 + 2 = 10
    _sum_case("two_stage_partial_stage2", 1, 70, 100),                    # k = 1 * 1 + 2 = 3
    _sum_case("two_stage_one_channel", 2, 1, 37),                         # k = 1 * 1 + 2 = 3
    _sum_case("channel_view", 2, 3, 36, ctot=7, coff=2),                  # k = 3
    _sum_case("one_block_off_16_bytes", 2, 128, 64, aligned=False),       # scalar although HW % 4 == 0: k = 2 * 1 + 2 = 4
    _sum_case("two_stage_off_16_bytes", 2, 3, 8192, aligned=False),       # scalar: k = 1 * 16 + 2 = 18
]


def channel_sum_input(c, seed=1):
    """[B, ctot, HW] float32; outside the view: values 1e6 times larger, so that a wrong channel shows"""
    r = rng(seed)
    x = f32(r.standard_normal((c.B, c.ctot, c.HW)) * 1e6)
    x[:, c.coff:c.coff + c.C] = f32(r.standard_normal((c.B, c.C, c.HW)))
    return x


def channel_sum_ref(x, c):
    v = x[:, c.coff:c.coff + c.C].astype(np.float64)
    return v.sum(axis=(0, 2)), c.k * U * np.abs(v).sum(axis=(0, 2))


# ------------------------------------------------------------------------------------------------ copies (common.h:76-130, misc.hip:29-37, backward.hip:103-112, entropy.hip:17-39)
CopyCase = namedtuple("CopyCase", "id B C H W ctot coff misalign path")       # path: "vector" | "scalar"; misalign: None | "x" | "y"


def _copy_case(id, B, C, H, W, ctot=None, coff=0, misalign=None):
    p = plane_copy_plan(B, C, H * W, misalign is None)
    return CopyCase(id, B, C, H, W, ctot or C, coff, misalign, "vector" if p else "scalar")


COPY_CASES = [
    _copy_case("vector_four_vectors_per_lane", 2, 3, 64, 64, ctot=7, coff=2),     # HW4 = 1024: every k of the four in flight is used
    _copy_case("vector_partial_fourth", 1, 2, 4, 773, ctot=5, coff=3),            # HW4 = 773: the k = 3 pass holds 5 vectors
    _copy_case("vector_one_vector_per_lane", 2, 3, 4, 4, ctot=5, coff=1),         # HW4 = 4: only k = 0 is in range
    _copy_case("scalar_odd_hw", 2, 3, 5, 7, ctot=7, coff=2),
    _copy_case("scalar_too_many_planes", 2, 32768, 2, 2),                         # B * C = 65536 > 65535
    _copy_case("scalar_x_off_16_bytes", 2, 3, 4, 8, ctot=5, coff=1, misalign="x"),
    _copy_case("scalar_y_off_16_bytes", 2, 3, 4, 8, ctot=5, coff=1, misalign="y"),
    _copy_case("scalar_past_cap", 1, 3, 701, 999, ctot=4, coff=1),                # 2100897 elements: 8192 * 256 + 3745
]
LANE_LOOP_CASE = _copy_case("vector_lane_loop", 2, 2048, 12, 683)                 # 4096 planes x HW = 8196: gx = 2, HW4 = 2049 > 2048
SENTINEL = -12345.0
GATE_CTOT = 3


def copy_inputs(c, seed=2):
    """x, noise [B, C, H, W] and gate [B, 3, H, W]: halves, so that round() meets ties of both parities and -0"""
    r = rng(seed)
    shape = (c.B, c.C, c.H, c.W)
    x = f32(r.randint(-9, 10, size=shape) * 0.5 + (r.rand(*shape) < 0.5) * f32(r.standard_normal(shape)))
    noise = f32(r.rand(*shape) - 0.5)
    gate = f32(r.rand(c.B, GATE_CTOT, c.H, c.W) + 0.25)
    return x, noise, gate


def quantize_ref32(x, mode, noise=None, gate=None, gate_c=0):
    """entropy.hip:25-27 in float32: round to nearest even | + noise | copy, then the gate product"""
    v = f32(np.rint(x)) if mode == "dequantize" else (f32(x + noise) if mode == "noise" else f32(x))
    return v if gate is None else f32(v * gate[:, gate_c:gate_c + 1])


def rounding_edges():
    """ties at +-(k + 0.5) and magnitudes up to 2^23 (above 2^23 every float32 is a whole number)"""
    k = np.array([0, 1, 2, 3, 4, 7, 126, 127, 1000, 2 ** 20, 2 ** 22 - 1, 2 ** 22, 2 ** 23 - 1], dtype=np.float64)
    v = np.concatenate([k + 0.5, -(k + 0.5), [0.0, -0.0, 0.49999997, -0.49999997, 2.0 ** 23, -2.0 ** 23, 2.0 ** 23 - 1, 0.25, -0.25]])
    return f32(v)


SYMBOLS_SHAPE = (2, 5, 1, 7)                                                      # C = 5, HW = 7: 70 elements
SYMBOLS_MEDIANS = f32([0.0, 0.5, -0.25, 1.5, 100.0])


def symbols_input():
    e = rounding_edges()
    n = int(np.prod(SYMBOLS_SHAPE))
    return f32(np.resize(e, n).reshape(SYMBOLS_SHAPE))


def symbols_ref(x, medians):
    """entropy.hip:35-37: (int32) rint(x - median[c]), the difference a float32"""
    m = np.zeros(x.shape[1], np.float32) if medians is None else medians
    return np.rint(f32(x - m.reshape(1, -1, 1, 1))).astype(np.int32)


# ------------------------------------------------------------------------------------------------ gate_bwd (backward.hip:114-144)
GateCase = namedtuple("GateCase", "id B C H W k")


def gate_k(C):
    """ggate: ceil(C / 16) fused multiply-adds per thread, then the 16 partial sums of a pixel in LDS"""
    return cdiv(C, 16) + 16


GATE_CASES = [GateCase(f"B{B}_C{C}_{H}x{W}", B, C, H, W, gate_k(C)) for B, C, H, W in
              [(3, 5, 5, 7),        # k = 17: 105 pixels, a 64-pixel block spans two images, C < 16
               (2, 1, 3, 5),        # k = 17
               (2, 16, 4, 4),       # k = 17
               (2, 33, 5, 7),       # k = 19
               (1, 384, 4, 5)]]     # k = 40


def gate_inputs(c, seed=3):
    r = rng(seed)
    g, x = (f32(r.standard_normal((c.B, c.C, c.H, c.W))) for _ in range(2))
    gate = f32(r.rand(c.B, GATE_CTOT, c.H, c.W) + 0.25)
    return g, x, gate


def gate_ref(g, x, gate, gate_c, k):
    """(gx float32: one product, bit for bit; ggate float64 [B, H, W]; its bound)"""
    gx = f32(g * gate[:, gate_c:gate_c + 1])
    t = g.astype(np.float64) * x.astype(np.float64)
    return gx, t.sum(axis=1), k * U * np.abs(t).sum(axis=1)


# ------------------------------------------------------------------------------------------------ softmax over K (entropy.hip:192-205, backward.hip:146-158)
# expf and logf on the device against float64 exp / log, in units of u |result| (a correctly rounded function: <= 1), rounded up.
# Measured with tools/micro/expf_logf_ulp.hip (the library's compiler flags) on an MI355X:
#   expf over every float32 in [-87, -0] (1118699521 arguments): worst 1.4108 u |result| (at -42.9318275), 0.8567 ulp  -> 2
#   logf over every float32 in [1e-9, 1]  (251039650 arguments): worst 2.7112 u |result| (at 1.50258893e-05), 2.2091 ulp -> 3
EXPF_ROUNDINGS = 2
LOGF_ROUNDINGS = 3
SoftmaxCase = namedtuple("SoftmaxCase", "id B M K H W")
SOFTMAX_CASES = [SoftmaxCase(f"K{K}_{B}x{M}x{H}x{W}", B, M, K, H, W) for K in (1, 3, 5, 8) for B, M, H, W in ((2, 7, 5, 7), (2, 4, 4, 8))]


def softmax_logits(c, seed=4):
    """[B, K*M, H, W] on a grid of 2^-12 below 128 in magnitude: x - max is exact in float32, so expf sees the exact argument.
    Pixel 0 of every map: all entries equal; pixel 1: one entry 100 above the rest (the rest underflow to zero)."""
    r = rng(seed)
    x = np.round(r.standard_normal((c.B, c.K, c.M, c.H * c.W)) * 3 * 4096) / 4096
    x[:, :, :, 0] = 1.25
    x[:, :, :, 1] = np.round(r.rand(c.B, c.K, c.M) * 4096) / 4096 - 50
    x[:, c.K // 2, :, 1] = 50.0
    x[:, :, :, 2] = x[:, :1, :, 2]                                   # equal entries again, random level
    return f32(x.reshape(c.B, c.K * c.M, c.H, c.W))


def softmax_k_fwd_k(K):
    """y_k = e_k / s: expf of an exact argument, the sum of K such terms (expf each, K - 1 additions), one division"""
    return 2 * EXPF_ROUNDINGS + (K - 1) + 1


def softmax_k_ref(x, c):
    """(y float64 [B, K*M, H, W], bound): k u y plus 2^-125 K for entries of exp() below the normal range (flushed or denormal)"""
    v = x.astype(np.float64).reshape(c.B, c.K, c.M, c.H * c.W)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    y = (e / e.sum(axis=1, keepdims=True)).reshape(x.shape)
    return y, softmax_k_fwd_k(c.K) * U * y + c.K * 2.0 ** -125


def softmax_k_bwd_k(K):
    """gx_k = y_k (g_k - dot): K fused multiply-adds for dot, the difference, the product"""
    return K + 2


def softmax_k_bwd_ref(g, y, c):
    """gx_k = y_k (g_k - sum_j g_j y_j) on the float32 y the kernel reads; magnitudes |y_k| (|g_k| + sum_j |g_j y_j|), plus 2^-125 for
    values below the normal range (the y of an underflowed entry: denormal or flushed, where roundings are absolute)"""
    shp = (c.B, c.K, c.M, c.H * c.W)
    g64, y64 = g.astype(np.float64).reshape(shp), y.astype(np.float64).reshape(shp)
    dot = (g64 * y64).sum(axis=1, keepdims=True)
    mag = np.abs(y64) * (np.abs(g64) + np.abs(g64 * y64).sum(axis=1, keepdims=True))
    return (y64 * (g64 - dot)).reshape(g.shape), (softmax_k_bwd_k(c.K) * U * mag + 2.0 ** -125).reshape(g.shape)


# ------------------------------------------------------------------------------------------------ GDN pieces (backward.hip:160-177)
GDN_PIECE_SIZES = (257, n_past(CAP_EW))
BETA_MIN = 1e-6


def gdn_piece_inputs(n, seed=5):
    """x, norm, g, u: every fourth norm within 1 % of beta_min"""
    r = rng(seed)
    x, g, u = (f32(r.standard_normal(n)) for _ in range(3))
    nrm = f32(BETA_MIN + np.abs(r.standard_normal(n)))
    nrm[::4] = f32(BETA_MIN * (1.0 + 0.01 * r.rand(len(nrm[::4]))))
    return x, nrm, g, u


def gdn_pre_ref(x, nrm, g, inverse):
    """s, t in float64 with their bounds.  Roundings: forward s = g / sqrt(n): 2; t = (-0.5 g x) / (n sqrt(n)): the product with x, the
    square root, n * r, the division: 4.  Inverse s = g sqrt(n): 2; t = (0.5 g x) / sqrt(n): 3.  (Products with 0.5 are exact.)"""
    x, nrm, g = (v.astype(np.float64) for v in (x, nrm, g))
    r = np.sqrt(nrm)
    if inverse:
        s, t, ks, kt = g * r, 0.5 * g * x / r, 2, 3
    else:
        s, t, ks, kt = g / r, -0.5 * g * x / (nrm * r), 2, 4
    return s, ks * U * np.abs(s), t, kt * U * np.abs(t)


def gdn_post_ref(x, s, u):
    """dx = fma(2 x, u, s): one rounding; held to 2^-23 |result|"""
    dx = 2.0 * x.astype(np.float64) * u.astype(np.float64) + s.astype(np.float64)
    return dx, 2 * U * np.abs(dx)


# ------------------------------------------------------------------------------------------------ (inverse) GDN backward, C <= 4 (backward.hip:179-277, :986-1006)
GdnSmallCase = namedtuple("GdnSmallCase", "id B C H W inverse sign")


def gdn_small_cases():
    one = [GdnSmallCase(f"one_block_C{C}_{'inv' if inv else 'fwd'}_{'pos' if sg > 0 else 'neg'}", 1, C, 5, 7, inv, sg)
           for C in (1, 2, 3, 4) for inv in (False, True) for sg in (1, -1)]
    big = [GdnSmallCase(f"past_cap_C{C}_{'inv' if inv else 'fwd'}", 2, C, 513, 512, inv, 1 if C % 2 else -1)
           for C in (1, 2, 3, 4) for inv in (False, True)]
    return one, big


def gdn_bounds():
    """the float32 bounds the launcher hands to the kernel (backward.hip:991-992)"""
    return float(np.float32(math.sqrt(BETA_MIN + PED))), float(np.float32(math.sqrt(PED)))


def gdn_small_inputs(c, seed=6):
    """x, g [B, C, H, W]; stored beta [C], gamma [C, C] with entries below their bounds.  g x has the sign `sign` (-1)^channel at every
    pixel, so every parameter sum has a definite sign (the LowerBound rule asks for the sign of the summed gradient) and both signs
    meet entries below the bound."""
    r = rng(seed + 7 * c.C + int(c.inverse))
    shape = (c.B, c.C, c.H, c.W)
    x = f32(r.standard_normal(shape))
    x = f32(np.where(np.abs(x) < 0.05, 0.05, x))
    sg = c.sign * np.where(np.arange(c.C) % 2 == 0, 1.0, -1.0).reshape(1, -1, 1, 1)
    g = f32(np.abs(r.standard_normal(shape)) * np.sign(x) * sg)
    b_bound, g_bound = gdn_bounds()
    beta = f32(1.0 + 0.2 * r.rand(c.C))
    gamma = f32(0.05 + 0.1 * r.rand(c.C, c.C) + 0.3 * np.eye(c.C))
    beta[0] = b_bound * 0.5                                            # below: beta^ = beta_min, norms near beta_min where gamma^ x^2 is small
    gamma[0, 0] = 0.0                                                  # below
    if c.C > 1:
        beta[1] = b_bound                                              # exactly at the bound: passes
        gamma[1, 0] = g_bound * 0.25
        gamma[0, 1] = g_bound
    return x, g, beta, gamma


class _LowerBound(torch.autograd.Function):
    """compressai/ops/bound_ops.py:36-42: max(x, bound); the gradient passes where x >= bound or where it is negative"""
    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.max(x, bound)

    @staticmethod
    def backward(ctx, g):
        x, bound = ctx.saved_tensors
        return ((x >= bound) | (g < 0)).to(g.dtype) * g, None


def gdn64(x, beta, gamma, inverse):
    """the oracle (inverse) GDN in torch float64, differentiable: compressai/layers/gdn.py with parametrizers.py:61-64"""
    b_bound, g_bound = (torch.tensor(v, dtype=torch.float64) for v in gdn_bounds())
    bet = _LowerBound.apply(beta, b_bound) ** 2 - PED
    gam = _LowerBound.apply(gamma, g_bound) ** 2 - PED
    n = torch.einsum("cj,bjhw->bchw", gam, x * x) + bet.reshape(1, -1, 1, 1)
    return x * torch.sqrt(n) if inverse else x / torch.sqrt(n)


def gdn_small_autograd(x, g, beta, gamma, inverse):
    """(gx, g_beta, g_gamma) float64 numpy: autograd of gdn64 at the float32 values"""
    xt, bt, gt = (torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for v in (x, beta, gamma))
    gdn64(xt, bt, gt, inverse).backward(torch.from_numpy(g.astype(np.float64)))
    return xt.grad.numpy(), bt.grad.numpy(), gt.grad.numpy()


def gdn_small_counts(c):
    """k of gx, g_beta, g_gamma.  Roundings, with no contraction beyond the kernel's own fmaf:
    n = beta^ + sum_j gamma^_cj x_j^2: beta^ and gamma^ two each (square, - pedestal), x^2 one, C fused multiply-adds: 3 + C;
    forward t = (-0.5 g x) / (n sqrt(n)): 1.5 (3 + C) for n^1.5, sqrt, n * r, * x, /: 1.5 (3 + C) + 4;  inverse t = (0.5 g x) / sqrt(n): 0.5 (3 + C) + 3;
    gx = fma(2 x, sum_c gamma^_cj t_c, s): gamma^ two, t, C fused multiply-adds, the last one: k_t + C + 3;
    sums: per-thread pixel count P additions, 6 butterfly levels, 2 levels over the four waves, the float64 finish (one unit), its
    rounding to float32, the product with 2 max(p, bound): k_t + P + 11, and one more for x^2 in the gamma sums."""
    kt = math.ceil((0.5 if c.inverse else 1.5) * (3 + c.C)) + (3 if c.inverse else 4)
    P = gdn_small_plan(c.B, c.C, c.H, c.W)["per_thread"]
    return kt + c.C + 3, kt + P + 11, kt + P + 12


def gdn_small_ref(c, x, g, beta, gamma):
    """closed form in float64: (gx, g_beta, g_gamma) and their bounds.  The magnitudes take beta^ and gamma^ as the two terms they are
    (p^2 and the pedestal: gamma^ of an entry at its bound is a difference of equals), and every k is scaled by rho = max n_mag / n,
    the growth of the norm's relative error through that cancellation (1 + O(1e-4) here)."""
    b_bound, g_bound = gdn_bounds()
    x, g, beta, gamma = (v.astype(np.float64) for v in (x, g, beta, gamma))
    bp, gp = np.maximum(beta, b_bound), np.maximum(gamma, g_bound)
    bet, gam, bet_mag, gam_mag = bp * bp - PED, gp * gp - PED, bp * bp + PED, gp * gp + PED
    x2 = x * x
    n = np.einsum("cj,bjhw->bchw", gam, x2) + bet.reshape(1, -1, 1, 1)
    n_mag = np.einsum("cj,bjhw->bchw", gam_mag, x2) + bet_mag.reshape(1, -1, 1, 1)
    rho = float(np.max(n_mag / n))
    r = np.sqrt(n)
    s, t = (g * r, 0.5 * g * x / r) if c.inverse else (g / r, -0.5 * g * x / (n * r))
    gx = s + 2 * x * np.einsum("cj,bchw->bjhw", gam, t)
    gx_mag = np.abs(s) + 2 * np.abs(x) * np.einsum("cj,bchw->bjhw", gam_mag, np.abs(t))
    db, dg = t.sum(axis=(0, 2, 3)), np.einsum("bchw,bjhw->cj", t, x2)
    db_mag, dg_mag = np.abs(t).sum(axis=(0, 2, 3)), np.einsum("bchw,bjhw->cj", np.abs(t), x2)
    gb, gg = 2 * bp * db, 2 * gp * dg
    g_beta = np.where((beta >= b_bound) | (gb < 0), gb, 0.0)
    g_gamma = np.where((gamma >= g_bound) | (gg < 0), gg, 0.0)
    kx, kb, kg = (k * rho for k in gdn_small_counts(c))
    return (gx, g_beta, g_gamma), (kx * U * gx_mag, kb * U * 2 * bp * db_mag, kg * U * 2 * gp * dg_mag), rho


# ------------------------------------------------------------------------------------------------ misc.hip helpers
def lower_bound_inputs(n, bound, seed=8):
    """x around the bound with entries exactly at it, g of both signs"""
    r = rng(seed)
    x = f32(bound + 0.5 * r.standard_normal(n))
    x[::5] = np.float32(bound)
    g = f32(r.standard_normal(n))
    return x, g


def lower_bound_ref32(x, g, bound):
    b = np.float32(bound)
    return f32(np.maximum(x, b)), f32(np.where((x >= b) | (g < 0), g, np.float32(0.0)))


def sse_ref(a, b):
    """sum (a - b)^2 in float64: the difference one rounding (twice in the square), the square one, the float64 sums one unit: k = 4"""
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).sum()), 4 * U * float((d * d).sum())


def sum_log_ref(a):
    """sum log(a): logf, and one unit for the float64 sums"""
    v = np.log(a.astype(np.float64))
    return float(v.sum()), (LOGF_ROUNDINGS + 1) * U * float(np.abs(v).sum())


def likelihood_input(n, seed=9):
    """likelihoods in [1e-9, 1]"""
    r = rng(seed)
    return f32(np.clip(np.exp(-np.abs(r.standard_normal(n)) * 4.0), 1e-9, 1.0))


def rd_bwd_ref32(a, b, sc, gv):
    """misc.hip:152 in float32: (sc (a - b)) g, or (sc / a) g for a likelihood tensor (b None)"""
    sc, gv = np.float32(sc), np.float32(gv)
    return f32(f32(sc / a) * gv) if b is None else f32(f32(sc * f32(a - b)) * gv)


# ------------------------------------------------------------------------------------------------ F16K elementwise / sums (f16k_ops.hip:130-258)
F16kCase = namedtuple("F16kCase", "id B C HW slope k")
F16K_CASES = [F16kCase(f"C{C}_HW{HW}_slope{slope}", 3, C, HW, slope, f16k_sum_plan(3, C, HW)["k"])
              for C in (16, 48) for HW in (5, 33, 216, 32 * 129 + 5) for slope in (0.0, 0.01)]
# k = ceil(ceil(HW / 32) / 128) + 128 + 2: 131 for HW = 5, 33, 216 (at most one pixel per lane), 132 for HW = 4133 (chunks of 130)
F16K_PAST_CAP_N = 8 * n_past(CAP_F16K_ACT)


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    return torch.from_numpy(f32(a)).bfloat16().float().numpy()


def f16k_inputs(B, C, HW, seed=10):
    """g, y [B, C, HW, 1] bf16-exact float32; y = +0 and -0 in the leading pixels of every channel"""
    r = rng(seed)
    g, y = (bf16_round(r.standard_normal((B, C, HW, 1))) for _ in range(2))
    y[:, :, 0] = 0.0
    y[:, :, min(1, HW - 1)] = -0.0
    return g, y


def f16k_act_bwd_ref(g, y, slope):
    """bf16 round-to-nearest-even of the float32 product g * (y > 0 ? 1 : slope), as float32"""
    return bf16_round(f32(g * np.where(y > 0, np.float32(1.0), np.float32(slope))))


def f16k_sum_ref(v, k):
    """per-channel float64 sums of a bf16-exact [B, C, HW, 1] array and their bound"""
    v = v.astype(np.float64)
    return v.sum(axis=(0, 2, 3)), k * U * np.abs(v).sum(axis=(0, 2, 3))


def to_f16k(x):
    """float32 [B, C, H, W] of bf16-exact values -> flat int16 F16K buffer [B][C/16][HW][16]"""
    t = torch.from_numpy(f32(x))
    B, C, H, W = t.shape
    return t.bfloat16().reshape(B, C // 16, 16, H * W).permute(0, 1, 3, 2).contiguous().view(torch.int16).reshape(-1)


def from_f16k(y16, B, C, H, W):
    """flat int16 F16K buffer -> float32 numpy [B, C, H, W]"""
    return y16.cpu().view(torch.bfloat16).reshape(B, C // 16, H * W, 16).permute(0, 1, 3, 2).reshape(B, C, H, W).float().numpy()


# ------------------------------------------------------------------------------------------------ eb_table_split (backward.hip:935-961)
EB_SHAPES = [(3, 1), (3, 3), (3, 3), (3, 3), (1, 3), (3, 1), (3, 1), (3, 1), (3, 1), (1, 1), (3, 1), (3, 1), (3, 1), (3, 1)]     # 58 columns
EB_SPLIT_CHANNELS = (1, 86, 192)


# ------------------------------------------------------------------------------------------------ which case takes which branch
def branch_sides():
    """{branch: set of sides taken by the case tables}: test_cpu_small_kernels.py asks for every side of every branch"""
    s = {}

    def take(name, side):
        s.setdefault(name, set()).add(side)
    for c in CHANNEL_SUM_CASES:
        p = channel_sum_plan(c.B, c.C, c.HW, c.aligned)
        take("channel_sum: B*HW <= 16384 && C >= 128", p["one_block"])
        take("channel_sum: float4 form", p["vec"])
        take("channel_sum: HW % 4", c.HW % 4 == 0)
        take("channel_sum: 16-byte base", c.aligned)
        take("channel_sum: more work items than CS_SPLIT", p["work"] > CS_SPLIT)
        take("channel_sum: ragged last chunk of 4096", p["ragged"])
        take("channel_sum: partial stage-2 block", p["stage2_partial"])
        take("channel_sum: more than one chunk in the one-block form", p["one_block"] and p["chunks"] > 1)
    for c in COPY_CASES + [LANE_LOOP_CASE]:
        p = plane_copy_plan(c.B, c.C, c.H * c.W, c.misalign is None)
        take("plane_copy: vector form", p is not None)
        take("plane_copy: HW % 4", (c.H * c.W) % 4 == 0)
        take("plane_copy: B*C <= 65535", c.B * c.C <= MAX_PLANES)
        take("plane_copy: 16-byte bases", c.misalign is None)
        if p:
            take("plane_copy: lane loop", p["lane_loop"])
            take("plane_copy: fourth vector in flight", p["k3"])
    for c in F16K_CASES:
        p = f16k_sum_plan(c.B, c.C, c.HW)
        take("f16k sums: fewer pixels than F16K_CS_CHUNKS", c.HW < F16K_CS_CHUNKS)
        take("f16k sums: empty chunks", p["empty_chunks"])
        take("f16k_act_bwd_sum: two loads in flight", p["two_load"])
        take("f16k_act_bwd_sum: single-load tail", p["single_tail"])
    one, big = gdn_small_cases()
    for c in one + big:
        p = gdn_small_plan(c.B, c.C, c.H, c.W)
        take("gdn_bwd_small: more than 512 partial rows", p["nb"] > GDN_FINISH_ROWS)
        take("gdn_bwd_small: past the 2048-block cap", p["per_thread"] > 1)
    return s


def cap_cases():
    """(kernel, items, cap) of every case meant to drive a grid-stride loop past its cap"""
    c = [c for c in COPY_CASES if c.id == "scalar_past_cap"][0]
    big = gdn_small_cases()[1][0]
    return [("ew_kernel", EW_SIZES[-1], CAP_EW), ("gdn_bwd_pre / gdn_bwd_post", GDN_PIECE_SIZES[-1], CAP_EW),
            ("copy_view / slice_copy / quantize scalar kernels", c.B * c.C * c.H * c.W, CAP_EW),
            ("lower_bound_fwd / lower_bound_bwd", n_past(CAP_EW), CAP_EW), ("mul_inplace", n_past(CAP_MUL), CAP_MUL),
            ("rd_bwd", n_past(CAP_RD_BWD), CAP_RD_BWD), ("reduce_stage1 (sse, sum_log)", n_past(CAP_RED), CAP_RED),
            ("gdn_bwd_small", big.B * big.H * big.W, CAP_GDN_SMALL), ("f16k_act_bwd (16-byte records)", F16K_PAST_CAP_N // 8, CAP_F16K_ACT)]
