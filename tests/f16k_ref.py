"""A plain torch-on-CPU reference of what the conv_f16k entry points promise (masic_amd/csrc/conv_f16k.hip), and the case record the
conv_f16k tests share (tests/f16k_row_cases.py, tests/test_cpu_f16k_rows.py, tests/test_gpu_f16k_rows.py).  Nothing here needs a GPU
or the compiled library (desc_of apart, which fills the library's descriptor).

Operands are what the kernel sees: bf16 values for the bf16 rows, for the fp8 rows values e4m3 holds exactly.  The convolution and the
bias are float64 (conv64); the epilogue is float32 in the kernel's order (epilogue32; the library is built with -ffp-contract=off):
    v = act(conv + bias);  v *= gate;  v *= act'(mask) ? 1 : slope;  y_pre = bf16(v);  v += res1;  v += res2;  y = bf16(v)
with one round-to-nearest-even to bf16 for an F16K output, which lands in channels out_coff .. of a buffer that keeps its prefill
everywhere else."""
import collections

import torch
import torch.nn.functional as F

from oracle import hsic_oracle as O

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
PREC_BF16, PREC_FP8 = 1, 2
F16K_GDN, F16K_NOSPLIT, F16K_MULTI = 1, 2, 4      # MASIC_F16K_*
PREFILL_BITS = 0x3f00                             # bf16 0.5: what an F16K buffer written through a view holds before the call
PREFILL = 0.5

# One layer: shape, operand precision, activation, the flags its kernel is asked with, and the input channel view (in_ctot, in_coff) or None
Case = collections.namedtuple("Case", "B Cin H W Cout k stride transposed masked prec act flags view")


def case_of(shape, prec=PREC_BF16, act=0, flags=0, view=None):
    return Case(*shape, prec, act, flags, tuple(view) if view else None)


def out_hw(c):
    if c.transposed:
        return (c.H - 1) * c.stride - 2 * (c.k // 2) + c.k + c.stride - 1, (c.W - 1) * c.stride - 2 * (c.k // 2) + c.k + c.stride - 1
    return (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1, (c.W + 2 * (c.k // 2) - c.k) // c.stride + 1


def phase_taps(c):
    """taps of each phase, in the order of the plan line's steps-per-chunk (conv_geom.h: make_geom)"""
    if c.masked:
        return [(c.k // 2) * c.k + c.k // 2]
    if not c.transposed:
        return [c.k * c.k]
    ax = [(c.k - (p + c.k // 2) % c.stride + c.stride - 1) // c.stride for p in range(c.stride)]
    return [a * b for a in ax for b in ax]


def macs(c):
    Ho, Wo = out_hw(c)
    n = c.B * c.Cin * c.Cout
    if c.transposed:
        return n * c.H * c.W * sum(phase_taps(c))
    return n * Ho * Wo * sum(phase_taps(c))


def desc_of(c, out_ctot=None, out_coff=0, gate_ctot=0, gate_c=0, act=None):
    from masic_amd import ops
    in_ctot, in_coff = c.view or (c.Cin, 0)
    return ops._make_conv_desc(c.B, c.Cin, c.H, c.W, c.Cout, c.k, c.k, c.stride, c.k // 2, transposed=bool(c.transposed), masked=bool(c.masked),
                               in_ctot=in_ctot, in_coff=in_coff, out_ctot=c.Cout if out_ctot is None else out_ctot, out_coff=out_coff,
                               act=c.act if act is None else act, gate_ctot=gate_ctot, gate_c=gate_c, prec=c.prec)


# ------------------------------------------------------------------------------------------------ operands
FP8_X = [0.0, 0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -3.0]        # tests/test_gpu_fp8.py: e4m3 holds these exactly
FP8_W = [0.0, 0.0, 0.0, 0.5, -0.5, 1.0, -1.0, 0.25]
FP8_XI = [0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0]
FP8_WI = [0.0, 0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -6.0]


def _pick(values, shape, g):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def inputs(c, seed, integers=False):
    """x (the whole input buffer, in_ctot channels), w, bias: float32 CPU tensors whose x and w are exact in the operand format.

    bf16 rows: x = bf16(2 randn), w = bf16(randn / sqrt(Cin k k)), bias = randn.  integers: all three rounded to whole numbers as
    tests/conv_ref.py draws them (|x| <~ 11, |w| <~ 8, |bias| <~ 40): exact in bf16, and with exact_bound() every partial sum is exact in
    float32 in any order.
    fp8 rows: values from short lists e4m3 holds exactly.  integers: whole numbers, and tap (0, 0) of input channel 0 is 448 for every
    output channel, so that the per-channel weight scale max|w| / 448 is 1 and nothing is rounded anywhere; otherwise that tap is 2
    (scale 1 / 224, as in tests/test_gpu_fp8.py: the dequantising multiply then rounds, ~1e-7)."""
    in_ctot = (c.view or (c.Cin, 0))[0]
    g = torch.Generator().manual_seed(seed)
    wshape = (c.Cin, c.Cout, c.k, c.k) if c.transposed else (c.Cout, c.Cin, c.k, c.k)
    if c.prec == PREC_FP8:
        x = _pick(FP8_XI if integers else FP8_X, (c.B, in_ctot, c.H, c.W), g)
        w = _pick(FP8_WI if integers else FP8_W, wshape, g)
        if c.transposed:
            w[0, :, 0, 0] = 448.0 if integers else 2.0
        else:
            w[:, 0, 0, 0] = 448.0 if integers else 2.0
        bias = torch.round(8.0 * torch.randn(c.Cout, generator=g)) if integers else 0.25 * torch.randn(c.Cout, generator=g)
        return x, w, bias
    x = 2.0 * torch.randn(c.B, in_ctot, c.H, c.W, generator=g)
    w = torch.randn(wshape, generator=g) * (c.Cin * c.k * c.k) ** -0.5
    bias = torch.randn(c.Cout, generator=g)
    if integers:
        return torch.round(x), torch.round(1.5 * (c.Cin * c.k * c.k) ** 0.5 * w), torch.round(8.0 * bias)
    return x.bfloat16().float(), w.bfloat16().float(), bias


def exact_bound(c, x, w, bias):
    """max|x| max|w| Cin k k + max|bias|: below 2^24 every partial sum of the layer, the bias included, is a float32 integer"""
    return float(x.abs().max()) * float(w.abs().max()) * c.Cin * c.k * c.k + float(bias.abs().max())


def to_f16k(x):
    """float32 NCHW (C % 16 == 0, bf16-exact or not) -> the F16K buffer [B][C/16][HW][16] bf16 as flat int16"""
    B, C, H, W = x.shape
    assert C % 16 == 0
    return x.bfloat16().reshape(B, C // 16, 16, H * W).permute(0, 1, 3, 2).contiguous().view(torch.int16).reshape(-1)


def from_f16k(y16, B, C, H, W):
    """flat int16 F16K buffer of C (% 16 == 0) channels -> bf16 NCHW (bits kept: compare .view(torch.int16) for the sign of zero)"""
    return y16.cpu().view(torch.bfloat16).reshape(B, C // 16, H * W, 16).permute(0, 1, 3, 2).reshape(B, C, H, W).contiguous()


def to_f8k(x):
    """float32 NCHW of e4m3-exact values (C % 32 == 0) -> the F8K buffer [B][C/32][HW][32] as flat uint8 (unit scale)"""
    B, C, H, W = x.shape
    assert C % 32 == 0
    q = x.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), x), "not exact in e4m3"
    return q.view(torch.uint8).reshape(B, C // 32, 32, H * W).permute(0, 1, 3, 2).contiguous().reshape(-1)


def from_f8k(y8, B, C, H, W):
    return y8.cpu().view(torch.float8_e4m3fn).float().reshape(B, C // 32, H * W, 32).permute(0, 1, 3, 2).reshape(B, C, H, W).contiguous()


def bits(t):
    """bit pattern of a float32 / bf16 tensor"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------ the layer
def conv64(c, x, w, bias):
    """conv(x[view]) + bias in float64, [B, Cout, Ho, Wo]"""
    in_ctot, in_coff = c.view or (c.Cin, 0)
    assert tuple(x.shape) == (c.B, in_ctot, c.H, c.W)
    xv, w = x[:, in_coff:in_coff + c.Cin].double(), w.double()
    if c.masked:
        w = O.masked_weight(w)
    b = None if bias is None else bias.double()
    if c.transposed:
        return F.conv_transpose2d(xv, w, b, stride=c.stride, padding=c.k // 2, output_padding=c.stride - 1)
    return F.conv2d(xv, w, b, stride=c.stride, padding=c.k // 2)


def act32(v, act):
    """apply_act (common.h) in float32"""
    assert v.dtype == torch.float32
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if act == ACT_LEAKY:
        return torch.where(v >= 0, v, torch.tensor(0.01, dtype=torch.float32) * v)
    return v


def epilogue32(v64, act=0, gate=None, mask=None, slope=0.0, res1=None, res2=None):
    """(value after the residual adds, value before them), float32, from conv + bias in float64 -- the order of the module docstring.
    gate: float32 [B, 1, Ho, Wo]; mask, res1, res2: float32 of bf16 values, [B, Cout, Ho, Wo]."""
    v = act32(v64.float(), act)
    if gate is not None:
        v = v * gate
    if mask is not None:
        v = v * torch.where(mask > 0, torch.tensor(1.0), torch.tensor(float(slope), dtype=torch.float32))
    pre = v
    if res1 is not None:
        v = v + res1
    if res2 is not None:
        v = v + res2
    return v, pre


def in_view(y, ctot, coff, prefill=PREFILL):
    """y as channels coff .. of a buffer of ctot channels that holds `prefill` elsewhere"""
    out = torch.full((y.shape[0], ctot) + tuple(y.shape[2:]), prefill, dtype=y.dtype)
    out[:, coff:coff + y.shape[1]] = y
    return out


def gdn64(v64, beta, gamma, inverse):
    """the oracle's (inverse) GDN, float64, of stored (reparametrised) float32 parameters"""
    return O.gdn(v64, beta.double(), gamma.double(), inverse=inverse)


def one_product_share(v64, beta, gamma, inverse):
    """q = max_i (S_i / n_i) |y_i| / max|y| with n = beta^ + S, S_i = sum_j gamma^_ij v_j^2, y = the (inverse) GDN of v.

    What the one-product fused GDN may cost: it rounds gamma^ and v^2 to bf16 (relative error <= 2^-8 each), so every term of S -- all
    are positive -- is off by <= 2^-7 of itself, n by <= 2^-7 S, and y = v n^(-+1/2) by <= 2^-8 (S / n) |y|: at most 2^-8 q of the peak.
    The project's gate for that form, 2^-9 of the peak, therefore follows for a correct kernel where q <= 1/2 and cannot be promised
    where the norm is mostly S (q -> 1).  The tests hold the form to one_product_bound(q) on their operands as drawn, and to the gate
    itself on the same operands times the power of two at which q <= 0.45."""
    bh, gh = O.nonneg_reparam(beta.double(), 1e-6), O.nonneg_reparam(gamma.double(), 0.0)
    S = torch.einsum("ij,bjhw->bihw", gh, v64 * v64)
    n = S + bh.view(1, -1, 1, 1)
    y = v64 * (n.sqrt() if inverse else n.rsqrt())
    return float(((S / n) * y.abs()).max() / y.abs().max())


ONE_PRODUCT_MARGIN = 2.0 ** -14


def one_product_bound(q):
    """what the one-product GDN may be off by, of the peak: 2^-8 q (one_product_share) + 2^-14 -- the margin covers the second-order
    terms of two 2^-8 roundings under a square root (2^-16 + 3/8 (2^-7)^2 < 2^-15), the float32 rounding of v^2, of the accumulation and of the product (a few 2^-24) and the 1 ulp
    of v_rsq_f32 / v_sqrt_f32 (2^-23), and is 1.6 % of the smallest bound it is added to (q = 0.45)"""
    return 2.0 ** -8 * q + ONE_PRODUCT_MARGIN


def one_product_scale(v64, beta, gamma, inverse, top=0.45):
    """the largest power of two s <= 1 with one_product_share(s v) <= top (the convolution is linear: s scales x and the bias)"""
    s = 1.0
    while one_product_share(s * v64, beta, gamma, inverse) > top:
        s *= 0.5
        assert s >= 2.0 ** -20
    return s


def multi_ref(v64, gate=None):
    """the four layouts of masic_conv_f16k_multi_fwd from v = conv + bias: y32 = v, round32 = rintf(v) (ties to even, -0 kept),
    round16 = bf16(rintf(v) * gate), abs16 = bf16(|v|)"""
    v = v64.float()
    r = torch.round(v)
    rg = r if gate is None else r * gate
    return {"y32": v, "round32": r, "round16": rg.bfloat16(), "abs16": v.abs().bfloat16()}


def few_ref(v64, act, res32, C):
    """masic_conv_f16k_few_fwd: channels 0 .. C-1 of act(conv + bias) + res32, float32"""
    v = act32(v64.float(), act)[:, :C]
    return v if res32 is None else v + res32


def d2s_weight(w, bias):
    """ConvTranspose2d(Cin -> C, k5, s2, p2, op1) weight [Cin, C, 5, 5] -> ([32, Cin, 3, 3], [32]) of the equivalent 3x3 convolution to
    channels 4c + 2ph + pw (include/masic_hip.h: masic_deconv_s2_as_conv_weight), written independently of masic_amd/ops.py"""
    Cin, C = w.shape[:2]
    wo, bo = torch.zeros(32, Cin, 3, 3), torch.zeros(32)
    for c in range(C):
        for ph in range(2):
            for pw in range(2):
                row = 4 * c + 2 * ph + pw
                bo[row] = bias[c]
                for u in range(3):
                    for v in range(3):
                        kh, kw = ph + 2 * (2 - u), pw + 2 * (2 - v)
                        if kh <= 4 and kw <= 4:
                            wo[row, :, u, v] = w[:, c, kh, kw]
    return wo, bo


def fp8_out_ref(v32, out_scale):
    """store_f8k_tile: fp8(clamp(v * (1 / out_scale), +-448)), round to nearest even, decoded (times out_scale)"""
    inv = torch.tensor(1.0 / out_scale, dtype=torch.float32)
    return (v32 * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * out_scale


# ------------------------------------------------------------------------------------------------ the fused GDN backward
def gdn_bwd_rule(d, p, bound):
    """the parametrizer's backward of gdn_bwd_reduce_kernel: g = 2 max(p, bound) d, passed where p >= bound or the step would raise p"""
    g = d * 2 * torch.maximum(p, bound)
    return torch.where((p >= bound) | (g < 0), g, torch.zeros_like(g))


def gdn_bwd_emulation(xf, gf, beta, gamma, inverse, beta_min=1e-6):
    """masic_gdn_bwd_fused with the kernel's roundings, everything else float64: gamma^, x^2 and t are rounded to bf16 where they enter
    a contraction.  xf, gf: [128, pixels] (any subset of the pixels: every pixel is independent but for the sums over them).  Returns
    float64 (dx [128, pixels], d beta [128], d gamma [128, 128], channel sums of dx [128]); the parameter gradients have passed the
    parametrizer's rule."""
    rnd = lambda t: t.float().bfloat16().double()
    ped = torch.tensor(2.0 ** -36, dtype=torch.float32)
    b_bound = torch.tensor((beta_min + 2.0 ** -36) ** 0.5, dtype=torch.float32)
    g_bound = torch.tensor((2.0 ** -36) ** 0.5, dtype=torch.float32)
    bh = (torch.maximum(beta, b_bound) ** 2 - ped).double()
    gh = rnd(torch.maximum(gamma, g_bound) ** 2 - ped)
    xf, gf = xf.double(), gf.double()
    x2 = rnd(xf * xf)
    n = bh[:, None] + gh @ x2
    if inverse:
        sv, tv = gf * n.sqrt(), 0.5 * gf * xf / n.sqrt()
    else:
        sv, tv = gf / n.sqrt(), -0.5 * gf * xf / (n * n.sqrt())
    tb = rnd(tv)
    dx = sv + 2.0 * xf * (gh.t() @ tb)
    return dx, gdn_bwd_rule(tb.sum(1), beta.double(), b_bound.double()), gdn_bwd_rule(tb @ x2.t(), gamma.double(), g_bound.double()), dx.sum(1)


def gdn_bwd_autograd64(xf, gf, beta, gamma, inverse):
    """(dx, d beta, d gamma) of the oracle's (inverse) GDN by float64 autograd; xf, gf: [128, pixels]"""
    xr = xf.double().reshape(1, 128, 1, -1).clone().requires_grad_(True)
    br, gr = beta.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True)
    O.gdn(xr, br, gr, inverse=inverse).backward(gf.double().reshape(1, 128, 1, -1))
    return xr.grad.reshape(128, -1), br.grad, gr.grad
