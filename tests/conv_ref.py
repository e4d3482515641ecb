"""A plain torch-on-CPU reference of what masic_conv2d_fwd_ex / masic_conv2d_f16k_out_fwd promise for a descriptor (float64 unless
asked otherwise), and the case record the NCHW convolution tests share (tests/conv_row_cases.py, tests/test_cpu_conv_rows.py,
tests/test_gpu_conv_rows.py).  Nothing here needs a GPU or the compiled library."""
import collections

import torch
import torch.nn.functional as F

from oracle import hsic_oracle as O

GATE, RES1, RES2, F16K_OUT = 1, 2, 4, 8          # MASIC_CONV_*
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SOFTMAX_C = 0, 1, 2, 3
INOP_NONE, INOP_ABS, INOP_ROUND = 0, 1, 2
PREC_F32, PREC_BF16 = 0, 1
PREFILL = 0.5                                    # what the output buffer holds before the call

# One call: the layer, its form (MASIC_CONV_* flags), its activation and its channel views (in_ctot, in_coff, out_ctot, out_coff) or None
# for whole buffers.  A gate is channel 1 of a 2-channel tensor, as in tests/golden/make_conv_fwd_digest.py.
Case = collections.namedtuple("Case", "B Cin H W Cout k stride transposed masked prec in_op form act view")


def case_of(shape, form=0, act=0, view=None):
    return Case(*shape, form, act, tuple(view) if view else None)


def views(c):
    return c.view or (c.Cin, 0, c.Cout, 0)


def out_hw(c):
    if c.transposed:
        return (c.H - 1) * c.stride - 2 * (c.k // 2) + c.k + c.stride - 1, (c.W - 1) * c.stride - 2 * (c.k // 2) + c.k + c.stride - 1
    return (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1, (c.W + 2 * (c.k // 2) - c.k) // c.stride + 1


def desc_of(c):
    from masic_amd import ops
    in_ctot, in_coff, out_ctot, out_coff = views(c)
    return ops._make_conv_desc(c.B, c.Cin, c.H, c.W, c.Cout, c.k, c.k, c.stride, c.k // 2, transposed=bool(c.transposed), masked=bool(c.masked),
                               in_ctot=in_ctot, in_coff=in_coff, out_ctot=out_ctot, out_coff=out_coff, in_op=c.in_op, act=c.act,
                               gate_ctot=2 if c.form & GATE else 0, gate_c=1 if c.form & GATE else 0, prec=c.prec)


def inputs(c, seed, integers=False):
    """x (the whole input buffer), w, bias, gate, res1, res2 -- float32 CPU tensors from one generator, drawn as
    tests/golden/make_conv_fwd_digest.py draws them (seed 4000 + i there: the digest's own inputs).

    integers: x, w and the bias rounded to whole numbers (|x| <~ 10, |w| <~ 6), for the large F16K-output cases.  Every product and
    every partial sum is then a whole number far below 2^24, so float32 accumulation in any order is exact and the bf16 rounding of the
    result -- ties included: the odd numbers above 256 -- is the one thing left to differ.  With real-valued operands a result that
    float32 noise carries across a rounding boundary differs from the rounded reference by a whole bf16 ulp, 2^-7 of the peak in the
    peak's binade: among 10^7 outputs that happens to a correct kernel (and to float32 on the CPU: 2.8e-3 measured)."""
    in_ctot = views(c)[0]
    Ho, Wo = out_hw(c)
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(c.B, in_ctot, c.H, c.W, generator=g)
    w = torch.randn((c.Cin, c.Cout, c.k, c.k) if c.transposed else (c.Cout, c.Cin, c.k, c.k), generator=g) * (c.Cin * c.k * c.k) ** -0.5
    bias = torch.randn(c.Cout, generator=g)
    if integers:
        x, w, bias = torch.round(x), torch.round(1.5 * (c.Cin * c.k * c.k) ** 0.5 * w), torch.round(8.0 * bias)
    gate, res1, res2 = (torch.rand(shape, generator=g) if c.form & bit else None
                        for bit, shape in ((GATE, (c.B, 2, Ho, Wo)), (RES1, (c.B, c.Cout, Ho, Wo)), (RES2, (c.B, c.Cout, Ho, Wo))))
    return x, w, bias, gate, res1, res2


def conv_ref(c, x, w, bias, gate=None, res1=None, res2=None, dtype=torch.float64, prefill=PREFILL):
    """The whole output buffer [B, out_ctot, Ho, Wo] of the call `c` describes, in `dtype` arithmetic.

    In the order of the kernels: the input channel view; in_op; for a bf16 descriptor the rounding of both operands to bf16 (after in_op,
    as tests/test_gpu_ops.py::test_conv_variants_bf16_operands has it); the masked weight; the convolution and the bias; the activation;
    then  act(conv + bias) * gate + res1 + res2  -- masic_amd/csrc/conv.hip, igemm_epilogue: `apply_act(acc + bias, act) * gv + rv` with
    rv = res1 + res2; conv_direct_f32 (softmax over the channels first, then `acc * gv`, `+= res1`, `+= res2`) and conv5s1_small
    (`apply_act(acc + bias) * gv`, `+= res1`) agree: the gate multiplies the activated value and never the residuals.  The result lands
    in channels out_coff .. out_coff + Cout of a buffer that holds `prefill` everywhere else.  With F16K_OUT in c.form the result is
    rounded to bf16 (igemm_epilogue_f16k; that form has no gate and no residual)."""
    in_ctot, in_coff, out_ctot, out_coff = views(c)
    assert tuple(x.shape) == (c.B, in_ctot, c.H, c.W)
    xv = x[:, in_coff:in_coff + c.Cin]
    if c.in_op == INOP_ABS:
        xv = xv.abs()
    elif c.in_op == INOP_ROUND:
        xv = torch.round(xv)                     # half to even, as rintf
    if c.prec == PREC_BF16:
        xv, w = xv.bfloat16(), w.bfloat16()
    xv, w = xv.to(dtype), w.to(dtype)
    if c.masked:
        w = O.masked_weight(w)
    b = None if bias is None else bias.to(dtype)
    if c.transposed:
        y = F.conv_transpose2d(xv, w, b, stride=c.stride, padding=c.k // 2, output_padding=c.stride - 1)
    else:
        y = F.conv2d(xv, w, b, stride=c.stride, padding=c.k // 2)
    if c.act == ACT_RELU:
        y = F.relu(y)
    elif c.act == ACT_LEAKY:
        y = F.leaky_relu(y, 0.01)
    elif c.act == ACT_SOFTMAX_C:
        y = F.softmax(y, dim=1)
    if gate is not None:
        y = y * gate[:, 1:2].to(dtype)
    if res1 is not None:
        y = y + res1.to(dtype)
    if res2 is not None:
        y = y + res2.to(dtype)
    if c.form & F16K_OUT:
        assert gate is None and res1 is None and res2 is None
        y = y.bfloat16().to(dtype)
    out = torch.full((c.B, out_ctot) + tuple(y.shape[2:]), prefill, dtype=dtype)
    out[:, out_coff:out_coff + c.Cout] = y
    return out


def gate_of(c):
    """the relative error (tests/util.py: of the reference's peak) a device result may have: the project's gates"""
    from tests.util import RTOL
    if c.form & F16K_OUT:
        return 2.0 ** -8
    return 2e-5 if c.prec == PREC_BF16 else RTOL
