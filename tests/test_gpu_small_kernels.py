"""The kernels the training graph runs between its contractions -- the non-contraction kernels of backward.hip, the helpers of misc.hip,
quantize / symbols / softmax_k of entropy.hip, the vector plane copy of common.h and the elementwise / sum kernels of f16k_ops.hip --
each called directly through masic_amd.ops and held to a float64 reference of the one operation, at the shapes of
tests/small_kernel_cases.py: every launcher branch on both sides, every grid-stride loop past its cap with a ragged last trip.

Operations with one rounding or none must equal the float32 evaluation bit for bit (the sign of zero included); everything else stays
within k 2^-24 (sum of the magnitudes of its terms), k counted from the case's shape (small_kernel_cases.py says how, per kernel).
tests/test_cpu_small_kernels.py holds the cases to their branches and the references to float64 autograd without a GPU.

Every test prints its worst error / bound.  On an MI355X the worst seen per kernel: channel_sum 0.065, gate_bwd ggate 0.101,
softmax_k 0.462, softmax_k_bwd 0.414, gdn_bwd_pre 0.977 (s: two roundings, both met at their worst among 2 M elements) / 0.939 (t),
gdn_bwd_post 0.500, gdn_bwd_small 0.358 (gx) / 0.116 (g_beta) / 0.126 (g_gamma), sse 0.045, sum_log 0.247, f16k_act_bwd_sum 0.002,
f16k_channel_sum 0.0002, AXPY 0.978, REPARAM 0.998, RECIP_SCALE 0.999 (a correctly rounded division just above a power of two).
expf / logf on the device (tools/micro/expf_logf_ulp.hip, every float32 of the range): expf 0.857 ulp on [-87, 0], logf 2.209 ulp on
[1e-9, 1]; in units of 2^-24 |result| 1.41 and 2.71, hence EXPF_ROUNDINGS = 2 and LOGF_ROUNDINGS = 3 in small_kernel_cases.py."""
import numpy as np
import pytest
import torch

from tests import small_kernel_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE, BIG = T.gdn_small_cases()


def _d(a, misalign=False):
    """numpy -> device; misalign: the first element 4 bytes past a 16-byte line"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if not misalign:
        assert t.data_ptr() % 16 == 0
        return t
    m = T.misaligned(t.numel(), DEV)
    m.copy_(t.reshape(-1))
    return m.view(t.shape)


def _h(t):
    return t.detach().cpu().numpy()


def _within(kernel, case, got, ref, bound):
    r = T.worst_ratio(_h(got) if isinstance(got, torch.Tensor) else got, ref, bound)
    print(f"small_kernels | {kernel} | {case} | worst error / bound {r:.4f}")
    assert r <= 1.0, f"{kernel} {case}: error {r:.3f} x its bound"
    return r


def _exact(kernel, case, got, want):
    got = _h(got) if isinstance(got, torch.Tensor) else got
    same = T.bit_equal(got, want)
    if not same:
        bad = np.flatnonzero(T.bits(got).reshape(-1) != T.bits(want).reshape(-1))
        print(f"small_kernels | {kernel} | {case} | {bad.size} of {got.size} elements differ, first at {bad[:8].tolist()}")
    assert got.shape == want.shape and same, f"{kernel} {case}: not bit-equal to the float32 evaluation"


# ------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("op", T.EW_OPS)
def test_elementwise(op):
    from masic_amd import ops
    code = T.EW_OPS.index(op)
    assert code == getattr(ops, "EW_" + op)
    variants = [dict(act=a) for a in (T.ACT_NONE, T.ACT_RELU, T.ACT_LEAKY)] if op == "ACT_BWD" else [dict(with_b=w) for w in (True, False)] if op == "AXPY" else [{}]
    worst = 0.0
    for n in T.EW_SIZES:
        for kw in variants:
            a, b, s0, s1 = T.ew_inputs(op, n, 100 + code, **kw)
            y = ops.elementwise(code, _d(a), None if b is None else _d(b), s0, s1)
            if op in T.EW_EXACT:
                _exact(op, f"n={n} {kw}", y, T.ew_ref32(op, a, b, s0, s1))
            else:
                ref, bound = T.ew_ref64(op, a, b, s0, s1)
                worst = max(worst, T.worst_ratio(_h(y), ref, bound))
                assert worst <= 1.0, f"{op} n={n} {kw}: error {worst:.3f} x its bound"
    print(f"small_kernels | elementwise {op} | n in {T.EW_SIZES} | " + ("bit-equal" if op in T.EW_EXACT else f"worst error / bound {worst:.4f}"))


# ------------------------------------------------------------------------------------------------ channel_sum
@pytest.mark.parametrize("c", T.CHANNEL_SUM_CASES, ids=[c.id for c in T.CHANNEL_SUM_CASES])
def test_channel_sum(c):
    from masic_amd import ops
    x = T.channel_sum_input(c)
    xd = _d(x, misalign=not c.aligned)
    assert (xd.data_ptr() % 16 == 0) == c.aligned
    ref, bound = T.channel_sum_ref(x, c)
    _within("channel_sum", f"{c.id} k={c.k}", ops.channel_sum(xd, C=c.C, coff=c.coff), ref, bound)


# ------------------------------------------------------------------------------------------------ copy_view / slice_copy / quantize
def _out_buffer(c):
    shape = (c.B, c.ctot, c.H, c.W)
    if c.misalign == "y":
        return T.misaligned(int(np.prod(shape)), DEV).fill_(T.SENTINEL).view(shape)
    return torch.full(shape, T.SENTINEL, dtype=torch.float32, device=DEV)


def _check_view(kernel, case, c, out, want):
    out = _h(out)
    _exact(kernel, case, out[:, c.coff:c.coff + c.C], want)
    rest = np.delete(out, np.s_[c.coff:c.coff + c.C], axis=1)
    assert np.all(rest == np.float32(T.SENTINEL)), f"{kernel} {case}: wrote outside its channel view"


@pytest.mark.parametrize("c", T.COPY_CASES, ids=[c.id for c in T.COPY_CASES])
def test_quantize_modes_gates_and_views(c):
    from masic_amd import ops
    x, noise, gate = T.copy_inputs(c)
    xd, nd, gd = _d(x, misalign=c.misalign == "x"), _d(noise), _d(gate)
    assert (T.plane_copy_plan(c.B, c.C, c.H * c.W, xd.data_ptr() % 16 == 0 and c.misalign != "y") is not None) == (c.path == "vector")
    for mode in ("dequantize", "noise", "copy"):
        for gate_c in (None, 0, 2):
            out = _out_buffer(c)
            assert (out.data_ptr() % 16 != 0) == (c.misalign == "y")
            ops.quantize(xd, mode, noise=nd if mode == "noise" else None, out=out, out_coff=c.coff, gate=None if gate_c is None else gd, gate_c=gate_c or 0)
            want = T.quantize_ref32(x, mode, noise, None if gate_c is None else gate, gate_c or 0)
            _check_view("quantize", f"{c.id} {mode} gate_c={gate_c}", c, out, want)
    print(f"small_kernels | quantize | {c.id} ({c.path} path) | 3 modes x 3 gates bit-equal, the view's surroundings untouched")


@pytest.mark.parametrize("c", T.COPY_CASES, ids=[c.id for c in T.COPY_CASES])
def test_copy_view_and_slice_copy(c):
    from masic_amd import ops
    x, _, _ = T.copy_inputs(c)
    out = _out_buffer(c)
    ops.copy_view(_d(x, misalign=c.misalign == "x"), out, c.coff)
    _check_view("copy_view", c.id, c, out, x)
    # the slice back out of a wider buffer whose other channels hold other values
    wide = T.f32(T.rng(21).standard_normal((c.B, c.ctot, c.H, c.W)) * 1e3)
    wide[:, c.coff:c.coff + c.C] = x
    y = ops.slice_copy(_d(wide, misalign=c.misalign is not None), c.coff, c.C)
    _exact("slice_copy", c.id, y, x)
    print(f"small_kernels | copy_view, slice_copy | {c.id} ({c.path} path) | bit-equal")


def test_plane_copy_lane_loop():
    """4096 planes x 8196 pixels: two workgroups per plane, and the vector past the first pass of four belongs to the lane loop.  Inputs are
    built on the device from an integer pattern and compared there with torch's own indexing."""
    from masic_amd import ops
    c = T.LANE_LOOP_CASE
    p = T.plane_copy_plan(c.B, c.C, c.H * c.W)
    assert p["lane_loop"] and p["passes"] == 2
    shape, n = (c.B, c.C, c.H, c.W), c.B * c.C * c.H * c.W
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    x = ((i * 2654435761) % 4001 - 2000).float().mul_(0.125).view(shape)
    noise = ((i * 40503) % 1021).float().div_(1024).sub_(0.5).view(shape)
    del i
    gate = _d(T.f32(T.rng(22).rand(c.B, T.GATE_CTOT, c.H, c.W) + 0.25))
    tail = 4 * 4 * 256 * p["gx"]                         # first pixel of the second pass

    def check(kernel, got, want):
        assert torch.equal(got.view(c.B * c.C, -1)[:, tail:], want.view(c.B * c.C, -1)[:, tail:]), f"{kernel}: the lane loop's second pass"
        assert torch.equal(got, want), kernel
    out = torch.full(shape, T.SENTINEL, dtype=torch.float32, device=DEV)
    check("copy_view", ops.copy_view(x, out, 0), x)
    check("slice_copy", ops.slice_copy(x, 0, c.C), x)
    out.fill_(T.SENTINEL)
    check("quantize copy", ops.quantize(x, "copy", out=out), x)
    out.fill_(T.SENTINEL)
    want = (x + noise) * gate[:, 2:3]
    check("quantize noise + gate", ops.quantize(x, "noise", noise=noise, out=out, gate=gate, gate_c=2), want)
    out.fill_(T.SENTINEL)
    check("quantize dequantize + gate", ops.quantize(x, "dequantize", out=out, gate=gate, gate_c=0), torch.round(x) * gate[:, 0:1])
    print(f"small_kernels | masic_plane_copy lane loop | {p} | equal to torch indexing on the device")


def test_rounding_ties_and_symbols():
    from masic_amd import ops
    e = T.rounding_edges()
    for shape in ((1, 1, 6, 6), (1, 1, 5, 7), (2, 3, 2, 4)):        # vector, scalar, vector with planes
        x = T.f32(np.resize(e, int(np.prod(shape))).reshape(shape))
        _exact("quantize dequantize", f"ties {shape}", ops.quantize(_d(x), "dequantize"), np.rint(x))
    x = T.symbols_input()
    for med in (T.SYMBOLS_MEDIANS, None):
        s = ops.symbols(_d(x), None if med is None else _d(med))
        assert s.dtype == torch.int32 and np.array_equal(_h(s), T.symbols_ref(x, med)), f"symbols, medians {med}"
    c = [c for c in T.COPY_CASES if c.id == "scalar_past_cap"][0]
    x, _, _ = T.copy_inputs(c)
    med = T.f32([0.0, 0.5, -0.25])
    assert np.array_equal(_h(ops.symbols(_d(x), _d(med))), T.symbols_ref(x, med)), "symbols past the grid cap"
    print("small_kernels | quantize ties, symbols | +-(k + 0.5) up to 2^23, C=5 HW=7 and past the cap | equal")


# ------------------------------------------------------------------------------------------------ gate_bwd
@pytest.mark.parametrize("c", T.GATE_CASES, ids=[c.id for c in T.GATE_CASES])
def test_gate_bwd(c):
    from masic_amd import ops
    g, x, gate = T.gate_inputs(c)
    for gate_c in (0, 2):
        gx, ggate = ops.gate_bwd(_d(g), _d(x), _d(gate), gate_c)
        want_gx, ref, bound = T.gate_ref(g, x, gate, gate_c, c.k)
        _exact("gate_bwd gx", f"{c.id} gate_c={gate_c}", gx, want_gx)
        gg = _h(ggate)
        assert gg.shape == gate.shape and np.all(gg[:, [k for k in range(T.GATE_CTOT) if k != gate_c]] == 0), "the other gate channels are zero"
        _within("gate_bwd ggate", f"{c.id} gate_c={gate_c} k={c.k}", gg[:, gate_c], ref, bound)


# ------------------------------------------------------------------------------------------------ softmax over K
@pytest.mark.parametrize("c", T.SOFTMAX_CASES, ids=[c.id for c in T.SOFTMAX_CASES])
def test_softmax_k_and_backward(c):
    """expf counts as T.EXPF_ROUNDINGS = 2 roundings: the device function's worst error over every float32 argument in [-87, 0], measured by
    tools/micro/expf_logf_ulp.hip on an MI355X, is 1.4108 x 2^-24 |result| (0.8567 ulp, at -42.9318275)."""
    from masic_amd import ops
    x = T.softmax_logits(c)
    ref, bound = T.softmax_k_ref(x, c)
    y = ops.softmax_k(_d(x), c.K)
    _within("softmax_k", f"{c.id} k={T.softmax_k_fwd_k(c.K)}", y, ref, bound)
    y32 = _h(y)
    if c.K == 1:
        assert np.all(y32 == 1.0)
    g = T.f32(T.rng(31).standard_normal(x.shape))
    gx = ops.softmax_k_bwd(_d(g), y, c.K)
    ref, bound = T.softmax_k_bwd_ref(g, y32, c)
    if c.K == 1:
        assert np.all(_h(gx) == 0), "K = 1: the backward is exactly zero"
    _within("softmax_k_bwd", f"{c.id} k={T.softmax_k_bwd_k(c.K)}", gx, ref, bound)


# ------------------------------------------------------------------------------------------------ GDN pieces
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("n", T.GDN_PIECE_SIZES)
def test_gdn_bwd_pre_and_post(n, inverse):
    from masic_amd import ops
    x, nrm, g, u = T.gdn_piece_inputs(n)
    s, t = ops.gdn_bwd_pre(_d(x), _d(nrm), _d(g), inverse)
    rs, bs, rt, bt = T.gdn_pre_ref(x, nrm, g, inverse)
    _within("gdn_bwd_pre s", f"n={n} inverse={inverse}", s, rs, bs)
    _within("gdn_bwd_pre t", f"n={n} inverse={inverse}", t, rt, bt)
    s32 = _h(s)
    dx = ops.gdn_bwd_post(_d(x), s, _d(u))
    ref, bound = T.gdn_post_ref(x, s32, u)
    _within("gdn_bwd_post", f"n={n}", dx, ref, bound)


# ------------------------------------------------------------------------------------------------ (inverse) GDN backward, C <= 4
@pytest.mark.parametrize("c", ONE + BIG, ids=[c.id for c in ONE + BIG])
def test_gdn_bwd_small(c):
    from masic_amd import ops
    x, g, beta, gamma = T.gdn_small_inputs(c)
    gx, gb, gg = ops.gdn_bwd_small(_d(x), _d(g), _d(beta), _d(gamma), inverse=c.inverse, beta_min=T.BETA_MIN)
    ax, ab, ag = T.gdn_small_autograd(x, g, beta, gamma, c.inverse)                 # the reference: float64 autograd of the oracle GDN
    (rx, rb, rg), (bx, bb, bg), rho = T.gdn_small_ref(c, x, g, beta, gamma)         # its closed form, for the magnitudes
    assert T.worst_ratio(rx, ax, bx) < 1e-6 and T.worst_ratio(rb, ab, bb) < 1e-6 and T.worst_ratio(rg, ag, bg) < 1e-6
    kx, kb, kg = T.gdn_small_counts(c)
    _within("gdn_bwd_small gx", f"{c.id} k={kx}", gx, ax, bx)
    _within("gdn_bwd_small g_beta", f"{c.id} k={kb}", gb, ab, bb)
    _within("gdn_bwd_small g_gamma", f"{c.id} k={kg}", gg, ag, bg)
    # the LowerBound rule: what autograd stops is exactly zero
    assert np.all(_h(gb)[ab == 0] == 0) and np.all(_h(gg)[ag == 0] == 0)


# ------------------------------------------------------------------------------------------------ misc.hip
def test_mul_inplace_and_lower_bound_past_their_caps():
    from masic_amd import ops
    n = T.n_past(T.CAP_MUL)
    a, m = T.f32(T.rng(41).standard_normal(n)), T.f32(T.rng(42).rand(n) < 0.5)
    _exact("mul_inplace", f"n={n}", ops.mul_inplace(_d(a), _d(m)), T.f32(a * m))
    n, bound = T.n_past(T.CAP_EW), 0.11
    x, g = T.lower_bound_inputs(n, bound)
    assert np.any(x == np.float32(bound))
    y, gx = T.lower_bound_ref32(x, g, bound)
    _exact("lower_bound", f"n={n}", ops.lower_bound(_d(x), bound), y)
    _exact("lower_bound_bwd", f"n={n}", ops.lower_bound_bwd(_d(x), _d(g), bound), gx)
    print("small_kernels | mul_inplace, lower_bound, lower_bound_bwd | past their caps | bit-equal")


def test_sse_sum_log_and_rd_loss_bwd_past_their_caps():
    """logf counts as T.LOGF_ROUNDINGS = 3 roundings: its worst error over every float32 in [1e-9, 1], measured by
    tools/micro/expf_logf_ulp.hip on an MI355X, is 2.7112 x 2^-24 |result| (2.2091 ulp, at 1.50258893e-05)."""
    from masic_amd import ops
    for n in (257, T.n_past(T.CAP_RED)):
        a, b = T.f32(T.rng(43).standard_normal(n)), T.f32(T.rng(44).standard_normal(n))
        ref, bound = T.sse_ref(a, b)
        got = ops.sse(_d(a), _d(b))
        assert got.dtype == torch.float64
        _within("sse", f"n={n}", got.reshape(1), [ref], [bound])
        lik = T.likelihood_input(n)
        ref, bound = T.sum_log_ref(lik)
        _within("sum_log", f"n={n}", ops.sum_log(_d(lik)).reshape(1), [ref], [bound])
    n = T.n_past(T.CAP_RD_BWD)
    pics = [T.f32(T.rng(45 + k).rand(n)) for k in range(4)]
    liks = [T.likelihood_input(300, 50), T.likelihood_input(n + 5, 51)]
    s_pic, s_lik, gv = float(np.float32(2.0 / n)), float(np.float32(-1.0 / (np.log(2.0) * 4096))), np.float32(1.7)
    g1, g2, gl = ops.rd_loss_bwd(*[_d(p) for p in pics], [_d(l) for l in liks], s_pic, s_lik, _d(np.array([gv], np.float32)))
    _exact("rd_loss_bwd g_x1", f"n={n}", g1, T.rd_bwd_ref32(pics[0], pics[1], s_pic, gv))
    _exact("rd_loss_bwd g_x2", f"n={n}", g2, T.rd_bwd_ref32(pics[2], pics[3], s_pic, gv))
    for k, l in enumerate(liks):
        _exact("rd_loss_bwd g_lik", f"tensor {k} n={l.size}", gl[k], T.rd_bwd_ref32(l, None, s_lik, gv))
    print("small_kernels | rd_loss_bwd | past its cap, likelihood tensors of other sizes | bit-equal")


# ------------------------------------------------------------------------------------------------ F16K
@pytest.mark.parametrize("c", T.F16K_CASES, ids=[c.id for c in T.F16K_CASES])
def test_f16k_act_bwd_and_sums(c):
    from masic_amd import ops
    g, y = T.f16k_inputs(c.B, c.C, c.HW)
    g16, y16 = T.to_f16k(g).to(DEV), T.to_f16k(y).to(DEV)
    want = T.f16k_act_bwd_ref(g, y, c.slope)
    out = ops.f16k_act_bwd(g16, y16, c.slope)
    _exact("f16k_act_bwd", c.id, T.from_f16k(out, c.B, c.C, c.HW, 1), want)
    out2, sums = ops.f16k_act_bwd_sum(g16, y16, c.slope, c.B, c.C, c.HW)
    assert torch.equal(out2, out), "f16k_act_bwd_sum's output is f16k_act_bwd's"
    ref, bound = T.f16k_sum_ref(want, c.k)                            # the sums of the stored bf16 output
    _within("f16k_act_bwd_sum", f"{c.id} k={c.k}", sums, ref, bound)
    ref, bound = T.f16k_sum_ref(g, c.k)
    _within("f16k_channel_sum", f"{c.id} k={c.k}", ops.f16k_channel_sum(g16, c.B, c.C, c.HW), ref, bound)


def test_f16k_act_bwd_past_its_cap():
    from masic_amd import ops
    n = T.F16K_PAST_CAP_N
    g, y = (T.bf16_round(T.rng(s).standard_normal(n)) for s in (61, 62))
    y[:16] = np.resize(T.f32([0.0, -0.0]), 16)
    as16 = lambda a: torch.from_numpy(a).bfloat16().view(torch.int16).to(DEV)
    for slope in (0.0, 0.01):
        out = ops.f16k_act_bwd(as16(g), as16(y), slope)
        _exact("f16k_act_bwd", f"n={n} slope={slope}", out.cpu().view(torch.bfloat16).float().numpy(), T.f16k_act_bwd_ref(g, y, slope))
    print(f"small_kernels | f16k_act_bwd | {n // 8} records past 8192 blocks | bit-equal")


# ------------------------------------------------------------------------------------------------ eb_table_split
@pytest.mark.parametrize("C", T.EB_SPLIT_CHANNELS)
def test_eb_table_split(C):
    from masic_amd import ops
    table = T.f32(T.rng(71).standard_normal((C, 58)))
    shapes = [(C,) + s for s in T.EB_SHAPES]
    parts = ops.eb_table_split(_d(table), shapes)
    assert len(parts) == 14
    col = 0
    for p, s in zip(parts, shapes):
        w = int(np.prod(s[1:]))
        assert tuple(p.shape) == s and p.is_contiguous()
        _exact("eb_table_split", f"C={C} columns {col}..{col + w}", p, table[:, col:col + w].reshape(s))
        col += w
    assert col == 58
