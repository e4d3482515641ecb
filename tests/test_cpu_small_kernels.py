"""tests/small_kernel_cases.py without a GPU: every launcher branch the cases are filed under is taken, on both sides where it has two;
every grid cap is exceeded by a case whose item count leaves some threads one iteration more than others; every float64 reference
agrees with torch float64 autograd of the defining expression (the oracle stays independent of the code under test); every derived
bound is finite and non-zero, and the reference evaluated in float32 on the CPU stays inside it -- the bound is neither vacuous nor
impossible."""
import numpy as np
import pytest
import torch

from tests import small_kernel_cases as T

ONE, BIG = T.gdn_small_cases()


# ------------------------------------------------------------------------------------------------ branches and caps
TWO_SIDED = ["channel_sum: B*HW <= 16384 && C >= 128", "channel_sum: float4 form", "channel_sum: HW % 4", "channel_sum: 16-byte base",
             "channel_sum: more work items than CS_SPLIT", "channel_sum: ragged last chunk of 4096", "channel_sum: partial stage-2 block",
             "channel_sum: more than one chunk in the one-block form",
             "plane_copy: vector form", "plane_copy: HW % 4", "plane_copy: B*C <= 65535", "plane_copy: 16-byte bases", "plane_copy: lane loop",
             "plane_copy: fourth vector in flight",
             "f16k sums: fewer pixels than F16K_CS_CHUNKS", "f16k sums: empty chunks", "f16k_act_bwd_sum: two loads in flight",
             "gdn_bwd_small: more than 512 partial rows", "gdn_bwd_small: past the 2048-block cap"]


def test_every_branch_is_taken():
    sides = T.branch_sides()
    for name in TWO_SIDED:
        assert sides[name] == {True, False}, (name, sides[name])
    assert True in sides["f16k_act_bwd_sum: single-load tail"]


def test_cases_sit_on_the_branch_they_name():
    by = {c.id: c for c in T.CHANNEL_SUM_CASES}
    assert by["one_block_float4_two_chunks"].one_block and by["one_block_float4_two_chunks"].vec
    assert T.channel_sum_plan(2, 128, 8192)["chunks"] == 2
    assert by["one_block_scalar"].one_block and not by["one_block_scalar"].vec
    assert by["one_block_at_16384"].one_block and not by["two_stage_at_16385"].one_block
    p = T.channel_sum_plan(2, 3, 4096 * 33 + 4)
    assert (p["work"], p["splits"], p["ragged"], p["vec"]) == (68, 64, True, True)
    assert T.channel_sum_plan(1, 70, 100)["stage2_partial"]
    # 4 bytes off a 16-byte line: the scalar form although HW % 4 == 0
    for id in ("one_block_off_16_bytes", "two_stage_off_16_bytes"):
        assert by[id].HW % 4 == 0 and not by[id].aligned and not by[id].vec
    assert by["one_block_off_16_bytes"].one_block and not by["two_stage_off_16_bytes"].one_block
    # k is the written figure
    want = dict(one_block_float4_two_chunks=18, one_block_scalar=5, one_block_at_16384=18, two_stage_at_16385=18, two_stage_68_items_ragged=10,
                two_stage_partial_stage2=3, two_stage_one_channel=3, channel_view=3, one_block_off_16_bytes=4, two_stage_off_16_bytes=18)
    assert {c.id: c.k for c in T.CHANNEL_SUM_CASES} == want

    cp = {c.id: c for c in T.COPY_CASES}
    assert [c.path for c in T.COPY_CASES] == ["vector", "vector", "vector", "scalar", "scalar", "scalar", "scalar", "scalar"]
    assert cp["scalar_too_many_planes"].B * cp["scalar_too_many_planes"].C == 65536
    c = T.LANE_LOOP_CASE
    p = T.plane_copy_plan(c.B, c.C, c.H * c.W)
    assert (p["planes"], c.H * c.W, p["gx"], p["passes"]) == (4096, 8196, 2, 2)
    # ... and it cannot be reached with fewer planes x pixels: HW4 > 4 * 256 * gx needs gx capped, i.e. ceil(HW4 / 1024) > ceil(8192 / planes)
    assert T.plane_copy_plan(2, 2048, 8192)["passes"] == 1 and T.plane_copy_plan(2, 1024, 8196)["passes"] == 1

    assert [g.k for g in T.GATE_CASES] == [17, 17, 17, 19, 40]
    assert {c.k for c in T.F16K_CASES if c.HW != 32 * 129 + 5} == {131} and {c.k for c in T.F16K_CASES if c.HW == 32 * 129 + 5} == {132}
    assert T.f16k_sum_plan(3, 16, 32 * 129 + 5)["per"] == 130
    for c in BIG:
        p = T.gdn_small_plan(c.B, c.C, c.H, c.W)
        assert (p["nb"], p["finish_passes"], p["per_thread"]) == (2048, 4, 2)
    assert {T.gdn_small_plan(c.B, c.C, c.H, c.W)["nb"] for c in ONE} == {1}
    assert {(c.C, c.inverse) for c in ONE} == {(C, i) for C in (1, 2, 3, 4) for i in (False, True)} == {(c.C, c.inverse) for c in BIG}
    c = T.SOFTMAX_CASES
    assert {s.K for s in c} == {1, 3, 5, 8} and any((s.B * s.M * s.H * s.W) % 256 == 0 for s in c) and any((s.B * s.M * s.H * s.W) % 256 for s in c)


def test_every_grid_cap_is_exceeded_unevenly():
    caps = T.cap_cases()
    assert {cap for _, _, cap in caps} >= {8192, 4096, 1024, 2048}
    for name, items, cap in caps:
        assert T.past_cap_uneven(items, cap), (name, items, cap)
        assert T.grid_for(items, cap) == cap
    assert T.EW_SIZES == (1, 255, 256, 257, 8192 * 256 + 257)


# ------------------------------------------------------------------------------------------------ references against autograd
def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)


@pytest.mark.parametrize("c", ONE, ids=[c.id for c in ONE])
def test_gdn_small_reference_is_autograd_of_the_oracle(c):
    x, g, beta, gamma = T.gdn_small_inputs(c)
    (gx, gb, gg), bounds, rho = T.gdn_small_ref(c, x, g, beta, gamma)
    ax, ab, ag = T.gdn_small_autograd(x, g, beta, gamma, c.inverse)
    for got, want, bound in ((gx, ax, bounds[0]), (gb, ab, bounds[1]), (gg, ag, bounds[2])):
        assert np.all(np.isfinite(bound)) and np.all(bound > 0)
        assert T.worst_ratio(got, want, bound) < 1e-6, c.id            # float64 against float64: far inside a float32 bound
    assert 1.0 <= rho < 1.001
    # the LowerBound rule is exercised: entries below their bounds, some gradients stopped and some let through
    b_bound, g_bound = T.gdn_bounds()
    below = np.concatenate([(beta < b_bound).reshape(-1), (gamma < g_bound).reshape(-1)])
    grads = np.concatenate([ab.reshape(-1), ag.reshape(-1)])
    assert below.any() and np.all(grads[below] <= 0) and (c.C == 1 or (np.any(grads[below] == 0) and np.any(grads[below] < 0)))
    assert np.all(grads[~below] != 0)


def test_lower_bound_rule_meets_both_signs_below_the_bound():
    seen = set()
    for c in ONE:
        x, g, beta, gamma = T.gdn_small_inputs(c)
        _, ab, ag = T.gdn_small_autograd(x, g, beta, gamma, c.inverse)
        seen.add((c.C, c.inverse, bool(ab[0] == 0)))
    assert seen == {(C, i, z) for C in (1, 2, 3, 4) for i in (False, True) for z in (False, True)}


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_pieces_compose_to_autograd(inverse):
    """gdn_bwd_pre -> u = gamma^T t -> gdn_bwd_post is dL/dx of the (inverse) GDN"""
    r = T.rng(11)
    B, C, H, W = 2, 5, 3, 4
    x, g = r.standard_normal((B, C, H, W)), r.standard_normal((B, C, H, W))
    bet, gam = 0.5 + r.rand(C), 0.1 * r.rand(C, C)
    xt = _t64(x)
    n = torch.einsum("cj,bjhw->bchw", torch.from_numpy(gam), xt * xt) + torch.from_numpy(bet).reshape(1, -1, 1, 1)
    y = xt * torch.sqrt(n) if inverse else xt / torch.sqrt(n)
    y.backward(torch.from_numpy(g))
    # the references take float32 arrays; hand them float32-exact values so that both sides see the same numbers
    x32, g32, n32 = T.f32(x), T.f32(g), T.f32(n.detach().numpy())
    s, sb, t, tb = T.gdn_pre_ref(x32.reshape(-1), n32.reshape(-1), g32.reshape(-1), inverse)
    u = np.einsum("cj,bchw->bjhw", gam, t.reshape(B, C, H, W))
    dx, db = T.gdn_post_ref(x32.reshape(-1), s, u.reshape(-1))
    assert np.allclose(dx.reshape(B, C, H, W), xt.grad.numpy(), rtol=1e-5, atol=1e-6)      # (float32-rounded x, g, n against float64 ones)
    for b in (sb, tb, db):
        assert np.all(np.isfinite(b)) and np.all(b >= 0) and np.any(b > 0)


@pytest.mark.parametrize("c", T.SOFTMAX_CASES, ids=[c.id for c in T.SOFTMAX_CASES])
def test_softmax_references_are_autograd_of_softmax(c):
    x = T.softmax_logits(c)
    y, yb = T.softmax_k_ref(x, c)
    xt = _t64(x.reshape(c.B, c.K, c.M, c.H * c.W))
    yt = torch.softmax(xt, dim=1)
    assert np.allclose(y.reshape(yt.shape), yt.detach().numpy(), rtol=1e-13, atol=0)
    assert np.all(np.isfinite(yb)) and np.all(yb > 0)
    # x - max is exact in float32, as the bound assumes
    v = x.reshape(c.B, c.K, c.M, -1)
    assert np.array_equal((v - v.max(axis=1, keepdims=True)).astype(np.float64), v.astype(np.float64) - v.astype(np.float64).max(axis=1, keepdims=True))
    if c.K > 1:
        assert float((v.max(axis=1) - v.min(axis=1)).max()) >= 99 and float((v.max(axis=1) - v.min(axis=1)).min()) == 0
    # the float32 evaluation stays inside the bound
    e = np.exp((v - v.max(axis=1, keepdims=True)).astype(np.float32))
    y32 = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    assert T.worst_ratio(y32.reshape(x.shape), y, yb) <= 1.0
    # backward: on the float32 y, against autograd through softmax at the float64 y (the difference of the two ys is second order here)
    g = T.f32(T.rng(12).standard_normal(x.shape))
    gx, gb = T.softmax_k_bwd_ref(g, y.astype(np.float64), c)
    yt.backward(torch.from_numpy(g.astype(np.float64).reshape(yt.shape)))
    assert np.allclose(gx.reshape(yt.shape), xt.grad.numpy(), rtol=1e-9, atol=1e-15)
    assert np.all(np.isfinite(gb)) and np.all(gb >= 0)
    if c.K == 1:
        assert np.all(gx == 0)
    y32in = y.astype(np.float32)
    ref, bound = T.softmax_k_bwd_ref(g, y32in, c)
    shp = (c.B, c.K, c.M, c.H * c.W)
    g4, y4 = g.reshape(shp), y32in.reshape(shp)
    dot = np.zeros((c.B, 1, c.M, c.H * c.W), np.float32)
    for k in range(c.K):
        dot = (dot + g4[:, k:k + 1] * y4[:, k:k + 1]).astype(np.float32)
    assert T.worst_ratio((y4 * (g4 - dot)).astype(np.float32).reshape(g.shape), ref, bound) <= 1.0


@pytest.mark.parametrize("c", T.GATE_CASES, ids=[c.id for c in T.GATE_CASES])
def test_gate_reference_is_autograd_of_the_product(c):
    g, x, gate = T.gate_inputs(c)
    for gate_c in (0, 2):
        gx, gg, bound = T.gate_ref(g, x, gate, gate_c, c.k)
        xt, gt = _t64(x), _t64(gate)
        (xt * gt[:, gate_c:gate_c + 1]).backward(torch.from_numpy(g.astype(np.float64)))
        assert np.array_equal(gx, xt.grad.numpy().astype(np.float32))              # one product: its float32 rounding
        assert np.allclose(gg, gt.grad.numpy()[:, gate_c], rtol=1e-13, atol=1e-15)
        assert np.all(gt.grad.numpy()[:, [k for k in range(T.GATE_CTOT) if k != gate_c]] == 0)
        assert np.all(np.isfinite(bound)) and np.all(bound > 0)
        gg32 = (g * x).sum(axis=1, dtype=np.float32)
        assert T.worst_ratio(gg32, gg, bound) <= 1.0


def test_abs_cat_slice_and_reparam_references():
    for op, fn in (("ABS_BWD", lambda a: a.abs()), ("SQUARE", None)):
        a, b, s0, s1 = T.ew_inputs("ABS_BWD", 257, 13)
        bt = _t64(b)
        bt.abs().backward(torch.from_numpy(a.astype(np.float64)))
        assert np.array_equal(T.ew_ref32("ABS_BWD", a, b, s0, s1), bt.grad.numpy().astype(np.float32))      # torch: abs'(+-0) = 0
    # ACT_BWD on the activation's output: the leaky / relu derivative by the sign of the output
    for act, f in ((T.ACT_RELU, torch.relu), (T.ACT_LEAKY, lambda v: torch.nn.functional.leaky_relu(v, 0.01))):
        a, b, s0, s1 = T.ew_inputs("ACT_BWD", 257, 14, act=act)
        pre = _t64(b)                                                    # same sign as the output; at 0 the kernel takes the negative side
        f(pre).backward(torch.from_numpy(a.astype(np.float64)))
        want = pre.grad.numpy()
        got = T.ew_ref32("ACT_BWD", a, b, s0, s1).astype(np.float64)
        nz = b != 0
        assert np.allclose(got[nz], want[nz], rtol=2 ** -23, atol=0)
    # REPARAM / REPARAM_BWD: parametrizers.py:61-64 through the LowerBound rule
    a, b, s0, s1 = T.ew_inputs("REPARAM_BWD", 257, 15)
    p = _t64(b)
    (T._LowerBound.apply(p, torch.tensor(s0, dtype=torch.float64)) ** 2 - T.PED).backward(torch.from_numpy(a.astype(np.float64)))
    assert np.array_equal(T.ew_ref32("REPARAM_BWD", a, b, s0, s1), p.grad.numpy().astype(np.float32))
    assert {(bool(pv >= s0), bool(gv < 0)) for pv, gv in zip(b[:6], a[:6])} == {(x, y) for x in (False, True) for y in (False, True)}
    assert b[2] == np.float32(s0)
    a, b, s0, s1 = T.ew_inputs("REPARAM", 257, 16)
    ref, bound = T.ew_ref64("REPARAM", a, b, s0, s1)
    want = (torch.clamp(torch.from_numpy(a.astype(np.float64)), min=s0) ** 2 - s1).numpy()
    assert np.array_equal(ref, want) and T.worst_ratio(T.ew_ref32("REPARAM", a, b, s0, s1), ref, bound) <= 1.0
    assert (a[:3] == np.float32(s0)).tolist() == [True, False, False] and a[1] < s0 < a.max()
    # cat / slice: copy_view into [coff, coff + C) is torch.cat's forward, slice_copy its backward
    c = T.COPY_CASES[2]
    x, _, _ = T.copy_inputs(c)
    left, right = np.full((c.B, c.coff, c.H, c.W), T.SENTINEL, np.float32), np.full((c.B, c.ctot - c.coff - c.C, c.H, c.W), T.SENTINEL, np.float32)
    xt = _t64(x)
    cat = torch.cat([torch.from_numpy(left).double(), xt, torch.from_numpy(right).double()], dim=1)
    assert np.array_equal(cat.detach().numpy()[:, c.coff:c.coff + c.C], x)
    w = T.rng(17).standard_normal(cat.shape)
    cat.backward(torch.from_numpy(w))
    assert np.array_equal(xt.grad.numpy(), w[:, c.coff:c.coff + c.C])


@pytest.mark.parametrize("op", T.EW_OPS)
def test_elementwise_references_agree_and_bounds_hold(op):
    a, b, s0, s1 = T.ew_inputs(op, 1000, 18)
    r32 = T.ew_ref32(op, a, b, s0, s1)
    assert r32.dtype == np.float32 and np.all(np.isfinite(r32))
    if op in T.EW_EXACT:
        return
    ref, bound = T.ew_ref64(op, a, b, s0, s1)
    assert np.all(np.isfinite(bound)) and np.all(bound > 0)
    assert T.worst_ratio(r32, ref, bound) <= 1.0
    if op == "AXPY":
        a, b, s0, s1 = T.ew_inputs(op, 1000, 18, with_b=False)
        ref, bound = T.ew_ref64(op, a, b, s0, s1)
        assert b is None and T.worst_ratio(T.ew_ref32(op, a, b, s0, s1), ref, bound) <= 1.0


@pytest.mark.parametrize("c", T.CHANNEL_SUM_CASES, ids=[c.id for c in T.CHANNEL_SUM_CASES])
def test_channel_sum_bound_holds_for_a_float32_sum(c):
    x = T.channel_sum_input(c)
    ref, bound = T.channel_sum_ref(x, c)
    assert np.all(np.isfinite(bound)) and np.all(bound > 0) and ref.shape == (c.C,)
    got = x[:, c.coff:c.coff + c.C].sum(axis=(0, 2), dtype=np.float64).astype(np.float32)     # the kernel's last step: float64 to float32
    assert T.worst_ratio(got, ref, bound) <= 1.0
    if c.ctot > c.C:     # a neighbouring channel would be off by far more than the bound
        wrong = x[:, c.coff + 1:c.coff + 1 + c.C].astype(np.float64).sum(axis=(0, 2))
        assert T.worst_ratio(wrong, ref, bound) > 1e6


def test_copy_quantize_and_symbols_references():
    c = T.COPY_CASES[0]
    x, noise, gate = T.copy_inputs(c)
    assert np.any(np.abs(x - np.trunc(x)) == 0.5) and np.any(np.signbit(np.rint(x)) & (np.rint(x) == 0))       # ties, and -0 after rounding
    t = torch.from_numpy(x)
    assert T.bit_equal(T.quantize_ref32(x, "dequantize"), torch.round(t).numpy())
    assert T.bit_equal(T.quantize_ref32(x, "noise", noise, gate, 2), ((t + torch.from_numpy(noise)) * torch.from_numpy(gate)[:, 2:3]).numpy())
    assert T.bit_equal(T.quantize_ref32(x, "copy"), x)
    e = T.rounding_edges()
    assert float(np.abs(e).max()) == 2.0 ** 23 and np.any(e == 2.5) and np.any(e == -3.5)
    assert T.bit_equal(np.rint(e), torch.round(torch.from_numpy(e)).numpy())
    assert np.rint(np.float32(2.5)) == 2 and np.rint(np.float32(-3.5)) == -4
    s = T.symbols_ref(T.symbols_input(), T.SYMBOLS_MEDIANS)
    xs = torch.from_numpy(T.symbols_input())
    assert np.array_equal(s, torch.round(xs - torch.from_numpy(T.SYMBOLS_MEDIANS).reshape(1, -1, 1, 1)).to(torch.int32).numpy())


def test_reductions_and_f16k_references():
    n = 5000
    a, b = T.f32(T.rng(19).standard_normal(n)), T.f32(T.rng(20).standard_normal(n))
    ref, bound = T.sse_ref(a, b)
    d = (a - b).astype(np.float32)
    assert 0 < bound < np.inf and abs(float((d * d).astype(np.float32).astype(np.float64).sum()) - ref) <= bound
    lik = T.likelihood_input(n)
    assert lik.min() >= np.float32(1e-9) and lik.max() <= 1
    ref, bound = T.sum_log_ref(lik)
    assert 0 < bound < np.inf and abs(float(np.log(lik).astype(np.float64).sum()) - ref) <= bound
    x, g = T.lower_bound_inputs(1000, 0.11)
    y, gx = T.lower_bound_ref32(x, g, 0.11)
    xt = _t64(x)
    T._LowerBound.apply(xt, torch.tensor(float(np.float32(0.11)), dtype=torch.float64)).backward(torch.from_numpy(g.astype(np.float64)))
    assert np.array_equal(gx, xt.grad.numpy().astype(np.float32)) and np.any(x == np.float32(0.11)) and np.array_equal(y, np.maximum(x, np.float32(0.11)))
    for c in T.F16K_CASES:
        g, y = T.f16k_inputs(c.B, c.C, c.HW)
        assert T.bit_equal(T.bf16_round(g), g) and np.signbit(y[:, :, min(1, c.HW - 1)]).all() and not np.signbit(y[:, :, 0]).any()
        out = T.f16k_act_bwd_ref(g, y, c.slope)
        want = (torch.from_numpy(g) * torch.where(torch.from_numpy(y) > 0, 1.0, float(np.float32(c.slope)))).bfloat16().float().numpy()
        assert T.bit_equal(out, want)
        ref, bound = T.f16k_sum_ref(out, c.k)
        assert np.all(np.isfinite(bound)) and (np.all(bound > 0) or c.slope == 0.0)
        assert T.worst_ratio(out.sum(axis=(0, 2, 3), dtype=np.float32), ref, np.maximum(bound, 1e-300)) <= 1.0
        # the layout helpers are inverse to each other
        assert T.bit_equal(T.from_f16k(T.to_f16k(out.reshape(c.B, c.C, c.HW, 1)), c.B, c.C, c.HW, 1), out)
    assert sum(int(np.prod(s)) for s in T.EB_SHAPES) == 58 and len(T.EB_SHAPES) == 14
