"""The cases of tests/test_gpu_gemm_rows.py without a GPU: the reference of tests/gemm_ref.py agrees with independent forms, the case
tables name exactly the six kernels and every case has the property it is filed under (computed from its integers and the kernels'
constants restated in tests/gemm_ref.py), its whole-number operands are exact in float32, it leaves room under its gate, and its
pixel lists hold what they promise."""
import pytest
import torch

from tests import f16k_ref as R
from tests import gemm_ref as G
from tests.util import rel_err

IDS = [c.id for c in G.CASES]
LIST_IDS = [c.id for c in G.LIST_CASES]


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("transposed", [False, True])
def test_layer64_is_the_modules_1x1(transposed):
    case = G._case("t", G.G2, 2, (3, 5), G.L(48, 64, transposed=transposed))
    l = case.layers[0]
    x, w, bias = G.operands(case, 0)
    mod = (torch.nn.ConvTranspose2d if transposed else torch.nn.Conv2d)(48, 64, 1).double()
    assert tuple(mod.weight.shape) == tuple(w.shape)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(bias)
        want = mod(x.double())
    assert rel_err(G.layer64(case, l, x, w, bias), want) <= 1e-12
    nb = G.layer64(case, l, x, w, None)
    assert rel_err(nb + bias.double().view(1, -1, 1, 1), want) <= 1e-12


def test_layer64_is_the_masked_module():
    from compressai.layers import MaskedConv2d
    case = G._case("t", G.SC, 2, (6, 7), G.L(32, 64), ctx=True)
    x, w, bias = G.operands(case, 0)
    assert bool((w[:, :, 2, 2:] != 0).any()) and bool((w[:, :, 3:] != 0).any()), "the drawn weight is not masked: the reference has to"
    mask = MaskedConv2d(32, 64, 5, padding=2).mask
    assert int(mask[0, 0].sum()) == G.SK_TAPS
    mod = torch.nn.Conv2d(32, 64, 5, padding=2).double()
    with torch.no_grad():
        mod.weight.copy_(w.double() * mask.double())
        mod.bias.copy_(bias)
        want = mod(x.double())
    assert rel_err(G.layer64(case, case.layers[0], x, w, bias), want) <= 1e-12


def test_expected_and_scatter_in_closed_form():
    l = G.L(1, 1, G.ACT_LEAKY, out="f16k")
    v = torch.tensor([-300.0, 0.0, 257.0, 259.0]).double().view(1, 1, 2, 2)
    got = G.expected(l, v)
    assert got.dtype == torch.bfloat16 and got.flatten().tolist() == [-3.0, 0.0, 256.0, 260.0]     # 0.01f * -300 rounds to bf16 -3; ties to even
    gate = torch.tensor([0.5, 1.0, 0.0, 2.0]).view(1, 1, 2, 2)
    assert G.expected(l._replace(out="nchw", act=G.ACT_RELU), v, gate).flatten().tolist() == [0.0, 0.0, 0.0, 518.0]
    f8 = G.expected(l._replace(out="f8k", act=G.ACT_NONE), torch.tensor([1000.0, -38.0, 34.0, 0.25]).double().view(1, 1, 2, 2), out_scale=2.0)
    assert f8.flatten().tolist() == [896.0, -40.0, 32.0, 0.25]        # saturates at 448 * 2; e4m3 holds 16, 18, 20: the ties 19 and 17 go to the even 20 and 16
    # a 2 x 3 latent of two images and two channels: value 100 b + 10 c + p
    full = torch.tensor([[[[100.0 * b + 10 * c + 3 * r + s for s in range(3)] for r in range(2)] for c in range(2)] for b in range(2)])
    out = G.scatter_ref(full, [4, -1, 12, 6, 11, 99], 2, 6, -7.0)
    want = torch.full((2, 2, 6), -7.0)
    want[0, :, 4] = torch.tensor([4.0, 14.0])
    want[1, :, 0] = torch.tensor([100.0, 110.0])
    want[1, :, 5] = torch.tensor([105.0, 115.0])
    assert torch.equal(out.view(2, 2, 6), want)
    assert torch.equal(G.whole_buffer(G.L(1, 2, view=(4, 1)), full, 0.5)[:, 1:3], full) and float(G.whole_buffer(G.L(1, 2, view=(4, 1)), full, 0.5)[0, 3, 0, 0]) == 0.5


def test_gates_are_the_projects():
    assert G.gate_for(G.L(16, 32)) == 2e-5 and G.gate_for(G.L(16, 32, out="f16k")) == 2.0 ** -8
    assert G.gate_for(G.L(16, 32, out="f8k")) is None and G.gate_for(G.L(16, 32, out="f8k-sat")) is None


# ------------------------------------------------------------------------------------------------ the tables
def test_the_kernel_column_covers_exactly_the_six_kernels():
    assert {c.kernel for c in G.CASES} == set(G.KERNELS) and len(set(G.KERNELS)) == 6
    assert len(set(IDS)) == len(IDS) == 24
    for c in G.CASES:
        assert G.kernel_of(c) == c.kernel, f"{c.id}: its argument kinds select {G.kernel_of(c)}"
        assert (c in G.LIST_CASES) == (c.kernel in (G.S1, G.SC))


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_case_forces_what_it_is_filed_under(case):
    p = G.properties(case)
    assert case.forces, "every case is in the table for a reason"
    for name, want in case.forces.items():
        assert p[name] == want, f"{case.id}: {name} is {p[name]}, the table says {want}"
    for l in case.layers:
        # what the entry points require (gemm_f16k.hip, skinny.hip: MASIC_REQUIRE)
        ctot, coff = l.view or (l.Cout, 0)
        assert 0 <= coff and coff + l.Cout <= ctot
        if case.kernel != G.RS:
            assert l.Cin % (32 if case.prec == G.PREC_FP8 else 16) == 0 and l.Cout % 32 == 0
            assert l.out == "nchw" or (ctot % (32 if case.prec == G.PREC_FP8 or l.out.startswith("f8k") else 16) == 0 and coff % 16 == 0)


def test_the_shared_layer_and_the_latent_sizes():
    a, b = G.by_id("g2-odd").layers[0], G.by_id("r-tiles").layers[0]
    assert (a.Cin, a.Cout, a.transposed) == (b.Cin, b.Cout, b.transposed) == (176, 160, True), "one layer for three kernels"
    assert {(c.H, c.W) for c in G.CASES} == {(5, 7), (9, 33), (13, 21)}
    assert G.by_id("g2-group3").layers == G.by_id("s1-group3").layers


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_whole_number_operands_are_exact_in_float32(case):
    for i, l in enumerate(case.layers):
        x, w, bias = G.operands(case, i, integers=True)
        assert torch.equal(x, torch.round(x)) and torch.equal(w, torch.round(w))
        assert G.exact_bound(case, l, x, w, bias) < 2 ** 24, case.id
        if case.prec == G.PREC_FP8:
            assert torch.equal(x.to(torch.float8_e4m3fn).float(), x) and torch.equal(w.to(torch.float8_e4m3fn).float(), w)
            assert float(w.abs().reshape(w.shape[0], w.shape[1]).amax(0 if l.transposed else 1).min()) == 448.0, "unit weight scales"
        else:
            assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w)


def test_the_saturating_case_saturates_and_meets_ties():
    case = G.by_id("g16-f8out")
    l = case.layers[0]
    x, w, bias = G.operands(case, 0, integers=True)
    v = R.act32(G.layer64(case, l, x, w, bias).float(), l.act)
    s = G.f8_scale(v, saturate=True)
    q = v / s
    assert 448.0 < float(q.abs().max()) <= 896.0 and int((q.abs() > 448).sum()) > 0
    grid = q.to(torch.float8_e4m3fn).float()
    lo, hi = torch.minimum(grid, q), torch.maximum(grid, q)
    step = torch.where(q.abs() >= 2.0 ** -6, 2.0 ** (torch.floor(torch.log2(q.abs().clamp(min=2.0 ** -6))) - 3), torch.tensor(2.0 ** -9))
    ties = ((hi - lo) == 0.5 * step) & (q.abs() <= 448)
    print(f"g16-f8out: out_scale {s}, {int((q.abs() > 448).sum())} outputs saturate, {int(ties.sum())} are e4m3 ties")
    assert int(ties.sum()) > 0


# ------------------------------------------------------------------------------------------------ room under the gate
@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_float32_on_the_cpu_is_within_a_quarter_of_the_gate(case):
    """the same reference evaluated in float32 (torch, CPU): a correct float32-accumulating kernel has this kind of error, the float32
    gate leaves four times that, and the bf16 rounding of that float32 result stays within 2^-8 of the reference"""
    gate = G.gate_plane(case, 500)
    for i, l in enumerate(case.layers):
        x, w, bias = G.operands(case, i, seed_shift=500)
        v64 = G.layer64(case, l, x, w, bias)
        g1 = None if gate is None else gate[:, case.gate[1]:case.gate[1] + 1]
        ref = G.expected(l._replace(out="nchw"), v64, g1).double()
        if case.ctx:
            v32 = torch.nn.functional.conv2d(x, G.O.masked_weight(w), bias, padding=2)
        else:
            w2 = w.reshape(w.shape[0], w.shape[1])
            v32 = torch.nn.functional.conv2d(x, (w2.t() if l.transposed else w2).reshape(l.Cout, l.Cin, 1, 1), bias)
        f32 = R.act32(v32, l.act)
        if g1 is not None:
            f32 = f32 * g1
        e32, e16 = rel_err(f32, ref), rel_err(f32.bfloat16().float(), ref)
        print(f"gemm_rows floor | {case.id} | {case.kernel} | layer {i} | float32 on the CPU {e32:.3e} (quarter gate 5.0e-06) | its bf16 rounding {e16:.3e} (2^-8)")
        assert e32 <= 0.25 * G.gate_for(l._replace(out="nchw")), (case.id, i, e32)
        assert e16 <= G.gate_for(l._replace(out="f16k")), (case.id, i, e16)


# ------------------------------------------------------------------------------------------------ the lists
@pytest.mark.parametrize("case", G.LIST_CASES, ids=LIST_IDS)
def test_pixel_lists_hold_what_they_name(case):
    N = case.B * case.H * case.W
    every, some, steps, one = G.pixel_lists(case)
    assert every.pix.tolist() == list(range(N)) and every.npix == N and every.step is None
    s = some.pix.tolist()
    valid = [q for q in s if 0 <= q < N]
    assert len(s) == some.npix and len(s) % 32 != 0
    assert len(valid) == len(set(valid)) == round(0.6 * N) and valid != sorted(valid)
    assert any(q == -1 for q in s) and any(q >= N for q in s) and N in s
    assert any(all(q == -1 for q in s[a:a + 32]) for a in range(0, len(s) - 31, 32)), "one aligned block of padding only"
    assert any(0 < sum(0 <= q < N for q in s[a:a + 32]) < len(s[a:a + 32]) for a in range(0, len(s), 32)), "a block with both kinds"
    rows = steps.pix.view(-1, steps.list_stride)
    assert steps.step == 1 and rows.shape[0] == 3 and steps.npix == steps.list_stride and steps.list_stride % 32 != 0
    live = [[q for q in r.tolist() if q >= 0] for r in rows]
    assert all(live) and not (set(live[1]) & (set(live[0]) | set(live[2]))) and int((rows[1] < 0).sum()) > 0
    assert steps.named == rows[1].tolist()
    assert one.npix == 1 and 0 <= one.named[0] < N and one.named[0] // (case.H * case.W) == case.B - 1
    if case.B > 1:
        assert {q // (case.H * case.W) for q in valid} == set(range(case.B)), "the shuffle reaches every image"
