"""The six kernels that compute the entropy parameters -- gemm_f16k2, gemm_f16k<2>, gemm_f16k<4, true> (gemm_f16k.hip),
gemm1x1_bf16_kernel (gemm_bf16.hip), skinny_f16k<4, false> and skinny_f16k<8, true> (skinny.hip) -- against the float64 reference of
tests/gemm_ref.py, case by case (its tables: what each case forces, asserted without a GPU by tests/test_cpu_gemm_rows.py).

Each case runs twice.
(a) Whole-number operands under the asserted bound max|x| max|w| K + max|bias| < 2^24: every partial sum is exact in float32 in any
    order, so a float32 output must equal the float64 reference bit for bit, an F16K output that reference rounded once to bf16 (bits:
    the sign of zero counts), an F8K output f16k_ref.fp8_out_ref of it, and everything outside an output view or a pixel list must
    keep its prefill.  The k orders of the kernels differ, the reference does not: gemm_f16k2, gemm1x1_bf16_kernel and
    skinny_f16k<4, false> are also run on ONE layer (g2-odd's) and compared with each other.
(b) Real operands at the project's gates (gemm_ref.gate_for): 2e-5 of the reference's peak for a float32 output, 2^-8 for an F16K
    output against the reference rounded to bf16.  An F8K output is launched and not compared: a result 2e-5 away from an e4m3 tie may
    round the other way, and run (a) is its comparison with the reference.
The pixel-list cases run with the four lists of gemm_ref.pixel_lists, each against gemm_ref.scatter_ref, and the results of the other
three at their pixels equal those of the all-pixels list bit for bit.  Measured errors: DESIGN.md section 2.3."""
import pytest
import torch

from tests import f16k_ref as R
from tests import gemm_ref as G
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _report(case, run, gate, err):
    print(f"gemm_rows | {case.id} | {case.kernel} | {run} | gate {gate} | error {err:.3e}")


def _x_buffer(case, x):
    """the activation buffer the kernel reads: F8K, or F16K with the channels padded to 16 by zeros (gemm1x1_bf16_kernel alone takes such)"""
    if case.prec == G.PREC_FP8:
        return _dev(R.to_f8k(x))
    pad = -x.shape[1] % 16
    return _dev(R.to_f16k(torch.nn.functional.pad(x, (0, 0, 0, 0, 0, pad)) if pad else x))


def _pack(case, l, w):
    """(packed weights, dequantisation scales or None) through the single-layer pack entry points"""
    from masic_amd import ops
    if case.ctx:
        return ops.pack_skinny_ctx_weight(_dev(w)), None            # the unmasked weight: the pack must take the 12 live taps only
    w2 = _dev(w.reshape(w.shape[0], w.shape[1]).contiguous())
    if case.kernel == G.RS:
        return ops.pack_gemm1x1_weight(w2, l.Cin, l.Cout, l.transposed), None
    if case.prec == G.PREC_FP8:
        return ops.pack_gemm_f8k_weight(w2, l.Cin, l.Cout, l.transposed)
    return ops.pack_gemm_f16k_weight(w2, l.Cin, l.Cout, l.transposed), None


def _out_buffer(l, B, H, W, listed=False):
    """the layer's whole output buffer, prefilled on the host (so that the bits of the prefill are the reference's)"""
    ctot = (l.view or (l.Cout, 0))[0]
    fill = torch.full((B, ctot, H, W), G.prefill_of(l, 1.0, listed))
    if l.out == "nchw":
        return fill.to(DEV)
    return _dev(R.to_f16k(fill)) if l.out == "f16k" else _dev(R.to_f8k(fill))


def _decode(l, buf, B, H, W, scale):
    ctot = (l.view or (l.Cout, 0))[0]
    if l.out == "nchw":
        return buf.cpu()
    return R.from_f16k(buf, B, ctot, H, W) if l.out == "f16k" else R.from_f8k(buf, B, ctot, H, W) * scale


def _same(l, got, want):
    """bit for bit (float32 and bf16: NaN prefill and the sign of zero included; a decoded F8K buffer by value)"""
    return torch.equal(R.bits(got), R.bits(want)) if l.out in ("nchw", "f16k") else torch.equal(got, want)


def _references(case, integers):
    """per layer: (x, w, bias, W x + b in float64, out_scale or None)"""
    refs = []
    for i, l in enumerate(case.layers):
        x, w, bias = G.operands(case, i, integers=integers, seed_shift=0 if integers else 500)
        if integers:
            assert G.exact_bound(case, l, x, w, bias) < 2 ** 24, "every partial sum must be a float32 integer"
        v64 = G.layer64(case, l, x, w, bias)
        scale = G.f8_scale(R.act32(v64.float(), l.act), l.out == "f8k-sat") if l.out.startswith("f8k") else None
        refs.append((x, w, bias, v64, scale))
    return refs


# ------------------------------------------------------------------------------------------------ full-latent GEMMs
def _run_full(case, refs, packs):
    """one launch of the case's layers into prefilled buffers; the decoded whole buffers, per layer"""
    from masic_amd import ops
    B, H, W = case.B, case.H, case.W
    xs = [_x_buffer(case, r[0]) for r in refs]
    biases = [_dev(r[2]) for r in refs]
    outs = [_out_buffer(l, B, H, W) for l in case.layers]
    if case.kernel == G.RS:
        (l,), (wp, _) = case.layers, packs[0]
        coff = (l.view or (0, 0))[1]
        if l.out == "nchw":
            ops.gemm1x1_bf16(xs[0], wp, biases[0], B, l.Cin, l.Cout, H, W, l.act, out_nchw=outs[0], out_coff=coff)
        else:
            outs[0] = ops.gemm1x1_bf16(xs[0], wp, biases[0], B, l.Cin, l.Cout, H, W, l.act)
        assert outs[0].numel() == B * (l.view or (l.Cout, 0))[0] * H * W
    else:
        # the raw entry point: the Python wrappers allocate their own whole outputs, these are prefilled views
        arr = (ops._lib.GemmGroup * len(case.layers))()
        for g, l, x, (wp, ws), b, y, r in zip(arr, case.layers, xs, packs, biases, outs, refs):
            ctot, coff = l.view or (l.Cout, 0)
            g.x, g.w_packed, g.wscale, g.bias = ops._p(x), ops._p(wp), ops._p(ws), ops._p(b)         # unit input scale: the weight scales are the call's
            g.y_f16k, g.y_f8k, g.y_nchw = (ops._p(y) if l.out.startswith(k) else None for k in ("f16k", "f8k", "nchw"))
            g.out_inv_scale = 1.0 / r[4] if r[4] else 0.0
            g.Cin, g.Cout, g.out_ctot, g.out_coff, g.act = l.Cin, l.Cout, ctot, coff, l.act
        ops.check(ops.lib.masic_gemm_f16k_group_fwd(arr, len(case.layers), B, H * W, ops._stream()), "gemm_f16k_group_fwd")
    torch.cuda.synchronize()
    return [_decode(l, y, B, H, W, r[4]) for l, y, r in zip(case.layers, outs, refs)]


def _check_full(case, refs, got, exact, tag=""):
    for i, (l, r, y) in enumerate(zip(case.layers, refs, got)):
        want = G.expected(l, r[3], out_scale=r[4])
        ctot, coff = l.view or (l.Cout, 0)
        own = slice(coff, coff + l.Cout)
        name = f"{case.id}{tag} layer {i} ({l.Cin} -> {l.Cout}, {l.out})"
        whole = G.whole_buffer(l, want, G.prefill_of(l, r[4] or 1.0))
        outside = torch.ones(ctot, dtype=torch.bool)
        outside[own] = False
        assert torch.equal(y[:, outside].float(), whole[:, outside].float()), f"{name}: the prefill outside the view"
        if exact:
            _report(case, f"(a) whole numbers{tag}, layer {i} {l.out}", "exact", rel_err(y[:, own].float(), want.float()))
            assert _same(l, y, whole), f"{name}: exact operands, exact sums"
        elif G.gate_for(l) is None:
            _report(case, f"(b) real operands{tag}, layer {i} {l.out}: launched, not compared", "none", 0.0)
            assert bool(torch.isfinite(y).all())
        else:
            e = rel_err(y[:, own].float(), want.float())
            _report(case, f"(b) real operands{tag}, layer {i} {l.out}", f"{G.gate_for(l):.1e}", e)
            assert e <= G.gate_for(l), f"{name}: {e:.3e} > {G.gate_for(l):.1e}"


@pytest.mark.parametrize("case", G.FULL_CASES, ids=[c.id for c in G.FULL_CASES])
def test_full_latent_gemm_vs_float64(case):
    for exact in (True, False):
        refs = _references(case, integers=exact)
        packs = [_pack(case, l, r[1]) for l, r in zip(case.layers, refs)]
        _check_full(case, refs, _run_full(case, refs, packs), exact)
        if case.id != "g2-group3":
            continue
        # the packs of one launch (ops.pack_gemm_f16k_weights) are the single packs; and the leading groups alone, against the reference
        from masic_amd import ops
        jobs = [(_dev(r[1].reshape(r[1].shape[0], r[1].shape[1]).contiguous()), l.Cin, l.Cout, l.transposed) for l, r in zip(case.layers, refs)]
        for one, (single, _) in zip(ops.pack_gemm_f16k_weights(jobs), packs):
            assert torch.equal(one, single), "pack_gemm_f16k_weights differs from pack_gemm_f16k_weight"
        for n in (2, 1):
            sub = case._replace(layers=case.layers[:n])
            _check_full(sub, refs[:n], _run_full(sub, refs[:n], packs[:n]), exact, tag=f", first {n} of 3 groups")


def test_wrappers_of_the_full_latent_gemms_agree_with_the_raw_entry_point():
    """ops.gemm_f16k / gemm_f16k_group / gemm_f8k (which allocate whole outputs themselves) on whole numbers: the same bits"""
    from masic_amd import ops
    for name in ("g2-even", "g2-group3", "g16-mixed", "g8-ring"):
        case = G.by_id(name)
        B, H, W = case.B, case.H, case.W
        refs = _references(case, integers=True)
        packs = [_pack(case, l, r[1]) for l, r in zip(case.layers, refs)]
        xs = [_x_buffer(case, r[0]) for r in refs]
        if name == "g2-even":
            l, = case.layers
            buf = _out_buffer(l, B, H, W)
            ops.gemm_f16k(xs[0], packs[0][0], _dev(refs[0][2]), B, l.Cin, l.Cout, H, W, l.act, out_nchw=buf, out_coff=l.view[1])
            outs, layers = [buf], [l]
        elif name == "g8-ring":
            l, = case.layers
            outs = [ops.gemm_f8k(xs[0], packs[0][0], packs[0][1], _dev(refs[0][2]), B, l.Cin, l.Cout, H, W, l.act, out="f8k", out_scale=refs[0][4])]
            layers = [l]
        else:
            layers = list(case.layers)
            outs = ops.gemm_f16k_group([dict(x=x, wp=p[0], bias=_dev(r[2]), Cin=l.Cin, Cout=l.Cout, act=l.act, out=l.out, out_scale=r[4])
                                        for l, x, p, r in zip(layers, xs, packs, refs)], B, H, W)
        for l, y, r in zip(layers, outs, refs):
            want = G.whole_buffer(l, G.expected(l, r[3], out_scale=r[4]), G.prefill_of(l, r[4] or 1.0))
            assert _same(l, _decode(l, y, B, H, W, r[4]), want), f"{name}: {l.Cin} -> {l.Cout} through the wrapper"


# ------------------------------------------------------------------------------------------------ pixel-list kernels
def _run_list(case, refs, packs, gate, plist):
    from masic_amd import ops
    B, H, W = case.B, case.H, case.W
    xs = [_x_buffer(case, r[0]) for r in refs]
    outs = [_out_buffer(l, B, H, W, listed=True) for l in case.layers]
    layers = []
    for l, x, (wp, _), r, y in zip(case.layers, xs, packs, refs, outs):
        ctot, coff = l.view or (l.Cout, 0)
        layers.append(dict(x=x, wp=wp, bias=_dev(r[2]), Cin=l.Cin, Cout=l.Cout, act=l.act, out_ctot=ctot, out_coff=coff,
                           **{"y16" if l.out == "f16k" else "y32": y}))
    step = None if plist.step is None else torch.tensor([plist.step], dtype=torch.int32, device=DEV)
    ops.skinny_group(layers, _dev(plist.pix), step, plist.list_stride, plist.npix, H, W, ctx=case.ctx, gate=_dev(gate),
                     gate_c=case.gate[1] if case.gate else 0, nimg=B)
    torch.cuda.synchronize()
    return [_decode(l, y, B, H, W, None) for l, y in zip(case.layers, outs)]


@pytest.mark.parametrize("case", G.LIST_CASES, ids=[c.id for c in G.LIST_CASES])
def test_pixel_list_kernel_vs_float64(case):
    B, HW = case.B, case.H * case.W
    lists = G.pixel_lists(case)
    for exact in (True, False):
        refs = _references(case, integers=exact)
        packs = [_pack(case, l, r[1]) for l, r in zip(case.layers, refs)]
        gate = G.gate_plane(case, 0 if exact else 500)
        g1 = None if gate is None else gate[:, case.gate[1]:case.gate[1] + 1]
        full = [G.whole_buffer(l, G.expected(l, r[3], g1), G.prefill_of(l, listed=True)) for l, r in zip(case.layers, refs)]
        every = None
        for plist in lists:
            got = _run_list(case, refs, packs, gate, plist)
            for i, (l, y, f) in enumerate(zip(case.layers, got, full)):
                name = f"{case.id}, list '{plist.name}', layer {i} ({l.Cin} -> {l.Cout}, {l.out})"
                want = G.scatter_ref(f, plist.named, B, HW, G.prefill_of(l, listed=True))
                named = ~torch.isnan(G.scatter_ref(torch.zeros(B, 1, case.H, case.W), plist.named, B, HW, float("nan")))[:, 0]
                ctot, coff = l.view or (l.Cout, 0)
                written = torch.zeros((B, ctot, case.H, case.W), dtype=torch.bool)
                written[:, coff:coff + l.Cout] = named[:, None]
                assert torch.equal(R.bits(y)[~written], R.bits(want)[~written]), f"{name}: unlisted pixels and the channels outside the view keep the prefill"
                if exact:
                    _report(case, f"(a) whole numbers, list '{plist.name}', layer {i} {l.out}", "exact", rel_err(y[written].float(), want[written].float()))
                    assert _same(l, y, want), f"{name}: exact operands, exact sums"
                else:
                    e = float((y[written].double() - want[written].double()).abs().max()) / float(f[:, coff:coff + l.Cout].double().abs().max())
                    _report(case, f"(b) real operands, list '{plist.name}', layer {i} {l.out}", f"{G.gate_for(l):.1e}", e)
                    assert e <= G.gate_for(l), f"{name}: {e:.3e} > {G.gate_for(l):.1e}"
                if every is not None:
                    assert torch.equal(R.bits(y)[written], R.bits(every[i])[written]), f"{name}: differs from the all-pixels launch at its pixels"
            if plist.name == "all":
                every = got


# ------------------------------------------------------------------------------------------------ three kernels, one layer
def test_three_kernels_compute_one_layer_to_the_same_bits():
    """g2-odd's layer (176 -> 160, ConvTranspose2d orientation, leaky, F16K; r-tiles is the same layer under ReLU) on whole numbers through
    gemm_f16k2, gemm1x1_bf16_kernel and skinny_f16k<4, false>: k orders 64-channel chunks, 16-channel steps and four interleaved waves"""
    case = G.by_id("g2-odd")
    l, = case.layers
    assert G.by_id("r-tiles").layers[0]._replace(act=l.act) == l
    refs = _references(case, integers=True)
    want = G.expected(l, refs[0][3])
    got = {}
    for kernel in (G.G2, G.RS):
        c = case._replace(kernel=kernel)
        got[kernel] = _run_full(c, refs, [_pack(c, l, refs[0][1])])[0]
    c = case._replace(kernel=G.S1)
    got[G.S1] = _run_list(c, refs, [_pack(c, l, refs[0][1])], None, G.pixel_lists(c)[0])[0]
    for kernel, y in got.items():
        assert torch.equal(R.bits(y), R.bits(want)), f"{kernel} against the reference"
    assert torch.equal(R.bits(got[G.G2]), R.bits(got[G.RS])) and torch.equal(R.bits(got[G.RS]), R.bits(got[G.S1]))
    print(f"gemm_rows | g2-odd / r-tiles | {G.G2} = {G.RS} = {G.S1} | (a) whole numbers, one layer | gate exact | error 0.000e+00")
