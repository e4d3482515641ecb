"""The latent written once, in the layouts its consumers read (conv_f16k_multi, masic_conv_f16k_multi_fwd), and the eval forward
that uses it.  The oracle of every comparison is the composition of launches this replaces and which stay in the library:
masic_conv_f16k_fwd -> float32 NCHW, then masic_quantize_fwd / masic_nchw_to_f16k_op / masic_nchw_to_f16k_view_op.  Comparisons are
torch.equal on the raw float32 / int16 bits."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 192


def _operator_data(B, H, W, seed):
    """128 -> 192, 5x5, stride 2: activations multiples of 0.5 in [-3, 3], weights +-1 on one to three (channel, tap) pairs per
    output channel, bias in {0, 0.5, -0.5}: every sum is an exact multiple of 0.5 (ties, values in (-0.5, 0) that round to -0).
    Three output channels sum a sign pattern over all 128 input channels of a patch set to 3 x that pattern: |v| >= 384 > 256,
    where bf16 has a spacing of 2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-6, 7, (B, 128, H, W), generator=g).float() * 0.5
    s = (torch.randint(0, 2, (128,), generator=g) * 2 - 1).float()
    x[:, :, : min(H, 6), : min(W, 8)] = 3.0 * s.view(1, 128, 1, 1)
    w = torch.zeros(M, 128, 5, 5)
    for co in range(M):
        for _ in range(1 + co % 3):
            ci, kh, kw = (int(torch.randint(0, n, (1,), generator=g)) for n in (128, 5, 5))
            w[co, ci, kh, kw] = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
    for co, sign in ((5, 1.0), (100, -1.0), (191, 1.0)):
        w[co] = 0
        w[co, :, 2, 2] = sign * s
    b = (torch.randint(-1, 2, (M,), generator=g).float() * 0.5)
    b[5], b[100] = 0.5, -0.5
    return x.to(DEV), w.to(DEV), b.to(DEV)


# (B, H, W, accumulator tiles per workgroup = 4 / co-block split): 32 output pixels in a 256-pixel tile, H != W; odd, ragged output;
# a multiple of 8 images (the per-XCD workgroup order); 72 and 162 workgroups = the two far sides of the split rule of plan_f16k
# (<= 64: 4, <= 160: 2, else 1; workgroups = tiles x co-blocks x B, a tile = 8 x 32 output pixels)
SHAPES = [(2, 8, 16, 1), (1, 34, 18, 1), (8, 8, 16, 1), (4, 48, 192, 2), (9, 48, 192, 4)]
SUBSETS = [("y32", "round32", "round16", "abs16"), ("y32", "round16", "abs16"), ("gated",)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "B%dx%dx%d" % s[:3])
def operator_case(request):
    """One shape: inputs, the descriptor, and the reference = the separate launches (computed once for the three subsets)."""
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16
    B, H, W, nm = request.param
    x, w, b = _operator_data(B, H, W, seed=1000 + B + H)
    d = ops.make_conv_desc(B, 128, H, W, M, 5, 5, 2, 2, in_ctot=128, prec=PREC_BF16)
    assert ops.conv_f16k_supported(d) and ops.conv_f16k_multi_supported(d)
    buf = ctypes.create_string_buffer(96)
    ops.lib.masic_conv_f16k_kernel_name(ctypes.byref(d), 0, buf, 96)
    assert buf.value.decode() == "conv_f16k<1, 5, 2, 6, 1, false, %d, 1, false>" % nm, buf.value
    x16 = ops.nchw_to_f16k(x)
    wp = ops.pack_conv_f16k_weight(w, d)
    g = torch.Generator().manual_seed(7)
    gates = torch.rand((B, 3, d.Ho, d.Wo), generator=g)
    gates[:, 2].view(B, -1)[:, 0::5] = 0.0
    gates[:, 2].view(B, -1)[:, 1::5] = 1.0
    gates = gates.to(DEV)
    y = ops.conv2d_f16k(x16, wp, b, d, want_nchw=True)
    ref = {"y32": y, "round32": ops.quantize(y, "dequantize"), "round16": ops.nchw_to_f16k(y, in_op=ops.INOP_ROUND),
           "abs16": ops.nchw_to_f16k(y, in_op=ops.INOP_ABS)}
    cat = torch.full((B * 960 * d.Ho * d.Wo,), 0x1234, dtype=torch.int16, device=DEV)
    ops.nchw_to_f16k_view(y, cat, 960, 768, in_op=ops.INOP_ROUND, gate=gates, gate_c=2)
    ref["gated"] = cat
    torch.cuda.synchronize()
    # the data must hold the cases the stores can get wrong
    frac = (y - torch.floor(y))
    assert int((frac == 0.5).sum()) > 100, "no exact ties"
    r = ref["round32"]
    assert int(((r == 0) & torch.signbit(r)).sum()) > 10, "no -0"
    assert int((y.abs() > 256).sum()) > 0 and int((y.abs() > 256).any(dim=0).any(dim=-1).any(dim=-1).sum()) <= 8, "|v| > 256 in a few channels"
    assert bool((gates[:, 2] == 0).any()) and bool((gates[:, 2] == 1).any())
    return {"d": d, "x16": x16, "wp": wp, "b": b, "gates": gates, "ref": ref}


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s))
def test_conv_f16k_multi_equals_separate_launches(operator_case, subset):
    from masic_amd import ops
    c = operator_case
    d, ref = c["d"], c["ref"]
    if subset == ("gated",):
        cat = torch.full_like(ref["gated"], 0x1234)
        out = ops.conv2d_f16k_multi(c["x16"], c["wp"], c["b"], d, want=("round16",), round16=cat, round16_ctot=960, round16_coff=768,
                                    gate=c["gates"], gate_c=2)
        torch.cuda.synchronize()
        assert set(out) == {"round16"} and out["round16"] is cat
        assert torch.equal(cat, ref["gated"]), "gated round16 view (the channels outside the view must stay untouched)"
        return
    out = ops.conv2d_f16k_multi(c["x16"], c["wp"], c["b"], d, want=subset)
    torch.cuda.synchronize()
    assert set(out) == set(subset)
    for k in subset:
        a, r = out[k], ref[k]
        if a.dtype == torch.float32:       # the bits, so that -0 != +0
            a, r = a.view(torch.int32), r.view(torch.int32)
        assert a.shape == r.shape and torch.equal(a, r), (k, int((a != r).sum()))


def test_gmm_likelihood_without_the_quantised_output():
    from masic_amd import ops
    B, K, H, W = 2, 5, 4, 8
    g = torch.Generator().manual_seed(3)
    y = (torch.randn((B, M, H, W), generator=g) * 4).to(DEV)
    sigma = (torch.rand((B, K * M, H, W), generator=g) * 3).to(DEV)
    mu = torch.randn((B, K * M, H, W), generator=g).to(DEV)
    wts = torch.randn((B, K * M, H, W), generator=g).to(DEV)
    y_hat, lik = ops.gmm_likelihood(y, sigma, mu, wts, K, weights_are_logits=True)
    none, lik2 = ops.gmm_likelihood(y, sigma, mu, wts, K, weights_are_logits=True, want_y_hat=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(y_hat, torch.round(y))
    assert torch.equal(lik.view(torch.int32), lik2.view(torch.int32))


def test_conv_igemm_bf16_f16k_output_equals_conversion_of_the_float32_result():
    """The second hyper-synthesis layer (ConvTranspose2d 192 -> 288, k5, s2, LeakyReLU) at B = 2, 4x8 -> 8x16: 288 channels = 18
    records, no multiple of the workgroup's channel tile (the last workgroup holds a 32-channel tile past Cout, which stores nothing)."""
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16
    B, Cin, Cout, H, W = 2, 192, 288, 4, 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, Cin, H, W), generator=g).to(DEV)
    w = (torch.randn((Cin, Cout, 5, 5), generator=g) * 0.02).to(DEV)
    b = (torch.randn((Cout,), generator=g) * 0.1).to(DEV)
    d = ops.make_conv_desc(B, Cin, H, W, Cout, 5, 5, 2, 2, transposed=True, act=ops.ACT_LEAKY, prec=PREC_BF16)
    assert (d.Ho, d.Wo) == (8, 16) and ops.conv2d_f16k_out_supported(d)
    wp = ops.pack_conv_weight(w, d)
    y = ops.conv2d(x, wp, b, d)
    want = ops.nchw_to_f16k(y)
    got = ops.conv2d_f16k_out(x, wp, b, d)
    torch.cuda.synchronize()
    assert int((y < 0).sum()) > 1000 and int((y > 0).sum()) > 1000, "both sides of the LeakyReLU"
    assert got.shape == want.shape == (B * 288 * 8 * 16,) and torch.equal(got, want), int((got != want).sum())


def test_entropy_bottleneck_reads_strided_medians_in_place():
    from masic_amd import ops
    from masic_amd._lib import EB_PARAMS_PER_CHANNEL
    B, C, H, W = 2, 128, 2, 4
    g = torch.Generator().manual_seed(5)
    z = (torch.randn((B, C, H, W), generator=g) * 3).to(DEV)
    table = (torch.randn((C, EB_PARAMS_PER_CHANNEL), generator=g) * 0.5).to(DEV)
    quantiles = torch.randn((C, 1, 3), generator=g).to(DEV)
    med = quantiles[:, 0, 1]
    assert not med.is_contiguous()
    a = ops.entropy_bottleneck(z, table, med.contiguous())
    b = ops.entropy_bottleneck(z, table, med)
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


class _Calls:
    """Every call through the C ABI, by symbol (the proxy of tools/launch_origins.py)."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.names.append(name)
            return fn(*a)
        return call


def _net():
    import MASIC
    from masic_amd import synth
    net = MASIC.HSIC(128, M, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31))
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def net():
    return _net()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("B,H,W", [(2, 64, 128), (1, 128, 128)])
def test_eval_forward_hands_its_consumers_what_the_separate_launches_made(net, monkeypatch, B, H, W):
    from masic_amd import nn as mnn, ops, synth
    from masic_amd.f16k import F16K
    from masic_amd.graph import GraphedHSIC
    x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=32))
    seen = {}

    def spy(obj, name, key, pick):
        orig = getattr(obj, name)

        def f(*a, **kw):
            seen.setdefault(key, []).append(pick(a, kw))
            return orig(*a, **kw)
        monkeypatch.setattr(obj, name, f)

    spy(net.decoder1, "reconstruct", "dec1", lambda a, kw: a[0] if isinstance(a[0], F16K) else None)
    spy(net, "_context", "ctx", lambda a, kw: (a[0], kw.get("round16")))
    spy(net._h_a1, "forward", "h_a1", lambda a, kw: kw.get("abs16"))
    spy(net, "_eval_right_entropy", "right", lambda a, kw: a)
    mnn.set_precision("bf16")
    try:
        with torch.no_grad():
            out = net(x1, x2, hm)
            torch.cuda.synchronize()
            # what the separate launches make of the same inputs
            y1 = net.encoder1.latent(x1)
            assert torch.equal(_bits(out["y1_hat"]), _bits(ops.quantize(y1, "dequantize")))
            r16 = ops.nchw_to_f16k(y1, in_op=ops.INOP_ROUND)
            assert seen["dec1"][0] is not None and torch.equal(seen["dec1"][0].buf, r16) and seen["dec1"][0].shape == tuple(y1.shape)
            ctx1 = [r for c, r in seen["ctx"] if c is net.context_prediction1]
            assert len(ctx1) == 1 and ctx1[0] is seen["dec1"][0], "context model and decoder1 share one round buffer"
            assert seen["h_a1"][0] is not None and torch.equal(seen["h_a1"][0].buf, ops.nchw_to_f16k(y1, in_op=ops.INOP_ABS))
            x1_hat_warp, right = seen["right"][0]
            h, w = y1.shape[-2:]
            want = torch.zeros_like(right["cat16"].buf)
            ops.nchw_to_f16k_view(net.encoder1.latent(x1_hat_warp), want, 5 * M, 4 * M, in_op=ops.INOP_ROUND, gate=right["gates"], gate_c=2)
            got = right["cat16"].buf.view(B, 5 * M // 16, h * w, 16)[:, 4 * M // 16:]
            assert torch.equal(got, want.view(B, 5 * M // 16, h * w, 16)[:, 4 * M // 16:]), "cat2 slice of the second encoder1 pass"
            # the right view: round(y2) / |y2| against the conversions of its float32 latent
            ctx2 = [r for c, r in seen["ctx"] if c is net.context_prediction2]
            assert torch.equal(ctx2[0].buf, ops.nchw_to_f16k(right["y2"], in_op=ops.INOP_ROUND))
            assert torch.equal(right["y2_abs16"].buf, ops.nchw_to_f16k(right["y2"], in_op=ops.INOP_ABS))
            # decoder2 on the F16K round(y2) against decoder2 on the float32 y2_hat
            assert torch.equal(_bits(out["x2_hat"]), _bits(net.decoder2(ops.quantize(right["y2"], "dequantize"), x1_hat_warp)))
            monkeypatch.undo()
            rep = GraphedHSIC(net, x1, x2, hm)(x1, x2, hm)
            torch.cuda.synchronize()
    finally:
        mnn.set_precision("f32")
    for k, v in out.items():
        if k == "likelihoods":
            for kk in v:
                assert torch.equal(_bits(rep[k][kk]), _bits(v[kk])), kk
        else:
            assert torch.equal(_bits(rep[k]), _bits(v)), k


def test_eval_forward_launches_no_conversion_of_a_latent(net, monkeypatch):
    """One eval forward at B = 2, 64 x 128: the three latent layers are multi-output launches, nothing quantises or converts a latent
    afterwards, the second hyper-synthesis layers write F16K themselves: no stand-alone float32 -> F16K conversion is left."""
    from masic_amd import nn as mnn, ops, synth
    x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(2, 64, 128, seed=32))
    mnn.set_precision("bf16")
    try:
        with torch.no_grad():
            net(x1, x2, hm)
            torch.cuda.synchronize()
            calls = _Calls(ops.lib)
            monkeypatch.setattr(ops, "lib", calls)
            net(x1, x2, hm)
            torch.cuda.synchronize()
            monkeypatch.undo()
    finally:
        mnn.set_precision("f32")
    n = {k: calls.names.count(k) for k in set(calls.names)}
    conversions = sum(v for k, v in n.items() if k.startswith("masic_nchw_to_f16k"))
    assert n.get("masic_conv_f16k_multi_fwd", 0) == 3, n
    assert n.get("masic_quantize_fwd", 0) == 0, n
    assert n.get("masic_nchw_to_f16k_view_op", 0) == 0 and n.get("masic_nchw_to_f16k_view", 0) == 0, n
    assert n.get("masic_conv2d_f16k_out_fwd", 0) == 2, n
    assert conversions == 0, n
