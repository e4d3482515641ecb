"""GPU parity tests (-m gpu) of the backward kernels: every differentiable node of the training graph against
torch autograd on the CPU oracle (same seeded inputs), then the whole training step against the gradient goldens the
reference produced (tests/golden/hsic_tiny.npz: d loss / d parameter for all 166 parameters)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hsic_oracle as O
from tests.util import assert_close, golden_state_dict, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = 2e-4


def _rand(*shape, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(size=shape) * scale).astype(np.float32))


CONV_BWD_CASES = [
    # name,        B, Cin, H,  W,  Cout, k, s, transposed, masked, act
    ("conv5s2",    2, 128, 32, 64, 128,  5, 2, False, False, 0),
    ("conv5s2_in3", 2, 3,  64, 96, 128,  5, 2, False, False, 0),
    ("conv5s1",    2, 192, 16, 24, 128,  5, 1, False, False, 1),
    ("conv3s1",    2, 288, 16, 24, 384,  3, 1, False, False, 0),
    ("conv1x1",    2, 768, 8,  12, 960,  1, 1, False, False, 2),
    ("deconv1x1",  2, 768, 8,  12, 1152, 1, 1, True,  False, 1),
    ("deconv5s2",  2, 192, 8,  12, 128,  5, 2, True,  False, 2),
    ("deconv_to3", 2, 128, 16, 24, 3,    5, 2, True,  False, 0),
    ("masked5",    2, 192, 16, 24, 384,  5, 1, False, True,  0),
    ("conv6to3",   2, 6,   32, 48, 3,    5, 1, False, False, 0),
    ("deconv6to3", 2, 6,   32, 48, 3,    5, 1, True,  False, 0),
    ("conv6to3_big", 1, 6, 260, 1400, 3, 5, 1, False, False, 0),      # conv_wgrad_small_s1: ragged tiles, several tiles per workgroup
    ("deconv6to3_big", 2, 6, 256, 704, 3, 5, 1, True, False, 0),
    ("m2w_3x3s2",  2, 3,   32, 48, 6,    3, 2, False, False, 1),
    ("ragged",     1, 20,  18, 36, 72,   5, 2, False, False, 2),
]


@pytest.mark.parametrize("case", CONV_BWD_CASES, ids=[c[0] for c in CONV_BWD_CASES])
def test_conv_backward(case):
    from masic_amd import autograd as A
    from masic_amd import nn as mnn
    from compressai.layers import MaskedConv2d
    name, B, Cin, H, W, Cout, k, s, tr, masked, act = case
    if masked:
        mod = MaskedConv2d(Cin, Cout, kernel_size=k, padding=k // 2, stride=s)
    elif tr:
        mod = mnn.ConvTranspose2d(Cin, Cout, k, stride=s, padding=k // 2, output_padding=s - 1)
    else:
        mod = mnn.Conv2d(Cin, Cout, k, stride=s, padding=k // 2)
    w = _rand(*mod.weight.shape, seed=2, scale=(2.0 / (Cin * k * k)) ** 0.5)
    b = _rand(Cout, seed=3, scale=0.1)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    mod = mod.to(DEV)
    x = _rand(B, Cin, H, W, seed=1, scale=2.0)
    # CPU reference through autograd
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    weff = O.masked_weight(wr) if masked else wr
    yr = (F.conv_transpose2d(xr, weff, br, stride=s, padding=k // 2, output_padding=s - 1) if tr
          else F.conv2d(xr, weff, br, stride=s, padding=k // 2))
    yr = {0: lambda t: t, 1: F.relu, 2: F.leaky_relu}[act](yr)
    go = _rand(*yr.shape, seed=4)
    yr.backward(go)
    xd = x.to(DEV).requires_grad_(True)
    y = A.conv(mod, xd, act)
    assert_close(y, yr, name + ":fwd")
    y.backward(go.to(DEV))
    assert_close(xd.grad, xr.grad, name + ":dx", GTOL)
    assert_close(mod.weight.grad, wr.grad, name + ":dw", GTOL)
    assert_close(mod.bias.grad, br.grad, name + ":db", GTOL)


@pytest.mark.parametrize("case", [c for c in CONV_BWD_CASES if c[0] in ("conv5s2", "conv5s1", "conv3s1", "deconv5s2", "masked5", "conv1x1", "deconv1x1", "ragged", "deconv_to3")],
                         ids=lambda c: c[0])
def test_conv_backward_bf16_mode(case):
    """set_precision("bf16"): forward, input gradient and weight gradient with bf16 operands / float32 accumulation, against
    float32 autograd at bf16 operand noise (2e-2 of each tensor's peak)."""
    from masic_amd import autograd as A
    from masic_amd import nn as mnn
    from compressai.layers import MaskedConv2d
    name, B, Cin, H, W, Cout, k, s, tr, masked, act = case
    act = 0            # an activation mask taken from a bf16-rounded output flips near zero: not a property of the gradient kernels
    if masked:
        mod = MaskedConv2d(Cin, Cout, kernel_size=k, padding=k // 2, stride=s)
    elif tr:
        mod = mnn.ConvTranspose2d(Cin, Cout, k, stride=s, padding=k // 2, output_padding=s - 1)
    else:
        mod = mnn.Conv2d(Cin, Cout, k, stride=s, padding=k // 2)
    w = _rand(*mod.weight.shape, seed=2, scale=(2.0 / (Cin * k * k)) ** 0.5)
    b = _rand(Cout, seed=3, scale=0.1)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    mod = mod.to(DEV)
    x = _rand(B, Cin, H, W, seed=1, scale=2.0)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    weff = O.masked_weight(wr) if masked else wr
    yr = (F.conv_transpose2d(xr, weff, b, stride=s, padding=k // 2, output_padding=s - 1) if tr else F.conv2d(xr, weff, b, stride=s, padding=k // 2))
    yr = {0: lambda t: t, 1: F.relu, 2: F.leaky_relu}[act](yr)
    go = _rand(*yr.shape, seed=4)
    yr.backward(go)
    mnn.set_precision("bf16")
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = A.conv(mod, xd, act)
        y.backward(go.to(DEV))
    finally:
        mnn.set_precision("f32")
    for nm, got, ref in (("y", y, yr), ("dx", xd.grad, xr.grad), ("dw", mod.weight.grad, wr.grad)):
        peak = float(ref.abs().max())
        err = float((got.detach().cpu() - ref.detach()).abs().max())
        assert err <= 2e-2 * peak, (name, nm, err, peak)


WGRAD_BF16_CASES = CONV_BWD_CASES + [          # 1x1 layers with 64 | H W take the GEMM-shaped kernel
    ("conv1x1_gemm",   2, 768, 16, 16, 960,  1, 1, False, False, 0),
    ("deconv1x1_gemm", 2, 200, 8,  16, 1152, 1, 1, True,  False, 0),
    ("conv1x1_gemm_r", 3, 72,  8,  8,  40,   1, 1, False, False, 0),
]


@pytest.mark.parametrize("case", WGRAD_BF16_CASES, ids=[c[0] for c in WGRAD_BF16_CASES])
def test_conv_wgrad_bf16_operands(case):
    """The bf16-operand weight gradient (training in the bf16 mode) == the float32 kernel run on bf16-rounded operands:
    rounding happens once per operand and every product / the accumulation stay float32, so the two agree to float32
    summation-order noise; against the unrounded float32 gradient the difference is bf16 rounding noise (<= 1e-2 of the peak)."""
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16, PREC_F32
    name, B, Cin, H, W, Cout, k, s, tr, masked, act = case
    pad = k // 2
    x = _rand(B, Cin, H, W, seed=11, scale=2.0).to(DEV)
    d32 = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, pad, transposed=tr, prec=PREC_F32)
    d16 = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, pad, transposed=tr, prec=PREC_BF16)
    dy = _rand(B, Cout, d32.Ho, d32.Wo, seed=12).to(DEV)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    got = ops.conv2d_wgrad(x, dy, d16, wshape)
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float32)
    want = ops.conv2d_wgrad(rnd(x), rnd(dy), d32, wshape)
    full = ops.conv2d_wgrad(x, dy, d32, wshape)
    peak = float(full.abs().max())
    assert float((got - want).abs().max()) <= 2e-5 * peak + 1e-6, name
    assert float((got - full).abs().max()) <= 1e-2 * peak, name


# conv_wgrad_packed_f32<2, bf16, det> (5 .. 8 column tiles of (tap, fine-side channel) pairs: 5x5 kernels with 6 .. 8 fine-side channels).
# A list of its own: tests/test_gpu_determinism.py records digests over CONV_BWD_CASES.  tests/test_cpu_conv_rows.py holds the cases
# to the four instantiations.
WGRAD_PACKED2_CASES = [
    # name,          B, Cin, H,  W,  Cout, k, s, transposed
    ("pre_conv_w50", 2, 6,   32, 50, 3,    5, 1, False),      # pre_conv at a width that is no multiple of 4 (else conv_wgrad_small_s1)
    ("conv6to128",   2, 6,   36, 44, 128,  5, 2, False),
    ("deconv128to6", 2, 128, 18, 22, 6,    5, 2, True),
    ("ragged_b1",    1, 7,   19, 37, 70,   5, 2, False),      # one image, odd sizes, 64 + 6 coarse-side channels, 7 fine-side ones
]


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", WGRAD_PACKED2_CASES, ids=[c[0] for c in WGRAD_PACKED2_CASES])
def test_conv_wgrad_packed2(case, prec, det):
    """ops.conv2d_wgrad on the packed kernel's wider instantiations against float64 autograd, as tests/test_gpu_determinism.py::
    test_conv2d_wgrad_det: GTOL for float32 operands, 2e-5 of the peak + 1e-6 on the bf16-rounded operands for bf16; the deterministic
    form is run twice and gives the same bits."""
    import contextlib
    from masic_amd import ops
    from masic_amd._lib import PREC_BF16, PREC_F32
    from masic_amd.determinism import deterministic
    from tests.test_gpu_determinism import _wgrad_ref      # float64 autograd
    name, B, Cin, H, W, Cout, k, s, tr = case
    d = ops.make_conv_desc(B, Cin, H, W, Cout, k, k, s, k // 2, transposed=tr, prec=PREC_BF16 if prec == "bf16" else PREC_F32)
    x = _rand(B, Cin, H, W, seed=11, scale=2.0)
    dy = _rand(B, Cout, d.Ho, d.Wo, seed=12)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    xd, dyd = x.to(DEV), dy.to(DEV)
    with (deterministic() if det else contextlib.nullcontext()):
        got = ops.conv2d_wgrad(xd, dyd, d, wshape)
        if det:
            assert torch.equal(ops.conv2d_wgrad(xd, dyd, d, wshape), got), name + ": two deterministic calls differ"
    if prec == "bf16":
        want = _wgrad_ref(x.bfloat16().float(), dy.bfloat16().float(), k, s, tr)
        err, peak = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
        print(f"{name} {prec} det={det}: |error| {err:.3e}, peak {peak:.3e}, relative {err / peak:.3e}")
        assert err <= 2e-5 * peak + 1e-6, name
    else:
        e = assert_close(got, _wgrad_ref(x, dy, k, s, tr), name + ":dw", GTOL)
        print(f"{name} {prec} det={det}: relative error {e:.3e}")


@pytest.mark.parametrize("C,H,W,inverse", [(128, 16, 32, False), (128, 8, 8, True), (3, 32, 48, False), (3, 24, 40, True), (16, 8, 12, False)])
def test_gdn_backward(C, H, W, inverse):
    from compressai.layers import GDN
    from masic_amd import synth
    rs = np.random.RandomState(C + H)
    beta = synth.synth_tensor("g.beta", (C,), rs)
    gamma = synth.synth_tensor("g.gamma", (C, C), rs)
    gamma[0, 1] = 1e-7
    gamma[1, 0] = 1e-7
    beta[0] = 1e-5
    x = _rand(2, C, H, W, seed=10, scale=3.0)
    xr, br, gr = x.clone().requires_grad_(True), beta.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    yr = O.gdn(xr, br, gr, inverse=inverse)
    go = _rand(*yr.shape, seed=11)
    yr.backward(go)
    m = GDN(C, inverse=inverse)
    with torch.no_grad():
        m.beta.copy_(beta)
        m.gamma.copy_(gamma)
    m = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    y.backward(go.to(DEV))
    assert_close(xd.grad, xr.grad, "gdn:dx", GTOL)
    assert_close(m.gamma.grad, gr.grad, "gdn:dgamma", GTOL)
    assert_close(m.beta.grad, br.grad, "gdn:dbeta", GTOL)


@pytest.mark.parametrize("B,H,W,inverse", [(2, 16, 32, False), (2, 8, 8, True), (3, 5, 7, False), (2, 24, 40, True), (1, 64, 64, False)])
def test_gdn_backward_fused_bf16(B, H, W, inverse):
    """masic_gdn_bwd_fused (the bf16-operand training mode) against (1) a float32 emulation with the kernel's roundings --
    gamma^, x^2 and t rounded to bf16 where they enter a contraction, everything else float32 -- tight, and (2) torch
    autograd on the CPU oracle's GDN, at bf16 operand noise.  Ragged pixel counts (105 pixels: a partial tile whose 32-pixel
    runs cross images) and stored parameters below their bound (the LowerBound rule) included."""
    from masic_amd import ops, synth
    C = 128
    rs = np.random.RandomState(B * H + W)
    beta = synth.synth_tensor("g.beta", (C,), rs)
    gamma = synth.synth_tensor("g.gamma", (C, C), rs)
    gamma[0, 1] = 1e-7
    gamma[1, 0] = 1e-7
    beta[0] = 1e-5
    x = _rand(B, C, H, W, seed=10, scale=3.0)
    go = _rand(B, C, H, W, seed=11)
    gx, gb, gg = ops.gdn_bwd_fused(x.to(DEV), go.to(DEV), beta.to(DEV), gamma.to(DEV), inverse=inverse, beta_min=1e-6)
    gx, gb, gg = gx.cpu(), gb.cpu(), gg.cpu()
    # (2) autograd
    xr, br, gr = x.clone().requires_grad_(True), beta.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    O.gdn(xr, br, gr, inverse=inverse).backward(go)
    # (1) emulation
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float32)
    ped = torch.tensor(2.0 ** -36, dtype=torch.float32)
    b_bound = torch.tensor((1e-6 + 2.0 ** -36) ** 0.5, dtype=torch.float32)
    g_bound = torch.tensor((2.0 ** -36) ** 0.5, dtype=torch.float32)
    bh = torch.maximum(beta, b_bound) ** 2 - ped
    gh = rnd(torch.maximum(gamma, g_bound) ** 2 - ped)
    xf = x.permute(1, 0, 2, 3).reshape(C, -1).double()
    gf = go.permute(1, 0, 2, 3).reshape(C, -1).double()
    x2 = rnd((xf * xf).float()).double()
    n = bh.double()[:, None] + gh.double() @ x2
    if inverse:
        sv, tv = gf * n.sqrt(), 0.5 * gf * xf / n.sqrt()
    else:
        sv, tv = gf / n.sqrt(), -0.5 * gf * xf / (n * n.sqrt())
    tb = rnd(tv.float()).double()
    dx = (sv + 2.0 * xf * (gh.double().t() @ tb)).float().reshape(C, B, H, W).permute(1, 0, 2, 3)
    dgh, dbh = (tb @ x2.t()).float(), tb.sum(1).float()
    rule = lambda d, p, bound: torch.where((p >= bound) | (d * 2 * torch.maximum(p, bound) < 0), d * 2 * torch.maximum(p, bound), torch.zeros_like(d))
    want = (dx, rule(dbh, beta, b_bound), rule(dgh, gamma, g_bound))
    for name, got, emu, ref in zip(("dx", "dbeta", "dgamma"), (gx, gb, gg), want, (xr.grad, br.grad, gr.grad)):
        peak = float(ref.abs().max())
        assert float((got - emu).abs().max()) <= 2e-3 * peak, (name, "emulation", float((got - emu).abs().max()), peak)
        assert float((got - ref).abs().max()) <= 3e-2 * peak, (name, "autograd", float((got - ref).abs().max()), peak)


@pytest.mark.parametrize("B,H,W,inverse", [(2, 16, 32, False), (3, 5, 7, True), (1, 64, 64, False)])
def test_gdn_backward_fused_f16k_operands(B, H, W, inverse):
    """masic_gdn_bwd_fused_ex: x and / or g handed over as F16K bf16, dx also written as F16K, and the per-channel sums of dx (the
    bias gradient of the convolution in front of the GDN) -- against masic_gdn_bwd_fused (pinned by the test above) on the same
    bf16-representable values: the operands are identical then, so dx, d beta, d gamma must agree bit for bit for all four operand
    combinations; the F16K dx is the bf16 rounding of the float32 dx; the sums equal a float64 channel sum of dx to float32 accuracy."""
    from masic_amd import ops, synth
    C = 128
    rs = np.random.RandomState(7 * B + H)
    beta = synth.synth_tensor("g.beta", (C,), rs).to(DEV)
    gamma = synth.synth_tensor("g.gamma", (C, C), rs).to(DEV)
    x = _rand(B, C, H, W, seed=20, scale=3.0).bfloat16().float().to(DEV)
    go = _rand(B, C, H, W, seed=21).bfloat16().float().to(DEV)
    gx0, gb0, gg0 = ops.gdn_bwd_fused(x, go, beta, gamma, inverse=inverse, beta_min=1e-6)
    x16, g16 = ops.nchw_to_f16k(x), ops.nchw_to_f16k(go)
    shape = (B, C, H, W)
    for xa, ga in ((x16, go), (x, g16), (x16, g16), (x, go)):
        gx, gx16, gs, gb, gg = ops.gdn_bwd_fused_ex(xa, ga, shape, beta, gamma, inverse=inverse, beta_min=1e-6, want_nchw=True, want_f16k=True, want_sum=True)
        assert torch.equal(gx, gx0) and torch.equal(gb, gb0) and torch.equal(gg, gg0), (xa.dtype, ga.dtype)
        assert torch.equal(ops.f16k_to_nchw_dev(gx16, B, C, H, W), gx0.bfloat16().float())
        want = gx0.double().sum((0, 2, 3))
        assert float((gs.double() - want).abs().max()) <= 1e-5 * float(gx0.abs().sum((0, 2, 3)).max()), "channel sums of dx"
    gx, gx16, gs, gb, gg = ops.gdn_bwd_fused_ex(x16, g16, shape, beta, gamma, inverse=inverse, beta_min=1e-6, want_nchw=False, want_f16k=True, want_sum=False)
    assert gx is None and gs is None and torch.equal(ops.f16k_to_nchw_dev(gx16, B, C, H, W), gx0.bfloat16().float()) and torch.equal(gg, gg0)
    with pytest.raises(RuntimeError):
        ops.gdn_bwd_fused_ex(x16, g16, shape, beta, gamma, want_nchw=False, want_f16k=False)


@pytest.mark.parametrize("B,Cout,Cin,H,W", [(2, 1152, 768, 16, 24), (3, 96, 160, 7, 9), (1, 768, 960, 32, 32), (2, 32, 48, 5, 3)])
def test_gemm_wgrad_f16k_1x1_layers(B, Cout, Cin, H, W):
    """masic_gemm_wgrad_bias_f16k -- the weight gradient of the 1x1 layers of the entropy-parameter stacks (reference MASIC.py:330-468) from
    F16K operands -- against a float64 contraction of the bf16-rounded operands the kernel sees (ragged pixel counts: partial 64-pixel
    tiles; channel counts that are not multiples of 128: partial output tiles), for the Conv2d orientation [Cout, Cin] and the
    ConvTranspose2d(k=1) orientation [Cin, Cout]; and through ConvFn in the bf16 mode against the float32 NCHW kernel's result."""
    from compressai.models.utils import conv, deconv
    from masic_amd import autograd as ag, nn as mnn, ops
    x = _rand(B, Cin, H, W, seed=1, scale=1.5)
    dy = _rand(B, Cout, H, W, seed=2)
    q = lambda t: t.bfloat16().double()
    want = torch.einsum("bohw,bchw->oc", q(dy), q(x))
    x16, g16 = ops.nchw_to_f16k(x.to(DEV)), ops.nchw_to_f16k(dy.to(DEV))
    got = ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W).cpu().double()
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()), "Conv2d orientation"
    got_t = ops.gemm_wgrad_f16k(x16, g16, B, Cin, Cout, H * W).cpu().double()
    assert float((got_t - want.t()).abs().max()) <= 2e-5 * float(want.abs().max()), "ConvTranspose2d orientation"
    # the bias gradient (channel sums of dy) from the same launch: dy as the rows operand (Conv2d), as the columns operand (transposed)
    bsum = q(dy).sum(dim=(0, 2, 3))
    dw1, db1 = ops.gemm_wgrad_f16k(g16, x16, B, Cout, Cin, H * W, bias_of=1)
    dw2, db2 = ops.gemm_wgrad_f16k(x16, g16, B, Cin, Cout, H * W, bias_of=2)
    assert float((dw1.cpu().double() - want).abs().max()) <= 2e-5 * float(want.abs().max())
    assert float((dw2.cpu().double() - want.t()).abs().max()) <= 2e-5 * float(want.abs().max())
    for db in (db1, db2):
        assert db.shape == (Cout,)
        assert float((db.cpu().double() - bsum).abs().max()) <= 2e-5 * float(bsum.abs().max()) + 1e-4, "bias gradient"
    if Cin % 32 == 0 and Cout % 32 == 0:
        mnn.set_precision("bf16")
        try:
            for mod, shape in ((conv(Cin, Cout, kernel_size=1, stride=1), (Cout, Cin, 1, 1)), (deconv(Cin, Cout, kernel_size=1, stride=1), (Cin, Cout, 1, 1))):
                mod = mod.to(DEV)
                xd = x.to(DEV).requires_grad_(True)
                y = ag.conv(mod, xd, ops.ACT_LEAKY)
                y.backward(dy.to(DEV))
                new = mod.weight.grad.clone()
                mod.weight.grad = None
                xd2 = x.to(DEV).requires_grad_(True)
                old_flag, ag._WGRAD1_F16K = ag._WGRAD1_F16K, False
                try:
                    ag.conv(mod, xd2, ops.ACT_LEAKY).backward(dy.to(DEV))
                finally:
                    ag._WGRAD1_F16K = old_flag
                assert tuple(new.shape) == shape
                assert_close(new, mod.weight.grad.cpu(), f"1x1 weight gradient through ConvFn {shape}", 2e-5)
                assert torch.equal(xd.grad, xd2.grad)
        finally:
            mnn.set_precision("f32")


@pytest.mark.parametrize("which", ["y1", "y2"])
def test_gmm_heads_fused_node_vs_per_layer_nodes(which, monkeypatch):
    """bf16-mode training: the entropy-parameter head (reference MASIC.py:330-468, nine 1x1 layers) as ONE autograd node on F16K
    (masic_amd.autograd.GmmHeadsFn: grouped GEMMs forward and for the input gradients, F16K weight gradients) against one ConvFn per
    layer: identical forward results (same GEMM kernel, same roundings), gradients of all 18 parameters and of the input within the
    bf16 operand noise of the two orders of rounding (relative L2 error <= 1 %, cosine >= 0.9999)."""
    import MASIC
    from masic_amd import autograd as ag, nn as mnn, synth
    N, M, K = 32, 32, 5
    cls = MASIC.gmm_hyper_y1_same_resolution if which == "y1" else MASIC.gmm_hyper_y2_same_resolution
    head = cls(N, M, K)
    head.load_state_dict(synth.synth_state_dict(head.state_dict(), seed=8))
    head = head.to(DEV).train()
    B, H, W = 2, 12, 20
    x0 = torch.randn(B, (4 if which == "y1" else 5) * M, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    gs = [torch.randn(B, M * K, H, W, generator=torch.Generator().manual_seed(10 + i)).to(DEV) for i in range(3)]
    mnn.set_precision("bf16")
    res = {}
    try:
        for fused in (False, True):
            monkeypatch.setattr(ag, "_GMM_HEADS_FN", fused)
            head.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            assert ag.gmm_heads_supported(head, x) == fused
            outs = head.heads(x)
            torch.autograd.backward(outs, gs)
            res[fused] = ([o.detach().clone() for o in outs], x.grad.clone(), {n: p.grad.clone() for n, p in head.named_parameters()})
    finally:
        mnn.set_precision("f32")
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b), "forward: the same GEMM kernel on the same operands"

    def check(name, a, b):
        a, b = a.double().flatten(), b.double().flatten()
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
        assert rel <= 1e-2 and cos >= 0.9999, (name, rel, cos)
    check("input gradient", res[True][1], res[False][1])
    assert len(res[True][2]) == 18
    for n in res[False][2]:
        check(n, res[True][2][n], res[False][2][n])


@pytest.mark.parametrize("transposed,B,Cin,Cout,H,W", [(False, 2, 128, 128, 32, 48), (True, 2, 128, 128, 16, 24), (False, 1, 128, 192, 64, 64), (True, 3, 192, 128, 8, 8)])
def test_conv_wgrad_bf16_nchw_operands(transposed, B, Cin, Cout, H, W):
    """masic_conv2d_wgrad_bf16in: the 5x5 stride-2 weight-gradient kernel reading bf16 NCHW operands (what masic_gdn_bwd_fused_ex2 and
    masic_f16k_to_nchw_bf16 write) must equal the float32-operand call on the same bf16-representable values (the float32 form rounds to
    bf16 on its way into LDS: identical operands, identical arithmetic) -- up to the order of the float atomics.  Plus the two producers:
    f16k_to_nchw(bf16=True) is exact, gdn_bwd_fused_ex(want_b16=True) is the bf16 rounding of its float32 output."""
    from masic_amd import ops, synth, _lib
    x = _rand(B, Cin, H, W, seed=3).bfloat16()
    d = ops.make_conv_desc(B, Cin, H, W, Cout, 5, 5, 2, 2, transposed=transposed, prec=_lib.PREC_BF16)
    dy = _rand(B, Cout, d.Ho, d.Wo, seed=4).bfloat16()
    assert ops.conv2d_wgrad_b16_supported(d)
    shape = (Cin, Cout, 5, 5) if transposed else (Cout, Cin, 5, 5)
    ref = ops.conv2d_wgrad(x.float().to(DEV), dy.float().to(DEV), d, shape)
    got = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), d, shape)
    assert_close(got, ref.cpu(), "bf16 NCHW operands vs float32 operands", 1e-5)
    with pytest.raises(RuntimeError):
        ops.conv2d_wgrad(x.to(DEV), dy.float().to(DEV), d, shape)                       # mixed operand types
    d3 = ops.make_conv_desc(B, Cin, H, W, Cout, 3, 3, 1, 1, prec=_lib.PREC_BF16)
    assert not ops.conv2d_wgrad_b16_supported(d3)
    if Cin == 128 and not transposed:
        x16 = ops.nchw_to_f16k(x.float().to(DEV))
        assert torch.equal(ops.f16k_to_nchw_dev(x16, B, Cin, H, W, bf16=True).cpu(), x)
        rs = np.random.RandomState(5)
        beta, gamma = synth.synth_tensor("g.beta", (128,), rs).to(DEV), synth.synth_tensor("g.gamma", (128, 128), rs).to(DEV)
        g = _rand(B, 128, H, W, seed=6).to(DEV)
        a = ops.gdn_bwd_fused_ex(x16, g, (B, 128, H, W), beta, gamma, want_nchw=True, want_f16k=False, want_sum=False)
        b = ops.gdn_bwd_fused_ex(x16, g, (B, 128, H, W), beta, gamma, want_nchw=True, want_f16k=True, want_sum=True, want_b16=True)
        assert b[0].dtype == torch.bfloat16 and torch.equal(b[0], a[0].bfloat16()) and torch.equal(b[3], a[3]) and torch.equal(b[4], a[4])


@pytest.mark.parametrize("B,Hc,Wc", [(2, 16, 24), (1, 20, 36), (3, 64, 64), (1, 5, 7)])
def test_picture_end_weight_gradients_f16k_operand(B, Hc, Wc):
    """ops.pic_wgrad_f16k: weight gradients of g_a_conv1 = Conv2d(3 -> 128, k5, s2) and g_s_conv4 = ConvTranspose2d(128 -> 3, k5, s2)
    (reference MASIC.py:515, :550) from the 128-channel operand in F16K and the 3-channel one in float32 NCHW, against torch autograd on
    the bf16-rounded operands (float32 accumulation either way; ragged k-tiles, tiles that straddle image rows)."""
    from masic_amd import ops
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float32)
    p = _rand(B, 128, Hc, Wc, seed=31)
    q = _rand(B, 3, 2 * Hc, 2 * Wc, seed=32, scale=2.0)
    p16 = ops.nchw_to_f16k(p.to(DEV))
    got = ops.pic_wgrad_f16k(p16, q.to(DEV), B, Hc, Wc).cpu()
    # Conv2d(3 -> 128): x = q, dy = p
    w = torch.zeros(128, 3, 5, 5, requires_grad=True)
    F.conv2d(rnd(q), w, None, stride=2, padding=2).backward(rnd(p))
    peak = float(w.grad.abs().max())
    assert float((got.view(128, 3, 5, 5) - w.grad).abs().max()) <= 2e-5 * peak, "conv 3 -> 128"
    # ConvTranspose2d(128 -> 3): x = p, dy = q
    wt = torch.zeros(128, 3, 5, 5, requires_grad=True)
    F.conv_transpose2d(rnd(p), wt, None, stride=2, padding=2, output_padding=1).backward(rnd(q))
    assert float((got.view(128, 3, 5, 5) - wt.grad).abs().max()) <= 2e-5 * float(wt.grad.abs().max()), "deconv 128 -> 3"
    # a channel view of a wider tensor
    q6 = torch.cat([_rand(B, 2, 2 * Hc, 2 * Wc, seed=33), q, _rand(B, 1, 2 * Hc, 2 * Wc, seed=34)], dim=1)
    got6 = ops.pic_wgrad_f16k(p16, q6.to(DEV), B, Hc, Wc, q_coff=2).cpu()
    assert torch.equal(got6, got)


def test_picture_end_input_gradients_f16k_forms():
    """bf16 mode, input gradients of the two picture-end layers (reference MASIC.py:515 g_a_conv1 = Conv2d(3 -> 128, k5, s2), :550
    g_s_conv4 = ConvTranspose2d(128 -> 3, k5, s2)) on the F16K kernels -- the depth-to-space transposed convolution and the
    first-layer kernel without its GDN -- against torch's float32 operators on the bf16-rounded operands the kernels see."""
    from compressai.models.utils import conv, deconv
    from masic_amd import autograd as ag, nn as mnn, ops
    from masic_amd.f16k import F16K
    q = lambda t: t.bfloat16().float()
    B, H, W = 2, 48, 80
    mnn.set_precision("bf16")
    try:
        ca = conv(3, 128).to(DEV)                                   # dx = ConvTranspose2d(128 -> 3)(dy)
        x = _rand(B, 3, H, W, seed=1).to(DEV)
        dy = _rand(B, 128, H // 2, W // 2, seed=2)
        want = F.conv_transpose2d(q(dy), q(ca.weight.detach().cpu()), None, stride=2, padding=2, output_padding=1)
        gx, gw, gb = ag.conv_backward(ca, x, ca.weight, None, dy.to(DEV), ops.ACT_NONE, need_gw=False, need_gb=False, g_f16k=F16K.from_nchw(dy.to(DEV)))
        assert gx.dtype == torch.float32 and gw is None and gb is None
        assert_close(gx, want, "dx of Conv2d(3->128) (depth-to-space form)", 2e-3)
        dt = deconv(128, 3).to(DEV)                                 # dx = Conv2d(3 -> 128)(dy)
        xin = _rand(B, 128, H // 2, W // 2, seed=3).to(DEV)
        dy = _rand(B, 3, H, W, seed=4)
        want = F.conv2d(q(dy), q(dt.weight.detach().cpu()), None, stride=2, padding=2)
        gx, _, _ = ag.conv_backward(dt, xin, dt.weight, None, dy.to(DEV), ops.ACT_NONE, need_gw=False, need_gb=False, gx_f16k=True)
        assert isinstance(gx, F16K) and gx.buf.dtype == torch.int16 and gx.shape == (B, 128, H // 2, W // 2) and gx.whole
        assert_close(ops.f16k_to_nchw_dev(gx.buf, B, 128, H // 2, W // 2), want, "dx of ConvTranspose2d(128->3) (first-layer kernel, no GDN)", 2 ** -8)
    finally:
        mnn.set_precision("f32")
    # the one-launch weight relayout equals the torch-op form
    w, b = _rand(128, 3, 5, 5, seed=5).to(DEV), _rand(3, seed=6).to(DEV)
    w1, b1 = ops.deconv_s2_as_conv_weight(w, b)
    w2, b2 = ops.deconv_s2_as_conv_weight_dev(w, b)
    assert torch.equal(w1, w2) and torch.equal(b1, b2)


@pytest.mark.parametrize("nliks", [4, 0, 2])
def test_rate_distortion_criterion_fused_launches(nliks, monkeypatch):
    """RateDistortionFn (newtrain_codec_real.py:73-87; 0 likelihood tensors: the CQE stage's distortion, newtrain_cqe_real.py:66-96) as
    two launches forward and one backward (masic_rd_loss / masic_rd_loss_bwd) against the chain of six reductions, torch scalar
    arithmetic and per-tensor elementwise kernels it replaces: the same summation order, so every value and gradient bit for bit."""
    from masic_amd import autograd as A
    x1, x2 = _rand(2, 3, 40, 56, seed=1).to(DEV), _rand(2, 3, 40, 56, seed=2).to(DEV)
    shapes = [(2, 192, 5, 7), (2, 192, 5, 7), (2, 128, 2, 2), (2, 128, 2, 2)][:nliks]
    res = {}
    for fused in (False, True):
        monkeypatch.setattr(A, "_RD_FUSED", fused)
        xh1 = (x1 + 0.05 * _rand(2, 3, 40, 56, seed=3).to(DEV)).requires_grad_(True)
        xh2 = (x2 + 0.05 * _rand(2, 3, 40, 56, seed=4).to(DEV)).requires_grad_(True)
        liks = [(_rand(*sh, seed=10 + i).to(DEV).abs() * 0.3 + 1e-3).requires_grad_(True) for i, sh in enumerate(shapes)]
        out = A.RateDistortionFn.apply(0.01, x1, x2, xh1, xh2, *liks)
        (out[0] * 3.0).backward()
        res[fused] = [o.detach().clone() for o in out] + [xh1.grad, xh2.grad] + [l.grad for l in liks]
    assert len(res[True]) == len(res[False]) == 4 + nliks + 2 + nliks
    for got, want in zip(res[True], res[False]):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want)
    assert float(res[True][0]) > 0


def test_entropy_bottleneck_backward_and_aux():
    from compressai.entropy_models import EntropyBottleneck
    from masic_amd import synth
    C, B, H, W = 24, 3, 4, 6
    eb = EntropyBottleneck(C)
    sd = synth.synth_state_dict({k: v for k, v in eb.state_dict().items()}, seed=5)
    eb.load_state_dict(sd)
    z = _rand(B, C, H, W, seed=11, scale=4.0)
    noise = torch.from_numpy(np.random.RandomState(12).uniform(-0.5, 0.5, size=(C, 1, H * W * B)).astype(np.float32))
    pn = [n for n, _ in eb.named_parameters()]
    sdr = {"eb." + k: (v.clone().requires_grad_(True) if k in pn else v) for k, v in sd.items()}
    zr = z.clone().requires_grad_(True)
    zh, lik = O.entropy_bottleneck(zr, sdr, "eb", training=True, noise=noise)
    g1, g2 = _rand(*z.shape, seed=13), _rand(*z.shape, seed=14)
    (zh * g1).sum().backward(retain_graph=True)
    (lik * g2).sum().backward()
    eb = eb.to(DEV).train()
    eb._get_noise_cached = lambda x: noise.to(DEV).reshape(x.shape).contiguous()
    zd = z.to(DEV).requires_grad_(True)
    zh_d, lik_d = eb(zd)
    ((zh_d * g1.to(DEV)).sum() + (lik_d * g2.to(DEV)).sum()).backward()
    assert_close(zd.grad, zr.grad, "eb:dz", GTOL)
    for n, p in eb.named_parameters():
        if n == "quantiles":
            continue
        assert_close(p.grad, sdr["eb." + n].grad, "eb:d" + n, GTOL)
    # aux loss: gradient w.r.t. the quantiles only
    for p in eb.parameters():
        p.grad = None
    aux = eb.loss()
    aux.backward()
    sq = {k: v.detach().clone() for k, v in sdr.items()}
    sq["eb.quantiles"].requires_grad_(True)
    O.eb_aux_loss(sq, "eb").backward()
    assert_close(eb.quantiles.grad, sq["eb.quantiles"].grad, "eb:aux dq", GTOL)
    assert all(p.grad is None for n, p in eb.named_parameters() if n != "quantiles")


def test_weight_packs_refreshed_by_one_launch_equal_single_packs():
    """ops.StreamPacks: inside a training step (ops.batched_packs) the conv_f16k weight packs of all registered layers -- forward and
    input-gradient orientation -- are refreshed by ONE launch when the parameters changed; every refreshed buffer must hold exactly
    what masic_conv_f16k_pack_weight writes for that layer, stale entries must be repacked after an optimizer step, and masked layers
    (which zero taps in place right before packing, without a version bump) must not be registered."""
    import ctypes
    import MASIC
    from masic_amd import nn as mnn, ops, synth
    from masic_amd.ops import lib
    from masic_amd.train import make_optimizers, train_step
    net = MASIC.HSIC(128, 32, 3)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=12))
    net = net.to(DEV).train()
    x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, 64, 64, seed=12))
    mnn.set_precision("bf16")
    ops._STREAM_PACKS.clear()        # (entries of earlier tests' models would dilute the "most entries are stale" rule)
    try:
        opt, aopt = make_optimizers(net)
        for _ in range(2):
            train_step(net, opt, aopt, x1, x2, hm, 0.01)
        sp = ops._stream_packs(x1.device)
        mine = {k: e for k, e in sp.entries.items() if any(e[0].data_ptr() == p.data_ptr() for p in net.parameters())}
        assert len(mine) >= 12                                   # analysis / synthesis / hyper layers, both orientations
        assert all(e[1].masked == 0 for e in mine.values())
        assert all(e[3] != e[0]._version for e in mine.values())  # the optimizer stepped: everything is stale
        with ops.batched_packs():
            net(x1, x2, hm)                                      # the first request refreshes every entry
        for key, e in mine.items():
            assert e[3] == e[0]._version, key
            ref = torch.empty_like(e[2])
            ops.check(lib.masic_conv_f16k_pack_weight(e[0].data_ptr(), ref.data_ptr(), ctypes.byref(e[1]), None), "pack")
            torch.cuda.synchronize()
            assert torch.equal(ref, e[2]), key
    finally:
        mnn.set_precision("f32")


def test_aux_step_two_launches_equal_autograd(monkeypatch):
    """train.aux_backward: the sum of EntropyBottleneck.loss() over HSIC's two bottlenecks and its gradient (newtrain_codec_real.py:
    143-144) written by two launches, against model.aux_loss().backward(): the same gradients bit for bit (both run the same tape),
    the loss to float32 summation noise; a second call accumulates into quantiles.grad as autograd does."""
    import MASIC
    from masic_amd import synth, train
    net = MASIC.HSIC(16, 32, 3)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=5))
    net = net.to(DEV).train()
    ebs = (net.entropy_bottleneck1, net.entropy_bottleneck2)
    monkeypatch.setattr(train, "_AUX_FUSED", False)
    want = train.aux_backward(net)
    wg = [m.quantiles.grad.clone() for m in ebs]
    for m in ebs:
        m.quantiles.grad = None
    monkeypatch.setattr(train, "_AUX_FUSED", True)
    got = train.aux_backward(net)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    for m, g in zip(ebs, wg):
        assert m.quantiles.grad.shape == m.quantiles.shape
        assert torch.equal(m.quantiles.grad, g)
    train.aux_backward(net)
    for m, g in zip(ebs, wg):
        assert torch.equal(m.quantiles.grad, g + g)


def test_gmm_backward():
    from masic_amd import autograd as A
    B, M, K, H, W = 2, 24, 5, 6, 10
    y = _rand(B, M, H, W, seed=13, scale=6.0)
    sigma = F.relu(_rand(B, K * M, H, W, seed=14, scale=2.0))
    mu = _rand(B, K * M, H, W, seed=15, scale=5.0)
    raw = _rand(B, K * M, H, W, seed=16, scale=2.0)
    y[0, 0, 0, :2] = torch.tensor([40.0, -35.0])
    noise = torch.from_numpy(np.random.RandomState(17).uniform(-0.5, 0.5, size=y.shape).astype(np.float32))
    t = [v.clone().requires_grad_(True) for v in (y, sigma, mu, raw)]
    yh = t[0] + noise
    lik = O.gmm_likelihood(yh, t[1], t[2], O._softmax_over_k(t[3], K), K)
    g1, g2 = _rand(*y.shape, seed=18), _rand(*y.shape, seed=19, scale=3.0)
    ((yh * g1).sum() + (lik * g2).sum()).backward()
    d = [v.to(DEV).requires_grad_(True) for v in (y, sigma, mu, raw)]
    yh_d, lik_d = A.GmmFn.apply(d[0], noise.to(DEV), d[1], d[2], d[3], K, 0.11, 1e-9)
    ((yh_d * g1.to(DEV)).sum() + (lik_d * g2.to(DEV)).sum()).backward()
    for a, b, n in zip(d, t, ("dy", "dsigma", "dmu", "dlogits")):
        assert_close(a.grad, b.grad, "gmm:" + n, GTOL)
    assert int((t[1].grad == 0).sum()) > 0      # LowerBound(sigma) blocked some gradients


def test_warp_gate_cat_softmax_abs_backward():
    from masic_amd import autograd as A
    from masic_amd import synth
    from masic_amd.homography import warp_matrices
    H, W = 40, 56
    x, _, hm = synth.synth_inputs(2, H, W, seed=4)
    xr = x.clone().requires_grad_(True)
    yr = O.warp_perspective(xr, hm, (H, W))
    go = _rand(*yr.shape, seed=5)
    yr.backward(go)
    m, _ = warp_matrices(hm.to(DEV), (H, W), (H, W))
    xd = x.to(DEV).requires_grad_(True)
    A.WarpFn.apply(xd, m, (H, W)).backward(go.to(DEV))
    assert_close(xd.grad, xr.grad, "warp:dsrc", GTOL)
    # gate + cat + softmax_k + abs in one small graph
    a, b = _rand(2, 5, 6, 7, seed=6), _rand(2, 4, 6, 7, seed=7)
    logits = _rand(2, 3, 6, 7, seed=8)
    ts = [v.clone().requires_grad_(True) for v in (a, b, logits)]
    gates = F.softmax(ts[2], dim=1)
    out = torch.cat((ts[0].abs() * gates[:, 0:1], ts[1] * gates[:, 2:3]), dim=1)
    go = _rand(*out.shape, seed=9)
    out.backward(go)
    td = [v.to(DEV).requires_grad_(True) for v in (a, b, logits)]
    gd = A.SoftmaxKFn.apply(td[2], 3)
    outd = A.cat(A.GateFn.apply(A.AbsFn.apply(td[0]), gd, 0), A.GateFn.apply(td[1], gd, 2))
    assert_close(outd, out, "graph:fwd")
    outd.backward(go.to(DEV))
    for u, v, n in zip(td, ts, ("da", "db", "dlogits")):
        assert_close(u.grad, v.grad, "graph:" + n, GTOL)


def test_training_step_gradients_vs_reference_golden():
    """HSIC(16,24,3) train-mode forward + RD loss + backward with the 7 recorded noise draws: every parameter gradient
    against the reference's (tests/golden/hsic_tiny.npz), then the aux loss gradient."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd.loss import rate_distortion
    fx = load_npz("hsic_tiny.npz")
    N, M, K = (int(v) for v in fx["NMK"])
    sd = golden_state_dict(fx, MASIC.HSIC(N, M, K).state_dict())
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x1, x2, H = (torch.from_numpy(fx[k]).to(DEV) for k in ("x1", "x2", "h_matrix"))
    queue = [torch.from_numpy(fx["train/noise_" + k]).to(DEV) for k in O.NOISE_KEYS]
    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = lambda self, x: queue.pop(0).reshape(x.shape).contiguous()
    try:
        out = net(x1, x2, H)
    finally:
        EntropyModel._get_noise_cached = orig
    assert not queue
    for k in ("x1_hat", "x2_hat"):
        assert_close(out[k], torch.from_numpy(fx["train/" + k]), "train:" + k)
    crit = rate_distortion(out, x1, x2, float(fx["lmbda"]))
    assert abs(float(crit["loss"]) - float(fx["train/loss_loss"])) <= 1e-4 * abs(float(fx["train/loss_loss"]))
    crit["loss"].backward()
    worst, worst_name, n = 0.0, "", 0
    grads = dict(net.named_parameters())
    for key in fx:
        if not key.startswith("train/grad/"):
            continue
        name = key[len("train/grad/"):]
        ref = torch.from_numpy(fx[key])
        got = grads[name].grad
        assert got is not None, name
        e = float((got.cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        n += 1
        if e > worst:
            worst, worst_name = e, name
    print(f"training step: {n} parameter gradients, worst relative error {worst:.2e} ({worst_name})")
    assert n == 164 and worst <= 1e-4, (n, worst, worst_name)     # the 2 quantiles get no gradient from the main loss
    assert net.entropy_bottleneck1.quantiles.grad is None
    # masked taps of the context model do receive gradient, as in the reference
    gm = net.context_prediction1.weight.grad
    assert float(gm[:, :, 3:, :].abs().max()) > 0
    net.zero_grad()
    aux = net.aux_loss()
    assert abs(float(aux) - float(fx["train/aux_loss"])) <= 1e-4 * float(fx["train/aux_loss"])
    aux.backward()
    for nm in ("entropy_bottleneck1.quantiles", "entropy_bottleneck2.quantiles"):
        assert_close(grads[nm].grad, torch.from_numpy(fx["train/auxgrad/" + nm]), "aux:" + nm, GTOL)


@pytest.mark.parametrize("N,M,K,B,H,W", [(16, 32, 3, 2, 64, 64), (128, 192, 5, 1, 128, 128)])
def test_graphed_train_step_equals_eager_steps(N, M, K, B, H, W):
    """masic_amd.graph.GraphedTrainStep -- the whole optimisation step of newtrain_codec_real.py:135-146 as one HIP-graph replay --
    against the eager masic_amd.train.train_step with the same (capturable) Adam on the same batches and the same noise (the
    seven draws of a step come from static buffers refilled before each step): losses per step and the parameters after three
    steps.  The weight gradients use float atomics, so two runs of the SAME path already differ in the last bits: tolerance, not equality.
    Also: the eager model keeps working after replays (per-version pack caches are invalidated), at full width the fused
    analysis / synthesis nodes are inside the capture."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn, synth, train
    from masic_amd.graph import GraphedTrainStep
    sd0 = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=55)
    batches = [tuple(t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=60 + i)) for i in range(3)]
    noises = [synth.synth_noise(B, N, M, H, W, seed=70 + i) for i in range(3)]
    slots = [noises[0][k].to(DEV).clone() for k in O.NOISE_KEYS]
    state = {"i": 0}

    def static_noise(self, x):
        t = slots[state["i"] % len(slots)]
        state["i"] += 1
        return t.reshape(x.shape)

    def load_noise(it):
        state["i"] = 0
        for s, k in zip(slots, O.NOISE_KEYS):
            s.copy_(noises[it][k].to(DEV))

    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = static_noise
    mnn.set_precision("bf16")
    # The capture is a one-stream step (HSIC._forward_graph keeps its side streams out of a capture): the eager step it is compared with
    # runs on one stream too.  With the side streams the float atomics of the weight gradients land in another order, and three Adam steps
    # turn that into percent-level differences of the reconstructions (2.3e-2 against this test's 2e-2 on a cold box, once in seven runs) --
    # which says nothing about the replay; tests/test_gpu_backward.py::test_two_stream_training_forward_is_the_one_stream_computation
    # covers the streams.
    prev_streams, MASIC._TRAIN_STREAMS = MASIC._TRAIN_STREAMS, False
    try:
        def fresh():
            net = MASIC.HSIC(N, M, K)
            net.load_state_dict(sd0)
            return net.to(DEV).train()
        # eager
        net_e = fresh()
        opt = torch.optim.Adam(list(net_e.parameters()), lr=1e-4, capturable=True, fused=True)        # the graph's optimizer flavour
        aopt = torch.optim.Adam(list(net_e.aux_parameters()), lr=1e-3, capturable=True, fused=True)
        want = []
        for it in range(3):
            load_noise(it)
            crit, aux = train.train_step(net_e, opt, aopt, *batches[it], 0.01)
            want.append((float(crit["loss"]), float(aux), float(crit["psnr1"])))
        # eager once more: what two runs of the SAME path differ by after three Adam steps (float atomics; Adam turns a sign flip of a
        # near-zero gradient element into a full +-lr step, so small, noisy tensors -- the last hyper-analysis layer sees a 2 x 2 output at
        # this picture size -- move by ~10 % of their three-step update from run to run)
        net_e2 = fresh()
        opt2 = torch.optim.Adam(list(net_e2.parameters()), lr=1e-4, capturable=True, fused=True)
        aopt2 = torch.optim.Adam(list(net_e2.aux_parameters()), lr=1e-3, capturable=True, fused=True)
        for it in range(3):
            load_noise(it)
            train.train_step(net_e2, opt2, aopt2, *batches[it], 0.01)
        # graphed
        net_g = fresh()
        load_noise(0)
        step = GraphedTrainStep(net_g, *batches[0], 0.01)
        for n, p in net_g.named_parameters():
            assert torch.equal(p.detach().cpu(), sd0[n]), f"warm-up steps must not leave a trace ({n})"
        got = []
        for it in range(3):
            load_noise(it)
            crit, aux = step(*batches[it])
            got.append((float(crit["loss"]), float(aux), float(crit["psnr1"])))
        torch.cuda.synchronize()
        for w, g in zip(want, got):
            for a, b in zip(w, g):
                assert abs(a - b) <= 5e-4 * abs(a) + 1e-6, (want, got)      # (float atomics in the weight gradients: run-to-run differences, amplified by Adam over three steps -- measured up to 2.1e-4 on the third)
        worst_floor = 0.0
        for (n, pe), (_, pg), (_, p2) in zip(net_e.named_parameters(), net_g.named_parameters(), net_e2.named_parameters()):
            de, dg, d2 = ((q.detach().cpu() - sd0[n]).double() for q in (pe, pg, p2))
            floor = float((de - d2).norm()) / (float(de.norm()) + 1e-30)
            worst_floor = max(worst_floor, floor)
            # (0.2: two eager runs are bit-identical most of the time and up to 0.07 apart when the atomics land in another order; the replay,
            # with its own timing, was measured up to 0.11 from the eager run on that layer; a stale pack or a misordered node moves whole
            # tensors by O(1))
            assert float((de - dg).norm()) <= max(0.2, 3.0 * floor) * float(de.norm()) + 1e-12, (n, float((de - dg).norm()), float(de.norm()), floor)
        print(f"largest eager-vs-eager difference of a tensor's three-step update: {worst_floor:.3f} of its norm")
        # the model still works eagerly after replays: its pack caches must not serve the packs of the capture
        net_g.eval()
        net_e.eval()
        with torch.no_grad():
            oe, og = net_e(*batches[0]), net_g(*batches[0])
        assert_close(og["x1_hat"], oe["x1_hat"].cpu(), "eager forward after graphed steps", 2e-2)
        with pytest.raises(RuntimeError):
            step(*batches[0])                      # eval mode: the capture was of the training-mode step
    finally:
        MASIC._TRAIN_STREAMS = prev_streams
        EntropyModel._get_noise_cached = orig
        mnn.set_precision("f32")


def test_two_optimizer_steps_match_cpu_oracle_training():
    """newtrain_codec_real.py:135-146 for two iterations (RD loss backward, Adam 1e-4, aux loss backward, aux Adam 1e-3)
    on HSIC(16,24,3): parameter updates against the same loop driven by torch autograd over the CPU oracle."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import synth
    from masic_amd.train import make_optimizers, train_step
    N, M, K = 16, 24, 3
    lmbda = 0.01
    sd0 = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=31)
    x1, x2, hm = synth.synth_inputs(2, 64, 64, seed=31)
    noises = [synth.synth_noise(2, N, M, 64, 64, seed=40 + i) for i in range(2)]
    # ---- CPU: oracle + torch autograd + Adam
    net_names = [n for n, _ in MASIC.HSIC(N, M, K).named_parameters()]
    sd = {k: (v.clone().requires_grad_(True) if k in net_names else v.clone()) for k, v in sd0.items()}
    main = [sd[n] for n in net_names if not n.startswith("entropy_bottleneck")]
    aux = [sd[n] for n in net_names if n.startswith("entropy_bottleneck")]
    opt, aopt = torch.optim.Adam(main, lr=1e-4), torch.optim.Adam(aux, lr=1e-3)
    ref_losses = []
    for it in range(2):
        opt.zero_grad(); aopt.zero_grad()
        with torch.no_grad():      # MaskedConv2d.forward zeroes the stored masked taps in place (layers.py:77)
            for cp in ("context_prediction1.weight", "context_prediction2.weight"):
                sd[cp].copy_(O.masked_weight(sd[cp].detach()))
        out = O.hsic_forward(sd, x1, x2, hm, K=K, training=True, noise=noises[it])
        loss = O.rd_loss(out, x1, x2, lmbda)["loss"]
        loss.backward()
        opt.step()
        a = O.eb_aux_loss(sd, "entropy_bottleneck1") + O.eb_aux_loss(sd, "entropy_bottleneck2")
        a.backward()
        aopt.step()
        ref_losses.append((float(loss), float(a)))
    # ---- HIP
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(sd0)
    net = net.to(DEV).train()
    optimizer, aux_optimizer = make_optimizers(net)
    queue = []
    orig = EntropyModel._get_noise_cached
    EntropyModel._get_noise_cached = lambda self, x: queue.pop(0).reshape(x.shape).contiguous()
    try:
        for it in range(2):
            queue[:] = [noises[it][k].to(DEV) for k in O.NOISE_KEYS]
            crit, aux_l = train_step(net, optimizer, aux_optimizer, x1.to(DEV), x2.to(DEV), hm.to(DEV), lmbda)
            assert abs(float(crit["loss"]) - ref_losses[it][0]) <= 2e-4 * abs(ref_losses[it][0]), (it, float(crit["loss"]), ref_losses[it])
            assert abs(float(aux_l) - ref_losses[it][1]) <= 2e-4 * abs(ref_losses[it][1])
    finally:
        EntropyModel._get_noise_cached = orig
    # Adam normalises each element's step to ~lr, so elements whose gradient is ~0 (|g| near eps=1e-8) amplify
    # rounding differences; compare per element against the step size and bound the fraction of such outliers.
    worst_frac, worst_name, total_bad, total = 0.0, "", 0, 0
    for n, p in net.named_parameters():
        lr = 1e-3 if n.startswith("entropy_bottleneck") else 1e-4
        du_ref = (sd[n].detach() - sd0[n]).double()
        du = (p.detach().cpu() - sd0[n]).double()
        bad = ((du - du_ref).abs() > 0.05 * lr)
        frac = float(bad.double().mean())
        total_bad += int(bad.sum()); total += bad.numel()
        if frac > worst_frac:
            worst_frac, worst_name = frac, n
        rel = float((du - du_ref).norm()) / (float(du_ref.norm()) + 1e-30)
        assert rel <= 0.5, (n, rel)
    print(f"two training steps: {total_bad}/{total} elements off by > 5% of a step; worst tensor {worst_name} ({worst_frac:.2%})")
    assert total_bad <= 0.002 * total and worst_frac <= 0.05
    # masked taps are re-zeroed by the next forward, exactly as in the reference
    net.eval()
    with torch.no_grad():
        net(x1.to(DEV), x2.to(DEV), hm.to(DEV))
    assert float(net.context_prediction1.weight[:, :, 3:, :].abs().max()) == 0.0


def test_training_step_bf16_mode_against_float32():
    """HSIC(128,192,5), 2 x 128 x 256 pairs, one training-mode forward + RD loss + backward in the bf16-operand mode (fused GDN
    backward, bf16 weight-gradient kernels incl. the 5x5 stride-2 and the GEMM-shaped 1x1 ones, F16K input gradients) against the
    float32 path with the same weights, inputs and noise.  Bounds are those of operand rounding, not of a parity claim: the
    loss to 2e-3, the median parameter-gradient error to 1 % (measured 0.6 %), every gradient's cosine >= 0.94 (measured: the
    worst -- the left hyper path, whose float32 gradients already move 9 % when only the INPUT is rounded to bf16 -- at 15)."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn, synth
    from masic_amd.loss import rate_distortion
    N, M, K = 128, 192, 5

    def run(prec):
        mnn.set_precision(prec)
        try:
            net = MASIC.HSIC(N, M, K)
            net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=7))
            net = net.to(DEV).train()
            x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(2, 128, 256, seed=7))
            g = torch.Generator(device=DEV)
            g.manual_seed(7)
            orig = EntropyModel._get_noise_cached
            EntropyModel._get_noise_cached = lambda self, x: torch.rand(x.shape, device=x.device, generator=g) - 0.5
            try:
                out = net(x1, x2, hm)
            finally:
                EntropyModel._get_noise_cached = orig
            crit = rate_distortion(out, x1, x2, 0.01)
            crit["loss"].backward()
            return float(crit["loss"].detach()), {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}
        finally:
            mnn.set_precision("f32")

    lf, gf = run("f32")
    lb, gb = run("bf16")
    assert abs(lb - lf) <= 2e-3 * abs(lf), (lf, lb)
    assert set(gf) == set(gb) and len(gf) == 164
    cos, rel = [], []
    for n in gf:
        a, b = gf[n].flatten(), gb[n].flatten()
        cos.append(float((a @ b) / (a.norm() * b.norm() + 1e-300)))
        rel.append(float((a - b).norm() / (a.norm() + 1e-300)))
    print(f"bf16-operand training step vs float32: loss {lb:.4f} vs {lf:.4f} ({abs(lb - lf) / abs(lf):.1e}), gradient cosine min {min(cos):.4f}, "
          f"relative error median {sorted(rel)[len(rel) // 2]:.2e} / max {max(rel):.2e}")
    # bounds = what is measured plus margin (round 3: cosine min 0.9616 -- the left hyper path, whose float32 gradients already move 9 % when
    # only the INPUT is rounded to bf16 -- median relative error 5.6e-3); the fused nodes themselves are held to cosine >= 0.995 per tensor
    # against the float32 graph in test_fused_transform_training_nodes_vs_float32_graph / the GmmHeadsFn and EnhancementBlockFn tests
    assert min(cos) >= 0.94, min(cos)
    assert sorted(rel)[len(rel) // 2] <= 1e-2, sorted(rel)[len(rel) // 2]


@pytest.mark.parametrize("which", ["analysis", "synthesis"])
def test_fused_transform_training_nodes_vs_float32_graph(which, monkeypatch):
    """The composite bf16 training nodes behind the quoted training step -- masic_amd/autograd.py: AnalysisFn (Encoder1: four strided
    convolutions + three GDNs as ONE node on the DMA-staged F16K kernels) and SynthesisFn (Decoder1) -- against the float32 node-per-layer
    graph of the same module (the parity path the 1e-4 gradient goldens pin), on synthetic weights, a random input and a random output
    gradient.  Gates as for EnhancementBlockFn (tests/test_gpu_cqe.py): the output within 1 % relative L2, every gradient (input + 14
    parameters) aligned with the float32 one (cosine >= 0.995) and no worse than 1.5 x the error the node-per-layer graph has with the
    SAME bf16 operands -- a dropped or mis-scaled term in one tensor's gradient fails both."""
    import MASIC
    from masic_amd import autograd as A, nn as mnn, synth
    net = MASIC.HSIC(128, 192, 5)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=41))
    mod = (net.encoder1 if which == "analysis" else net.decoder1).to(DEV).train()
    g = torch.Generator().manual_seed(41)
    if which == "analysis":
        x = torch.rand((2, 3, 128, 192), generator=g).to(DEV).requires_grad_(True)
        fwd, sup = (lambda: mod.latent_train(x)), "analysis_supported"
    else:
        x = (torch.randn((2, 192, 8, 12), generator=g) * 4.0).to(DEV).requires_grad_(True)
        fwd, sup = (lambda: mod.reconstruct_train(x)), "synthesis_supported"
    gy = None

    def run():
        nonlocal gy
        mod.zero_grad()
        x.grad = None
        y = fwd()
        if gy is None:
            gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(42)).to(DEV)
        y.backward(gy)
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in mod.parameters() if p.grad is not None]
    r32 = run()                                                      # float32 mode: the node-per-layer graph
    mnn.set_precision("bf16")
    try:
        assert getattr(A, sup)(mod, x)
        fused = run()
        monkeypatch.setattr(A, sup, lambda *a: False)
        unfused = run()
    finally:
        mnn.set_precision("f32")

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def cos(a, b):
        return float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm()))
    assert len(fused) == len(r32) == len(unfused) == 16
    ef, eu = [rel(a, b) for a, b in zip(fused, r32)], [rel(a, b) for a, b in zip(unfused, r32)]
    cs = [cos(a, b) for a, b in zip(fused, r32)]
    print(f"{which} transform, fused bf16 node vs float32 graph: out {ef[0]:.2e}, dx {ef[1]:.2e} (node-per-layer bf16 {eu[1]:.2e}), parameter "
          f"gradients worst {max(ef[2:]):.2e} (node-per-layer bf16 {max(eu[2:]):.2e}), lowest cosine {min(cs):.5f}")
    assert ef[0] <= 1e-2 and min(cs) >= 0.995, (ef[0], cs)
    for k in range(1, 16):
        assert ef[k] <= 1.5 * eu[k] + 1e-3, (k, ef[k], eu[k])


def test_two_stream_training_forward_is_the_one_stream_computation():
    """HSIC._forward_graph issues the right view's front part (warp, encoder2, h_a2, EB2, h_s2_up, context model 2, masks, gates) and the
    left view's entropy chain (h_a1, EB1, h_s1_up, context model 1, heads, mixture likelihood) on side streams; autograd runs each
    node's backward on its forward's stream.  Same noise draws in host order, same kernels: outputs and
    all 166 gradients must agree with the one-stream schedule to the run-to-run floor of the float atomics, every time (a workspace shared
    by two streams' kernels -- the GDN backward's partial sums were, once -- shows as an occasional O(1) difference)."""
    import MASIC
    from compressai.entropy_models import EntropyModel
    from masic_amd import nn as mnn, synth
    from masic_amd.loss import rate_distortion
    N, M, K, B, H, W = 128, 192, 5, 1, 128, 128
    sd0 = synth.synth_state_dict(MASIC.HSIC(N, M, K).state_dict(), seed=57)
    batch = tuple(t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=61))
    noise = synth.synth_noise(B, N, M, H, W, seed=71)
    slots = [noise[k].to(DEV) for k in O.NOISE_KEYS]
    state = {"i": 0}

    def static_noise(self, x):
        t = slots[state["i"] % len(slots)]
        state["i"] += 1
        return t.reshape(x.shape)

    orig, prev = EntropyModel._get_noise_cached, MASIC._TRAIN_STREAMS
    EntropyModel._get_noise_cached = static_noise
    mnn.set_precision("bf16")
    try:
        net = MASIC.HSIC(N, M, K)
        net.load_state_dict(sd0)
        net = net.to(DEV).train()

        def run(streams):
            MASIC._TRAIN_STREAMS = streams
            state["i"] = 0
            for _, p in net.named_parameters():
                p.grad = None
            out = net(*batch)
            crit = rate_distortion(out, batch[0], batch[1], 0.01)
            crit["loss"].backward()
            torch.cuda.synchronize()
            return float(crit["loss"]), {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}

        run(False)
        l0, g0 = run(False)
        l1, g1 = run(False)
        floor = max(float((g0[n] - g1[n]).norm() / (g0[n].norm() + 1e-30)) for n in g0)
        worst = 0.0
        for _ in range(12):
            l2, g2 = run(True)
            assert g2.keys() == g0.keys()
            assert abs(l2 - l0) <= 1e-6 * abs(l0)
            worst = max(worst, max(float((g0[n] - g2[n]).norm() / (g0[n].norm() + 1e-30)) for n in g0))
        print(f"two-stream vs one-stream gradients, worst relative difference over 12 runs {worst:.2e} (one-stream run-to-run floor {floor:.2e})")
        assert worst <= max(1e-5, 20 * floor), (worst, floor)
    finally:
        EntropyModel._get_noise_cached = orig
        MASIC._TRAIN_STREAMS = prev
        mnn.set_precision("f32")


@pytest.mark.parametrize("kind", ["synthetic", "identity", "rotation", "magnify", "minify", "strong_minify", "strong_magnify", "horizon", "to_smaller"])
def test_warp_backward_gather_form_is_the_adjoint(kind):
    """masic_warp_perspective_bwd_gather against autograd through the oracle's kornia.warp_perspective restatement (reference
    MASIC.py:781) and against the scatter form: the synthetic pairs, identity, a 12 degree rotation, 1.5 x magnification, 0.6 x and 0.2 x
    minification stay on the gather path (flag 0); 4 x magnification (~64 destination pixels reach every source pixel) and a horizon
    inside the picture raise the flag and come out of the device-side scatter fallback -- the same values either way.  Also a destination
    of another size."""
    import math
    from masic_amd import ops, synth
    from masic_amd.homography import warp_matrices
    B, C, H, W = 2, 5, 48, 64
    Hd, Wd = (H, W) if kind != "to_smaller" else (32, 40)
    x, _, hm = synth.synth_inputs(B, H, W, seed=14)
    x = torch.cat([x, x[:, :2] * 0.5], 1)
    cx, cy = (W - 1) / 2, (H - 1) / 2

    def about_centre(a, b_, c, d):         # [[a, b], [c, d]] about the picture centre
        return torch.tensor([[a, b_, cx - a * cx - b_ * cy], [c, d, cy - c * cx - d * cy], [0.0, 0.0, 1.0]])
    if kind == "identity":
        hm = torch.eye(3).repeat(B, 1, 1)
    elif kind == "rotation":
        t = math.radians(12)
        hm = about_centre(math.cos(t), -math.sin(t), math.sin(t), math.cos(t)).repeat(B, 1, 1)
    elif kind == "magnify":
        hm = about_centre(1.5, 0.0, 0.0, 1.5).repeat(B, 1, 1)
    elif kind == "minify":
        hm = about_centre(0.6, 0.0, 0.0, 0.6).repeat(B, 1, 1)
    elif kind == "strong_minify":
        hm = about_centre(0.2, 0.0, 0.0, 0.2).repeat(B, 1, 1)
    elif kind == "strong_magnify":
        hm = about_centre(4.0, 0.0, 0.0, 4.0).repeat(B, 1, 1)
    elif kind == "horizon":
        hm = torch.eye(3).repeat(B, 1, 1)
        hm[:, 2, 0] = -1.0 / 40.0           # w = 1 - x / 40 changes sign inside the picture
    elif kind == "to_smaller":
        hm = hm.clone()
        hm[:, :2] *= 0.6
    xr = x.clone().requires_grad_(True)
    yr = O.warp_perspective(xr, hm, (Hd, Wd))
    go = _rand(*yr.shape, seed=15)
    yr.backward(go)
    m, _ = warp_matrices(hm.to(DEV), (H, W), (Hd, Wd))
    g = go.to(DEV).contiguous()
    got, flag = ops.warp_perspective_bwd(g, m, (B, C, H, W), want_flag=True)
    ref = ops.zeros((B, C, H, W), torch.float32, DEV)
    ops.check(ops.lib.masic_warp_perspective_bwd(ops._p(g), ops._p(m), ops._p(ref), B, C, H, W, Hd, Wd, ops._stream()), "warp_perspective_bwd")
    fell_back = bool(int(flag.item()))
    print(f"{kind}: gather form {'fell back to the scatter form' if fell_back else 'used'}; max |gather - scatter| = {float((got - ref).abs().max()):.3e}, "
          f"max |gather - oracle| = {float((got.cpu() - xr.grad).abs().max()):.3e}, max |oracle| = {float(xr.grad.abs().max()):.3e}")
    assert fell_back == (kind in ("strong_magnify", "horizon")), (kind, fell_back)
    assert_close(got, ref.cpu(), "warp gather vs scatter", 2e-5)
    if kind != "horizon":                   # (on the horizon the sampling points are unbounded: the oracle's float32 grid and ours agree only off it)
        assert_close(got, xr.grad, "warp gather vs oracle autograd", GTOL)
