"""The entropy-model kernels in the rate's own domain (-m gpu): gmm_fwd/bwd_kernel<1..8>, eb_fwd/bwd_kernel, the aux-loss kernels,
sum_log / rd_loss / rd_loss_bwd -- bits and the gradients of sum(bits) against the float64 reference of tests/entropy_ref.py, each
quantity in units of its own scale (tests.util.scaled_err) and bounded by TOL[regime][quantity], which is 8 x the float32 CPU
oracle's error under the same ruler (never the kernels' own).  Everything goes through masic_amd.ops and masic_amd.autograd.

`pytest -m gpu -s tests/test_gpu_entropy_bits.py` prints the worst figure per regime and quantity at the end (profiles/
entropy_bits.txt is that table); MASIC_ENTROPY_BITS_REPORT=<file> also writes it."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import hsic_oracle as O
from tests import entropy_ref as R
from tests.util import scaled_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SB, LB = 0.11, 1e-9               # as the modules pass them: the C ABI takes floats, so the kernels see float32(0.11), float32(1e-9)
_WORST = {}


def _ops():
    from masic_amd import ops
    return ops


def _A():
    from masic_amd import autograd
    return autograd


def _check(regime, q, got, ref, what=""):
    e = scaled_err(got, *ref)
    key = (regime, q)
    _WORST[key] = max(_WORST.get(key, 0.0), e)
    tol = R.TOL[regime][q]
    print(f"{regime}/{q} {what}: {e:.3e} (TOL {tol:.2e})")
    assert e <= tol, f"{regime}/{q} {what}: scaled error {e:.3e} > TOL {tol:.2e}"


def _report():
    lines = ["# worst scaled error of the HIP kernels per regime and quantity (tests/test_gpu_entropy_bits.py), MI355X",
             f"# {'regime':10s} {'quantity':8s} {'gpu':>10s} {'TOL':>10s} {'TOL/gpu':>8s}"]
    for (regime, q), e in sorted(_WORST.items()):
        tol = R.TOL[regime][q]
        lines.append(f"  {regime:10s} {q:8s} {e:10.3e} {tol:10.2e} {tol / e if e > 0 else math.inf:8.1f}")
    return "\n".join(lines)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    text = _report()
    print("\n" + text)
    path = os.environ.get("MASIC_ENTROPY_BITS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


# ------------------------------------------------------------------------------------------------------------ Gaussian mixture
@functools.lru_cache(maxsize=None)
def _gmm_in(regime, K, shape):
    inp = R.gmm_inputs(regime, K, shape)
    return inp, {k: v.to(DEV) for k, v in inp.items()}


def _gmm_ref(regime, K, shape, ymode, logits):
    inp, _ = _gmm_in(regime, K, shape)
    return R.gmm_ref(R.gmm_y_hat(inp, ymode), inp["sigma"], inp["mu"], inp["logits"] if logits else inp["weights"], K, logits)


@pytest.mark.parametrize("regime", R.GMM_REGIMES)
@pytest.mark.parametrize("K", R.GMM_KS)
def test_gmm_forward_bits(K, regime):
    """ops.gmm_likelihood in every mode: training 0 (round), 1 (noise), 2 (as given) x logits / given weights, want_weights, and
    want_y_hat=False giving the same likelihood bits; y_hat bit-equal to the CPU rounding / noise add."""
    ops = _ops()
    for shape in R.GMM_SHAPES:
        inp, d = _gmm_in(regime, K, shape)
        for training, ymode in enumerate(R.GMM_YMODES):
            yh_cpu = R.gmm_y_hat(inp, ymode)
            for logits in (True, False):
                ref = _gmm_ref(regime, K, shape, ymode, logits)
                args = (d["y"], d["sigma"], d["mu"], d["logits"] if logits else d["weights"], K)
                kw = dict(training=training, noise=d["noise"] if training == 1 else None, weights_are_logits=logits, scale_bound=SB, lik_bound=LB)
                yh, lik, wout = ops.gmm_likelihood(*args, want_weights=True, **kw)
                assert torch.equal(yh.cpu(), yh_cpu), f"y_hat {ymode}"
                assert float(lik.min()) >= np.float32(R.B_L) and bool(torch.isfinite(lik).all())
                what = f"K={K} {shape} {ymode} logits={logits}"
                _check(regime, "bits", R.bits_of(lik.cpu()), ref["bits"], what)
                if logits:
                    _check(regime, "w", wout.cpu(), ref["w"], what)
                else:
                    assert wout is None
                yh2, lik2 = ops.gmm_likelihood(*args, want_y_hat=False, **kw)
                assert (yh2 is None) == (training != 2)
                assert torch.equal(lik2, lik), "want_y_hat=False changes likelihood bits"


@pytest.mark.parametrize("regime", R.GMM_REGIMES)
@pytest.mark.parametrize("K", R.GMM_KS)
def test_gmm_backward_rate_gradient(K, regime):
    """GmmFn (noise inside) and GmmLikFn (y_hat given) under (-log2 lik).sum().backward() on the device: the real, negative,
    up-to-1e9 rate gradient reaches gmm_bwd_kernel<K>; bits, dy, d sigma, d mu and d logits / dw inside TOL."""
    A = _A()
    for shape in R.GMM_SHAPES:
        inp, d = _gmm_in(regime, K, shape)
        for ymode in ("noise", "given"):
            for logits in (True, False):
                ref = _gmm_ref(regime, K, shape, ymode, logits)
                t = [d[k].clone().requires_grad_(True) for k in ("y", "sigma", "mu", "logits" if logits else "weights")]
                if ymode == "noise":
                    yh, lik = A.GmmFn.apply(t[0], d["noise"], t[1], t[2], t[3], K, SB, LB, logits)
                    assert torch.equal(yh.detach().cpu(), R.gmm_y_hat(inp, "noise"))
                else:
                    lik = A.GmmLikFn.apply(t[0], t[1], t[2], t[3], K, SB, LB, logits)
                (-torch.log2(lik)).sum().backward()
                what = f"K={K} {shape} {ymode} logits={logits}"
                _check(regime, "bits", R.bits_of(lik.cpu()), ref["bits"], what)
                for v, q in zip(t, ("dy", "dsigma", "dmu", "dlogits" if logits else "dw")):
                    _check(regime, q, v.grad.cpu(), ref[q], what)


@pytest.mark.parametrize("K", (1, 3, 8))
def test_gmm_gates_are_exact(K):
    """LowerBound passes a gradient iff input >= bound or gradient < 0.  A positive g_lik where the float64 likelihood is below
    0.5e-9: all four gradients exactly 0.  sigma strictly below float32(0.11) with a positive d sigma: exactly 0; sigma exactly
    float32(0.11): passes."""
    A = _A()
    shape = R.GMM_SHAPES[0]
    inp, d = _gmm_in("tail", K, shape)
    ref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], K, True, g_lik=torch.ones(shape))
    t = [d[k].clone().requires_grad_(True) for k in ("y", "sigma", "mu", "logits")]
    A.GmmLikFn.apply(t[0], t[1], t[2], t[3], K, SB, LB, True).sum().backward()
    below = ref["lik_raw"][0] < 0.5e-9
    assert int(below.sum()) >= 10
    belowk = below.unsqueeze(1).expand(shape[0], K, *shape[1:]).reshape(inp["sigma"].shape)
    assert float(t[0].grad.cpu()[below].abs().max()) == 0.0
    for v in t[1:]:
        assert float(v.grad.cpu()[belowk].abs().max()) == 0.0
    open_ = ref["lik_raw"][0] > 2e-9                       # ... and where the likelihood is above the bound the gate is open
    assert bool((t[0].grad.cpu()[open_] != 0).any()) and bool((ref["dy"][0][open_] != 0).any())

    inp, d = _gmm_in("sharp", K, shape)
    ref = _gmm_ref("sharp", K, shape, "given", True)
    t = [d[k].clone().requires_grad_(True) for k in ("y", "sigma", "mu", "logits")]
    (-torch.log2(A.GmmLikFn.apply(t[0], t[1], t[2], t[3], K, SB, LB, True))).sum().backward()
    raw, scale = ref["dsigma_raw"]
    positive = raw > 1e-3 * torch.clamp(scale, min=1e-6 * float(scale.max()))      # clearly positive: float32 cannot see it negative
    sg, got = inp["sigma"], t[1].grad.cpu()
    blocked, at_bound = positive & (sg < np.float32(R.B_S)), positive & (sg == np.float32(R.B_S))
    assert int(blocked.sum()) >= 10 and int(at_bound.sum()) >= 5
    assert float(got[blocked].abs().max()) == 0.0
    assert bool((got[at_bound] > 0).all())
    assert float(((got.double() - raw).abs() / scale)[at_bound].max()) <= R.TOL["sharp"]["dsigma"]
    negative = (raw < -1e-3 * torch.clamp(scale, min=1e-6 * float(scale.max()))) & (sg < np.float32(R.B_S))
    if int(negative.sum()):                                # a negative gradient passes below the bound
        assert bool((got[negative] < 0).all())


# ------------------------------------------------------------------------------------------------------------ EntropyBottleneck
def _eb_leaves(table):
    mats, bias, fac = R.eb_table_parts(table)
    return [p.to(DEV).requires_grad_(True) for p in mats + bias + fac]


@pytest.mark.parametrize("pset", R.EB_PSETS)
@pytest.mark.parametrize("shape", R.EB_SHAPES, ids=lambda s: f"C{s[0]}xL{s[1] * s[2] * s[3]}")
def test_bottleneck_bits_and_gradients(shape, pset):
    """eb_fwd_kernel (training and eval; medians contiguous and read in place at stride 3 from the quantiles parameter) and
    eb_bwd_kernel's one-workgroup-per-channel loop below, at and above 256 elements, through EntropyBottleneckFn and EbTableFn
    (eb_table_split): bits, dz and the 58 parameter gradients per channel, every parameter set x regime."""
    ops, A = _ops(), _A()
    C, B, H, W = shape
    table, quant = R.eb_params(pset, C)
    qd = quant.to(DEV)
    med_view, med_c = qd[:, 0, 1], qd[:, 0, 1].contiguous()
    assert C == 1 or med_view.stride(0) == 3
    for regime in R.EB_REGIMES:
        inp = R.eb_inputs(regime, shape)
        what = f"{pset} {shape}"
        # training, with gradients
        leaves = _eb_leaves(table)
        tab = A.eb_param_table(leaves[:5], leaves[5:10], leaves[10:])
        assert torch.equal(tab.detach().cpu(), table)
        z = inp["z"].to(DEV).requires_grad_(True)
        noise = inp["noise"].to(DEV)
        zh, lik = A.EntropyBottleneckFn.apply(z, tab, noise, med_c, LB)
        zh_cpu = R.eb_quantize(inp["z"], quant[:, 0, 1], True, inp["noise"])
        assert torch.equal(zh.detach().cpu(), zh_cpu)
        (-torch.log2(lik)).sum().backward()
        ref = R.eb_ref(zh_cpu, table)
        assert float(lik.min()) >= np.float32(R.B_L)
        _check("eb_" + regime, "bits", R.bits_of(lik.cpu()), ref["bits"], what + " training")
        _check("eb_" + regime, "dz", z.grad.cpu(), ref["dz"], what)
        got = R.eb_table([p.grad.cpu() for p in leaves[:5]], [p.grad.cpu() for p in leaves[5:10]], [p.grad.cpu() for p in leaves[10:]])
        _check("eb_" + regime, "dparams", got, ref["dparams"], what)
        _, lik_v = ops.entropy_bottleneck(z.detach(), tab.detach(), med_view, training=True, noise=noise, lik_bound=LB)
        assert torch.equal(lik_v, lik.detach())
        # eval
        zh_cpu = R.eb_quantize(inp["z"], quant[:, 0, 1], False)
        ref = R.eb_ref(zh_cpu, table)
        outs = [ops.entropy_bottleneck(z.detach(), tab.detach(), m, training=False, lik_bound=LB) for m in (med_c, med_view)]
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "strided medians"
        assert torch.equal(outs[0][0].cpu(), zh_cpu)
        _check("eb_" + regime, "bits", R.bits_of(outs[1][1].cpu()), ref["bits"], what + " eval")


def test_bottleneck_parameter_sets_are_the_projects():
    """tests/entropy_ref.py restates (it may not import masic_amd) the synthetic state dict and the module's initialisation."""
    from compressai.entropy_models import EntropyBottleneck
    from masic_amd import synth
    eb = EntropyBottleneck(3)
    sd = synth.synth_state_dict(dict(eb.state_dict()), seed=5)
    table, quant = R.eb_params("synth", 3, seed=5)
    want = R.eb_state_dict(table, quant, "eb")
    for k, v in want.items():
        assert torch.equal(v, sd[k[3:]]), k
    table, quant = R.eb_params("default", 3)
    init = R.eb_state_dict(table, quant, "eb")
    live = eb.state_dict()
    for k, v in init.items():
        if "_biases" not in k:                              # (the module draws its biases from torch's generator)
            assert torch.equal(live[k[3:]], v), k


@pytest.mark.parametrize("C", R.AUX_CS)
def test_aux_loss_value_and_quantile_gradient(C):
    """eb_auxloss_kernel strides one 256-thread block over 3C items, eb_auxloss_bwd_kernel uses ceil(3C / 256) blocks: 3C = 3, 255,
    258 and 576 -- below, at and above one pass, where the models (C = 128, 192) run."""
    ops = _ops()
    for pset in R.EB_PSETS:
        table, quant = R.eb_params(pset, C)
        ref = R.aux_ref(table, quant)
        td, qd = table.to(DEV), quant.to(DEV)
        _check("eb_aux", "aux", ops.entropy_bottleneck_auxloss(td, qd).reshape(1).cpu(), ref["aux"], f"{pset} C={C}")
        _check("eb_aux", "aux_dq", ops.entropy_bottleneck_auxloss_bwd(td, qd, 1.0).cpu(), ref["aux_dq"], f"{pset} C={C}")


class _TwoBottlenecks(torch.nn.Module):
    def __init__(self, widths, pset):
        super().__init__()
        from compressai.entropy_models import EntropyBottleneck
        self.ebs = torch.nn.ModuleList(EntropyBottleneck(C) for C in widths)
        for eb, C in zip(self.ebs, widths):
            table, quant = R.eb_params(pset, C)
            eb.load_state_dict({k[3:]: v for k, v in R.eb_state_dict(table, quant, "eb").items()}, strict=False)


@pytest.mark.parametrize("pset", R.EB_PSETS)
def test_aux_step_fused_path_86_and_192_channels(pset):
    """train.aux_backward on a model whose two bottlenecks have 86 and 192 channels (ops.entropy_bottleneck_aux_step: eb_aux_fused_kernel
    with two and three blocks per bottleneck, eb_aux_sum_kernel past one pass): loss and quantile gradients against float64."""
    from masic_amd import train
    widths = (86, 192)
    net = _TwoBottlenecks(widths, pset).to(DEV).train()
    refs = [R.aux_ref(*R.eb_params(pset, C)) for C in widths]
    loss = train.aux_backward(net)
    val = sum(r["aux"][0] for r in refs), sum(r["aux"][1] for r in refs)
    _check("eb_aux", "aux", loss.reshape(1).cpu(), val, f"{pset} fused")
    for eb, r, C in zip(net.ebs, refs, widths):
        _check("eb_aux", "aux_dq", eb.quantiles.grad.cpu(), r["aux_dq"], f"{pset} fused C={C}")
        assert all(p.grad is None for n, p in eb.named_parameters() if n != "quantiles")


# ------------------------------------------------------------------------------------------------------------ criterion
@functools.lru_cache(maxsize=None)
def _crit():
    return R.criterion_liks(O)


def _pictures(seed):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.uniform(0, 1, size=(1, 3, 8, 8)).astype(np.float32)).to(DEV) for _ in range(4)]


def test_sum_log_and_rd_loss_on_tail_likelihoods():
    """ops.sum_log and ops.rd_loss on likelihoods that include exact float32(1e-9) and go up to 1, with 1, 255, 257 and 3*50*17*11
    elements, against sum(log) in float64 of the same float32 values, relative to sum |log lik|."""
    ops = _ops()
    liks = _crit()
    assert [l.numel() for l in liks] == list(R.CRIT_NS)
    assert all(float(l.reshape(-1)[0]) == np.float32(R.B_L) for l in liks) and float(liks[-1].max()) == 1.0
    assert float((liks[-1] == np.float32(R.B_L)).double().mean()) >= 0.05
    tol = R.TOL["criterion"]["sum_log"]
    dl = [l.to(DEV) for l in liks]
    for l, d in zip(liks, dl):
        e = R.sum_log_err(ops.sum_log(d).cpu(), l)
        _WORST[("criterion", "sum_log")] = max(_WORST.get(("criterion", "sum_log"), 0.0), e)
        print(f"sum_log n={l.numel()}: {e:.3e} (TOL {tol:.2e})")
        assert e <= tol, f"sum_log n={l.numel()}: {e:.3e} > {tol:.2e}"
    x1, x2, x1h, x2h = _pictures(1)
    cb, cm = 1.0 / (-math.log(2) * 64), 0.01 * 255 ** 2
    loss, mse1, mse2, bpp, per = ops.rd_loss(x1h, x1, x2h, x2, dl, cb, cm)
    logs = [torch.log(l.double()) for l in liks]
    mag = sum(float(v.abs().sum()) for v in logs)
    for got, v in zip(per, logs):
        e = abs(float(got) / cb - float(v.sum())) / float(v.abs().sum())
        print(f"rd_loss per-tensor n={v.numel()}: {e:.3e}")
        assert e <= tol
    bpp_ref = cb * sum(float(v.sum()) for v in logs)
    assert abs(float(bpp) - bpp_ref) <= tol * abs(cb) * mag
    m = [float(((a.double() - b.double()) ** 2).mean()) for a, b in ((x1h, x1), (x2h, x2))]
    # mse: a float32 difference and a float32 square per element (2 roundings, 2^-23 relative to every term), summed in float64
    assert abs(float(mse1) - m[0]) <= 2.0 ** -22 * m[0] and abs(float(mse2) - m[1]) <= 2.0 ** -22 * m[1]
    loss_ref = cm * (m[0] + m[1]) + bpp_ref
    # the loss: the float64 sum rounded once to float32, on top of the bounds of its two parts
    assert abs(float(loss) - loss_ref) <= 2.0 ** -24 * abs(loss_ref) + tol * abs(cb) * mag + 2.0 ** -22 * cm * (m[0] + m[1])


def test_rd_loss_bwd_likelihood_gradient():
    """g_lik = (s_lik / lik) * g in rd_bwd_kernel: the float32 cast of s_lik at the C ABI, one division and one product -- three
    correctly rounded float32 operations, as counted in misc.hip -- so every element is within 2^-22 relative of s_lik g / lik."""
    ops = _ops()
    liks = _crit()
    dl = [l.to(DEV) for l in liks]
    x1, x2, x1h, x2h = _pictures(2)
    cb = 1.0 / (-math.log(2) * 64)
    g = torch.tensor(0.75, dtype=torch.float32, device=DEV)
    _, _, gl = ops.rd_loss_bwd(x1h, x1, x2h, x2, dl, 0.01 * 255 ** 2 * 2.0 / x1.numel(), cb, g)
    for got, l in zip(gl, liks):
        want = cb * 0.75 / l.double()
        rel = ((got.cpu().double() - want).abs() / want.abs()).max()
        print(f"rd_loss_bwd n={l.numel()}: {float(rel):.3e} (2^-22 = {2.0 ** -22:.3e})")
        assert float(rel) <= 2.0 ** -22


def test_chain_rate_gradient_from_the_criterion():
    """GmmLikFn + EntropyBottleneckFn feed RateDistortionFn at 1x3x8x8 pictures; loss.backward(): the g_lik the training step really
    produces (rd_bwd_kernel's, not a synthetic one) reaches both backward kernels.  Against the float64 chain: the gradients of
    sum(bits) times 1 / (B H W) = -cb ln2, with the same scales times that factor."""
    A = _A()
    K, gshape, eshape = 3, (1, 4, 4, 4), (3, 1, 2, 2)
    inp = R.gmm_inputs("tail", K, gshape)
    t = [inp[k].to(DEV).requires_grad_(True) for k in ("y", "sigma", "mu", "logits")]
    table, quant = R.eb_params("synth", 3)
    ez = R.eb_inputs("tail", eshape)
    leaves = _eb_leaves(table)
    z = ez["z"].to(DEV).requires_grad_(True)
    x1, x2, x1h, x2h = _pictures(3)
    lik_y = A.GmmLikFn.apply(t[0], t[1], t[2], t[3], K, SB, LB, True)
    zh, lik_z = A.EntropyBottleneckFn.apply(z, A.eb_param_table(leaves[:5], leaves[5:10], leaves[10:]), ez["noise"].to(DEV),
                                            quant.to(DEV)[:, 0, 1].contiguous(), LB)
    out = A.RateDistortionFn.apply(0.01, x1, x2, x1h, x2h, lik_y, lik_z)
    out[0].backward()
    n = 64.0
    gref = R.gmm_ref(inp["y"], inp["sigma"], inp["mu"], inp["logits"], K)
    eref = R.eb_ref(R.eb_quantize(ez["z"], quant[:, 0, 1], True, ez["noise"]), table)
    for v, q in zip(t, ("dy", "dsigma", "dmu", "dlogits")):
        _check("tail", q, v.grad.cpu().double() * n, gref[q], "chain")
    _check("eb_tail", "dz", z.grad.cpu().double() * n, eref["dz"], "chain")
    got = R.eb_table([p.grad.cpu() for p in leaves[:5]], [p.grad.cpu() for p in leaves[5:10]], [p.grad.cpu() for p in leaves[10:]])
    _check("eb_tail", "dparams", got.double() * n, eref["dparams"], "chain")
    rate = (float(gref["bits"][0].sum()) + float(eref["bits"][0].sum())) / n
    dist = 0.01 * 255 ** 2 * sum(float(((a.double() - b.double()) ** 2).mean()) for a, b in ((x1h, x1), (x2h, x2)))
    # the loss: every element's bits inside TOL of its scale, the distortion as in the criterion test, one rounding to float32
    slack = (R.TOL["tail"]["bits"] * float(gref["bits"][1].sum()) + R.TOL["eb_tail"]["bits"] * float(eref["bits"][1].sum())) / n
    assert abs(float(out[0]) - (rate + dist)) <= slack + 2.0 ** -22 * dist + 2.0 ** -24 * (rate + dist)
