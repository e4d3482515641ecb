"""GPU tests (-m gpu) of the UDH homography net (coremasic/mywork/model.py on masic_amd/csrc/udh.hip + the float32 convolution):
parity with the reference's float32 CPU outputs (tests/golden/udh_net.npz, rebuilt weights and inputs: tests/udh_weights.py),
reproducibility and batch invariance, graph capture, pack freshness, and the hand-over to homography_from_corners.

Parity bound: tests/util.assert_close at 1e-4 of the tensor's peak, the project's float32-path contract.  The reference's own
float32-against-float64 deviation on these cases is 4e-7 to 1e-6 of the peak (printed by tests/golden/make_udh_goldens.py), so the
bound sits two orders above the rounding floor and far below any layout, tap-order, pooling or flatten-order mistake.
Measured worst error on an MI355X: DESIGN.md section 8.4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import udh_weights as UW
from tests.util import assert_close, load_npz, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
_NETS = {}


def _ops():
    from masic_amd import ops
    return ops


def _net(p, seed=UW.WEIGHT_SEED, shared=True):
    import model
    if shared and (p, seed) in _NETS:
        return _NETS[(p, seed)]
    net = model.Net(patch_size=p).to(DEV).eval()
    UW.fill(net, seed)
    if shared:
        _NETS[(p, seed)] = net
    return net


def _inputs(p, B, seed=None):
    a, b = UW.patches(UW.case_seed(p, B) if seed is None else seed, B, p)
    return a.to(DEV), b.to(DEV)


@pytest.fixture(scope="module")
def fx():
    return load_npz("udh_net.npz")


@pytest.mark.parametrize("p,B", UW.CASES)
def test_parity_with_the_reference(fx, p, B):
    net = _net(p)
    a, b = _inputs(p, B)
    blocks = net.features(a, b)
    delta = net(a, b)
    assert tuple(delta.shape) == (B, 4, 2)
    errs = {f"block{i}": rel_err(x.reshape(-1)[::UW.SAMPLE_STRIDE], torch.from_numpy(fx[f"c{p}_{B}/block{i}"])) for i, x in enumerate(blocks)}
    errs["delta"] = rel_err(delta, torch.from_numpy(fx[f"c{p}_{B}/delta"]))
    errs["delta_vs_float64"] = rel_err(delta, torch.from_numpy(fx[f"c{p}_{B}/delta64"]))
    print(f"udh parity p={p} B={B}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for i, x in enumerate(blocks):
        assert_close(x.reshape(-1)[::UW.SAMPLE_STRIDE], torch.from_numpy(fx[f"c{p}_{B}/block{i}"]), f"block{i}")
    assert_close(delta, torch.from_numpy(fx[f"c{p}_{B}/delta"]), "delta")


def test_first_layer_pool_and_linear_kernels_against_torch():
    """Each new kernel on its own through its ops wrapper, at shapes with ragged tiles: an odd-sized picture for the first layer
    (more than one workgroup, a partial last one), odd plane counts and a NaN for the pool, a remainder row group for the linears."""
    ops = _ops()
    rs = np.random.default_rng(3)
    a = torch.from_numpy(rs.standard_normal((3, 1, 37, 29), dtype=np.float32))
    b = torch.from_numpy(rs.standard_normal((3, 1, 37, 29), dtype=np.float32))
    w = torch.from_numpy(rs.standard_normal((32, 2, 3, 3), dtype=np.float32) / 4)
    bias = torch.from_numpy(rs.uniform(-0.5, 0.5, 32).astype(np.float32))
    want = F.relu(F.conv2d(torch.cat((a, b), 1).double(), w.double(), bias.double(), padding=1))
    assert_close(ops.udh_conv1(a.to(DEV), b.to(DEV), w.to(DEV), bias.to(DEV)), want, "udh_conv1")

    x = torch.from_numpy(rs.standard_normal((3, 5, 14, 6), dtype=np.float32))
    x[1, 2, 3, 4] = float("nan")
    got = ops.maxpool2(x.to(DEV)).cpu()
    want = F.max_pool2d(x, 2, 2)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(want).sum()) == 1
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    with pytest.raises(RuntimeError):
        ops.maxpool2(torch.zeros(1, 1, 3, 4, device=DEV))

    B, K, N, M = 11, 1536, 256, 8
    x = torch.from_numpy(rs.standard_normal((B, K), dtype=np.float32))
    w1 = torch.from_numpy(rs.standard_normal((N, K), dtype=np.float32) / 32)
    b1 = torch.from_numpy(rs.uniform(-0.5, 0.5, N).astype(np.float32))
    w2 = torch.from_numpy(rs.standard_normal((M, N), dtype=np.float32) / 16)
    b2 = torch.from_numpy(rs.uniform(-0.5, 0.5, M).astype(np.float32))
    hidden, out = ops.udh_fc(x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), want_hidden=True)
    want_h = F.relu(x.double() @ w1.double().t() + b1.double())
    assert_close(hidden, want_h, "linear 1")
    assert_close(out, want_h @ w2.double().t() + b2.double(), "linear 2")
    with pytest.raises(RuntimeError):
        ops.udh_fc(x[:, :1000].contiguous().to(DEV), w1[:, :1000].contiguous().to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))


def test_reproducible_and_batch_invariant():
    """The same call twice is bitwise equal, and row i of the (64, 9) batch equals the B = 1 call on pair i: bit for bit for the
    first-layer kernel, the pool and the linear kernels, and for the whole net (the reused float32 convolution keeps its K chunk,
    hence its summation order, across batch sizes at these shapes: DESIGN.md section 8.4)."""
    ops = _ops()
    p, B = 64, 9
    net = _net(p)
    a, b = _inputs(p, B)
    c0 = net.cnn[0].layers[0]
    l1, l2 = net.fc[2], net.fc[5]
    first = ops.udh_conv1(a, b, c0.weight.detach(), c0.bias.detach())
    pooled = ops.maxpool2(first)
    feat = net.features(a, b)[-1]
    hidden, out = ops.udh_fc(feat, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach(), want_hidden=True)
    delta = net(a, b)
    assert torch.equal(delta, net(a, b))
    assert torch.equal(delta.reshape(B, 8), out)
    worst = 0.0
    for i in range(B):
        ai, bi = a[i:i + 1].contiguous(), b[i:i + 1].contiguous()
        fi = ops.udh_conv1(ai, bi, c0.weight.detach(), c0.bias.detach())
        assert torch.equal(fi[0], first[i]), f"first layer, pair {i}"
        assert torch.equal(ops.maxpool2(fi)[0], pooled[i]), f"pool, pair {i}"
        hi, oi = ops.udh_fc(feat[i:i + 1].contiguous(), l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach(), want_hidden=True)
        assert torch.equal(hi[0], hidden[i]) and torch.equal(oi[0], out[i]), f"linear layers, pair {i}"
        di = net(ai, bi)
        worst = max(worst, float((di[0] - delta[i]).abs().max()) / float(delta.abs().max()))
        assert torch.equal(di[0], delta[i]), f"whole net, pair {i}: {worst:.2e} of the peak"
    print(f"udh batch invariance: whole net worst deviation {worst:.2e} of the peak")


def test_forward_is_capturable_into_a_graph():
    p, B = 128, 2
    net = _net(p)
    a1, b1 = _inputs(p, B)
    a2, b2 = _inputs(p, B, seed=77)
    sa, sb = a1.clone(), b1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(sa, sb)                                    # weight packs and allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(sa, sb)
    g.replay()
    assert torch.equal(out, net(a1, b1))
    sa.copy_(a2)
    sb.copy_(b2)
    g.replay()
    torch.cuda.synchronize()
    eager = net(a2, b2)
    assert torch.equal(out, eager)
    assert not torch.equal(eager, net(a1, b1))


def test_block_on_its_own_takes_the_same_kernels_as_inside_net():
    """Block(2, 64) called with a concatenated [B,2,H,W] tensor splits it into its planes for the first-layer kernel: bitwise what
    Net computes for its first block from the two patch tensors."""
    p, B = 32, 3
    net = _net(p)
    a, b = _inputs(p, B)
    assert torch.equal(net.cnn[0](torch.cat((a, b), dim=1)), net.features(a, b)[0])
    assert torch.equal(net.cnn[1](net.features(a, b)[0]), net.features(a, b)[1])


def test_load_state_dict_never_serves_stale_packs():
    p, B = 32, 3
    net = _net(p, shared=False)
    a, b = _inputs(p, B)
    out7 = net(a, b)
    UW.fill(net, 8)
    out8 = net(a, b)
    assert not torch.equal(out7, out8)
    assert torch.equal(out8, _net(p, seed=8, shared=False)(a, b))
    assert torch.equal(out7, _net(p)(a, b))


def test_get_h_and_h_matrix():
    """Both are ops.homography_from_corners applied to the net's delta, bitwise; the result agrees with the float64 restatement
    oracle/udh_oracle.py within that file's 2e-6 bound (tests/test_gpu_ops.py::test_homography_from_corners_vs_restatement)."""
    ops = _ops()
    from oracle import udh_oracle as U
    p, B = 128, 2
    net = _net(p)
    a, b = _inputs(p, B)
    corners = torch.tensor([[[40., 52.], [168., 52.], [168., 180.], [40., 180.]],
                            [[64., 31.], [192., 31.], [192., 159.], [64., 159.]]], device=DEV)
    delta = net(a, b)
    assert torch.equal(net.get_h(a, b, corners), ops.homography_from_corners(corners, delta, (1, 1), (1, 1)))
    ori, resized = (512, 896), (256, 256)
    shifted = corners - corners[:, :1]
    got = net.h_matrix(a, b, corners, ori, resized)
    assert torch.equal(got, ops.homography_from_corners(shifted, delta, ori, resized))
    want = U.h_matrix_from_corners(shifted.cpu().numpy(), delta.cpu().numpy(), ori, resized)
    assert np.abs(got.cpu().numpy() - want).max() <= 2e-6 * np.abs(want).max()
    want1 = U.h_matrix_from_corners(corners.cpu().numpy(), delta.cpu().numpy(), (1, 1), (1, 1))
    assert np.abs(net.get_h(a, b, corners).cpu().numpy() - want1).max() <= 2e-6 * np.abs(want1).max()


def test_argument_errors_on_the_device():
    net = _net(32)
    a, b = _inputs(32, 2)
    with pytest.raises(ValueError):
        net(a, b[:1])
    with pytest.raises(ValueError):
        net(*_inputs(64, 1))
    with pytest.raises(RuntimeError):
        net(a.double(), b.double())
    with pytest.raises(RuntimeError):
        net(a.transpose(2, 3), b.transpose(2, 3))
