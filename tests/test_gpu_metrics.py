"""GPU tests (-m gpu) of the per-pair reductions (masic_amd/csrc/metrics.hip, masic_amd/metrics.py).  Every comparison is exact:
pair_rd against ops.sse / ops.sum_log of each image's slice with == on float64, u8_sse against numpy's int64 sum."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from masic_amd import metrics, ops
    return metrics, ops


def _case(B, pic_shape, lik_shapes, seed):
    """x1_hat, x1, x2_hat, x2 [B, *pic_shape] in [0, 1] and likelihood tensors [B, *shape] in [1e-9, 1], both ends present"""
    g = torch.Generator().manual_seed(seed)
    pics = [torch.rand((B, *pic_shape), generator=g) for _ in range(4)]
    liks = []
    for s in lik_shapes:
        l = torch.rand((B, *s), generator=g).clamp_(1e-9, 1.0)
        l.view(B, -1)[:, 0] = 1e-9
        l.view(B, -1)[:, -1] = 1.0
        liks.append(l)
    return [p.to(DEV) for p in pics], [l.to(DEV) for l in liks]


def _want(pics, liks, b):
    """row b from the per-batch reductions applied to image b's slices alone"""
    _, ops = _mods()
    x1h, x1, x2h, x2 = (p[b:b + 1].contiguous() for p in pics)
    row = [ops.sse(x1h, x1), ops.sse(x2h, x2)] + [ops.sum_log(l[b:b + 1].contiguous()) for l in liks]
    return torch.stack(row + [torch.zeros((), dtype=torch.float64, device=DEV)] * (6 - len(row)))


CASES = {
    # 105 elements per image (below one block), likelihood slices of 2, 48, 3 and 7 elements
    "small": (3, (3, 5, 7), [(2,), (3, 4, 4), (3,), (7,)]),
    # one tensor of 1024 * 256 + 37 elements per image: the grid cap and the strided loop, with an odd slice offset
    "grid_cap": (3, (3, 5, 7), [(2,), (1024 * 256 + 37,)]),
    # the CQE stage's distortion-only case; 3 * 33 * 41 = 4059 elements: several blocks, the last one partial
    "no_liks": (3, (3, 33, 41), []),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_rd_rows_are_the_slices_own_reductions(name):
    metrics, _ = _mods()
    B, pic_shape, lik_shapes = CASES[name]
    pics, liks = _case(B, pic_shape, lik_shapes, seed=len(name))
    got = metrics.pair_rd(*pics, liks)
    assert got.shape == (B, 6) and got.dtype == torch.float64
    want = torch.stack([_want(pics, liks, b) for b in range(B)])
    print(name, got.cpu().numpy(), sep="\n")
    assert bool((got == want).all()), (got - want).abs().max()
    assert bool((got[:, :2] > 0).all()) and bool((got[:, 2:2 + len(liks)] < 0).all()) and bool((got[:, 2 + len(liks):] == 0).all())
    # a batch of one has the row of the batch call, and the rows differ from each other (no image read twice)
    for b in range(B):
        one = metrics.pair_rd(*(p[b:b + 1].contiguous() for p in pics), [l[b:b + 1].contiguous() for l in liks])
        assert torch.equal(one, got[b:b + 1]), b
    assert len({tuple(r) for r in got.cpu().tolist()}) == B


def test_pair_rd_on_a_side_stream():
    metrics, _ = _mods()
    pics, liks = _case(3, (3, 5, 7), [(2,), (300,)], seed=5)
    want = metrics.pair_rd(*pics, liks)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = metrics.pair_rd(*pics, liks)
    side.synchronize()
    assert torch.equal(got, want)


def test_pair_rd_refusals_leave_the_output_untouched():
    from masic_amd import _lib
    metrics, ops = _mods()
    pics, liks = _case(2, (3, 5, 7), [(4,)], seed=6)
    out = torch.full((2, 6), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib.masic_metrics_pair_rd_workspace_bytes(2), dtype=torch.uint8, device=DEV)
    arr, cnt = (ctypes.c_void_p * 1)(liks[0].data_ptr()), (ctypes.c_size_t * 1)(4)
    p = [ops._p(t) for t in pics]

    def call(B=2, nliks=1, x2=p[3], liks_=arr):
        return _lib.lib.masic_metrics_pair_rd(p[0], p[1], p[2], x2, 105, liks_, cnt, nliks, B, ops._p(out), ops._p(ws), ops._stream())

    for kw in ({"B": 0}, {"B": 65536}, {"nliks": 5}, {"nliks": -1}, {"x2": None}, {"liks_": None}):
        assert call(**kw) == _lib.ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    assert torch.equal(out, metrics.pair_rd(*pics, liks))
    with pytest.raises(RuntimeError, match="one shape"):
        metrics.pair_rd(pics[0], pics[1], pics[2], pics[3][:, :, :, :6].contiguous(), liks)
    with pytest.raises(RuntimeError, match="at most 4"):
        metrics.pair_rd(*pics, liks * 5)
    with pytest.raises(RuntimeError, match="hold 2 images"):
        metrics.pair_rd(*pics, [liks[0][:1]])
    with pytest.raises(RuntimeError, match="contiguous"):
        metrics.pair_rd(pics[0].transpose(2, 3), *pics[1:], liks)


def _u8_pair(P, shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (P, *shape), dtype=np.uint8)
    b = rng.integers(0, 256, (P, *shape), dtype=np.uint8)
    a.reshape(P, -1)[:, :2], b.reshape(P, -1)[:, :2] = (0, 255), (255, 0)           # the largest difference, both signs, in the head
    a.reshape(P, -1)[:, -1], b.reshape(P, -1)[:, -1] = 255, 0                        # and in the tail
    return a, b


def _np_sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).reshape(len(a), -1).sum(axis=1)


@pytest.mark.parametrize("P,shape", [(3, (5, 7, 3)), (2, (37, 129, 3)), (1, (16,)), (4, (1, 1, 3))])
def test_u8_sse_equals_numpy(P, shape):
    """5 x 7 x 3: pictures start at bytes 105 and 210, unaligned, and hold fewer pieces than lanes; 37 x 129 x 3 = 14319 bytes: several
    blocks of pieces plus head and tail; 16 bytes: one aligned piece alone; 3 bytes: less than one piece"""
    metrics, _ = _mods()
    a, b = _u8_pair(P, shape, seed=P)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = metrics.u8_sse(da, db)
    assert got.shape == (P,) and got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), _np_sse(a, b))
    assert np.array_equal(metrics.u8_sse(da, da).cpu().numpy(), np.zeros(P, dtype=np.int64))
    for p in range(P):                                                               # a picture's sum does not depend on its mates
        assert torch.equal(metrics.u8_sse(da[p:p + 1], db[p:p + 1]), got[p:p + 1])


def test_u8_sse_differently_aligned_stacks():
    """a starts 1 byte and b 2 bytes into their buffers: no 16-byte piece of a lines up with one of b, the bytewise path takes it all"""
    metrics, _ = _mods()
    a, b = _u8_pair(2, (37, 43, 3), seed=9)
    n = a[0].size
    ba, bb = torch.zeros(2 * n + 16, dtype=torch.uint8, device=DEV), torch.zeros(2 * n + 16, dtype=torch.uint8, device=DEV)
    da, db = ba[1:1 + 2 * n].view(2, n), bb[2:2 + 2 * n].view(2, n)
    da.copy_(torch.from_numpy(a.reshape(2, n)))
    db.copy_(torch.from_numpy(b.reshape(2, n)))
    assert da.data_ptr() % 16 == 1 and db.data_ptr() % 16 == 2 and da.is_contiguous()
    assert np.array_equal(metrics.u8_sse(da, db).cpu().numpy(), _np_sse(a, b))
    da2 = bb[1:1 + 2 * n].view(2, n)                                               # and both 1 byte in: head, pieces, tail
    da2.copy_(torch.from_numpy(b.reshape(2, n)))
    assert np.array_equal(metrics.u8_sse(da, da2).cpu().numpy(), _np_sse(a, b))


def test_u8_sse_passes_32_bits():
    metrics, _ = _mods()
    zeros = torch.zeros((2, 160, 160, 3), dtype=torch.uint8, device=DEV)
    full = torch.full((2, 160, 160, 3), 255, dtype=torch.uint8, device=DEV)
    got = metrics.u8_sse(zeros, full).cpu().tolist()
    assert got == [4993920000, 4993920000] and got[0] > 2 ** 32
    assert metrics.u8_sse(full, zeros).cpu().tolist() == got


def test_u8_sse_refusals_leave_the_output_untouched():
    from masic_amd import _lib
    metrics, ops = _mods()
    a = torch.zeros((2, 40), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    ws = torch.empty(_lib.lib.masic_metrics_u8_sse_workspace_bytes(2), dtype=torch.uint8, device=DEV)
    for n, P, b in ((0, 2, a), (40, 0, a), (40, 65536, a), (40, 2, None)):
        assert _lib.lib.masic_metrics_u8_sse(ops._p(a), ops._p(b), n, P, ops._p(out), ops._p(ws), ops._stream()) == _lib.ERR_ARG, (n, P)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7, 7]
    with pytest.raises(RuntimeError, match="one shape"):
        metrics.u8_sse(a, a[:, :39].contiguous())
    with pytest.raises(RuntimeError, match="torch.uint8"):
        metrics.u8_sse(a.float(), a.float())
    with pytest.raises(RuntimeError, match="non-empty"):
        metrics.u8_sse(a[:, :0].contiguous(), a[:, :0].contiguous())
