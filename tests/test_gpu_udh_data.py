"""GPU tests (-m gpu) of the UDH training batches cut on the device: masic_udh_views_prep (masic_amd/csrc/data.hip) behind
ops.udh_views_prep, and DeviceStereoFolder.udh_batch / udh_batches on top of it.  Every comparison is bitwise (torch.equal) against
the host chain of tests/udh_data_ref.py: Pillow's Image.resize(BILINEAR), then the torch CPU operations of ToTensor / Normalize / mean.

Shapes are the smallest that reach every branch of the kernel: both passes, no pass (the picture has pic_size already, with and without
a crop offset), up-scaling (ksize 3), the largest ksize served (35), xmin clamped at 0 and xmax at the size (the first and last tile of
every picture), tiles cut at the right and bottom edge, a row window of several 32-row chunks (64 x 100 and 256 x 300 at 16), and
both store paths (out_w % 4 == 0 or not)."""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests import udh_data_ref as R
from tests import udh_weights as UW
from tests.udh_train_cases import load_udh_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}

# name -> ((H, W) of each pair, pic_size, patch_size, rho)
CASES = {
    "down": (((37, 53), (64, 100), (23, 200)), 16, 8, 2),      # both passes; 23 x 200: a 1.44 scale next to a 12.5-tap window
    "up": (((50, 50),), 64, 32, 8),                            # up-scaling: ksize 3
    "same": (((40, 40),), 40, 16, 4),                          # no pass on either axis; tiles of 16, 16, 8
    "same_offset": (((40, 50),), 40, 16, 4),                   # no pass, the centre crop starts at column 5
    "cap": (((256, 300),), 16, 8, 2),                          # scale 16 on the shorter side, 16.7 (ksize 35) on the longer
    "scalar": (((96, 128),), 32, 10, 2),                       # out_w % 4 != 0: scalar stores, tiles of 10 columns
}


def _ops():
    from masic_amd import ops
    return ops


def _data():
    from masic_amd import data
    return data


def _pictures(sizes, seed):
    rng = np.random.default_rng(seed)
    lefts, rights = [], []
    for H, W in sizes:
        for side in (lefts, rights):
            pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            pic[:H // 3, :W // 4] = 255
            pic[-(H // 4):, -(W // 3):] = 0
            side.append(pic)
    return lefts, rights


def _case(name):
    """(dataset, lefts, rights, reference grey pictures [(img_a, img_b)], pic_size, patch_size, rho) -- computed once per case"""
    if name not in _CACHE:
        sizes, S, p, rho = CASES[name]
        lefts, rights = _pictures(sizes, 40 + len(name))
        ds = _data().DeviceStereoFolder.from_arrays(lefts, rights, patch_size=(16, 16), seed=7)
        ref = [(R.grey_picture(l, S), R.grey_picture(r, S)) for l, r in zip(lefts, rights)]
        _CACHE[name] = (ds, lefts, rights, ref, S, p, rho)
    return _CACHE[name]


def _windows(S, p, rho):
    """The four corners of the range the reference draws from, and (0, 0)"""
    lo, hi = rho, S - rho - p
    assert hi >= lo
    return [(lo, lo), (hi, lo), (lo, hi), (hi, hi), (0, 0)]


# ------------------------------------------------------------------------------------------ 1. the kernel against the host chain
@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_equals_the_host_chain(name):
    ds, lefts, rights, ref, S, p, rho = _case(name)
    wins = _windows(S, p, rho)
    index = [i for i in range(len(ds)) for _ in wins]
    draws = [w for _ in range(len(ds)) for w in wins]
    b = ds.udh_batch(index, draws=draws, pic_size=S, patch_size=p, rho=rho, want_img_b=True)
    B = len(index)
    assert b.img_a.shape == b.img_b.shape == (B, 1, S, S) and b.patch_a.shape == b.patch_b.shape == (B, 1, p, p)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (b.img_a, b.img_b, b.patch_a, b.patch_b, b.corners))
    assert b.delta_gt is None and b.index == tuple(index) and b.names == tuple(ds.names[i] for i in index)
    got = [t.cpu() for t in (b.img_a, b.img_b, b.patch_a, b.patch_b)]
    for k, (i, (x, y)) in enumerate(zip(index, draws)):
        want = (ref[i][0], ref[i][1], ref[i][0][:, y:y + p, x:x + p], ref[i][1][:, y:y + p, x:x + p])
        for what, g, w in zip(("img_a", "img_b", "patch_a", "patch_b"), got, want):
            assert torch.equal(g[k], w), (name, what, k, i, (x, y), float((g[k] - w).abs().max()))
        assert np.array_equal(b.corners[k].cpu().numpy(), np.float32([[x, y], [x + p, y], [x + p, y + p], [x, y + p]]))
    # the same through the item function of the reference module, which cuts the windows itself
    a, bb, pa, pb = R.item(lefts[0], rights[0], wins[3][0], wins[3][1], S, p)
    assert torch.equal(got[0][3], a) and torch.equal(got[1][3], bb) and torch.equal(got[2][3], pa) and torch.equal(got[3][3], pb)


def test_default_batch_has_no_img_b_and_an_offset_output():
    """want_img_b=False: launch 1 takes the B left views only; and ops.udh_views_prep into a tensor 4 bytes off the 16-byte grid
    (scalar stores although out_w % 4 == 0)."""
    ops = _ops()
    ds, _, _, ref, S, p, rho = _case("down")
    b = ds.udh_batch([2, 0], draws=[(2, 6), (6, 2)], pic_size=S, patch_size=p, rho=rho)
    assert b.img_b is None and b.delta_gt is None and b.img_a.shape == (2, 1, S, S) and b.patch_b.shape == (2, 1, p, p)
    assert torch.equal(b.img_a[0].cpu(), ref[2][0]) and torch.equal(b.patch_b[1].cpu(), ref[0][1][:, 2:2 + p, 6:6 + p])
    t = ds.udh_tables(S)
    rows = t.rows([int(ds.offsets[1, 1]), int(ds.offsets[2, 0])], [ds.sizes[1], ds.sizes[2]], [(0, 0), (0, 0)])
    buf = torch.full((2 * S * S + 1,), -1.0, device=DEV)
    out = buf[1:].view(2, 1, S, S)
    assert out.data_ptr() % 16 == 4
    got = ops.udh_views_prep(ds.arena, rows, t.words, (S, S), S, out=out)
    assert got.data_ptr() == out.data_ptr() and float(buf[0]) == -1.0
    assert torch.equal(got[0].cpu(), ref[1][1]) and torch.equal(got[1].cpu(), ref[2][0])


# ------------------------------------------------------------------------------------------ 2. the batch
def test_patches_are_slices_of_the_pictures():
    ds, _, _, _, S, p, rho = _case("down")
    fresh = _data().DeviceStereoFolder.from_arrays(*_pictures(CASES["down"][0], 40 + len("down")), patch_size=(16, 16), seed=3)
    b = fresh.udh_batch([0, 1, 2, 1], pic_size=S, patch_size=p, rho=rho, want_img_b=True)
    xy = b.corners[:, 0].cpu().numpy().astype(int)
    assert len({tuple(v) for v in xy}) > 1 and (xy >= rho).all() and (xy <= S - rho - p).all()
    for k, (x, y) in enumerate(xy):
        assert torch.equal(b.patch_a[k], b.img_a[k, :, y:y + p, x:x + p]) and torch.equal(b.patch_b[k], b.img_b[k, :, y:y + p, x:x + p]), k


def test_mixed_sizes_and_independence_of_batch_mates():
    """Three picture sizes in one batch; a view's bits depend neither on its mates nor on its position"""
    ds, _, _, _, S, p, rho = _case("down")
    index, draws = [0, 1, 2, 1, 0], [(2, 3), (6, 2), (4, 4), (2, 6), (5, 5)]
    b = ds.udh_batch(index, draws=draws, pic_size=S, patch_size=p, rho=rho, want_img_b=True)
    rev = ds.udh_batch(index[::-1], draws=draws[::-1], pic_size=S, patch_size=p, rho=rho, want_img_b=True)
    for k, (i, d) in enumerate(zip(index, draws)):
        one = ds.udh_batch([i], draws=[d], pic_size=S, patch_size=p, rho=rho, want_img_b=True)
        for x1, xb, xr in zip(one[:5], b[:5], rev[:5]):
            assert torch.equal(x1[0], xb[k]) and torch.equal(xr[len(index) - 1 - k], xb[k]), k


def test_reproducible_from_the_seed():
    sizes = CASES["down"][0]
    mk = lambda seed: _data().DeviceStereoFolder.from_arrays(*_pictures(sizes, 50), patch_size=(16, 16), seed=seed)  # noqa: E731
    a, b, c = mk(11), mk(11), mk(12)
    kw = dict(pic_size=16, patch_size=8, rho=2, want_img_b=True, want_delta_gt=True)
    ba, bb, bc = a.udh_batch([0, 1, 2], **kw), b.udh_batch([0, 1, 2], **kw), c.udh_batch([0, 1, 2], **kw)
    for x, y in zip(ba[:6], bb[:6]):
        assert torch.equal(x, y)
    assert not torch.equal(ba.corners, bc.corners) or not torch.equal(ba.delta_gt, bc.delta_gt)
    # the draws are the reference's for this seed: random.Random for the windows, torch's generator for delta_gt
    from masic_amd import udh_data
    draws = udh_data.draw_udh_items(random.Random(11), 3, 16, 8, 2)
    assert np.array_equal(ba.corners.cpu().numpy(), udh_data.corners_of(draws, 8))
    torch.manual_seed(11)
    want = torch.stack([torch.randint_like(torch.zeros(4, 2, dtype=torch.int64), -2, 2) for _ in range(3)]).float()
    assert ba.delta_gt.shape == (3, 4, 2) and torch.equal(ba.delta_gt.cpu(), want)
    orders = [tuple(i for bt in mk(s).udh_batches(2, pic_size=16, patch_size=8, rho=2, drop_last=False) for i in bt.index) for s in range(6)]
    assert all(sorted(o) == [0, 1, 2] for o in orders) and len(set(orders)) > 1
    assert [bt.index for bt in a.udh_batches(2, shuffle=False, pic_size=16, patch_size=8, rho=2)] == [(0, 1)]      # drop_last


def test_codec_batches_do_not_see_the_udh_batches():
    sizes = ((37, 53), (64, 71), (70, 90), (33, 32))
    mk = lambda: _data().DeviceStereoFolder.from_arrays(*_pictures(sizes, 51), patch_size=(32, 32), homopic=16, homopatch=8, rho=2, seed=5)  # noqa: E731
    plain, mixed, udh_only = mk(), mk(), mk()
    kw = dict(pic_size=16, patch_size=8, rho=2)
    want = [plain.batch([0, 1, 2, 3]), plain.batch([3, 1]), *plain.batches(2)]
    u1 = mixed.udh_batch([0, 1, 2, 3], **kw)
    got = [mixed.batch([0, 1, 2, 3])]
    u2 = list(mixed.udh_batches(2, **kw))
    got.append(mixed.batch([3, 1]))
    u3 = mixed.udh_batch([2, 2], **kw)
    got.extend(mixed.batches(2))
    assert len(want) == len(got) == 4
    for w, g in zip(want, got):
        assert w.index == g.index
        for x, y in zip(w[:5], g[:5]):
            assert torch.equal(x, y)
    # and the other way round: the UDH stream is what it is without any codec batch
    v1, v2, v3 = udh_only.udh_batch([0, 1, 2, 3], **kw), list(udh_only.udh_batches(2, **kw)), udh_only.udh_batch([2, 2], **kw)
    for a, b in zip([u1, *u2, u3], [v1, *v2, v3]):
        assert a.index == b.index and torch.equal(a.corners, b.corners) and torch.equal(a.patch_b, b.patch_b)


# ------------------------------------------------------------------------------------------ 3. bad descriptors and tables
def test_bad_descriptors_and_tables_write_nothing():
    """The wrapper refuses a bad row before it launches.  The kernel, given the same rows past that check, skips the view: its outputs
    keep the sentinel, the good view of the same call is correct, nothing is read outside the arena or the tables."""
    from masic_amd._lib import check, lib
    ops = _ops()
    ds, _, _, ref, S, p, rho = _case("down")
    t = ds.udh_tables(S)
    words = t.words.numel()
    good = t.rows([int(ds.offsets[0, 0]), int(ds.offsets[1, 0])], [ds.sizes[0], ds.sizes[1]], [(2, 6), (6, 2)])
    want0 = ref[0][0][:, 6:6 + p, 2:2 + p]
    want1 = ref[1][0][:, 2:2 + p, 6:6 + p]
    f = {n: i for i, n in enumerate(ops.UDH_VIEW_DESC_FIELDS)}
    variants = [("offset", ds.arena.numel()),                      # a picture past the arena
                ("H", ds.sizes[1][0] + 4096),                      # ... whose end leaves it (ksize 0 no longer fits either)
                ("v_table", words - 16),                           # a table past table_words
                ("h_table", words),
                ("x0", S - p + 1), ("y0", -1),                     # a rectangle leaving pic_size
                ("h_ksize", 7), ("v_ksize", 0)]                    # a ksize the sizes do not give (64 x 100 -> 16 x 25: 9 and 9)
    out = torch.full((2, 1, p, p), 7.0, device=DEV)
    for name, value in variants:
        rows = good.copy()
        rows[1, f[name]] = value
        with pytest.raises((RuntimeError, ValueError)):
            ops.udh_views_prep(ds.arena, rows, t.words, (p, p), S, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    stream = ops._stream()
    for name, value in variants:
        rows = good.copy()
        rows[1, f[name]] = value
        dev_rows = torch.from_numpy(ops.pack_udh_view_descriptors(rows)).to(DEV)
        out.fill_(7.0)
        check(lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(t.words), words, ops._p(dev_rows), 2, p, p, S, ops._p(out), stream))
        torch.cuda.synchronize()
        assert bool((out[1] == 7.0).all()) and torch.equal(out[0].cpu(), want0), name
    # table CONTENT that leaves its range (every xmin of the tables far outside the picture): the tiles that read it are skipped
    spoiled = t.words.clone()
    h_table = int(good[1, f["h_table"]])
    spoiled[h_table:h_table + S] = 1 << 20
    dev_rows = torch.from_numpy(ops.pack_udh_view_descriptors(good)).to(DEV)
    out.fill_(7.0)
    check(lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(spoiled), words, ops._p(dev_rows), 2, p, p, S, ops._p(out), stream))
    torch.cuda.synchronize()
    assert bool((out[1] == 7.0).all()) and torch.equal(out[0].cpu(), want0)
    # the good rows do write both
    got = ops.udh_views_prep(ds.arena, good, t.words, (p, p), S, out=out)
    assert torch.equal(got[0].cpu(), want0) and torch.equal(got[1].cpu(), want1)
    # argument errors of the C entry are reported, not launched
    assert lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(t.words), words, None, 2, p, p, S, ops._p(out), stream) == -1
    assert lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(t.words), words, ops._p(dev_rows), 65536, p, p, S, ops._p(out), stream) == -1
    assert lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(t.words), words, ops._p(dev_rows), 2, 0, p, S, ops._p(out), stream) == -1
    assert lib.masic_udh_views_prep(ops._p(ds.arena), ds.arena.numel(), ops._p(t.words), words, ops._p(dev_rows), 2, p, p, S,
                                    ctypes.c_void_p(out.data_ptr() + 2), stream) == -1                 # misaligned output
    with pytest.raises(RuntimeError):
        ops.udh_views_prep(ds.arena.cpu(), good, t.words, (p, p), S)


def test_scale_above_the_cap_is_refused_before_any_launch():
    lefts, rights = _pictures(((272, 300),), 52)
    ds = _data().DeviceStereoFolder.from_arrays(lefts, rights, patch_size=(16, 16), seed=1)
    with pytest.raises(ValueError, match="scale above 16"):
        ds.udh_batch([0], pic_size=16, patch_size=8, rho=2)
    assert ds.udh_batch([0], pic_size=32, patch_size=8, rho=2).img_a.shape == (1, 1, 32, 32)      # 8.5: served


# ------------------------------------------------------------------------------------------ 4. into the training step
def test_one_training_step_equals_the_step_on_host_made_tensors():
    """udh_train.Net(32) in training mode with fixed dropout masks, photometric loss, backward: on a UDHBatch and on the tensors of
    tests/udh_data_ref.py uploaded from the host.  Both steps run in the library's deterministic mode, as the step's own
    reproducibility test does (tests/test_gpu_udh_train.py): outside it the convolutions' weight gradients are summed with float
    atomics, and two runs on the very same tensors differ in their last bits.  Inside it equal inputs give equal bits."""
    from masic_amd import determinism
    M = load_udh_model()
    S, p, rho = 64, 32, 8
    sizes = ((70, 90), (128, 96), (64, 64))
    lefts, rights = _pictures(sizes, 53)
    rights = [np.roll(l, 2, axis=1) for l in lefts]                  # a second view that resembles the first
    ds = _data().DeviceStereoFolder.from_arrays(lefts, rights, patch_size=(16, 16), seed=2)
    b = ds.udh_batch([0, 1, 2], pic_size=S, patch_size=p, rho=rho)
    xy = b.corners[:, 0].cpu().numpy().astype(int)
    items = [R.item(lefts[i], rights[i], int(x), int(y), S, p) for i, (x, y) in enumerate(xy)]
    img_a, patch_a, patch_b = (torch.stack([it[k] for it in items]).to(DEV) for k in (0, 2, 3))
    corners = torch.from_numpy(np.float32([[[x, y], [x + p, y], [x + p, y + p], [x, y + p]] for x, y in xy])).to(DEV)
    assert torch.equal(img_a, b.img_a) and torch.equal(patch_a, b.patch_a) and torch.equal(patch_b, b.patch_b) and torch.equal(corners, b.corners)
    net = M.Net(patch_size=p).to(DEV)
    UW.fill(net, UW.WEIGHT_SEED)
    net.train()
    rs = np.random.default_rng(54)
    masks = tuple(torch.from_numpy((rs.random((3, k)) >= 0.5).astype(np.uint8)).to(DEV) for k in (128 * (p // 8) ** 2, 1024))

    def step(pa, pb, img, cn):
        net.zero_grad(set_to_none=True)
        delta = net(pa, pb, dropout_masks=masks)
        loss = M.photometric_loss(delta, img, pb, cn)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: q.grad.clone() for n, q in net.named_parameters()}

    with determinism.deterministic():
        l1, g1 = step(b.patch_a, b.patch_b, b.img_a, b.corners)
        l2, g2 = step(patch_a, patch_b, img_a, corners)
    assert bool(torch.isfinite(l1)) and float(l1) > 0 and len(g1) == 20
    assert torch.equal(l1, l2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    assert any(float(g.abs().max()) > 0 for g in g1.values())
