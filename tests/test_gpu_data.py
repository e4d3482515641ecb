"""GPU tests (-m gpu) of the device-resident stereo dataset: the two batched kernels behind ops.views_prep (masic_amd/csrc/data.hip) on a
ragged arena, and masic_amd.data.DeviceStereoFolder / StereoBatch on top of them.  Every comparison is bitwise: a view of a batch is
ops.pair_prep of that picture and oracle/data_oracle.py's restatement of the reference's per-item chain."""
import os
import random

import numpy as np
import pytest
import torch

from tests import udh_weights as UW

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ((37, 53), (64, 71), (70, 90), (33, 32))      # odd widths: the row starts of a crop hit every byte alignment
_CACHE = {}


def _ops():
    from masic_amd import ops
    return ops


def _data():
    from masic_amd import data
    return data


def _pictures():
    """left and right pictures of SHAPES, with flat 0 and 255 regions"""
    if "pics" not in _CACHE:
        rng = np.random.default_rng(20)
        lefts, rights = [], []
        for H, W in SHAPES:
            for side in (lefts, rights):
                pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                pic[:7, :9] = 255
                pic[-6:, -11:] = 0
                side.append(pic)
        _CACHE["pics"] = (lefts, rights)
    return _CACHE["pics"]


def _dataset(**kw):
    lefts, rights = _pictures()
    args = dict(patch_size=(32, 32), homopic=16, homopatch=8, rho=2, seed=5)
    args.update(kw)
    return _data().DeviceStereoFolder.from_arrays(lefts, rights, names=[f"{i}.png" for i in range(len(lefts))], **args)


def _arena():
    """(the dataset, its pictures in arena order, their device copies)"""
    if "arena" not in _CACHE:
        ds = _dataset()
        lefts, rights = _pictures()
        pics = [p for pair in zip(lefts, rights) for p in pair]
        _CACHE["arena"] = (ds, pics, [torch.from_numpy(p).to(DEV) for p in pics])
    return _CACHE["arena"]


def _rows(ds, pics, views):
    """views: [(picture, start_h, start_w, patch_x, patch_y)] -> descriptor rows in the order of ops.VIEW_DESC_FIELDS"""
    flat = ds.offsets.reshape(-1)
    return np.array([[flat[k], pics[k].shape[1], pics[k].shape[0], sh, sw, px, py] for k, sh, sw, px, py in views], dtype=np.int64)


def _check_views(views, crop, homopic, homopatch, planes=None, patches=None):
    """Every view against ops.pair_prep on its own picture and against the numpy restatement"""
    from oracle import data_oracle as D
    ops = _ops()
    ds, pics, dev = _arena()
    got = ops.views_prep(ds.arena, _rows(ds, pics, views), crop, homopic, homopatch, planes=planes, patches=patches)
    assert got.planes.shape == (len(views), 3) + tuple(crop) and got.patches.shape == (len(views), 1, homopatch, homopatch)
    for p, (k, sh, sw, px, py) in enumerate(views):
        pic, patch = ops.pair_prep(dev[k], (sh, sw), crop, homopic, (px, py), homopatch)
        assert torch.equal(got.planes[p], pic) and torch.equal(got.patches[p], patch), (p, views[p])
        want_pic, want_patch = D.prepare_view(pics[k], sh, sw, crop[0], crop[1], homopic, px, py, homopatch)
        assert np.array_equal(got.planes[p].cpu().numpy(), want_pic) and np.array_equal(got.patches[p].cpu().numpy(), want_patch), (p, views[p])
    return got


# ------------------------------------------------------------------------------------------ 1. the kernels on a ragged arena
def test_arena_layout():
    ds, pics, _ = _arena()
    flat = ds.offsets.reshape(-1)
    assert (flat % 16 == 0).all() and ds.arena.dtype == torch.uint8 and ds.arena.numel() % 16 == 0 == ds.arena.data_ptr() % 16
    assert ds.nbytes == ds.arena.numel() == flat[-1] + 33 * 32 * 3           # the last picture ends where the arena ends
    host = ds.arena.cpu().numpy()
    for k, pic in enumerate(pics):
        assert np.array_equal(host[flat[k]:flat[k] + pic.size].reshape(pic.shape), pic), k
    assert len(ds) == 4 and ds.crop == (32, 32) and ds.sizes == SHAPES


@pytest.mark.parametrize("crop", [(32, 32), (32, 30)])          # 16-byte stores; scalar stores (pw % 4 != 0)
def test_views_vs_pair_prep_and_restatement(crop):
    ds, pics, _ = _arena()
    views = []
    for k, pic in enumerate(pics):
        H, W = pic.shape[:2]
        views.append((k, 0, 0, 0, 0))
        views.append((k, H - crop[0], W - crop[1], 8, 8))              # the last valid start; for the last picture: the arena's last bytes
        views.append((k, (H - crop[0]) // 2, (W - crop[1]) // 3, k % 9, 8 - k % 9))
    _check_views(views, crop, 32 if crop[1] == 30 else 16, 8)          # (32 x 30 -> 32: identity rows, up-scaled columns)


def test_views_crop_equal_to_the_picture_and_offset_output():
    """The whole last picture (33 x 32, ending at the arena's end) and a planes tensor 4 bytes off the 16-byte grid (scalar stores)."""
    _, pics, _ = _arena()
    last = len(pics) - 1
    _check_views([(last, 0, 0, 0, 0), (last - 1, 0, 0, 4, 8)], (33, 32), 16, 8)
    views = [(k, 1, 0, k, 8 - k) for k in range(len(pics))]
    buf = torch.full((len(views) * 3 * 32 * 32 + 1,), -1.0, device=DEV)
    out = buf[1:].view(len(views), 3, 32, 32)
    assert out.data_ptr() % 16 == 4
    got = _check_views(views, (32, 32), 16, 8, planes=out)
    assert got.planes.data_ptr() == out.data_ptr() and float(buf[0]) == -1.0


@pytest.mark.parametrize("crop,homopic", [((32, 32), 16),      # the exact 2x decimation: rounded box mean
                                         ((24, 40), 16),      # fixed-point bilinear down, scales 1.5 and 2.5
                                         ((12, 12), 16)])     # fixed-point bilinear up
def test_views_resize_branches(crop, homopic):
    _, pics, _ = _arena()
    fit = [k for k, p in enumerate(pics) if p.shape[0] >= crop[0] and p.shape[1] >= crop[1]]
    spots = ((0, 0), (8, 8), (3, 5), (8, 0))
    views = [(k, (pics[k].shape[0] - crop[0]) * (i % 2), (pics[k].shape[1] - crop[1]) // (1 + i % 3), *spots[i % 4]) for i, k in enumerate(fit)]
    assert len(views) >= 6
    _check_views(views, crop, homopic, 8)


def test_views_every_segment_shape():
    """The lane layouts of a row: 64 lanes x 4 rows (above), 128 x 2, 256 x 1, and two segments of 192 lanes with idle lanes in the last;
    one long picture of its own (descriptors by hand, the arena built here)."""
    ops = _ops()
    rng = np.random.default_rng(21)
    pic = rng.integers(0, 256, (9, 1101, 3), dtype=np.uint8)
    dev = torch.from_numpy(pic).to(DEV)
    arena = torch.zeros(16 + -(-pic.size // 16) * 16, dtype=torch.uint8, device=DEV)
    arena[16:16 + pic.size] = dev.reshape(-1)
    for crop, start in (((5, 500), (2, 301)), ((3, 1024), (6, 77)), ((6, 1090), (3, 11)), ((6, 1091), (1, 10)), ((9, 1101), (0, 0))):
        got = ops.views_prep(arena, [[16, 1101, 9, start[0], start[1], 2, 3]], crop, 16, 8)
        pic_ref, patch_ref = ops.pair_prep(dev, start, crop, 16, (2, 3), 8)
        assert torch.equal(got.planes[0], pic_ref) and torch.equal(got.patches[0], patch_ref), crop


def test_bad_descriptors_launch_nothing():
    ops = _ops()
    ds, pics, _ = _arena()
    good = [(0, 0, 0, 0, 0), (3, 2, 5, 1, 1)]
    planes = torch.full((2, 3, 32, 32), 7.0, device=DEV)
    patches = torch.full((2, 1, 8, 8), 7.0, device=DEV)
    for bad_view in ((1, 37 - 32 + 1, 0, 0, 0),          # the crop leaves the picture at the bottom
                     (1, 0, 53 - 32 + 1, 0, 0),          # ... at the right
                     (1, 0, 0, 9, 0)):                   # the patch leaves the resized crop
        with pytest.raises(RuntimeError, match="view 1 "):
            ops.views_prep(ds.arena, _rows(ds, pics, [good[0], bad_view]), (32, 32), 16, 8, planes=planes, patches=patches)
    rows = _rows(ds, pics, good)
    rows[0, 0] = ds.arena.numel()                                          # a picture past the arena
    with pytest.raises(RuntimeError, match="view 0 "):
        ops.views_prep(ds.arena, rows, (32, 32), 16, 8, planes=planes, patches=patches)
    rows[0, 0] = ds.offsets[3, 1] + 16                                     # the last picture moved by 16 bytes: its end leaves the arena
    rows[0, 1:3] = (32, 33)
    with pytest.raises(RuntimeError, match="view 0 "):
        ops.views_prep(ds.arena, rows, (32, 32), 16, 8, planes=planes, patches=patches)
    with pytest.raises(RuntimeError):
        ops.views_prep(ds.arena.cpu(), _rows(ds, pics, good), (32, 32), 16, 8)
    torch.cuda.synchronize()
    assert bool((planes == 7.0).all()) and bool((patches == 7.0).all())
    ops.views_prep(ds.arena, _rows(ds, pics, good), (32, 32), 16, 8, planes=planes, patches=patches)      # the good table does write them
    assert not bool((planes == 7.0).any()) and not bool((patches == 7.0).any())


# ------------------------------------------------------------------------------------------ 2. the dataset
def test_batch_is_reproducible_and_independent_of_its_mates():
    data, ops = _data(), _ops()
    _, pics, dev = _arena()
    a, b = _dataset(), _dataset()
    index = [0, 1, 2, 3, 2]
    draws = data.draw_items(random.Random(5), [SHAPES[i] for i in index], (32, 32), 16, 8, 2)
    ba, bb = a.batch(index), b.batch(index)
    for x, y in zip(ba[:5], bb[:5]):
        assert torch.equal(x, y)
    assert ba.index == tuple(index) and ba.names == ("0.png", "1.png", "2.png", "3.png", "2.png")
    assert ba.d1.shape == (5, 3, 32, 32) and ba.homo1.shape == (5, 1, 8, 8) and ba.corners.shape == (5, 4, 2)
    assert ba.d1.is_contiguous() and ba.d2.is_contiguous() and ba.homo1.is_contiguous() and ba.homo2.is_contiguous()
    assert draws[3][:2] == (0, 0) and any(d[0] > 0 for d in draws)      # 33 x 32 cropped to 32 x 32: the documented start_w = 0
    for i, (n, (sh, sw, x, y)) in enumerate(zip(index, draws)):
        # the draws are the reference's for this seed; left and right share the window; the corners are the patch's, clockwise from (x, y)
        left, hl = ops.pair_prep(dev[2 * n], (sh, sw), (32, 32), 16, (x, y), 8)
        right, hr = ops.pair_prep(dev[2 * n + 1], (sh, sw), (32, 32), 16, (x, y), 8)
        assert torch.equal(ba.d1[i], left) and torch.equal(ba.d2[i], right) and torch.equal(ba.homo1[i], hl) and torch.equal(ba.homo2[i], hr), i
        want = np.array([[x, y], [x + 8, y], [x + 8, y + 8], [x, y + 8]], dtype=np.float32)
        assert ba.corners.dtype == torch.float32 and np.array_equal(ba.corners[i].cpu().numpy(), want), i
        one = a.batch([n], draws=[draws[i]])
        for x1, xb in zip(one[:5], ba[:5]):
            assert torch.equal(x1[0], xb[i]), i
    assert not torch.equal(a.batch(index).d1, ba.d1)                    # the generator moved on


def test_batches_cover_an_epoch():
    ds = _dataset(seed=11)
    for shuffle in (True, False):
        got = [b.index for b in ds.batches(3, shuffle=shuffle)]
        assert [len(g) for g in got] == [3]                               # drop_last: 4 pairs, one batch of 3
        got = [b.index for b in ds.batches(3, shuffle=shuffle, drop_last=False)]
        assert [len(g) for g in got] == [3, 1] and sorted(i for g in got for i in g) == [0, 1, 2, 3]
        if not shuffle:
            assert got == [(0, 1, 2), (3,)]
    orders = {tuple(i for b in _dataset(seed=s).batches(2) for i in b.index) for s in range(6)}
    assert len(orders) > 1 and all(sorted(o) == [0, 1, 2, 3] for o in orders)


def test_whole_pictures():
    """patch_size=None: the pictures are the crops (here 33 x 32, the scalar-free vector path on an odd number of rows)"""
    lefts, rights = _pictures()
    ds = _data().DeviceStereoFolder.from_arrays([lefts[3], rights[3]], [rights[3], lefts[3]], patch_size=None, homopic=16, homopatch=8, rho=9)
    b = ds.batch([1, 0])
    assert b.d1.shape == (2, 3, 33, 32) and np.array_equal(b.corners[0].cpu().numpy(), np.float32([[0, 0], [8, 0], [8, 8], [0, 8]]))
    want = rights[3].astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    assert np.array_equal(b.d1[0].cpu().numpy(), want) and np.array_equal(b.d2[1].cpu().numpy(), want)


def test_from_disk_equals_from_arrays(tmp_path):
    from PIL import Image
    data = _data()
    rng = np.random.default_rng(22)
    names = ["b.png", "a.png", "c.png"]
    lefts = [rng.integers(0, 256, (40 + i, 45, 3), dtype=np.uint8) for i in range(3)]
    rights = [rng.integers(0, 256, (40 + i, 45, 3), dtype=np.uint8) for i in range(3)]
    for n, l, r in zip(names, lefts, rights):
        for side, pic in (("left", l), ("right", r)):
            os.makedirs(tmp_path / "train" / side, exist_ok=True)
            Image.fromarray(pic).save(tmp_path / "train" / side / n)
    args = dict(patch_size=(32, 32), homopic=16, homopatch=8, rho=1, seed=3)
    disk = data.DeviceStereoFolder(str(tmp_path), **args)
    order = [1, 0, 2]                                                    # sorted names: a, b, c
    mem = data.DeviceStereoFolder.from_arrays([lefts[i] for i in order], [rights[i] for i in order], names=sorted(names), **args)
    assert disk.names == mem.names == ("a.png", "b.png", "c.png") and disk.nbytes == mem.nbytes and torch.equal(disk.arena, mem.arena)
    bd, bm = disk.batch([2, 0, 1]), mem.batch([2, 0, 1])
    for x, y in zip(bd[:5], bm[:5]):
        assert torch.equal(x, y)
    assert bd.names == bm.names == ("c.png", "a.png", "b.png")


def test_upload_in_several_runs(monkeypatch):
    """Staging buffers smaller than the arena: the runs of pictures go through two pinned buffers in turn"""
    data = _data()
    ds, _, _ = _arena()
    monkeypatch.setattr(data, "STAGE_BYTES", 16)                          # -> one picture (the largest, 70 x 90) per buffer
    assert torch.equal(_dataset().arena, ds.arena)


# ------------------------------------------------------------------------------------------ 3. into the training step
def _udh32():
    if "udh" not in _CACHE:
        import model
        net = model.Net(patch_size=32).to(DEV).eval()
        UW.fill(net, UW.WEIGHT_SEED)
        _CACHE["udh"] = net
    return _CACHE["udh"]


def _big_dataset():
    rng = np.random.default_rng(23)
    lefts = [rng.integers(0, 256, (70 + i, 90, 3), dtype=np.uint8) for i in range(3)]
    rights = [np.roll(l, 2, axis=1) for l in lefts]
    return _data().DeviceStereoFolder.from_arrays(lefts, rights, patch_size=(64, 64), homopic=64, homopatch=32, rho=8, seed=1)


def test_h_matrix_is_the_drivers_chain():
    from masic_amd import homography
    net = _udh32()
    b = _big_dataset().batch([0, 2, 1])
    assert b.homo1.shape == (3, 1, 32, 32) and b.d1.shape == (3, 3, 64, 64)
    rel = b.corners - b.corners[:, 0].view(-1, 1, 2)
    delta = net(b.homo1, b.homo2)
    want = homography.h_matrix_from_corners(rel, delta, (64, 64), (32, 32))
    got = b.h_matrix(net)
    assert got.shape == (3, 3, 3) and not got.requires_grad and torch.equal(got, want) and bool(torch.isfinite(got).all())

    class Shifted(torch.nn.Module):             # delta's producer with a parameter of its own (model.Net itself records no graph)
        def __init__(self):
            super().__init__()
            self.shift = torch.nn.Parameter(torch.zeros(4, 2, device=DEV))

        def forward(self, a, c):
            return net(a, c) + self.shift

    shifted = Shifted()
    h = b.h_matrix(shifted, detach=False)
    assert h.requires_grad and torch.equal(h.detach(), want)
    h.sum().backward()
    g = shifted.shift.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert not b.h_matrix(shifted).requires_grad


def test_one_training_step_on_a_batch():
    import MASIC
    import model
    from masic_amd import synth, train
    udh = model.Net(patch_size=32).to(DEV).eval()
    UW.fill(udh, UW.WEIGHT_SEED)
    with torch.no_grad():
        udh.fc[5].weight.zero_()            # the offsets are the last layer's bias, within 0.1 px: a homography next to the identity
    b = _big_dataset().batch([0, 1])
    h = b.h_matrix(udh)
    assert float((h - torch.eye(3, device=DEV)).abs().max()) < 0.5
    net = MASIC.HSIC(32, 48, 3)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=21))
    net = net.to(DEV).train()
    opt, aux_opt = train.make_optimizers(net)
    crit, aux = train.train_step(net, opt, aux_opt, b.d1, b.d2, h, 0.01)
    for v in (crit["loss"], crit["bpp_loss"], crit["mse_loss"], aux):
        assert np.isfinite(float(v.detach()))
