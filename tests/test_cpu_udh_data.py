"""CPU tests of the host side of the UDH training batches (masic_amd/udh_data.py, ops.check_udh_view_descriptors): the coefficient
tables against Pillow itself, bit for bit; the restated torchvision geometry; the reference's draws; the descriptor check."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from tests import udh_data_ref as R

# (H, W) -> (oh, ow): the cases the tables were first checked on, then a 12.5-tap window next to a 1.4375 scale, and the scale cap
RESIZE_CASES = (((37, 53), (16, 22)), ((64, 100), (32, 50)), ((860, 1080), (256, 321)), ((300, 200), (384, 256)), ((100, 260), (128, 332)),
                ((256, 300), (256, 300)), ((1080, 860), (642, 512)), ((50, 50), (64, 64)), ((23, 200), (16, 139)), ((256, 300), (16, 18)))


def _U():
    from masic_amd import udh_data
    return udh_data


def _picture(H, W, seed):
    rng = np.random.default_rng(seed)
    pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pic[:H // 3, :W // 4] = 255          # flat regions at both ends of the range: the clip and the coefficient sum
    pic[-(H // 4):, -(W // 3):] = 0
    return pic


def _apply(px, xmin, n, k):
    """One pass along axis 0 of px (uint8 [in, ...]): clip8((2^21 + sum px * k) >> 22), int64 accumulation"""
    out = np.empty((len(xmin),) + px.shape[1:], np.uint8)
    for i in range(len(xmin)):
        acc = np.full(px.shape[1:], 1 << 21, np.int64)
        for j in range(int(n[i])):
            acc += px[int(xmin[i]) + j].astype(np.int64) * int(k[i, j])
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def _resize_by_tables(pic, out_hw):
    """Pillow's order: the horizontal pass first, a pass skipped when its axis keeps its size"""
    U = _U()
    H, W = pic.shape[:2]
    oh, ow = out_hw
    if ow != W:
        pic = _apply(pic.transpose(1, 0, 2), *U.pil_bilinear_tables(W, ow)).transpose(1, 0, 2)
    if oh != H:
        pic = _apply(pic, *U.pil_bilinear_tables(H, oh))
    return pic


@pytest.mark.parametrize("in_hw,out_hw", RESIZE_CASES)
def test_tables_equal_pillow(in_hw, out_hw):
    U = _U()
    pic = _picture(in_hw[0], in_hw[1], 31)
    want = R.pil_resize(pic, out_hw)
    got = _resize_by_tables(pic, out_hw)
    diff = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())
    print(f"tables vs Pillow {in_hw} -> {out_hw}: max difference {diff}")
    assert got.shape == want.shape and diff == 0
    for a, b in ((in_hw[0], out_hw[0]), (in_hw[1], out_hw[1])):
        xmin, n, k = U.pil_bilinear_tables(a, b)
        ks = 2 * int(np.ceil(max(a / b, 1.0))) + 1
        assert k.shape == (b, ks) and xmin.dtype == n.dtype == k.dtype == np.int32
        assert (k >= 0).all() and (xmin >= 0).all() and (n >= 1).all() and (n <= ks).all() and (xmin + n <= a).all()
        assert all((k[i, n[i]:] == 0).all() for i in range(b))
        assert np.abs(k.sum(1) - (1 << 22)).max() <= ks                # int32 accumulation: 255 * sum + 2^21 < 2^31
        assert 255 * int(k.sum(1).max()) + (1 << 21) < 1 << 31
        if a != b:
            assert U.axis_ksize(a, b) == ks
        # a window of positions is the same rows of the whole table
        first, count = b // 3, b - b // 3 - b // 4
        w = U.pil_bilinear_tables(a, b, first, count)
        assert all(np.array_equal(p, q[first:first + count]) for p, q in zip(w, (xmin, n, k)))


def test_resize_geometry():
    U = _U()
    g = U.resize_geometry
    assert g((1080, 860), 256) == ((321, 256), (32, 0))             # portrait (W <= H): int(256 * 1080 / 860) = 321; 65 / 2 -> 32 (half to even)
    assert g((860, 1080), 256) == ((256, 321), (0, 32))             # landscape
    assert g((50, 50), 64) == ((64, 64), (0, 0))                    # square, up-scaled
    assert g((40, 40), 40) == ((40, 40), (0, 0))                    # nothing to do
    assert g((256, 300), 256) == ((256, 300), (0, 22))              # the short side is pic_size already: no pass on either axis
    assert g((323, 256), 256) == ((323, 256), (34, 0))              # 67 / 2 -> 34 (half to even)
    assert g((321, 256), 256) == ((321, 256), (32, 0))              # 65 / 2 -> 32
    assert g((23, 200), 16) == ((16, 139), (0, 62))                 # 123 / 2 = 61.5 -> 62
    assert g((256, 300), 16) == ((16, 18), (0, 1))                  # scale 16, the cap; the longer side comes to 300 / 18 = 16.7
    assert U.axis_ksize(256, 16) == 33 and U.axis_ksize(300, 18) == 35 == U.MAX_KSIZE
    with pytest.raises(ValueError, match="scale above 16"):
        g((272, 300), 16)                                           # 17
    with pytest.raises(ValueError, match="scale above 16"):
        g((300, 257), 16)
    with pytest.raises(ValueError, match="scale above 17"):
        g((32, 79), 2)                                              # 16 on the shorter side, 79 / 4 = 19.75 on the longer
    with pytest.raises(ValueError):
        g((0, 5), 16)
    assert U.axis_ksize(50, 64) == 3 and U.axis_ksize(64, 64) == 0 and U.axis_ksize(860, 256) == 9


def test_draw_udh_items_consumes_random_as_the_reference():
    U = _U()
    for pic, patch, rho in ((256, 128, 45), (16, 8, 2), (64, 32, 8)):
        rng, ref = random.Random(9), random.Random(9)
        got = U.draw_udh_items(rng, 5, pic, patch, rho)
        want = []
        for _ in range(5):                                          # dataset.py:60-62
            x = ref.randint(rho, pic - rho - patch)
            y = ref.randint(rho, pic - rho - patch)
            want.append((x, y))
        assert got == want and rng.getstate() == ref.getstate()
        assert all(rho <= v <= pic - rho - patch for xy in got for v in xy)
    rng = random.Random(9)
    state = rng.getstate()
    assert U.draw_udh_items(rng, 3, 64, 32, 17) == [(0, 0)] * 3 and rng.getstate() == state      # 64 - 17 - 32 < 17: nothing is drawn
    c = U.corners_of([(3, 5), (0, 0)], 8)
    assert c.dtype == np.float32 and np.array_equal(c[0], np.float32([[3, 5], [11, 5], [11, 13], [3, 13]])) and c.shape == (2, 4, 2)


def test_delta_gt_is_the_references_randint_like():
    U = _U()
    rho, seed = 45, 1234
    corners = torch.from_numpy(U.corners_of([(50, 60), (45, 83), (70, 46)], 128)).long()
    torch.manual_seed(seed)
    want = torch.stack([torch.randint_like(c, -rho, rho) for c in corners]).float()           # dataset.py:75, :97, item by item
    gen = torch.Generator().manual_seed(seed)
    got = U.draw_delta_gt(gen, 3, rho)
    assert got.dtype == torch.float32 and got.shape == (3, 4, 2) and torch.equal(got, want)
    assert int(got.min()) >= -rho and int(got.max()) < rho


def test_grey_tail_of_the_kernel_equals_the_torch_chain():
    """The float32 tail the kernel shares with the codec's patches -- ((v / 255 - MEAN) / STD per channel, ((n0 + n1) + n2) / 3, MEAN and
    STD summed left to right in float32 -- against the torch CPU chain of tests/udh_data_ref.py, on every grey level and random colours."""
    f = np.float32
    mean = (f(0.485) + f(0.456) + f(0.406)) / f(3.0)
    std = (f(0.229) + f(0.224) + f(0.225)) / f(3.0)
    assert mean == R.MEAN.numpy()[0] and std == R.STD.numpy()[0]
    rng = np.random.default_rng(5)
    pic = np.concatenate([np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1), rng.integers(0, 256, (768, 3), dtype=np.uint8)]).reshape(32, 32, 3)
    want = R.grey_picture(pic, 32).numpy()[0]
    n = (pic.astype(f) / f(255.0) - mean) / std
    got = ((n[..., 0] + n[..., 1]) + n[..., 2]) / f(3.0)
    assert got.dtype == f and np.array_equal(got, want)


def test_check_udh_view_descriptors():
    from masic_amd import ops
    U = _U()
    S, arena = 16, 1 << 20
    H, W = 37, 53                                                   # -> 16 x 22: ksize 7 both ways
    h, v, ksh, ksv = U.picture_tables((H, W), S)
    assert (ksh, ksv) == (7, 7) and h.size == v.size == S * 9
    words = h.size + v.size
    good = np.array([[0, W, H, 0, h.size, ksh, ksv, 0, 0], [16 * 368, W, H, 0, h.size, ksh, ksv, 8, 8]], dtype=np.int64)
    assert np.array_equal(ops.check_udh_view_descriptors(good, arena, words, (8, 8), S), good)
    packed = ops.pack_udh_view_descriptors(good)
    assert packed.shape == (2, 10) and packed.dtype == np.int32 and packed[1].tolist() == [16 * 368, 0, W, H, 0, h.size, 7, 7, 8, 8]
    for col, value in ((0, arena - 16), (0, 8),                     # a picture past the arena; an offset off the 16-byte grid
                       (4, h.size + 1), (3, words),                 # a table past table_words
                       (7, 9), (8, 9), (7, -1),                     # a rectangle leaving pic_size
                       (5, 9), (6, 0), (6, 5)):                     # a ksize the sizes do not give
        bad = good.copy()
        bad[1, col] = value
        with pytest.raises(RuntimeError, match="view 1 "):
            ops.check_udh_view_descriptors(bad, arena, words, (8, 8), S)
    with pytest.raises(RuntimeError, match="view 0 "):
        ops.check_udh_view_descriptors(good, H * W * 3 - 1, words, (8, 8), S)
    with pytest.raises(RuntimeError, match="view 0 "):
        ops.check_udh_view_descriptors(good, arena, words - 1, (8, 8), S)
    with pytest.raises(RuntimeError):
        ops.check_udh_view_descriptors(good[:, :8], arena, words, (8, 8), S)
    with pytest.raises(RuntimeError):
        ops.check_udh_view_descriptors(good.astype(np.float32), arena, words, (8, 8), S)
    far = good.copy()
    far[0, 1:3] = (300, 272)                                        # 272 rows to 16: scale 17, refused before any launch
    with pytest.raises(ValueError, match="scale above 16"):
        ops.check_udh_view_descriptors(far, arena, words, (8, 8), S)
    # an axis that keeps its size has ksize 0 and needs no table
    same = np.array([[0, 40, 40, 0, 0, 0, 0, 8, 8]], dtype=np.int64)
    assert np.array_equal(ops.check_udh_view_descriptors(same, arena, 1, (32, 32), 40), same)


def test_tables_of_a_dataset_are_laid_out_per_distinct_size():
    U = _U()
    h, v, ksh, ksv = U.picture_tables((64, 100), 16)                # -> 16 x 25, crop origin left = round(9 / 2) = 4
    xmin, n, k = U.pil_bilinear_tables(100, 25, 4, 16)
    assert ksh == 9 and ksv == 9 and np.array_equal(h, np.concatenate([xmin, n, k.reshape(-1)])) and v.size == 16 * 11
    h0, v0, ksh0, ksv0 = U.picture_tables((40, 40), 40)
    assert h0 is None and v0 is None and (ksh0, ksv0) == (0, 0)
    t = U.UDHTables([(64, 100), (16, 20), (64, 100), (16, 16)], 16, "cpu")       # (16, 16): no table; (16, 20): none either, both axes keep their size
    assert sorted(t.entry) == [(16, 16), (16, 20), (64, 100)] and t.entry[(16, 16)] == t.entry[(16, 20)] == (0, 0, 0, 0)
    assert t.entry[(64, 100)] == (0, h.size, 9, 9) and t.words.dtype == torch.int32 and t.words.numel() == h.size + v.size
    assert np.array_equal(t.words.numpy(), np.concatenate([h, v]))
    rows = t.rows([32, 0], [(64, 100), (16, 16)], [(1, 2), (0, 0)])
    assert rows.tolist() == [[32, 100, 64, 0, h.size, 9, 9, 1, 2], [0, 16, 16, 0, 0, 0, 0, 0, 0]]
    img = Image.fromarray(_picture(20, 30, 1))                      # Pillow is the oracle of every table above; keep its filter name pinned
    assert Image.BILINEAR == Image.Resampling.BILINEAR and img.size == (30, 20)
