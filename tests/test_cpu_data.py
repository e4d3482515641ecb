"""The host side of the device-resident stereo dataset (masic_amd/data.py), no GPU: the file lists, the decoder, the draws against a
literal restatement of the reference's __getitem__ (compressai/datasets/utils.py:315-365) on the global `random`, the constructor's
refusals, and the host check of the view descriptors."""
import os
import random

import numpy as np
import pytest
from PIL import Image

from masic_amd import data


def _rgb(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _tree(root, split, names, hw=(6, 7), right_names=None):
    for side, ns in (("left", names), ("right", names if right_names is None else right_names)):
        os.makedirs(os.path.join(root, split, side), exist_ok=True)
        for i, n in enumerate(ns):
            Image.fromarray(_rgb(hw[0], hw[1], i)).save(os.path.join(root, split, side, n))


# ------------------------------------------------------------------------------------------ scan_pairs
def test_scan_pairs_order_and_root_add(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tree(a, "train", ["10.png", "9.png", "1.png"])                 # written out of order; sorted as strings, like the reference
    _tree(b, "train", ["0.png", "z.png"])
    pairs = data.scan_pairs(a, "train")
    assert pairs == [(os.path.join(a, "train", "left", n), os.path.join(a, "train", "right", n)) for n in ("1.png", "10.png", "9.png")]
    both = data.scan_pairs(a, "train", root_add=b)
    assert both[:3] == pairs                                        # root_add's lists are APPENDED, not merged into the order
    assert [os.path.basename(l) for l, _ in both[3:]] == ["0.png", "z.png"]
    assert all(os.path.dirname(r) == os.path.join(b, "train", "right") for _, r in both[3:])


def test_scan_pairs_refusals(tmp_path):
    a = str(tmp_path / "a")
    _tree(a, "train", ["1.png", "2.png"])
    with pytest.raises(RuntimeError, match="Invalid directory"):
        data.scan_pairs(a, "val")
    with pytest.raises(RuntimeError, match="Invalid directory"):
        data.scan_pairs(a, "train", root_add=str(tmp_path / "nothing"))
    m = str(tmp_path / "m")
    _tree(m, "train", ["1.png", "2.png"], right_names=["1.png", "3.png"])
    with pytest.raises(ValueError, match="cannot compare pictures"):
        data.scan_pairs(m, "train")
    c = str(tmp_path / "c")
    _tree(c, "train", ["1.png", "2.png"], right_names=["1.png"])
    with pytest.raises(ValueError):
        data.scan_pairs(c, "train")


# ------------------------------------------------------------------------------------------ decode_rgb8
def test_decode_rgb8_png_modes(tmp_path):
    rgb = _rgb(9, 11, 1)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    got = data.decode_rgb8(str(tmp_path / "rgb.png"))
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, rgb)

    grey = _rgb(9, 11, 2)[..., 0]
    Image.fromarray(grey).save(tmp_path / "l.png")
    assert np.array_equal(data.decode_rgb8(str(tmp_path / "l.png")), np.repeat(grey[..., None], 3, axis=2))

    index = np.random.default_rng(3).integers(0, 256, (9, 11), dtype=np.uint8)
    palette = _rgb(256, 1, 4).reshape(256, 3)
    im = Image.frombytes("P", (11, 9), index.tobytes())
    im.putpalette(palette.reshape(-1).tolist())
    im.save(tmp_path / "p.png")
    assert Image.open(tmp_path / "p.png").mode == "P"
    assert np.array_equal(data.decode_rgb8(str(tmp_path / "p.png")), palette[index])

    rgba = np.concatenate([rgb, _rgb(9, 11, 5)[..., :1]], axis=2)      # alpha is dropped, not blended
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    assert np.array_equal(data.decode_rgb8(str(tmp_path / "rgba.png")), rgb)


def test_decode_rgb8_refuses_16_bit(tmp_path):
    deep = np.random.default_rng(6).integers(0, 65536, (9, 11), dtype=np.uint16)
    Image.fromarray(deep).save(tmp_path / "deep.png")
    with pytest.raises(ValueError, match="16-bit"):
        data.decode_rgb8(str(tmp_path / "deep.png"))
    Image.fromarray(np.random.default_rng(7).random((9, 11), dtype=np.float32)).save(tmp_path / "f.tiff")
    with pytest.raises(ValueError):
        data.decode_rgb8(str(tmp_path / "f.tiff"))


# ------------------------------------------------------------------------------------------ draw_items
def _reference_item(H, W, patch_size, homopic_size, homopatch_size, rho):
    """utils.py:315-365 as written there, on the global `random`"""
    if patch_size[0] > H:
        temp_patch_size_0 = H
    else:
        temp_patch_size_0 = patch_size[0]
    if patch_size[1] > W:
        temp_patch_size_1 = W
    else:
        temp_patch_size_1 = patch_size[1]
    if temp_patch_size_0 == H:
        startH = 0
        startW = 0
    else:
        startH = random.randint(0, H - temp_patch_size_0 - 1)
        startW = random.randint(0, W - temp_patch_size_1 - 1)
    if homopic_size - rho - homopatch_size >= rho:
        x = random.randint(rho, homopic_size - rho - homopatch_size)
        y = random.randint(rho, homopic_size - rho - homopatch_size)
    else:
        x = 0
        y = 0
    return startH, startW, x, y


# larger than the patch, as tall as it only, equal to it, smaller in both, smaller in height only, many times over so the streams
# would drift apart after one misplaced draw
SIZES = [(100, 120), (64, 120), (64, 80), (40, 50), (40, 200), (65, 81), (300, 81)] * 5


@pytest.mark.parametrize("rho", [45, 64, 65, 0])            # 256 - rho - 128 >= rho holds up to rho = 64
def test_draw_items_consumes_random_as_the_reference(rho):
    patch = (64, 80)
    state = random.getstate()
    try:
        random.seed(1234)
        want = [_reference_item(H, W, patch, 256, 128, rho) for H, W in SIZES]
        after = random.random()
    finally:
        random.setstate(state)
    rng = random.Random(1234)
    got = data.draw_items(rng, SIZES, patch, 256, 128, rho)
    assert got == want
    assert rng.random() == after                                 # the same number of draws, not only the same values
    if rho > 64:
        assert all(g[2:] == (0, 0) for g in got)
    else:
        assert all(rho <= g[2] <= 128 - rho and rho <= g[3] <= 128 - rho for g in got)
    assert all(g[:2] == (0, 0) for g, (H, W) in zip(got, SIZES) if H <= 64)         # the quirk: nothing drawn when the crop is as tall
    assert any(g[0] > 0 and g[1] > 0 for g in got)


def test_draw_items_deviation_and_whole_pictures():
    """A crop as wide as the picture but shorter: the reference's randint(0, -1) raises; here start_w = 0 and no draw for it."""
    with pytest.raises(ValueError):
        state = random.getstate()
        try:
            _reference_item(100, 80, (64, 80), 256, 128, 45)
        finally:
            random.setstate(state)
    rng, twin = random.Random(9), random.Random(9)
    (sh, sw, x, y), = data.draw_items(rng, [(100, 80)], (64, 80))
    assert (sh, sw, x, y) == (twin.randint(0, 35), 0, twin.randint(45, 83), twin.randint(45, 83))
    assert rng.random() == twin.random()
    rng, twin = random.Random(10), random.Random(10)
    assert data.draw_items(rng, [(33, 47)] * 3, None) == [(0, 0, twin.randint(45, 83), twin.randint(45, 83)) for _ in range(3)]
    assert data.effective_crop((33, 47), None) == (33, 47) and data.effective_crop((33, 47), (32, 64)) == (32, 47)


# ------------------------------------------------------------------------------------------ constructor refusals
def test_constructor_refusals_need_no_device(tmp_path):
    pics = [_rgb(40, 50, i) for i in range(4)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceStereoFolder.from_arrays(pics[:2], pics[2:], device="cpu")
    with pytest.raises(ValueError, match="one shape"):
        data.DeviceStereoFolder.from_arrays(pics[:2], [pics[2], _rgb(40, 51, 9)], names=["a.png", "b.png"])
    with pytest.raises(ValueError, match=r"c\.png"):                # the first pair whose crop differs is named
        data.DeviceStereoFolder.from_arrays(pics[:2] + [_rgb(30, 50, 8)], pics[2:] + [_rgb(30, 50, 7)], names=["a.png", "b.png", "c.png"],
                                            patch_size=(32, 32))
    with pytest.raises(ValueError, match="one shape"):
        data.DeviceStereoFolder.from_arrays(pics[:1] + [_rgb(41, 50, 8)], pics[2:3] + [_rgb(41, 50, 7)], patch_size=None)
    need = 4 * 40 * 50 * 3                                          # 6000 bytes a picture, a multiple of 16
    with pytest.raises(ValueError, match=str(need)):
        data.DeviceStereoFolder.from_arrays(pics[:2], pics[2:], max_bytes=need - 1)
    with pytest.raises(ValueError):
        data.DeviceStereoFolder.from_arrays(pics[:2], pics[2:3])
    with pytest.raises(ValueError, match="uint8"):
        data.DeviceStereoFolder.from_arrays([pics[0].astype(np.float32)], [pics[1]])

    root = str(tmp_path / "d")
    _tree(root, "train", ["1.png", "2.png"], hw=(40, 50))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceStereoFolder(root, device="cpu")
    with pytest.raises(ValueError, match="max_bytes"):
        data.DeviceStereoFolder(root, max_bytes=1000)
    with pytest.raises(RuntimeError, match="Invalid directory"):
        data.DeviceStereoFolder(root, split="val")
    Image.fromarray(_rgb(41, 50, 3)).save(os.path.join(root, "train", "right", "2.png"))
    with pytest.raises(ValueError, match=r"2\.png"):
        data.DeviceStereoFolder(root)


def test_descriptor_check_on_the_host():
    """What ops.views_prep refuses before it launches (the kernels cannot be asked: a bad read is a fault)."""
    from masic_amd import ops
    good = np.array([[0, 53, 37, 5, 21, 0, 8], [5888, 32, 33, 1, 0, 8, 0]], dtype=np.int64)     # offset W H start_h start_w patch_x patch_y
    arena = 5888 + 33 * 32 * 3
    assert np.array_equal(ops.check_view_descriptors(good, arena, (32, 32), 16, 8), good)
    for row, col, value in ((0, 3, 6), (0, 4, 22), (0, 3, -1), (1, 0, 5904), (1, 0, 5889), (0, 0, -16), (1, 5, 9), (1, 6, -1), (0, 1, 0),
                            (0, 2, 1 << 40)):
        bad = good.copy()
        bad[row, col] = value
        with pytest.raises(RuntimeError, match=f"view {row} "):
            ops.check_view_descriptors(bad, arena, (32, 32), 16, 8)
    with pytest.raises(RuntimeError, match="view 1 "):
        ops.check_view_descriptors(good, arena - 4, (32, 32), 16, 8)
    with pytest.raises(RuntimeError):
        ops.check_view_descriptors(good[:, :6], arena, (32, 32), 16, 8)
    with pytest.raises(RuntimeError):
        ops.check_view_descriptors(good.astype(np.float32), arena, (32, 32), 16, 8)
