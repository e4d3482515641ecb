"""The training batch of the homography net (UDH), drawn on the GPU: the item of the reference's udh/udh/dataset.py (SyntheticDataset)
out of the device-resident arena of masic_amd.data.DeviceStereoFolder.

The reference prepares an item on the host: PIL opens both pictures, torchvision's Resize(pic_size) -- PIL's antialiased bilinear --,
CenterCrop(pic_size), ToTensor, Normalize with scalar MEAN / STD, the mean over the channels, then one window (x, y) of patch_size cut
from both views.  Here the host draws (x, y) per item (draw_udh_items) and, once per dataset, computes PIL's coefficient tables for
each distinct picture size (pil_bilinear_tables); everything per pixel runs in masic_udh_views_prep (masic_amd/csrc/data.hip), two
launches per batch:

    ds = DeviceStereoFolder("/data/instereo2k", "train")
    for b in ds.udh_batches(8):
        delta = net(b.patch_a, b.patch_b)
        loss = photometric_loss(delta, b.img_a, b.patch_b, b.corners)

Parity.  The resize is PINNED to Pillow: its arithmetic is integer end to end (22-bit coefficients, uint8 after each pass) and the
tables are computed in float64 by the steps of Pillow's precompute_coeffs / normalize_coeffs_8bpc, so a view has the bits of
Image.resize(..., Image.BILINEAR) followed by the torch CPU chain (tests/udh_data_ref.py).  torchvision is not installed where this was
written: its output-size rule (Resize(int)) and its crop origin (CenterCrop) are RESTATED in resize_geometry from its source, parity
for those two rules is unpinned.

Deviations from the reference.  It opens the file with PIL without converting, so a greyscale PNG gives it ONE channel, whose "mean
over channels" is the value n itself; the arena holds three equal channels and ((n + n) + n) / 3 can differ from n in the last bit.
Likewise RGBA: the arena has dropped alpha, the reference would average four normalised channels, alpha among them."""
import collections
import math

import numpy as np

PRECISION_BITS = 22          # Pillow's 8-bit resampling: coefficients are int(0.5 + w * 2^22)
MAX_SCALE = 16               # the largest Resize served: shorter side / pic_size
MAX_KSIZE = 35               # the kernel's taps per position: ceil(in / out) <= 17 on the longer side, whose output size is rounded down


def axis_ksize(in_size, out_size):
    """Taps per output position of one axis as Pillow allocates them: 2 * ceil(max(in / out, 1)) + 1; 0 when the axis keeps its size
    (Pillow runs no pass over it, and neither does the kernel)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size == out_size:
        return 0
    return 2 * int(math.ceil(max(in_size / out_size, 1.0))) + 1


def resize_geometry(size_hw, pic_size):
    """((oh, ow), (top, left)): the size Resize(pic_size) gives a picture of size_hw = (H, W), and the origin of CenterCrop(pic_size) in
    it.  Both rules are restated from torchvision's source, which is not on the machine this was written on -- parity for them is
    unpinned (the resize itself is pinned to Pillow):
      Resize(int S):  if W <= H: ow, oh = S, int(S * H / W)   else: oh, ow = S, int(S * W / H)      (the shorter side becomes S)
      CenterCrop(S):  top = int(round((oh - S) / 2.0)), left = int(round((ow - S) / 2.0))           (Python's round: half to even)
    ValueError for an empty picture or a scale the kernel does not serve: above 16 on the shorter side (the scale Resize is asked
    for), or ceil(in / out) above 17 on the longer one, whose rounded-down output size raises its scale a little (256 x 300 at
    pic_size 16 is served: 16 and 300 / 18 = 16.7; a pic_size below 16 can push the longer side further)."""
    H, W, S = int(size_hw[0]), int(size_hw[1]), int(pic_size)
    if H < 1 or W < 1 or S < 1:
        raise ValueError(f"resize_geometry: picture {H} x {W}, pic_size {S}")
    if W <= H:
        ow, oh = S, int(S * H / W)
    else:
        oh, ow = S, int(S * W / H)
    if min(H, W) > MAX_SCALE * S:
        raise ValueError(f"resize_geometry: {min(H, W)} to {S} is a scale above {MAX_SCALE} (picture {H} x {W})")
    if max(axis_ksize(H, oh), axis_ksize(W, ow)) > MAX_KSIZE:
        raise ValueError(f"resize_geometry: {H} x {W} to {oh} x {ow} is a scale above {MAX_SCALE + 1} on the longer side (pic_size {S})")
    top = int(round((oh - S) / 2.0))
    left = int(round((ow - S) / 2.0))
    return (oh, ow), (top, left)


def pil_bilinear_tables(in_size, out_size, first=0, count=None):
    """(xmin[count], n[count], k[count][ksize]) int32: the taps of output positions first .. first + count - 1 of one axis resized from
    in_size to out_size by PIL's BILINEAR filter, by the steps of Pillow's precompute_coeffs and normalize_coeffs_8bpc in float64:
        scale = in / out; filterscale = max(scale, 1); support = filterscale; ksize = 2 * ceil(support) + 1
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0); xmax = min(int(center + support + 0.5), in)        (int: towards zero)
        w[x] = triangle((x + xmin - center + 0.5) * (1 / filterscale)), x < xmax - xmin; ww = their sum, added left to right
        k[x] = int(0.5 + (w[x] / ww) * 2^22)
    (Pillow multiplies by the reciprocal 1 / filterscale, so this does.)  Unused slots of k are 0; the output pixel is
    clip8((2^21 + sum_x px[xmin + x] * k[x]) >> 22).  Coefficients are not negative and sum to 2^22 within a few units."""
    in_size, out_size, first = int(in_size), int(out_size), int(first)
    count = out_size - first if count is None else int(count)
    if in_size < 1 or out_size < 1 or first < 0 or count < 0 or first + count > out_size:
        raise ValueError(f"pil_bilinear_tables: positions {first} .. {first + count} of an axis resized from {in_size} to {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin_out = np.zeros(count, np.int32)
    n_out = np.zeros(count, np.int32)
    k_out = np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        x = np.arange(xmax, dtype=np.float64)
        w = 1.0 - np.abs((x + xmin - center + 0.5) * ss)
        w[w <= 0.0] = 0.0                                   # the filter is 0 from |x| = 1 on
        ww = 0.0
        for v in w:                                         # left to right, as Pillow adds them
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        xmin_out[i], n_out[i] = xmin, xmax
        k_out[i, :xmax] = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)       # not negative: truncation is int()
    return xmin_out, n_out, k_out


def picture_tables(size_hw, pic_size):
    """The table words of one picture size: (h_words int32 or None, v_words int32 or None, h_ksize, v_ksize), each table laid out as
    masic_udh_views_prep reads it -- xmin[S], n[S], k[S][ksize] for the S = pic_size positions that survive the centre crop; None and
    ksize 0 for an axis that keeps its size."""
    (oh, ow), (top, left) = resize_geometry(size_hw, pic_size)
    out = []
    for in_size, out_size, first in ((int(size_hw[1]), ow, left), (int(size_hw[0]), oh, top)):
        if in_size == out_size:
            out.append(None)
        else:
            xmin, n, k = pil_bilinear_tables(in_size, out_size, first, int(pic_size))
            out.append(np.concatenate([xmin, n, k.reshape(-1)]).astype(np.int32))
    return out[0], out[1], axis_ksize(size_hw[1], ow), axis_ksize(size_hw[0], oh)


def draw_udh_items(rng, n, pic_size=256, patch_size=128, rho=45):
    """[(x, y)] for n items, consuming rng (a random.Random) as dataset.py:60-65 consumes `random`: per item, if pic_size - rho -
    patch_size >= rho, x = randint(rho, pic_size - rho - patch_size), then y likewise; otherwise x = y = 0 and nothing is drawn."""
    hi = int(pic_size) - int(rho) - int(patch_size)
    out = []
    for _ in range(int(n)):
        if hi >= rho:
            x = rng.randint(rho, hi)
            y = rng.randint(rho, hi)
        else:
            x = y = 0
        out.append((x, y))
    return out


def corners_of(draws, patch_size):
    """float32 [B,4,2] in the reference's order: (x, y), (x + p, y), (x + p, y + p), (x, y + p)"""
    p = int(patch_size)
    xy = np.asarray(draws, dtype=np.float32).reshape(-1, 1, 2)
    return xy + np.asarray([[0, 0], [p, 0], [p, p], [0, p]], dtype=np.float32)[None]


def draw_delta_gt(gen, n, rho):
    """The reference's supervised label (dataset.py:75, which its own training step never reads): per item
    torch.randint_like(corners, -rho, rho) on the int64 corners, drawn on the CPU from the torch.Generator `gen`, as float32 [n,4,2]."""
    import torch
    out = [torch.randint(-int(rho), int(rho), (4, 2), generator=gen, dtype=torch.int64) for _ in range(int(n))]
    return torch.stack(out).float()


class UDHBatch(collections.namedtuple("UDHBatch", "img_a img_b patch_a patch_b corners delta_gt index names")):
    """What the reference's collated item holds (dataset.py:97): img_a (img_b) float32 [B,1,pic_size,pic_size], the grey normalised
    resized and centre-cropped left (right) picture; patch_a, patch_b float32 [B,1,patch_size,patch_size], the window (x, y) of both;
    corners float32 [B,4,2]; delta_gt float32 [B,4,2].  img_b and delta_gt are None unless the batch was asked for them.  index: the
    items' indices; names: the basenames of the left pictures."""
    __slots__ = ()


class UDHTables:
    """One device buffer of coefficient tables for the distinct picture sizes of a dataset at one pic_size: built once, on the host,
    from float64; the kernel computes no coefficient.  entry[(H, W)] = (h_table, v_table, h_ksize, v_ksize), word offsets."""

    def __init__(self, sizes, pic_size, device):
        import torch
        self.pic_size = int(pic_size)
        self.entry = {}
        words, end = [], 0
        for size in sorted(set((int(h), int(w)) for h, w in sizes)):
            h, v, ksh, ksv = picture_tables(size, self.pic_size)
            offs = []
            for t in (h, v):
                offs.append(end if t is not None else 0)
                if t is not None:
                    words.append(t)
                    end += t.size
            self.entry[size] = (offs[0], offs[1], ksh, ksv)
        host = np.concatenate(words) if words else np.zeros(1, np.int32)          # never empty: the kernel gets a real pointer
        self.words = torch.from_numpy(host).to(device)

    def rows(self, offsets, sizes, xy):
        """int64 [P,9] descriptor rows in the order of ops.UDH_VIEW_DESC_FIELDS for pictures at arena `offsets` of `sizes` [(H, W)] with
        rectangles at xy [(x0, y0)]"""
        rows = np.empty((len(offsets), 9), dtype=np.int64)
        for i, (off, (h, w), (x0, y0)) in enumerate(zip(offsets, sizes, xy)):
            rows[i] = (off, w, h) + self.entry[(int(h), int(w))] + (x0, y0)
        return rows
