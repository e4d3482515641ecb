"""A stereo dataset that lives in device memory: the training batches of the reference's paired ImageFolder
(compressai/datasets/utils.py:88-404), drawn on the GPU.

The reference prepares every item in DataLoader workers on the host -- cv2.imread, crop, cv2.resize, normalise, grey patch -- and
uploads the batch.  A training step of this library takes 11-13 ms for 8 pairs of 512 x 512; no 16 CPUs decode PNGs at that rate.
Here every picture is decoded ONCE, when the dataset is built, and its uint8 bytes stay in one device buffer (the arena; InStereo2K's
training split is about 11 GB of the MI355X's 288 GB).  A batch is then two launches over a table of one descriptor per view
(ops.views_prep): no pixel crosses PCIe, no worker runs and the host touches no pixel per step.  What the host still does per batch is
what the reference's __getitem__ does with `random`: draw the crop and patch positions (draw_items), a few integers per item.

Every view of a batch has the bits of ops.pair_prep on that picture, and so of oracle/data_oracle.py's restatement of the reference's
per-item chain.  Drawing a batch never waits for the device.

    ds = DeviceStereoFolder("/data/instereo2k", "train", patch_size=(512, 512))
    for b in ds.batches(8):
        h = b.h_matrix(udh_net)
        train_step(model, opt, aux_opt, b.d1, b.d2, h, lmbda)

The homography net itself trains on another item, that of udh/udh/dataset.py (PIL's antialiased Resize, CenterCrop, grey, one window):
udh_batch / udh_batches cut it from the same arena (masic_amd/udh_data.py), with draws from a generator of their own.
"""
import collections
import glob
import os
import random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ALIGN = 16                  # every picture starts at a multiple of it in the arena
STAGE_BYTES = 64 << 20      # pinned staging buffers of the upload (two of them), unless one picture is larger


# ------------------------------------------------------------------------------------------ files
def _split_lists(root, split):
    splitdir = Path(root) / split
    if not splitdir.is_dir():
        raise RuntimeError(f'Invalid directory "{root}"')
    return (sorted(glob.glob(os.path.join(splitdir / "left", "*"))), sorted(glob.glob(os.path.join(splitdir / "right", "*"))))


def scan_pairs(root, split, root_add=""):
    """[(left_path, right_path)] in the reference's order: sorted(glob(<root>/<split>/left/*)) paired with the same of right/, then
    root_add's lists appended (utils.py:89-98, :138-148).  RuntimeError('Invalid directory ...') for a missing split directory as there;
    ValueError when the two lists differ in length or a pair differs in its basenames (utils.py:297-299 raises that per item)."""
    left, right = _split_lists(root, split)
    if root_add != "":
        more_left, more_right = _split_lists(root_add, split)
        left, right = left + more_left, right + more_right
    if len(left) != len(right):
        raise ValueError(f"cannot compare pictures: {len(left)} left and {len(right)} right pictures")
    for a, b in zip(left, right):
        if os.path.basename(a) != os.path.basename(b):
            raise ValueError(f"cannot compare pictures: {a} and {b}")
    return list(zip(left, right))


def _png_bit_depth(path):
    with open(path, "rb") as f:
        head = f.read(26)
    return head[24] if len(head) >= 26 and head[:8] == b"\x89PNG\r\n\x1a\n" else None


def _open_8bit(path):
    from PIL import Image
    im = Image.open(path)
    if im.mode in ("I", "F") or im.mode.startswith("I;16") or _png_bit_depth(path) == 16:
        im.close()
        raise ValueError(f"{path}: 16-bit and float pictures are not supported (cv2.imread's scaling of them is not restated here)")
    if im.mode not in ("RGB", "RGBA", "L", "LA", "P", "PA", "1", "CMYK", "YCbCr"):
        mode = im.mode
        im.close()
        raise ValueError(f"{path}: picture mode {mode} is not supported")
    return im


def decode_rgb8(path):
    """The picture as uint8 [H,W,3], RGB: what cv2.imread + COLOR_BGR2RGB gives for 8-bit PNGs (utils.py:301-304) -- RGB as it is, grey
    replicated into the three channels, a palette expanded, alpha dropped (not blended).  16-bit and float pictures raise ValueError:
    cv2.imread would scale them, and that scaling is not guessed here.  PNG decoding is exact, so PIL and cv2 agree on every 8-bit PNG;
    JPEG parity with cv2 is UNPINNED: the two link different decoders (IDCT and chroma upsampling differ by a level or two), and cv2
    also applies the EXIF orientation, which PIL does not."""
    with _open_8bit(path) as im:
        if im.mode in ("L", "LA", "1"):
            grey = np.asarray(im.convert("L"))
            out = np.repeat(grey[:, :, None], 3, axis=2)
        else:
            out = np.asarray(im.convert("RGB"))           # RGBA -> RGB drops the alpha channel, P -> RGB looks the palette up
    out = np.ascontiguousarray(out, dtype=np.uint8)
    assert out.ndim == 3 and out.shape[2] == 3
    return out


def _picture_hw(path):
    with _open_8bit(path) as im:
        return im.size[1], im.size[0]


# ------------------------------------------------------------------------------------------ the draws
def effective_crop(size_hw, patch_size):
    """min(patch, picture) per axis (utils.py:315-322); patch_size None: the whole picture"""
    H, W = int(size_hw[0]), int(size_hw[1])
    if patch_size is None:
        return H, W
    return min(int(patch_size[0]), H), min(int(patch_size[1]), W)


def draw_items(rng, sizes, patch_size, homopic=256, homopatch=128, rho=45):
    """[(start_h, start_w, x, y)] for pictures of `sizes` [(H, W)], consuming rng (a random.Random) exactly as utils.py:315-365
    consumes the global `random`, item by item: if the effective crop is as tall as the picture both starts are 0 and nothing is drawn
    (also when it is narrower than the picture: the reference's quirk), otherwise start_h = randint(0, H - ph - 1), then start_w =
    randint(0, W - pw - 1); then, if homopic - rho - homopatch >= rho, x and y = randint(rho, homopic - rho - homopatch) each, else 0.
    One deviation: a crop as wide as the picture but shorter makes the reference call randint(0, -1), which raises; here start_w = 0 and
    nothing is drawn for it."""
    out = []
    hi = homopic - rho - homopatch
    for size in sizes:
        H, W = int(size[0]), int(size[1])
        ph, pw = effective_crop((H, W), patch_size)
        if ph == H:
            start_h = start_w = 0
        else:
            start_h = rng.randint(0, H - ph - 1)
            start_w = rng.randint(0, W - pw - 1) if W - pw - 1 >= 0 else 0
        if hi >= rho:
            x = rng.randint(rho, hi)
            y = rng.randint(rho, hi)
        else:
            x = y = 0
        out.append((start_h, start_w, x, y))
    return out


# ------------------------------------------------------------------------------------------ the batch
class StereoBatch(collections.namedtuple("StereoBatch", "d1 d2 homo1 homo2 corners index names")):
    """d1, d2 float32 [B,3,ph,pw] in [0, 1]; homo1, homo2 float32 [B,1,homopatch,homopatch]; corners float32 [B,4,2] = (x, y),
    (x + p, y), (x + p, y + p), (x, y + p) -- what the reference's collated item holds (utils.py:367-396) --; index: the items' indices;
    names: the basenames of the left pictures."""
    __slots__ = ()

    def h_matrix(self, net, detach=True):
        """The h_matrix of the batch from the homography net `net` (newtrain_codec_real.py:123-132): corners relative to corner 0,
        delta = net(homo1, homo2), h = h_adjust(inverse(get_perspective_transform(corners, corners + delta))) for pictures of the
        crop's size.  detach=False keeps it differentiable in delta (masic_amd.homography.h_matrix_from_corners), so a loss on the
        codec's output reaches net's parameters."""
        from .homography import h_matrix_from_corners
        rel = self.corners - self.corners[:, 0].view(-1, 1, 2)
        delta = net(self.homo1, self.homo2)
        if detach:
            delta = delta.detach()
        return h_matrix_from_corners(rel, delta, tuple(self.d1.shape[-2:]), tuple(self.homo1.shape[-2:]))


class DeviceStereoFolder:
    """The stereo pairs of <root>/<split>/{left,right}/ (and root_add's), decoded once into device memory.

    batch(indices) / batches(batch_size) hand out StereoBatch objects cut from it by two kernel launches.  All pairs must give the
    same effective crop min(patch_size, picture) -- a batch has one shape --, which holds for every dataset at least as large as the
    patch; patch_size=None takes whole pictures, which then must all have one size.  The crop and patch positions come from the
    dataset's own random.Random(seed), consumed per item as the reference's __getitem__ consumes `random` (draw_items)."""

    def __init__(self, root, split="train", patch_size=(256, 256), root_add="", homopic=256, homopatch=128, rho=45, seed=0, device="cuda",
                 max_bytes=64 << 30):
        self._configure(patch_size, homopic, homopatch, rho, seed, device, max_bytes)
        pairs = scan_pairs(root, split, root_add)
        files = [p for pair in pairs for p in pair]
        threads = self._threads()
        with ThreadPoolExecutor(threads) as pool:
            sizes = list(pool.map(_picture_hw, files))
        self._layout(sizes, [os.path.basename(a) for a, _ in pairs], files)
        self._upload(lambda k: decode_rgb8(files[k]), threads)

    @classmethod
    def from_arrays(cls, lefts, rights, names=None, patch_size=(256, 256), homopic=256, homopatch=128, rho=45, seed=0, device="cuda",
                    max_bytes=64 << 30):
        """The dataset of pictures that are decoded already: lefts, rights = sequences of uint8 [H,W,3] arrays."""
        self = cls.__new__(cls)
        self._configure(patch_size, homopic, homopatch, rho, seed, device, max_bytes)
        if len(lefts) != len(rights):
            raise ValueError(f"cannot compare pictures: {len(lefts)} left and {len(rights)} right pictures")
        names = [str(i) for i in range(len(lefts))] if names is None else [str(n) for n in names]
        if len(names) != len(lefts):
            raise ValueError(f"{len(names)} names for {len(lefts)} pairs")
        pics = []
        for n, a, b in zip(names, lefts, rights):
            for side, x in (("left", a), ("right", b)):
                x = np.asarray(x)
                if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                    raise ValueError(f"{n} ({side}): pictures must be uint8 [H,W,3] arrays, got {x.dtype} {x.shape}")
                pics.append(x)
        self._layout([p.shape[:2] for p in pics], names, [f"{n} ({side})" for n in names for side in ("left", "right")])
        self._upload(lambda k: pics[k], 1)
        return self

    # ---- construction
    def _configure(self, patch_size, homopic, homopatch, rho, seed, device, max_bytes):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"masic_amd.data: the dataset lives on a CUDA (HIP) device, got {device!r} -- the MI355X path has no CPU fallback")
        self.patch_size = None if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        self.homopic, self.homopatch, self.rho = int(homopic), int(homopatch), int(rho)
        if self.patch_size is not None and min(self.patch_size) < 1:
            raise ValueError(f"patch_size {patch_size}")
        if not 0 < self.homopatch <= self.homopic:
            raise ValueError(f"homopatch {homopatch} of homopic {homopic}")
        self.max_bytes = int(max_bytes)
        self._rng = random.Random(seed)
        self._udh_rng = random.Random(seed)      # the UDH batches' own stream: codec and UDH batches draw as if the other were absent
        self._udh_seed = seed
        self._udh_gen = None                     # torch.Generator of delta_gt, made when first asked for
        self._udh_tables = {}                    # pic_size -> udh_data.UDHTables

    @staticmethod
    def _threads():
        return max(1, min(16, len(os.sched_getaffinity(0))))

    def _layout(self, sizes, names, labels):
        """sizes: (H, W) of left 0, right 0, left 1, ... -> the per-picture table; every refusal happens here, before any allocation"""
        if not names:
            raise ValueError("no stereo pairs")
        sizes = [(int(h), int(w)) for h, w in sizes]
        crop = None
        for i in range(len(names)):
            if sizes[2 * i] != sizes[2 * i + 1]:
                raise ValueError(f"{labels[2 * i]} is {sizes[2 * i][0]} x {sizes[2 * i][1]} and {labels[2 * i + 1]} "
                                 f"{sizes[2 * i + 1][0]} x {sizes[2 * i + 1][1]}: the views of a pair must have one shape")
            c = effective_crop(sizes[2 * i], self.patch_size)
            if min(c) < 1:
                raise ValueError(f"{labels[2 * i]}: empty picture")
            if crop is None:
                crop = c
            elif c != crop:
                raise ValueError(f"{labels[2 * i]} ({sizes[2 * i][0]} x {sizes[2 * i][1]}) gives a crop of {c[0]} x {c[1]}, the pairs before it "
                                 f"{crop[0]} x {crop[1]}: a batch has one shape (patch_size {self.patch_size})")
        offsets, end = [], 0
        for h, w in sizes:
            offsets.append(end)
            end = -(-(end + h * w * 3) // ALIGN) * ALIGN
        if end > self.max_bytes:
            raise ValueError(f"the decoded pictures need an arena of {end} bytes, max_bytes is {self.max_bytes}")
        self.crop = crop
        self.names = tuple(names)
        self.sizes = tuple(sizes[0::2])                                   # (H, W) per pair
        self.offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 2)      # [pair][left, right]
        self._bytes = [h * w * 3 for h, w in sizes]
        self._arena_bytes = end

    def _upload(self, decode, threads):
        """decode(k) -> uint8 [H,W,3] of picture k (arena order).  Runs of pictures are decoded by the pool straight into one of two
        pinned staging buffers and copied from there asynchronously, so decoding a run overlaps the copy of the one before."""
        import torch
        flat = self.offsets.reshape(-1)
        arena = torch.zeros(self._arena_bytes, dtype=torch.uint8, device=self.device)
        stage_bytes = max(STAGE_BYTES, -(-max(self._bytes) // ALIGN) * ALIGN)
        stage_bytes = min(stage_bytes, self._arena_bytes)
        stages = [torch.zeros(stage_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2 if stage_bytes < self._arena_bytes else 1)]
        busy = [None] * len(stages)

        def fill(k, view, base):
            pic = decode(k)
            if pic.nbytes != self._bytes[k]:
                raise ValueError(f"picture {k} decoded to {pic.shape}, its header said {self._bytes[k]} bytes")
            view[int(flat[k]) - base:int(flat[k]) - base + pic.nbytes] = pic.reshape(-1)

        with ThreadPoolExecutor(threads) as pool, torch.cuda.device(self.device):
            k, turn = 0, 0
            while k < len(flat):
                base, first = int(flat[k]), k
                while k < len(flat) and int(flat[k]) + self._bytes[k] - base <= stage_bytes:
                    k += 1
                end = int(flat[k]) if k < len(flat) else self._arena_bytes
                s = turn % len(stages)
                if busy[s] is not None:
                    busy[s].synchronize()                                  # the copy that last read this buffer
                view = stages[s].numpy()
                list(pool.map(lambda j: fill(j, view, base), range(first, k)))
                arena[base:end].copy_(stages[s][:end - base], non_blocking=True)
                busy[s] = torch.cuda.Event()
                busy[s].record()
                turn += 1
            torch.cuda.current_stream().synchronize()
        self.arena = arena

    # ---- use
    def __len__(self):
        return len(self.names)

    @property
    def nbytes(self):
        """bytes of device memory the pictures take"""
        return self._arena_bytes

    def draw(self, indices):
        """The reference's draws for these items, from the dataset's own generator: [(start_h, start_w, x, y)]"""
        return draw_items(self._rng, [self.sizes[i] for i in indices], self.patch_size, self.homopic, self.homopatch, self.rho)

    def descriptors(self, indices, draws):
        """int64 [2B,7] in the order of ops.VIEW_DESC_FIELDS: the B left views, then the B right views; a pair shares its window"""
        idx = np.asarray(indices, dtype=np.int64)
        dr = np.asarray(draws, dtype=np.int64).reshape(len(idx), 4)
        hw = np.asarray([self.sizes[i] for i in idx], dtype=np.int64).reshape(len(idx), 2)
        one = np.stack([np.zeros(len(idx), np.int64), hw[:, 1], hw[:, 0], dr[:, 0], dr[:, 1], dr[:, 2], dr[:, 3]], axis=1)
        desc = np.concatenate([one, one])
        desc[:len(idx), 0] = self.offsets[idx, 0]
        desc[len(idx):, 0] = self.offsets[idx, 1]
        return desc

    def batch(self, indices, draws=None):
        """StereoBatch of the items `indices`.  draws: [(start_h, start_w, x, y)] per item to place the windows by hand; by default they
        are drawn from the dataset's generator (draw).  The 2B views go through ops.views_prep together: two launches, one small
        asynchronous copy for the descriptors and one for the corners, no wait for the device."""
        import torch
        from . import ops
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("an empty batch")
        for i in indices:
            if not 0 <= i < len(self):
                raise IndexError(f"item {i} of a dataset of {len(self)} pairs")
        if draws is None:
            draws = self.draw(indices)
        if len(draws) != len(indices):
            raise ValueError(f"{len(draws)} draws for {len(indices)} items")
        B, p = len(indices), self.homopatch
        with torch.cuda.device(self.device):
            planes, patches = ops.views_prep(self.arena, self.descriptors(indices, draws), self.crop, self.homopic, p)
            host = torch.empty((B, 4, 2), dtype=torch.float32, pin_memory=True)
            xy = np.asarray(draws, dtype=np.float32).reshape(B, 4)[:, None, 2:4]
            host.numpy()[...] = xy + np.asarray([[0, 0], [p, 0], [p, p], [0, p]], dtype=np.float32)[None]
            corners = host.to(self.device, non_blocking=True)
        return StereoBatch(planes[:B], planes[B:], patches[:B], patches[B:], corners, tuple(indices), tuple(self.names[i] for i in indices))

    def batches(self, batch_size, shuffle=True, drop_last=True):
        """One epoch: every index once, in an order taken from the dataset's generator (as it is if shuffle is False)"""
        order = list(range(len(self)))
        if shuffle:
            self._rng.shuffle(order)
        for i in range(0, len(order), int(batch_size)):
            chunk = order[i:i + int(batch_size)]
            if len(chunk) < int(batch_size) and drop_last:
                return
            yield self.batch(chunk)

    # ---- the homography net's own training batches (udh/udh/dataset.py: SyntheticDataset)
    def udh_draw(self, n, pic_size=256, patch_size=128, rho=45):
        """The reference's window draws for n items from the dataset's UDH generator: [(x, y)] (udh_data.draw_udh_items)"""
        from .udh_data import draw_udh_items
        return draw_udh_items(self._udh_rng, n, pic_size, patch_size, rho)

    def udh_tables(self, pic_size):
        """The coefficient tables of this dataset's distinct picture sizes at pic_size, on the device; built on first use"""
        from .udh_data import UDHTables
        key = int(pic_size)
        if key not in self._udh_tables:
            self._udh_tables[key] = UDHTables(set(self.sizes), key, self.device)
        return self._udh_tables[key]

    def udh_batch(self, indices, draws=None, pic_size=256, patch_size=128, rho=45, want_img_b=False, want_delta_gt=False):
        """UDHBatch of the items `indices`: what the reference's SyntheticDataset collates (masic_amd/udh_data.py), cut from the arena by
        two launches of ops.udh_views_prep -- the B left views (2B with want_img_b) at pic_size x pic_size, then the 2B windows of
        patch_size at (x, y); a right view never computes more than its window unless img_b is asked for.  Pictures of different
        sizes may share a batch.  draws: [(x, y)] per item to place the windows by hand; by default they come from the dataset's UDH
        generator, a random.Random(seed) of its own, so batch() / batches() draw exactly what they would without any UDH batch.
        delta_gt (want_delta_gt) is the reference's unused supervised label, drawn on the CPU from a torch.Generator the dataset
        owns.  Two small asynchronous copies (descriptors, corners) per batch; nothing waits for the device, except that the first
        batch of a pic_size uploads the coefficient tables.  A greyscale or RGBA file deviates from the reference in the last bit
        or more (udh_data's docstring): the arena holds three channels."""
        import torch
        from . import ops
        from .udh_data import UDHBatch, corners_of, draw_delta_gt
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("an empty batch")
        for i in indices:
            if not 0 <= i < len(self):
                raise IndexError(f"item {i} of a dataset of {len(self)} pairs")
        S, p, rho = int(pic_size), int(patch_size), int(rho)
        if not 0 < p <= S:
            raise ValueError(f"patch_size {patch_size} of pic_size {pic_size}")
        if draws is None:
            draws = self.udh_draw(len(indices), S, p, rho)
        if len(draws) != len(indices):
            raise ValueError(f"{len(draws)} draws for {len(indices)} items")
        draws = [(int(x), int(y)) for x, y in draws]
        B = len(indices)
        tables = self.udh_tables(S)                                   # ValueError for a picture scaled by more than 16
        sizes = [self.sizes[i] for i in indices]
        left, right = [int(self.offsets[i, 0]) for i in indices], [int(self.offsets[i, 1]) for i in indices]
        with torch.cuda.device(self.device):
            full = tables.rows(left + (right if want_img_b else []), sizes * (2 if want_img_b else 1), [(0, 0)] * (2 * B if want_img_b else B))
            imgs = ops.udh_views_prep(self.arena, full, tables.words, (S, S), S)
            patches = ops.udh_views_prep(self.arena, tables.rows(left + right, sizes * 2, draws * 2), tables.words, (p, p), S)
            host = torch.empty((B, 4, 2), dtype=torch.float32, pin_memory=True)
            host.numpy()[...] = corners_of(draws, p)
            corners = host.to(self.device, non_blocking=True)
            delta_gt = None
            if want_delta_gt:
                if self._udh_gen is None:
                    self._udh_gen = torch.Generator().manual_seed(int(self._udh_seed))
                delta_gt = draw_delta_gt(self._udh_gen, B, rho).pin_memory().to(self.device, non_blocking=True)
        return UDHBatch(imgs[:B], imgs[B:] if want_img_b else None, patches[:B], patches[B:], corners, delta_gt, tuple(indices),
                        tuple(self.names[i] for i in indices))

    def udh_batches(self, batch_size, shuffle=True, drop_last=True, **kw):
        """One epoch of UDH batches: every index once, in an order taken from the dataset's UDH generator (as it is if shuffle is False);
        kw: udh_batch's pic_size, patch_size, rho, want_img_b, want_delta_gt"""
        order = list(range(len(self)))
        if shuffle:
            self._udh_rng.shuffle(order)
        for i in range(0, len(order), int(batch_size)):
            chunk = order[i:i + int(batch_size)]
            if len(chunk) < int(batch_size) and drop_last:
                return
            yield self.udh_batch(chunk, **kw)
