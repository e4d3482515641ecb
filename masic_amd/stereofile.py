"""Self-contained stereo files: 8-bit pictures in, one `.msf` file per pair, 8-bit pictures out (INTEGRATION.md section 9b,
DESIGN.md section 8.5).

`HSIC.compress` writes two files that only the process which encoded them can decode: the decoder needs `h_matrix`, which the UDH
net computes from the original pictures.  The container here carries what is missing -- the original picture size and the eight
corner offsets the homography is built from -- in front of those two files, byte for byte:

    magic b"MSF1" | u8 version = 1 | u8 flags = 0 | u16 H0, W0 | 8 x i16 corner offsets q | u32 len(header), len(streams)
    | u32 zlib.crc32 of the 34 bytes before it | header section (= <name>.npz) | stream section (= <name>.bin)       little-endian

The homography patch is fixed by the format: x = y = 64 in the 256 x 256 resized picture, 128 wide, so only the offsets travel.
They are quantised to 1/64 pixel, q = clamp(rint(delta * 64)), and BOTH sides build `h_matrix` from q / 64 by the same call
(`h_matrix_from_offsets`): the encoder never codes with a matrix the decoder cannot rebuild bit for bit.

`pack` / `parse` / `quantise` / `dequantise` are host functions and need no device.  `StereoCodec` ties the stages together:
ops.pairs_prep -> UDH net -> quantised h_matrix -> HSIC.compress_batch on the padded planes -> pack, and parse ->
HSIC.decompress_batch -> (Independent_EN) -> crop -> ops.planes_to_u8.  The inner files pass through a temporary directory, so
compress / decompress write, read and check exactly what they do on their own.
"""
import collections
import os
import struct
import tempfile
import zlib

import numpy as np
import torch

from . import codec

MAGIC = b"MSF1"
VERSION = 1
PAD_TO = 64                   # HSIC.compress codes multiples of 64 only; the planes are padded up to it and the pictures cropped back
HOMOPIC = 256                 # the homography net sees the unpadded picture resized to HOMOPIC x HOMOPIC ...
PATCH_XY = (64, 64)           # ... and of it the HOMOPATCH x HOMOPATCH window at (x, y) = PATCH_XY, inside the reference's
HOMOPATCH = 128               # [rho, 256 - rho - 128] = [45, 83] range of random positions (compressai/datasets/utils.py:246-248)
OFFSET_SCALE = 64             # corner offsets travel in 1/64 pixel of the resized picture
_HEAD = struct.Struct("<4sBBHH8hII")
HEADER_BYTES = _HEAD.size + 4

StereoFile = collections.namedtuple("StereoFile", "H0 W0 delta_q header streams")


def padded_hw(H0, W0):
    return -(-int(H0) // PAD_TO) * PAD_TO, -(-int(W0) // PAD_TO) * PAD_TO


def quantise(delta):
    """Corner offsets (any shape holding 8 values per pair, float) -> int16 of the same shape: clamp(rint(delta * 64), -32768, 32767),
    ties to even; NaN -> 0."""
    d = np.nan_to_num(np.asarray(delta, dtype=np.float32), nan=0.0, posinf=np.float32(1e9), neginf=np.float32(-1e9))
    return np.clip(np.rint(d * np.float32(OFFSET_SCALE)), -32768, 32767).astype(np.int16)


def dequantise(q):
    """int16 offsets -> float32 q / 64 (exact)."""
    return np.asarray(q, dtype=np.int16).astype(np.float32) / np.float32(OFFSET_SCALE)


def pack(H0, W0, delta_q, header, streams):
    """One .msf file as bytes.  delta_q: the eight int16 offsets in the order of delta.reshape(8); header / streams: the bytes of the
    .npz / .bin files HSIC.compress wrote for the pair padded to a multiple of 64."""
    q = np.asarray(delta_q)
    if q.size != 8 or not np.issubdtype(q.dtype, np.integer) or q.min() < -32768 or q.max() > 32767:
        raise ValueError("masic_amd.stereofile.pack: delta_q must hold eight int16 corner offsets")
    if not (1 <= int(H0) <= 65535 and 1 <= int(W0) <= 65535):
        raise ValueError(f"masic_amd.stereofile.pack: picture size {H0}x{W0} outside 1 .. 65535")
    if max(padded_hw(H0, W0)) > 65535:
        raise ValueError(f"masic_amd.stereofile.pack: picture size {H0}x{W0} padded to a multiple of {PAD_TO} exceeds 65535 (the inner header "
                         "stores it as uint16)")
    header, streams = bytes(header), bytes(streams)
    head = _HEAD.pack(MAGIC, VERSION, 0, int(H0), int(W0), *(int(v) for v in q.reshape(8)), len(header), len(streams))
    return head + struct.pack("<I", zlib.crc32(head)) + header + streams


def parse(data, who="masic_amd.stereofile.parse", pair=0):
    """The bytes of one .msf file -> StereoFile(H0, W0, delta_q int16 [8], header bytes, streams bytes).  codec.CorruptStreamError
    (a ValueError) for a foreign magic or version, non-zero flags, a checksum mismatch, an empty picture, section lengths that do not add
    up to the file's size, or an inner header of another size than H0 x W0 rounded up to 64.  The sections themselves are checked by the
    parsers of HSIC.decompress, which StereoCodec.decode hands them to."""
    def bad(msg):
        return codec.CorruptStreamError(pair, f"{who}: {msg}")          # pair: the file's index in the caller's batch

    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise bad(f"truncated file: the stereo header needs {HEADER_BYTES} bytes, {len(data)} are there")
    magic, version, flags, H0, W0, *rest = _HEAD.unpack_from(data)
    q, n_header, n_streams = rest[:8], rest[8], rest[9]
    if magic != MAGIC:
        raise bad("not a stereo file of this library (magic %r)" % magic)
    if version != VERSION:
        raise bad(f"stereo file version {version}; this library reads version {VERSION}")
    if flags != 0:
        raise bad(f"reserved flags {flags:#04x} set")
    crc, = struct.unpack_from("<I", data, _HEAD.size)
    if crc != zlib.crc32(data[:_HEAD.size]):
        raise bad("the checksum of the stereo header does not match (damaged file)")
    if H0 == 0 or W0 == 0:
        raise bad(f"empty picture ({H0}x{W0})")
    if HEADER_BYTES + n_header + n_streams != len(data):
        raise bad(f"the sections take {n_header} + {n_streams} bytes after the {HEADER_BYTES}-byte header, the file holds {len(data)} "
                  "(truncated, or bytes follow the streams)")
    header = data[HEADER_BYTES:HEADER_BYTES + n_header]
    streams = data[HEADER_BYTES + n_header:]
    if n_header < 4:
        raise bad("the header section is too short for its picture size")
    H, W = struct.unpack_from("<HH", header)
    if (H, W) != padded_hw(H0, W0):
        raise bad(f"the inner header codes {H}x{W}, a {H0}x{W0} picture is coded as %dx%d" % padded_hw(H0, W0))
    return StereoFile(H0, W0, np.array(q, dtype=np.int16), header, streams)


def h_matrix_from_offsets(delta_q, hw, device):
    """h_matrix [B,3,3] in the pixel coordinates of the H0 x W0 = hw pictures from int16 offsets [B,8]: the call both sides make."""
    from . import ops
    q = np.asarray(delta_q, dtype=np.int16).reshape(-1, 8)
    delta = torch.from_numpy(dequantise(q).reshape(-1, 4, 2)).to(device)
    s = float(HOMOPATCH)          # the patch corners shifted to the first one (newtrain_codec_real.py:123), in dataset order
    corners = torch.tensor([[0.0, 0.0], [s, 0.0], [s, s], [0.0, s]], dtype=torch.float32, device=device).repeat(q.shape[0], 1, 1)
    return ops.homography_from_corners(corners, delta, (int(hw[0]), int(hw[1])), (HOMOPIC, HOMOPIC))


def _inner_names(names):
    return [f"{i}-{os.path.basename(n)}" for i, n in enumerate(names)]


class StereoCodec:
    """encode: B stereo pairs of 8-bit pictures -> B .msf files; decode: the files -> the pictures, from nothing but the files and the
    weights.  hsic (MASIC.HSIC), udh (any eval-mode module mapping two patches to `delta`: model.Net at patch size 128, or
    masic_amd.align.PatchAligner, which needs no weights; needed by encode only) and cqe (MASIC.Independent_EN; needed for
    decode(enhance=True) only) are modules of this tree on one MI355X device, in eval mode.  The operand mode is
    masic_amd.nn.set_precision's, as for HSIC.compress; the file records it.  band_rows (0 .. 255): HSIC.compress_batch's, for encode
    only -- the inner .bin carries the value, so decode needs nothing and a codec built without it decodes the files.  refine (None:
    off, today's files byte for byte): a masic_amd.refine.RefineConfig with steps > 0 and its lmbda set (the rate-distortion weight the
    checkpoint was trained with -- the codec has no other source for it); encode then refines every batch's latents
    (refine.refine_latents) before coding them; a config with a bit budget (budget_bpp -- per pixel of the padded size H x W, a
    sequence of them one per pair of every encode call -- or budget_rel) refines under it, the budget being on the estimated bits of
    the inner streams, not on the .msf file's bytes.  For encode only: the bytes layout, decode and evaluate_files are untouched."""

    def __init__(self, hsic, udh=None, cqe=None, band_rows=0, refine=None):
        from .bands import check_band_rows
        self.hsic, self.udh, self.cqe = hsic, udh, cqe
        self.band_rows = check_band_rows(band_rows, "StereoCodec")
        if refine is not None:
            from .refine import RefineConfig
            if not isinstance(refine, RefineConfig):
                raise TypeError(f"StereoCodec: refine must be a masic_amd.refine.RefineConfig or None, got {type(refine).__name__}")
            if refine.steps > 0 and refine.lmbda is None:
                raise ValueError("StereoCodec: refine needs RefineConfig(lmbda=...), the rate-distortion weight of the checkpoint")
            if refine.steps == 0:
                refine = None
        self.refine = refine

    def _check_modules(self, who, *mods):
        for name, m in mods:
            if m.training:
                raise RuntimeError(f"{who}: the {name} module is in training mode -- call .eval() first")
        dev = next(self.hsic.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"{who}: the modules must live on a CUDA (HIP) device -- the MI355X path has no CPU fallback")
        return dev

    def encode(self, left_u8, right_u8, names, path=""):
        """left_u8, right_u8: uint8 [B,H0,W0,3] (or [H0,W0,3]) device tensors, any H0, W0 >= 1; names: B strings (or one).  Writes
        <path>/<name_i>.msf and returns a dict: "bytes" / "bpp" (lists of B; the whole file, over the H0 * W0 pixels), "h_matrix"
        [B,3,3] (from the quantised offsets), "delta_q" int16 [B,8], "left_hat" / "right_hat" uint8 [B,H0,W0,3] (what decode will
        return), "x1_hat" / "x2_hat" float32 [B,3,H,W] of the padded size."""
        from . import ops
        who = "StereoCodec.encode"
        if self.udh is None:
            raise RuntimeError(f"{who}: this codec was built without the homography net (udh=None): it can decode only")
        dev = self._check_modules(who, ("hsic", self.hsic), ("udh", self.udh))
        for t, name in ((left_u8, "left"), (right_u8, "right")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{who}: {name} must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
            if t.dtype != torch.uint8:
                raise ValueError(f"{who}: {name} must be uint8 (decoded 8-bit pictures), got {t.dtype}")
        if left_u8.shape != right_u8.shape:
            raise ValueError(f"{who}: left is {tuple(left_u8.shape)}, right is {tuple(right_u8.shape)}: the two views must have one shape")
        if isinstance(names, str):
            names = [names]
        names = [str(n) for n in names]
        if left_u8.dim() == 3:
            left_u8, right_u8 = left_u8[None], right_u8[None]
        if left_u8.dim() != 4 or left_u8.shape[3] != 3 or min(left_u8.shape) < 1:
            raise ValueError(f"{who}: pictures must be [B,H0,W0,3] or [H0,W0,3], got {tuple(left_u8.shape)}")
        B, H0, W0 = left_u8.shape[:3]
        if len(names) != B:
            raise ValueError(f"{who}: {B} pairs and {len(names)} names")
        if self.refine is not None:
            self.refine.budget_bpp_for(B, who)          # a budget per pair must be one per pair of this call
        H, W = padded_hw(H0, W0)
        if max(H, W) > 65535:
            raise ValueError(f"{who}: picture size {H0}x{W0} padded to {H}x{W} exceeds 65535 (the header stores sizes as uint16)")
        with torch.no_grad():
            planes, patches = ops.pairs_prep(torch.cat((left_u8, right_u8)).contiguous(), PAD_TO, HOMOPIC, PATCH_XY, HOMOPATCH)
            # the net runs pair by pair: a pair's file must not depend on its batch mates, and the float32 convolutions pick their
            # summation order by batch shape
            delta = torch.cat([self.udh(patches[i:i + 1], patches[B + i:B + i + 1]) for i in range(B)])
            delta_q = quantise(delta.reshape(B, 8).cpu().numpy())
            h_matrix = h_matrix_from_offsets(delta_q, (H0, W0), dev)
            inner = _inner_names(names)
            with tempfile.TemporaryDirectory(prefix="masic_msf_") as tmp:
                if self.refine is None:
                    out = self.hsic.compress_batch(planes[:B], planes[B:], h_matrix, inner, tmp, band_rows=self.band_rows)
                else:
                    from .refine import refine_latents
                    latents = refine_latents(self.hsic, planes[:B], planes[B:], h_matrix, None, self.refine)
                    out = self.hsic.compress_batch(planes[:B], planes[B:], h_matrix, inner, tmp, band_rows=self.band_rows, latents=latents)
                files = []
                for i, n in enumerate(inner):
                    with open(os.path.join(tmp, n + ".npz"), "rb") as f:
                        header = f.read()
                    with open(os.path.join(tmp, n + ".bin"), "rb") as f:
                        files.append(pack(H0, W0, delta_q[i], header, f.read()))
            for n, data in zip(names, files):
                with open(os.path.join(path, n + ".msf"), "wb") as f:
                    f.write(data)
            nbytes = [len(d) for d in files]
            return {"bytes": nbytes, "bpp": [n * 8.0 / (H0 * W0) for n in nbytes], "h_matrix": h_matrix,
                    "delta_q": torch.from_numpy(delta_q.copy()), "left_hat": ops.planes_to_u8(out["x1_hat"], (H0, W0)),
                    "right_hat": ops.planes_to_u8(out["x2_hat"], (H0, W0)), "x1_hat": out["x1_hat"], "x2_hat": out["x2_hat"]}

    def decode(self, names, path="", enhance=False):
        """names: B strings (or one) of files encode wrote, all of one picture size -> dict: "left" / "right" uint8 [B,H0,W0,3],
        "h_matrix" [B,3,3], "x1_hat" / "x2_hat" float32 [B,3,H,W] of the padded size (after the enhancement network when enhance).
        codec.CorruptStreamError (a ValueError) for a file parse refuses or whose streams do not decode; HSIC.decompress's ValueError
        for sections its parsers refuse, a file written in another operand mode among them."""
        from . import ops
        who = "StereoCodec.decode"
        if enhance and self.cqe is None:
            raise RuntimeError(f"{who}: enhance=True needs the enhancement network, and this codec was built with cqe=None")
        dev = self._check_modules(who, ("hsic", self.hsic), *((("cqe", self.cqe),) if enhance else ()))
        if isinstance(names, str):
            names = [names]
        names = [str(n) for n in names]
        if not names:
            raise ValueError(f"{who}: no names")
        files = []
        for i, n in enumerate(names):
            with open(os.path.join(path, n + ".msf"), "rb") as f:
                files.append(parse(f.read(), f"{who}: pair {i} ({n})" if len(names) > 1 else who, i))
        H0, W0 = files[0][:2]
        for i, f in enumerate(files):
            if (f.H0, f.W0) != (H0, W0):
                raise ValueError(f"{who}: pair {i} ({names[i]}) is {f.H0}x{f.W0}, pair 0 is {H0}x{W0}: one picture size per call")
        with torch.no_grad():
            h_matrix = h_matrix_from_offsets(np.stack([f.delta_q for f in files]), (H0, W0), dev)
            inner = _inner_names(names)
            with tempfile.TemporaryDirectory(prefix="masic_msf_") as tmp:
                for n, f in zip(inner, files):
                    for ext, section in ((".npz", f.header), (".bin", f.streams)):
                        with open(os.path.join(tmp, n + ext), "wb") as g:
                            g.write(section)
                try:
                    out = self.hsic.decompress_batch(inner, h_matrix, tmp)
                except codec.CorruptStreamError:
                    raise
                except codec.PairStreamError as e:
                    # a damaged stream can also run out of words before its last symbol, which decompress reports as a plain
                    # PairStreamError; for a file that carries everything it is decoded with, either way the file is damaged
                    raise codec.CorruptStreamError(e.pair, f"{who}: {e}") from e
            x1_hat, x2_hat = out["x1_hat"], out["x2_hat"]
            if enhance:
                out = self.cqe(x1_hat, x2_hat, h_matrix)
                x1_hat, x2_hat = out["x1_hat"], out["x2_hat"]
            return {"left": ops.planes_to_u8(x1_hat, (H0, W0)), "right": ops.planes_to_u8(x2_hat, (H0, W0)), "h_matrix": h_matrix,
                    "x1_hat": x1_hat, "x2_hat": x2_hat}
