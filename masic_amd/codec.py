"""Coding of the y latents for HSIC.compress / decompress (reference MASIC.py:855-1408).

The reference walks the latent in raster order and, per pixel, re-runs the masked context convolution on a 5x5 crop and
the nine 1x1 head layers, builds one CDF per non-zero channel on the host and calls a Python range coder per symbol.
Here:
  * the coding order is the anti-diagonal wavefront t = j + 3 i of the type-A 5x5 mask (pixel (i, j) needs rows i-2, i-1 up
    to column j+2 and the two pixels left of it: all have a smaller t), so a 32x32 latent takes 125 dependent steps
    instead of 1024, each coding all pixels of its wavefront x all non-zero channels at once;
  * the tables are built on the device (masic_gmm_cdf_rows_batch) and only cross to the host as u16 rows for the decoder, or
    as (start, freq) pairs for the encoder;
  * the coder is the library's rANS (masic_rans_*) with ONE STREAM PER LATENT CHANNEL: a stream is one serial dependency chain, the
    channels' chains are independent, so the decoder's symbol search runs on the device -- one wavefront per channel stream
    (masic_rans_decode_step_batch) -- and writes the decoded values straight into the latent.  The whole loop over coding steps stays on the
    GPU: per step one HIP-graph replay (context convolution + nine head layers + table kernel + decode kernel), no table rows, symbols
    or synchronisation crossing PCIe until the last step (round 2 copied ~0.5 MB of u16 table rows to the host per step, searched
    them on one core and scattered the values back: two thirds of its 54 ms per 512 x 512 pair).
Encoder and decoder evaluate the SAME kernels on tensors of the same shape, and the masked taps of the context
convolution are exact zeros, so a not-yet-decoded neighbour (zero in the decoder, the true value in the encoder) never
changes a bit of the parameters of the pixel being coded: the encoder needs ONE pass over the full latent, the decoder
one pass per wavefront.  The encoder's rANS chains run on the device too, one lane per channel stream over the (start, freq) table
(masic_rans_encode_channels_batch), and a second kernel frames the pairs: only the flags, the pairs' offsets and the finished bytes
cross to the host.  The host coder (encode_channels) is kept as its byte-for-byte checker (encode_views(coder="host")).
Container (.bin): b"MSR2", u8 precision id (0 f32 / 1 bf16 / 2 fp8 operands: the tables depend on it), u8 flags (bit 0: an
activation-scale table follows), 2 pad bytes (b"MSR3": u8 band_rows >= 1 -- the row bands of wavefront_steps -- and 1 pad byte), [u32 length + the fp8 mode's calibration table as JSON, masic_amd/fp8.py], then per
view u32 number of channel streams n, n x u32 stream lengths in bytes, the streams back to back (round 2's "MSR1" had one stream per view).  The .npz header keeps the reference's layout (MASIC.py:916-948).
The container carries no checksum; what is read back is checked instead: split_views parses the framing strictly, and after the last
coding step every channel stream must have consumed exactly its words and left the coder at 2^31, the state every encoder starts from
(masic_rans_decode_finish_batch, CorruptStreamError)."""
import ctypes

import numpy as np
import torch

from ._lib import check, lib

MAGIC = b"MSR2"
MAGIC_BANDS = b"MSR3"            # the same layout with byte 6 = band_rows >= 1 (wavefront_steps)


import functools


@functools.lru_cache(maxsize=16)
def _wavefront_steps(h, w, S):
    ii = np.arange(h)
    steps = []
    for t in range(w + 3 * (S - 1)):
        j = t - 3 * (ii % S)
        keep = (j >= 0) & (j < w)
        steps.append((ii[keep] * w + j[keep]).astype(np.int32))
    return steps


def wavefront_steps(h, w, band_rows=0):
    """Pixel indices (i * w + j), rows ascending, of each wavefront t = j + 3 i.  (A function of the latent's shape alone: cached -- the
    125 numpy selections of a 32 x 32 latent were 0.5 ms of every encode_views / decode_views call.  Callers must not write to the arrays.)
    band_rows = S in 1 .. h - 1: the latent's rows are cut into bands of S rows whose context model does not look across the band's top
    edge (masic_amd/bands.py), the bands' wavefronts run side by side -- step t holds the pixels with j + 3 (i mod S) = t, still at most
    one per row, and there are w + 3 (S - 1) steps.  0, or S >= h (one band): the lists above, the same cached object."""
    return _wavefront_steps(h, w, band_rows if 0 < band_rows < h else h)


def effective_band_rows(h, band_rows):
    """band_rows as the kernels and step lists take it: 0 when one band covers the latent."""
    return band_rows if 0 < band_rows < h else 0


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def gmm_tables(sigma, mu, logits, M, K, pix, chan, minmax, scale_bound, y_hat=None, want_starts=True):
    """Tables of rows (pix[i], chan[j]) of one image -> (starts int16-viewed-u16 [rows][L] or None, start_freq int32 [rows][2] or None,
    err).  The batched table kernel with a one-pair stream table."""
    for t in (sigma, mu, logits):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.shape[0] == 1 and t.shape[1] == K * M):
            raise RuntimeError("masic_amd.codec: head outputs must be contiguous float32 [1, K*M, h, w] device tensors")
    if not 1 <= minmax <= 511:      # the kernels flag it per row (err bit 0); here, where the table is built, it is an argument error
        raise RuntimeError(f"masic_hip gmm_cdf_rows_batch: error -4 (MASIC_ERR_UNSUPPORTED): minmax={minmax} (alphabet of at most 1024 symbols)")
    HW = sigma.shape[-2] * sigma.shape[-1]
    npix, L = pix.numel(), 2 * minmax + 1
    dev = sigma.device
    desc, n, _, rows = _stream_table([chan.tolist()], [minmax], npix, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    starts = torch.empty((rows, L), dtype=torch.int16, device=dev) if want_starts else None
    sf = torch.empty((rows, 2), dtype=torch.int32, device=dev) if y_hat is not None else None
    if rows:
        check(lib.masic_gmm_cdf_rows_batch(_p(sigma), _p(mu), _p(logits), M, K, HW, _p(pix), None, npix, npix, _p(desc), n, float(scale_bound),
                                           _p(y_hat) if y_hat is not None else None, _p(starts) if starts is not None else None,
                                           _p(sf) if sf is not None else None, _p(err),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gmm_cdf_rows_batch")
    return starts, sf, err


def encode_freqs(start_freq):
    sf = np.ascontiguousarray(start_freq, dtype=np.int32).reshape(-1, 2)
    cap = (sf.shape[0] + 2) * 4
    out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    check(lib.masic_rans_encode_freqs(sf.ctypes.data_as(ctypes.c_void_p), sf.shape[0], out.ctypes.data_as(ctypes.c_void_p), cap,
                                      ctypes.byref(n)), "rans_encode_freqs")
    return out[:n.value].tobytes()


class AdaptiveDecoder:
    """Incremental rANS decoder over per-symbol tables (masic_rans_decoder_*)."""

    def __init__(self, data):
        self._buf = np.frombuffer(bytes(data), dtype=np.uint8)
        self._h = ctypes.c_void_p()
        check(lib.masic_rans_decoder_open(self._buf.ctypes.data_as(ctypes.c_void_p), self._buf.size, ctypes.byref(self._h)), "rans_decoder_open")

    def decode_rows(self, starts_u16):
        s = np.ascontiguousarray(starts_u16)
        out = np.empty(s.shape[0], dtype=np.int32)
        check(lib.masic_rans_decoder_decode_rows(self._h, s.ctypes.data_as(ctypes.c_void_p), s.shape[0], s.shape[1],
                                                 out.ctypes.data_as(ctypes.c_void_p)), "rans_decoder_decode_rows")
        return out

    def finished(self):
        """True when every word of the stream is consumed and the coder is back in the state every encoder starts from (2^31): what a
        correctly read stream ends in once its last symbol is decoded, and a damaged one only by a ~2^-31 coincidence."""
        ok = ctypes.c_int(0)
        check(lib.masic_rans_decoder_finished(self._h, ctypes.byref(ok)), "rans_decoder_finished")
        return bool(ok.value)

    def close(self):
        if self._h:
            lib.masic_rans_decoder_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self.close()


def encode_channels(start_freq, npix, nch):
    """(start, freq) rows [npix * nch][2] in coding order (pixel-major) -> u32 count, u32 lengths[nch], the nch rANS streams."""
    sf = np.ascontiguousarray(start_freq, dtype=np.int32).reshape(-1, 2)
    cap = (sf.shape[0] + 2 * max(nch, 1)) * 4 + 64
    out = np.empty(cap, dtype=np.uint8)
    lengths = np.zeros(max(nch, 1), dtype=np.uint32)
    n = ctypes.c_size_t(0)
    if nch:
        check(lib.masic_rans_encode_channels(sf.ctypes.data_as(ctypes.c_void_p), int(npix), int(nch), out.ctypes.data_as(ctypes.c_void_p), cap,
                                             lengths.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)), "rans_encode_channels")
    return np.array([nch], dtype=np.uint32).tobytes() + lengths[:nch].tobytes() + out[:n.value].tobytes()


def split_channels(blob):
    """Inverse of encode_channels' framing -> (list of per-channel byte strings, bytes consumed)."""
    nch = int(np.frombuffer(blob[:4], dtype=np.uint32)[0])
    lengths = np.frombuffer(blob[4:4 + 4 * nch], dtype=np.uint32)
    off, out = 4 + 4 * nch, []
    for n in lengths:
        out.append(blob[off:off + int(n)])
        off += int(n)
    return out, off


def split_views(rest, nviews):
    """The strict form of split_channels for bytes read from a file: `rest` must hold exactly nviews framings (u32 n, n x u32 lengths,
    the n streams), each stream a whole rANS stream (>= 8 bytes: the two state words; a multiple of 4) -> the nviews framed views, what
    decode_views takes.  ValueError for a count or length field that reaches past the buffer, a length no stream can have, or bytes
    left over after the last view (split_channels slices with Python semantics and accepts all three)."""
    out, off = [], 0
    for v in range(nviews):
        if off + 4 > len(rest):
            raise ValueError(f"masic_amd.codec: the y streams end before the stream count of view {v + 1}")
        nch = int(np.frombuffer(rest[off:off + 4], dtype=np.uint32)[0])
        if 4 * nch > len(rest) - off - 4:
            raise ValueError(f"masic_amd.codec: view {v + 1} counts {nch} channel streams, more than the file holds")
        lengths = np.frombuffer(rest[off + 4:off + 4 + 4 * nch], dtype=np.uint32).astype(np.int64)
        if nch and (int(lengths.min()) < 8 or (lengths % 4).any()):
            raise ValueError(f"masic_amd.codec: view {v + 1} holds a length field no rANS stream has (below 8 bytes or not a multiple of 4)")
        end = off + 4 + 4 * nch + int(lengths.sum())
        if end > len(rest):
            raise ValueError(f"masic_amd.codec: the channel streams of view {v + 1} reach {end - len(rest)} bytes past the end of the file")
        out.append(rest[off:end])
        off = end
    if off != len(rest):
        raise ValueError(f"masic_amd.codec: {len(rest) - off} bytes follow the last view's streams")
    return out


# ---- the coding loops, over the views of B >= 1 pairs (HSIC.compress / decompress: B = 1; compress_batch / decompress_batch).  The
# framing and container are per pair; the device work of a coding step covers all B pairs: one skinny launch per layer over every pair's
# pixels (list entries b * h * w + p), one table launch and one decode launch over every pair's channel streams (masic_code_stream_t),
# so the fixed costs of a step -- launch latency, the graph replay, the serial rANS chain -- are paid once for B pairs.
class PairStreamError(RuntimeError):
    """A coding error of one pair (`pair`: its index in the call)."""

    def __init__(self, pair, msg):
        super().__init__(msg)
        self.pair = pair


class CorruptStreamError(PairStreamError, ValueError):
    """A channel stream decoded to the end without the coder reaching its final state (err bit 3, masic_rans_decode_finish_batch): the
    bytes are not what the encoder wrote for these tables."""


def check_errs(err, what, names=None):
    """err: the kernels' flags, one int per pair -> PairStreamError for the first pair with a bit set; it names the pair when the call
    holds several or `names` is given."""
    flags = err.cpu().tolist()
    for i, e in enumerate(flags):
        kind = PairStreamError
        if e & 1:
            msg = "a coding table could not be normalised to 2^16"
        elif e & 2:
            msg = "a symbol lies outside the alphabet (minmax too small)"
        elif e & 4:
            msg = "a channel stream ended before its last symbol (truncated or foreign data)"
        elif e & 8:
            kind = CorruptStreamError
            msg = ("a channel stream did not end in the coder's final state (corrupt data, a header from another file, other weights or "
                   "another operand mode than the encoder's)")
        elif e & 16:
            msg = "the encoder was given a symbol interval outside [0, 2^16]"
        else:
            continue
        raise kind(i, f"masic_amd.codec: {what}: {msg}{_pair_tag(i, len(flags), names, ' -- pair %s of the batch')}")


check_err = check_errs      # the name gmm_tables' callers use for its one flag


def _pair_tag(i, B, names, fmt):
    if B == 1 and names is None:
        return ""
    return fmt % (f"{i} ({names[i]})" if names is not None else str(i))


def _stream_table(chans, minmaxes, rows_per_stream, device, words=None):
    """masic_code_stream_t per (pair, coded channel) as an int32 device tensor [n, 8], and the u16 size of the starts buffer.  Pair b's
    table rows are pixel-major ([pixel][its channels]: start_freq rows row0 + i * nch_b, the layout encode_channels reads), its starts
    rows a block of rows_per_stream * nch_b rows of its own alphabet.  words: per pair (word offsets, word counts) or None."""
    blocks, row_base, s_base = [np.zeros((0, 8), dtype=np.int64)], 0, 0
    for b, (ch, mm) in enumerate(zip(chans, minmaxes)):
        nch, L = len(ch), 2 * int(mm) + 1
        t, c = np.zeros((nch, 8), dtype=np.int64), np.arange(nch)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 5] = b, ch, mm, nch, row_base + c, s_base + c * L
        if words is not None:
            t[:, 6], t[:, 7] = words[b]
        blocks.append(t)
        row_base += rows_per_stream * nch
        s_base += rows_per_stream * nch * L
    t = np.concatenate(blocks).astype(np.uint32).view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(t)).to(device), t.shape[0], s_base, row_base


def _encode_pairs(jobs):
    """encode_channels over the pairs of a batch: the host rANS coder releases the GIL (ctypes), so a few threads run the pairs at once."""
    if len(jobs) == 1:
        return [encode_channels(*jobs[0])]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as ex:
        return list(ex.map(lambda j: encode_channels(*j), jobs))


def _pixel_list_form(params_fn, B, who):
    """Which of the two parameter forms params_fn is: the pixel-list kernels over B images (HSIC._PixelParams with `skinny`: bf16
    operands) -> True, or a callable y_hat -> (sigma, mu, logits) over the full latent of ONE pair (float32 / fp8 operands) -> False."""
    if getattr(params_fn, "skinny", False):
        return True
    if B != 1:
        raise RuntimeError(f"masic_amd.codec.{who}: several pairs need the pixel-list parameter kernels (bf16 operands)")
    return False


def _full_latent_params(params_fn, y_hat, KM):
    out = params_fn(y_hat)
    for t in out:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (1, KM) + tuple(y_hat.shape[-2:])):
            raise RuntimeError("masic_amd.codec: head outputs must be contiguous float32 [1, K*M, h, w] device tensors")
    return out


def _encode_device(sf, desc, nstreams, npix, first, err, names=None, raise_errs=True):
    """The device coder on the (start, freq) table `sf` of B pairs (masic_rans_encode_channels_batch + masic_rans_pack_pairs_batch) -> the
    B framed blobs, byte for byte encode_channels' of each pair's rows, and the pairs' flags as a list.  first: per pair the index of its
    first stream, plus nstreams; err: the call's flags, int32 [B] on the device (the table kernel's bits are in it already).  Two copies
    leave the device: the flags together with the pairs' byte offsets, and -- once check_errs has passed -- the used bytes of the blobs."""
    B, dev = len(first) - 1, sf.device
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    meta = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)          # flags [B], byte offsets [B + 1]
    meta[:B] = err
    first_d = torch.tensor(first, dtype=torch.int32).to(dev)
    ws = torch.empty(max(lib.masic_rans_encode_batch_workspace_bytes(nstreams, npix) // 4, 1), dtype=torch.int32, device=dev)
    lengths = torch.empty(max(nstreams, 1), dtype=torch.int32, device=dev)
    blob = torch.empty(lib.masic_rans_pack_pairs_bound(nstreams, npix, B) // 4, dtype=torch.int32, device=dev)
    check(lib.masic_rans_encode_channels_batch(_p(sf), _p(desc), nstreams, npix, _p(ws), _p(lengths), _p(meta), st), "rans_encode_channels_batch")
    check(lib.masic_rans_pack_pairs_batch(_p(ws), _p(lengths), _p(desc), nstreams, npix, _p(first_d), B, _p(blob), _p(meta[B:]), st),
          "rans_pack_pairs_batch")
    meta_h = meta.cpu()
    if raise_errs:
        check_errs(meta_h[:B], "encode", names)
    off = meta_h[B:].numpy().view(np.uint32).astype(np.int64)
    data = blob[:int(off[B]) // 4].cpu().numpy().tobytes()
    return [data[off[b]:off[b + 1]] for b in range(B)], meta_h[:B].tolist()


def encode_channels_device(sf_dev, desc, nstreams, npix, B, first):
    """The device form of encode_channels for the B pairs of one stream table (desc, nstreams: _stream_table's, built with npix rows per
    stream; first: the pairs' first stream indexes, B + 1 entries; sf_dev: int32 [rows][2] on the device) -> (the B blobs, the pairs'
    error flags as a list of B ints).  A flagged pair (bit 4: a row no coder can take) raises nothing here; its blob codes the other
    rows.  For tests of the kernels without a model."""
    if len(first) != B + 1 or first[0] != 0 or first[B] != nstreams or any(first[b] > first[b + 1] for b in range(B)):
        raise ValueError("masic_amd.codec.encode_channels_device: first must hold B + 1 ascending stream indexes from 0 to nstreams")
    if not (sf_dev.is_cuda and sf_dev.is_contiguous() and sf_dev.dtype == torch.int32):
        raise RuntimeError("masic_amd.codec.encode_channels_device: start_freq must be a contiguous int32 device tensor")
    err = torch.zeros(B, dtype=torch.int32, device=sf_dev.device)
    return _encode_device(sf_dev, desc, nstreams, npix, [int(f) for f in first], err, raise_errs=False)


def _first_streams(chans):
    return [0] + np.cumsum([len(ch) for ch in chans]).tolist()


def encode_views(params_fn, y_hat, M, K, chans, minmaxes, scale_bound, names=None, coder="device", band_rows=0):
    """One pass over B pairs: y_hat [B, M, h, w]; chans / minmaxes: pair b's coded channels (int sequence) and alphabet half-width;
    params_fn: see _pixel_list_form.  Parameters of every pixel -> (start, freq) of every coded symbol in wavefront order -> per pair
    u32 n, n x u32 lengths and one rANS stream per coded channel.  A pair's bytes do not depend on its batch mates (the same parameters
    bit for bit: a pixel's result depends on its own operands only; the same table arithmetic on them).
    coder: "device" codes and frames the streams where the table is (one lane per channel stream; the flags, the pairs' offsets and the
    finished bytes are all that cross to the host); "host" copies the table to the host and runs encode_channels per pair -- the same
    bytes, kept as the checker of the device coder.
    band_rows: the row bands of wavefront_steps -- the order of the pass and the band top of the context model (params_fn.run's
    band_rows; a full-latent params_fn must evaluate the same band top itself); the decoder must be given the same value."""
    if coder not in ("device", "host"):
        raise ValueError(f"masic_amd.codec.encode_views: coder={coder!r} (\"device\" or \"host\")")
    B, _, h, w = y_hat.shape
    HW, dev = h * w, y_hat.device
    pixel_list = _pixel_list_form(params_fn, B, "encode_views")
    band_rows = effective_band_rows(h, band_rows)
    desc, n, _, nrows = _stream_table(chans, minmaxes, HW, dev)
    err = torch.zeros(B, dtype=torch.int32, device=dev)
    sf = torch.empty((max(nrows, 1), 2), dtype=torch.int32, device=dev)
    if n:
        order = np.concatenate(wavefront_steps(h, w, band_rows))
        pix = torch.from_numpy((np.arange(B, dtype=np.int64)[:, None] * HW + order[None, :]).reshape(-1).astype(np.int32)).to(dev)
        if pixel_list:                                        # the decoder's own kernels, on all pixels at once (bit-identical parameters)
            params_fn.set_latent(y_hat)
            params_fn.run(pix, None, 0, B * HW, **_band_kw(band_rows))
            sigma, mu, logits = params_fn.sigma, params_fn.mu, params_fn.logits
        else:
            sigma, mu, logits = _full_latent_params(params_fn, y_hat, K * M)
        check(lib.masic_gmm_cdf_rows_batch(_p(sigma), _p(mu), _p(logits), M, K, HW, _p(pix), None, B * HW, HW,
                                           _p(desc), n, float(scale_bound), _p(y_hat), None, _p(sf), _p(err),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gmm_cdf_rows_batch")
    if coder == "device":
        return _encode_device(sf, desc, n, HW, _first_streams(chans), err, names)[0]
    check_errs(err, "encode", names)
    sf_h = sf.cpu().numpy()
    jobs, r0 = [], 0
    for ch in chans:
        jobs.append((sf_h[r0:r0 + HW * len(ch)], HW if len(ch) else 0, len(ch)))
        r0 += HW * len(ch)
    return _encode_pairs(jobs)


_BATCH_LISTS = {}


def _band_kw(band_rows):
    """params_fn.run's keyword: only passed with bands on, so that a params_fn without bands keeps its four-argument run."""
    return {"band_rows": band_rows} if band_rows else {}


def _batch_step_lists(h, w, B, device, band_rows=0):
    """Per coding step, two int32 [steps][B * h] device lists of entries b * h * w + p (-1 padded), kept per shape: the tables' and the
    decoder's (pair b's pixels at [b * h, (b + 1) * h), the layout of one pair's list), and the pixel-list kernels' (the same pixels packed
    to the front: workgroups whose 32 entries are all padding leave at once)."""
    key = (h, w, B, str(device), effective_band_rows(h, band_rows))
    t = _BATCH_LISTS.get(key)
    if t is None:
        steps = wavefront_steps(h, w, band_rows)
        per = np.full((len(steps), B, h), -1, dtype=np.int64)
        packed = np.full((len(steps), B * h), -1, dtype=np.int64)
        for i, p in enumerate(steps):
            q = np.arange(B, dtype=np.int64)[:, None] * (h * w) + p[None, :]
            per[i, :, :p.size] = q
            packed[i, :q.size] = q.reshape(-1)
        if len(_BATCH_LISTS) >= 16:
            _BATCH_LISTS.clear()
        t = _BATCH_LISTS[key] = tuple(torch.from_numpy(a.reshape(-1).astype(np.int32)).to(device) for a in (per, packed))
    return t


def decode_views(params_fn, datas, shape, M, K, chans, minmaxes, scale_bound, device, names=None, use_graph=True, verify=True,
                 band_rows=0):
    """The inverse of encode_views (datas: pair b's y stream as it framed it) -> y_hat [B, M, h, w]; a pair's slice does not depend on
    its batch mates.  Coding step by coding step, entirely on the device: parameters from what is decoded so far -> tables of the
    step's pixels -> one wavefront per channel stream finds the symbols and writes them into the latent.  The device side of a step
    (context convolution, nine head layers, table kernel, decode kernel, each over every pair: ~18 launches of a few microseconds) is
    captured once into a HIP graph over static buffers and replayed w + 3 (h - 1) times back to back (w + 3 (band_rows - 1) times with
    the row bands of wavefront_steps: band_rows must be the encoder's); the step index lives in device
    memory (incremented by the decode kernel), so the host neither feeds nor waits for anything until the last replay.  After the
    last step one more launch (masic_rans_decode_finish_batch, outside the graph) checks that every channel stream consumed exactly its
    words and left the coder in the encoder's initial state; its flag comes back with the others in the one read of `err`
    (verify=False leaves the launch out: for timing the check).  A stream error names its pair (PairStreamError; CorruptStreamError
    for the final-state check)."""
    h, w = shape
    B, HW = len(datas), h * w
    pixel_list = _pixel_list_form(params_fn, B, "decode_views")
    band_rows = effective_band_rows(h, band_rows)
    y_hat = torch.zeros((B, M, h, w), dtype=torch.float32, device=device)
    blobs, wo, wc, base = [], [], [], 0
    for b, data in enumerate(datas):
        streams, _ = split_channels(data)
        nch = len(chans[b])
        if len(streams) != nch or any(len(s_) < 8 or len(s_) % 4 for s_ in streams):
            raise ValueError(f"masic_amd.codec: the y stream{_pair_tag(b, B, names, ' of pair %s')} does not hold one rANS stream per coded channel")
        cnt = np.array([len(s_) // 4 for s_ in streams], dtype=np.int64)
        wo.append(base + np.cumsum(cnt) - cnt)
        wc.append(cnt)
        base += int(cnt.sum())
        blobs.extend(streams)
    if not blobs:
        return y_hat
    desc, n, nstarts, _ = _stream_table(chans, minmaxes, h, device, words=list(zip(wo, wc)))
    words = np.frombuffer(b"".join(blobs), dtype=np.uint32)
    off = np.concatenate(wo)
    state0 = words[off].astype(np.uint64) | (words[off + 1].astype(np.uint64) << np.uint64(32))
    words_d = torch.from_numpy(words.copy().view(np.int32)).to(device)
    state_init = torch.from_numpy(state0.view(np.int64)).to(device)
    state_d = state_init.clone()
    pos_d = torch.full((n,), 2, dtype=torch.int32, device=device)
    step_d = torch.zeros(1, dtype=torch.int32, device=device)
    done_d = torch.zeros(1, dtype=torch.int32, device=device)
    err = torch.zeros(B, dtype=torch.int32, device=device)
    starts = torch.empty(nstarts, dtype=torch.int16, device=device)
    pix_d, pix_packed = _batch_step_lists(h, w, B, device, band_rows)
    y16 = params_fn.y16 if pixel_list else None

    def device_step():
        if pixel_list:                                        # the step's <= B * h pixels only (masic_amd/csrc/skinny.hip)
            params_fn.run(pix_packed, step_d, B * h, B * h, **_band_kw(band_rows))
            sigma, mu, logits = params_fn.sigma, params_fn.mu, params_fn.logits
        else:
            sigma, mu, logits = _full_latent_params(params_fn, y_hat, K * M)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.masic_gmm_cdf_rows_batch(_p(sigma), _p(mu), _p(logits), M, K, HW, _p(pix_d), _p(step_d), B * h, h,
                                           _p(desc), n, float(scale_bound), None, _p(starts), None, _p(err), st), "gmm_cdf_rows_batch")
        check(lib.masic_rans_decode_step_batch(_p(words_d), _p(desc), n, _p(state_d), _p(pos_d), _p(starts), _p(pix_d), B * h, _p(step_d), h, M,
                                               _p(y_hat), _p(y16) if y16 is not None else None, HW, _p(err), _p(done_d), st), "rans_decode_step_batch")

    def reset():
        y_hat.zero_()
        if y16 is not None:
            y16.zero_()
        state_d.copy_(state_init)
        pos_d.fill_(2)
        step_d.zero_()
        done_d.zero_()
        err.zero_()

    nsteps = len(wavefront_steps(h, w, band_rows))
    cur = torch.cuda.current_stream()
    if use_graph:
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            device_step()                                     # weight packs and allocator warm before the capture (advances the coder: reset below)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            device_step()
        reset()
        for _ in range(nsteps):
            graph.replay()
    else:
        for _ in range(nsteps):
            device_step()
    if verify:
        check(lib.masic_rans_decode_finish_batch(_p(desc), n, _p(state_d), _p(pos_d), _p(err), ctypes.c_void_p(cur.cuda_stream)),
              "rans_decode_finish_batch")
    check_errs(err, "decode", names)
    return y_hat
