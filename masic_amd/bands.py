"""The masked 5x5 context model on a pixel list with the latent cut into independent row bands: the banded form of skinny_f16k<8, true>
(masic_amd/csrc/skinny.hip; DESIGN.md section 8.1 "Row bands").

    bands.skinny_ctx(group, pix, step, list_stride, npix, nimg, h, w, gate, gate_ctot, gate_c, band_rows, stream)

A tap whose row lies above the top of its pixel's band reads zeros, as a tap above the latent's top does: the bands' coding wavefronts
do not depend on each other and run side by side (codec.wavefront_steps(h, w, band_rows)).  Callers go through
`ops.skinny_group(..., ctx=True, band_rows=S)`, which fills the masic_gemm_group_t and routes here for S > 0.

The entry point is declared in include/masic_bands.h, a side header of libmasic_hip.so bound by _lib.bind_header.  No CPU path.
"""
import contextlib
import ctypes
import operator

from . import _lib

HEADER_PATH = _lib.header_path("masic_bands.h")
MAX_BAND_ROWS = 255               # the .bin header stores band_rows in one byte (coremasic/mywork/MASIC.py: _write_pair)

SIGNATURES = _lib.bind_header(HEADER_PATH, "masic_bands_")          # name -> (restype, argtypes) of every prototype of masic_bands.h


def check_band_rows(band_rows, who):
    """band_rows as the public interface takes it -> int in 0 .. 255 (0: no bands); ValueError for anything else (bools, floats and
    strings included: a value that is written into a file header is not coerced)."""
    try:
        v = None if isinstance(band_rows, bool) else operator.index(band_rows)
    except TypeError:
        v = None
    if v is None or not 0 <= v <= MAX_BAND_ROWS:
        raise ValueError(f"{who}: band_rows must be an integer in 0 .. {MAX_BAND_ROWS} (0: one band, the whole latent), got {band_rows!r}")
    return v


@contextlib.contextmanager
def model_band_rows(hsic, band_rows):
    """`with model_band_rows(hsic, S):` -- hsic.band_rows = S inside (the context model every forward, the training graph, the latent
    refinement and evaluate_folder's estimate then model is that of a file coded with band_rows = S), the earlier value after it."""
    S = check_band_rows(band_rows, "model_band_rows")
    before = hsic.band_rows
    hsic.band_rows = S
    try:
        yield hsic
    finally:
        hsic.band_rows = before


def skinny_ctx(group, pix, step, list_stride, npix, nimg, h, w, gate, gate_ctot, gate_c, band_rows, stream):
    """masic_bands_skinny_ctx_fwd_batch; group: one _lib.GemmGroup (or an array's first), the pointers ctypes.c_void_p."""
    _lib.check(_lib.lib.masic_bands_skinny_ctx_fwd_batch(ctypes.cast(ctypes.pointer(group), ctypes.c_void_p), pix, step, int(list_stride),
                                                         int(npix), int(nimg), int(h), int(w), gate, int(gate_ctot), int(gate_c),
                                                         int(band_rows), stream), "bands_skinny_ctx_fwd_batch")
