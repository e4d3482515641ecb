/* masic_bands.h -- the masked 5x5 context model on a pixel list with the latent cut into independent row bands (the banded form of
 * skinny_f16k<8, true>, masic_amd/csrc/skinny.hip; DESIGN.md section 8.1 "Row bands").
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/bands.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only, so the layer description is passed as a `const void*` to a
 * masic_gemm_group_t of masic_hip.h.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the message in masic_last_error()),
 * device pointers, no allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_BANDS_H
#define MASIC_BANDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ctx case of masic_skinny_group_fwd_batch with a band top: `group` points to ONE masic_gemm_group_t (the 5x5 type-A masked
 * convolution; w_packed from masic_skinny_ctx_pack_weight), every other argument means what it means there.  The latent's rows are
 * cut into bands of band_rows rows (the last one shorter when h is no multiple); a tap of pixel (pr, pc) whose row lies above the
 * pixel's band, r < (pr / band_rows) * band_rows, reads zeros -- as a tap above the latent's own top does.  Columns behave as there.
 * The result at a pixel is, bit for bit, what masic_skinny_group_fwd_batch computes for it on its band cut out as an image of its own;
 * band_rows >= h is that call itself.  MASIC_ERR_ARG for band_rows < 1. */
int masic_bands_skinny_ctx_fwd_batch(const void* group, const int32_t* pix, const int32_t* step, int list_stride, int npix, int nimg,
                                     int h, int w, const float* gate, int gate_ctot, int gate_c, int band_rows, void* stream);

#ifdef __cplusplus
}
#endif

#endif
