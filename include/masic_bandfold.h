/* masic_bandfold.h -- the row bands of the y latents as a batch of images, and back (masic_amd/csrc/band_fold.hip; DESIGN.md section 8.1
 * "Row bands in the model").
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/bandfold.py.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the message in
 * masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 *
 * A float32 NCHW latent [B, C, h, w] is cut into T = ceil(h / S) bands of S rows, the last one shorter when h is no multiple of S.
 * Folded, the bands are the images of a batch [B T, C, S, w]: image b T + t holds rows t S .. t S + S - 1 of picture b, and the
 * rows a short last band lacks are +0.0.  A convolution with zero padding on the folded batch sees, above each band, what it sees
 * above the latent's own top.  Each call below is one kernel launch; fold and the ungated float32 unfold are each other's adjoint.
 * MASIC_ERR_ARG for a null tensor, S < 1 and non-positive sizes; MASIC_ERR_SHAPE for a channel slice outside its buffer.
 */
#ifndef MASIC_BANDFOLD_H
#define MASIC_BANDFOLD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dst[b T + t, c, s, x] = src[b, c, t S + s, x] where t S + s < h, +0.0 elsewhere: every element of dst [B T, C, S, w] is written. */
int masic_bandfold_fold(const float* src, float* dst, int B, int C, int h, int w, int S, void* stream);

/* The inverse index map, padding rows dropped: dst[b, dst_coff + c, r, x] = src[b T + r / S, c, r % S, x] [* gate[b, gate_c, r, x]]
 * for a float32 NCHW dst of dst_ctot channels (a concat buffer; its other channels are not touched).  gate: float32
 * [B, gate_ctot, h, w] or null; the product is a float32 multiplication. */
int masic_bandfold_unfold(const float* src, float* dst, int B, int C, int h, int w, int S, int dst_ctot, int dst_coff,
                          const float* gate, int gate_ctot, int gate_c, void* stream);

/* ... into channels [dst_coff, dst_coff + C) of an F16K buffer [B][dst_ctot / 16][h w][16] of bf16 records (dst_ctot and dst_coff
 * multiples of 16): one rounding to bf16 after the float32 gate product, the rounding and the record stores of
 * masic_nchw_to_f16k_view_op -- 16-byte half records, the channels of the last one past C stored as zeros. */
int masic_bandfold_unfold_f16k(const float* src, void* dst, int B, int C, int h, int w, int S, int dst_ctot, int dst_coff,
                               const float* gate, int gate_ctot, int gate_c, void* stream);

/* The float32 kernels walk their elements with a grid of at most this many workgroups of 256 lanes. */
int masic_bandfold_max_blocks(void);

#ifdef __cplusplus
}
#endif

#endif
