/* masic_d2s.h -- the 128 -> C (C <= 8) 5x5 stride-2 transposed last layer of the synthesis transforms on a kernel of its own
 * (masic_amd/csrc/d2s_layer.hip).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/d2s_layer.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the
 * message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_D2S_H
#define MASIC_D2S_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if masic_d2s_layer_f16k_fwd runs a [B][128][Hi][Wi] input, else 0.  The form is fixed -- the equivalent stride-1 3x3 convolution of
 * ConvTranspose2d(128, C <= 8, 5, stride 2, padding 2, output_padding 1) to 32 padded rows (masic_deconv_s2_as_conv_weight), a whole
 * bf16 F16K input, bf16 operands, the depth-to-space store of masic_conv_f16k_d2s_fwd -- so anything else (other channel counts, a
 * channel view of the input, fp8) is the caller's to keep on masic_conv_f16k_d2s_fwd. */
int masic_d2s_layer_f16k_supported(int B, int Hi, int Wi);

/* 1 where the eval forward takes masic_d2s_layer_f16k_fwd instead of masic_conv_f16k_d2s_fwd: masic_conv_f16k_d2s_fwd runs the shape on
 * conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false> -- the 16-channel-chunk row whose slab stream and sum order this kernel shares: Wi >= 32
 * and at least 512 tiles of 32 x 32 pixels, times B -- and the tile count reaches the measured threshold (profiles/d2s_layer_ab.txt).
 * 0 for an unsupported shape.  On that row the bits do not depend on the choice. */
int masic_d2s_layer_f16k_preferred(int B, int Hi, int Wi);

/* The layer, bit for bit what masic_conv_f16k_d2s_fwd stores for the same inputs where it runs the row named above.
 * x_f16k [B][8][Hi*Wi][16] bf16; w_packed: masic_conv_f16k_pack_weight's stream of the equivalent convolution in that row's order
 * (8 chunks of 16 channels x 5 steps of 2 taps x 4 KiB); bias [32] float32 (row 4c + phase) or null; y_nchw float32
 * [B][y_ctot][2 Hi][2 Wi], written at channels y_coff .. y_coff + C - 1.  max_wgs: 0 = the launcher's own grid (one persistent workgroup
 * per CU); a positive value caps it -- the result does not depend on it. */
int masic_d2s_layer_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y_nchw, int C, int y_ctot, int y_coff,
                             int B, int Hi, int Wi, int max_wgs, void* stream);

/* The symbol of the kernel that call launches, as rocprofv3 prints it. */
int masic_d2s_layer_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n);

#ifdef __cplusplus
}
#endif

#endif
