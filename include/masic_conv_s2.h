/* masic_conv_s2.h -- the 5x5 stride-2 128 -> 128 convolution with fused forward GDN of the analysis transforms on a kernel of its own
 * (masic_amd/csrc/conv_s2_gdn.hip).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/conv_s2.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the
 * message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_CONV_S2_H
#define MASIC_CONV_S2_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if masic_conv_s2_gdn_f16k_fwd runs a [B][128][Hi][Wi] input, else 0.  The form is fixed -- Conv2d(128, 128, 5, stride 2, padding 2),
 * bf16 F16K input and output without a channel view, one-product forward GDN -- so anything else (other channel counts, the inverse or
 * the three-product GDN, a channel view, fp8, a second pre-GDN output) is the caller's to keep on masic_conv_f16k_gdn_fwd. */
int masic_conv_s2_gdn_f16k_supported(int B, int Hi, int Wi);

/* y = GDN(conv(x) + bias), bit for bit what masic_conv_f16k_gdn_fwd (gdn_inverse = 0, F16K output) stores.
 * x_f16k [B][8][Hi*Wi][16] bf16; w_packed: masic_conv_f16k_pack_weight's stream for the layer's descriptor; bias [128] float32 or
 * null; gdn_packed: masic_gdn_pack_f16k's image; y_f16k [B][8][Ho*Wo][16] bf16 with Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1. */
int masic_conv_s2_gdn_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, void* y_f16k,
                               int B, int Hi, int Wi, void* stream);

/* The symbol of the kernel that call launches, as rocprofv3 prints it. */
int masic_conv_s2_gdn_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n);

#ifdef __cplusplus
}
#endif

#endif
