/* masic_deconv.h -- the transposed 5x5 stride-2 128 -> 128 convolution with fused inverse GDN of the synthesis transforms on a kernel of
 * its own (masic_amd/csrc/deconv_igdn.hip).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/deconv.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the
 * message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_DECONV_H
#define MASIC_DECONV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if masic_deconv_igdn_f16k_fwd runs a [B][128][Hi][Wi] input, else 0.  The form is fixed -- ConvTranspose2d(128, 128, 5, stride 2,
 * padding 2, output_padding 1), bf16 F16K input and output without a channel view, one-product inverse GDN -- so anything else
 * (other channel counts, the three-product GDN, a channel view, fp8, a second pre-GDN output) is the caller's to keep on
 * masic_conv_f16k_gdn_fwd. */
int masic_deconv_igdn_f16k_supported(int B, int Hi, int Wi);

/* y = IGDN(conv_transpose(x) + bias), bit for bit what masic_conv_f16k_gdn_fwd (gdn_inverse = 1, F16K output) stores.
 * x_f16k [B][8][Hi*Wi][16] bf16; w_packed: masic_conv_f16k_pack_weight's stream for the layer's descriptor; bias [128] float32 or
 * null; gdn_packed: masic_gdn_pack_f16k's image; y_f16k [B][8][4*Hi*Wi][16] bf16.
 * tile: 0 = chosen from the shape, 1 = 16 x 32 input pixels per workgroup, 2 = 8 x 32.  split: workgroups per tile -- 4 = one output
 * phase each (what 0 chooses), 2 = phases {0, 3} and {1, 2}, 1 = all four phases in one workgroup.  The result depends on neither. */
int masic_deconv_igdn_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, void* y_f16k,
                               int B, int Hi, int Wi, int tile, int split, void* stream);

/* The symbol of the kernel that call launches, as rocprofv3 prints it. */
int masic_deconv_igdn_f16k_kernel_name(int B, int Hi, int Wi, int tile, int split, char* buf, size_t n);

#ifdef __cplusplus
}
#endif

#endif
