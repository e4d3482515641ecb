/* masic_latent.h -- the 5x5 stride-2 128 -> 192 latent layer of the analysis transforms on a kernel of its own
 * (masic_amd/csrc/conv_s2_latent.hip).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/latent.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the
 * message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_LATENT_H
#define MASIC_LATENT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if masic_latent_s2_f16k_fwd runs a [B][128][Hi][Wi] input, else 0.  The form is fixed -- Conv2d(128, 192, 5, stride 2, padding 2),
 * a whole bf16 F16K input, bf16 operands, no activation, the outputs of masic_conv_f16k_multi_fwd -- so anything else (other channel
 * counts or geometry, a channel view of the input, fp8) is the caller's to keep on masic_conv_f16k_multi_fwd. */
int masic_latent_s2_f16k_supported(int B, int Hi, int Wi);

/* 1 where the eval forward takes masic_latent_s2_f16k_fwd instead of masic_conv_f16k_multi_fwd: the launch has at least as many
 * workgroups (tiles of 4 x 32 output pixels, times B) as the measured threshold (profiles/conv_s2_latent_ab.txt).  0 for an unsupported
 * shape.  The bits do not depend on the choice. */
int masic_latent_s2_f16k_preferred(int B, int Hi, int Wi);

/* v = conv(x) + bias stored in up to four layouts, bit for bit what masic_conv_f16k_multi_fwd stores for the same inputs.
 * x_f16k [B][8][Hi*Wi][16] bf16; w_packed: masic_conv_f16k_pack_weight's stream for the layer's descriptor; bias [192] float32 or
 * null.  The outputs are masic_f16k_multi_out_t's fields, each optional (null), at least one given, with Ho = (Hi - 1) / 2 + 1,
 * Wo = (Wi - 1) / 2 + 1: y32 float32 [B][192][Ho][Wo] v; round32 float32 [B][192][Ho][Wo] rintf(v); round16 F16K of round16_ctot
 * channels, written at channels round16_coff .. (both multiples of 16): bf16(rintf(v) * gate); abs16 F16K [B][12][Ho*Wo][16] bf16(|v|);
 * gate float32 [B][gate_ctot][Ho][Wo], channel gate_c (round16 only), or null. */
int masic_latent_s2_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y32, float* round32, void* round16,
                             void* abs16, const float* gate, int B, int Hi, int Wi, int round16_ctot, int round16_coff, int gate_ctot,
                             int gate_c, void* stream);

/* The symbol of the kernel that call launches, as rocprofv3 prints it. */
int masic_latent_s2_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n);

#ifdef __cplusplus
}
#endif

#endif
