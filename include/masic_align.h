/* masic_align.h -- weight-free homography estimation by coarse-to-fine photometric alignment.
 *
 * A second header of libmasic_hip.so, written in the forms masic_amd/_lib.parse_header accepts and bound by masic_amd/align.py.
 * include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not part of that pinned
 * ABI live here.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the message in masic_last_error()), device pointers, no
 * allocation, `stream` a hipStream_t.
 */
#ifndef MASIC_ALIGN_H
#define MASIC_ALIGN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the caller-owned workspace of masic_align_patches: the pyramid levels below the finest of both patches of every pair
 * (0 at P = 32; 0 as well for a B or P the launch refuses). */
size_t masic_align_workspace_bytes(int B, int P);

/* delta [B,4,2] with b(u) ~ a(W(u; delta)), W(s_k) = s_k + delta_k on the square s = (0,0), (P,0), (P,P), (0,P), from the grey
 * patches a, b [B,1,P,P] (float32, P in {32, 64, 128}); one launch, workgroup i handles pair i, 1 <= B <= 65535.
 * delta0 [B,4,2] or null: the start value; with null the start is zero and an integer translation search in
 * [-search_radius, search_radius]^2 (0 <= search_radius <= 15) on the 32 x 32 level comes first.
 * it0, it1, it2: Gauss-Newton steps per level, coarse to fine, 0 <= it <= 1000; the finest level takes it2, the one below it1
 * (P = 64 uses it1 and it2, P = 32 it2 alone).
 * damping: lambda of (J^T J + lambda diag(J^T J)) dp = J^T r.
 * info [B,4]: masked MSE at the start value, masked MSE and valid fraction at the returned delta, status (0: delta is the
 * estimate; 1: a guard fired -- delta is the start value exactly, the MSEs are NaN and the fraction 0; 2: the estimate's MSE exceeds
 * the start's -- delta is the start value exactly). */
int masic_align_patches(const float* a, const float* b, const float* delta0, float* delta, float* info, void* workspace,
                        int B, int P, int search_radius, int it0, int it1, int it2, float damping, void* stream);

#ifdef __cplusplus
}
#endif

#endif
