/* masic_metrics.h -- per-pair reductions of the test-split evaluation (masic_amd/csrc/metrics.hip, masic_amd/metrics.py,
 * masic_amd/evaluate.py).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/metrics.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK,
 * the message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.  No atomics: both reductions are a
 * stage over blocks and a finishing launch, so a result never depends on the order in which blocks ran.
 */
#ifndef MASIC_METRICS_H
#define MASIC_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The six sums of masic_rd_loss, per pair.  x1_hat, x1, x2_hat, x2: contiguous float32 [B, n_pic]; liks: a HOST array of nliks (0 .. 4)
 * device pointers to contiguous float32 [B, lik_n[k]] tensors, lik_n a host array of the element counts per image.  out: B rows of six
 * float64, row b = { sum (x1_hat - x1)^2, sum (x2_hat - x2)^2, sum log liks[0], .., sum log liks[3] } over image b's slices; the
 * entries of absent likelihood tensors are 0.  Row b holds, bit for bit, what masic_sse / masic_sum_log return for image b's slice
 * alone: the same partition of the slice into blocks, the same float64 order within a block and the same finishing order.
 * workspace: masic_metrics_pair_rd_workspace_bytes(B) bytes.  MASIC_ERR_ARG for a null pointer, nliks outside 0 .. 4 or B outside
 * 1 .. 65535 (the image is a grid dimension); nothing is launched then. */
size_t masic_metrics_pair_rd_workspace_bytes(int B);
int masic_metrics_pair_rd(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                          const float* const* liks, const size_t* lik_n, int nliks, int B, double* out, void* workspace, void* stream);

/* Sums of squared byte differences of P pairs of 8-bit pictures.  a, b: contiguous uint8 [P, n] (e.g. [P,H0,W0,3]), picture p at byte
 * p * n of each; out[p] = sum_i (a[p][i] - b[p][i])^2 as uint64: exact, so independent of any order of summation.  Any n >= 1 and any
 * alignment: lanes read 16-byte pieces where both pictures allow it and single bytes at a picture's head and tail (or throughout, where
 * the two pictures are aligned differently).  workspace: masic_metrics_u8_sse_workspace_bytes(P) bytes.  MASIC_ERR_ARG for a null
 * pointer, n < 1 or P outside 1 .. 65535; nothing is launched then. */
size_t masic_metrics_u8_sse_workspace_bytes(int P);
int masic_metrics_u8_sse(const uint8_t* a, const uint8_t* b, size_t n, int P, uint64_t* out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
