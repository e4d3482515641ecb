/* masic_refine.h -- the elementwise kernels of the encoder-side latent refinement (masic_amd/csrc/refine.hip, masic_amd/refine.py;
 * DESIGN.md section 8.10).
 *
 * A header of libmasic_hip.so beside include/masic_hip.h, written in the forms masic_amd/_lib.parse_header accepts and bound by
 * masic_amd/refine.py.  include/masic_hip.h is pinned declaration by declaration (tests/golden/abi.json); entry points that are not
 * part of that pinned ABI live in headers of their own.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK,
 * the message in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.
 *
 * The refinement works on FOUR float32 tensors at a time (the latents y1, y2, z1, z2 of B pairs, or their noise, gradients and Adam
 * states): `float* const* t` is a HOST array of four device pointers, `n` a HOST array of the four element counts PER PAIR; tensor k is
 * contiguous [B, n[k]].  Every kernel is elementwise over a bounded grid with a grid-stride loop, moves 16 bytes per lane where the
 * addresses allow it and single floats at the head and tail of a pair's slice (a slice of n floats starts on a 16-byte boundary only
 * when n % 4 == 0), uses no atomics and no grid-wide synchronisation, and reads nothing on the host: every launch can be captured.
 * MASIC_ERR_ARG for a null pointer, B outside 1 .. 65535 (the pair is a grid dimension) or an element count of 0; nothing is launched
 * then.
 */
#ifndef MASIC_REFINE_H
#define MASIC_REFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[k][b][i] = (w >> 8) * 2^-24 - 1/2 in [-1/2, 1/2), w = word 0 of Philox4x32-10 with key (seed, pair_keys[b]) and counter
 * (i mod 2^32, k, *step, i >> 32).  pair_keys: B uint32 on the device; step: one int32 on the device (a captured loop replays the
 * launch while the scalar counts on).  One launch for the four tensors.  Pair b's values depend on (seed, pair_keys[b], *step) only. */
int masic_refine_noise(float* const* out, const size_t* n, int B, uint32_t seed, const uint32_t* pair_keys, const int32_t* step,
                       void* stream);

/* One bias-corrected Adam step on the four tensors, float32 state, one launch: with t = *step (>= 1, an int32 on the device),
 *   m = 0.9 m + 0.1 g;  v = 0.999 v + 0.001 g g;  p -= lr * (m / (1 - 0.9^t)) / (sqrt(v / (1 - 0.999^t)) + 1e-8).
 * No weight decay.  p, g, m, v: tensor k contiguous [B, n[k]]. */
int masic_refine_adam(float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n, int B, double lr,
                      const int32_t* step, void* stream);

/* For every pair b with j_now[b] < j_best[b]: best[k][b][:] = cur[k][b][:] for the four tensors, then j_best[b] = j_now[b] (a second,
 * B-lane launch after the copies: no block reads j_best while another writes it).  j_now, j_best: float64 [B] on the device.  A NaN
 * j_now never replaces anything. */
int masic_refine_keep_best(const float* const* cur, float* const* best, const size_t* n, int B, const double* j_now, double* j_best,
                           void* stream);

/* Backward of the per-pair objective J_b = bits_b / hw + lmbda 255^2 (MSE1_b + MSE2_b) (masic_amd.autograd.PairRateDistortionFn):
 *   g1[b][i] = g[b] * 2 lmbda 255^2 (x1_hat - x1) / n_pic,  g2 likewise,  gl[k][b][i] = -g[b] / (ln 2 * hw * liks[k][b][i])
 * in one launch; g: float64 [B] on the device, or null for ones.  x*: contiguous float32 [B, n_pic] (n_pic = 3 H W); liks / gl: HOST
 * arrays of nliks (0 .. 4) device pointers, lik_n the element counts per pair. */
int masic_refine_rd_seeds(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                          const float* const* liks, const size_t* lik_n, int nliks, int B, double lmbda, double hw, const double* g,
                          float* g1, float* g2, float* const* gl, void* stream);

#ifdef __cplusplus
}
#endif

#endif
