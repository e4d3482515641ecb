/* masic_budget.h -- the kernels of the latent refinement under a bit budget (masic_amd/csrc/refine_budget.hip, masic_amd/refine.py;
 * DESIGN.md section 8.10): per pair b, minimise D_b = MSE1_b + MSE2_b subject to R_b <= T_b (bits), with a multiplier mu_b on the rate.
 *
 * A header of libmasic_hip.so beside include/masic_hip.h and include/masic_refine.h, written in the forms masic_amd/_lib.parse_header
 * accepts and bound by masic_amd/refine.py.  Prototypes only.  Conventions are masic_hip.h's: int status (0 = MASIC_OK, the message
 * in masic_last_error()), device pointers, no allocation, `stream` a hipStream_t.  Tensors and host pointer arrays are
 * masic_refine.h's: `float* const* t` is a HOST array of four device pointers, `n` a HOST array of the four element counts PER PAIR,
 * tensor k contiguous [B, n[k]].  The elementwise kernels run over a bounded grid with a grid-stride loop, the pair a grid dimension
 * (B in 1 .. 65535), 16 bytes per lane where a slice's addresses allow it and single floats at its head and tail; the [B]-sized
 * state (r_best, d_best, mu: float64 on the device) is updated by B-lane launches.  No atomics, no grid-wide synchronisation,
 * nothing read on the host: every launch can be captured.  MASIC_ERR_ARG for a null required pointer, B out of range, an element
 * count of 0 or a scalar outside its range; nothing is launched then.
 *
 * Launches per check of the loop: 3 -- masic_budget_select's two (the copies, then r_best / d_best) and masic_budget_mu's one.
 * masic_budget_rd_seeds is one launch per step, as masic_refine_rd_seeds is.
 */
#ifndef MASIC_BUDGET_H
#define MASIC_BUDGET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of J_b(mu) = mu_b bits_b / hw + lmbda 255^2 (MSE1_b + MSE2_b) (masic_amd.autograd.PairBudgetFn): masic_refine_rd_seeds
 * with the likelihood seeds scaled by the pair's multiplier,
 *   g1[b][i] = g[b] * 2 lmbda 255^2 (x1_hat - x1) / n_pic,  g2 likewise,  gl[k][b][i] = -g[b] mu[b] / (ln 2 * hw * liks[k][b][i])
 * in one launch.  g, mu: float64 [B] on the device, or null for ones.  The factor of a slice is (float)((g[b] * mu[b]) * s) with s the
 * float64 constant masic_refine_rd_seeds uses: with mu null or all ones every output is bit-equal to masic_refine_rd_seeds'. */
int masic_budget_rd_seeds(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                          const float* const* liks, const size_t* lik_n, int nliks, int B, double lmbda, double hw, const double* g,
                          const double* mu, float* g1, float* g2, float* const* gl, void* stream);

/* The constrained keep-best.  Pair b's candidate (r_now[b], d_now[b]) replaces the kept iterate (r_best[b], d_best[b]) if and only if
 * neither candidate value is NaN and, with "feasible" meaning r <= target[b],
 *   the candidate is feasible and the kept one is not,  or  both are feasible and d_now < d_best,  or  both are infeasible and
 *   r_now < r_best.
 * Equality never replaces; an infeasible candidate never replaces a feasible one.  Where it wins, best[k][b][:] = cur[k][b][:] for
 * the four tensors; then, in a second, B-lane launch after the copies (no block reads state another writes), r_best[b] = r_now[b] and
 * d_best[b] = d_now[b].  All five [B] arrays float64 on the device; cur is only read. */
int masic_budget_select(const float* const* cur, float* const* best, const size_t* n, int B, const double* r_now, const double* d_now,
                        const double* target, double* r_best, double* d_best, void* stream);

/* mu[b] = min(max(mu[b] * exp(gain * (r_now[b] / target[b] - 1)), mu_min), mu_max) in float64, one B-lane launch; a NaN r_now[b]
 * leaves mu[b] as it is.  gain, mu_min, mu_max: finite and positive, mu_min <= mu_max. */
int masic_budget_mu(double* mu, const double* r_now, const double* target, int B, double gain, double mu_min, double mu_max,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif
