// refine_budget.hip -- the kernels of the latent refinement under a bit budget (include/masic_budget.h; masic_amd/refine.py; DESIGN.md
// section 8.10): the seeds of J_b(mu)'s backward, the constrained keep-best and the multiplier update.
//
// The elementwise ones take refine.hip's launch shape (refine_slices.h); the [B]-sized state is updated by B-lane launches that follow
// them on the stream.  No atomics, no grid-wide synchronisation, nothing read by the host.
#include <cmath>

#include "common.h"
#include "masic_budget.h"
#include "refine_slices.h"

namespace {

// the rule of masic_budget_select for one pair; every comparison with a NaN is false
__device__ __forceinline__ bool candidate_wins(double r, double d, double t, double rb, double db) {
    if (r != r || d != d) return false;
    const bool fc = r <= t, fk = rb <= t;
    if (fc != fk) return fc;
    return fc ? d < db : r < rb;
}

struct SelectOp {
    const float* cur[NT]; float* best[NT]; size_t n[NT];
    const double* r_now; const double* d_now; const double* target; const double* r_best; const double* d_best;
    const float* c; float* d;
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        if (!candidate_wins(r_now[b], d_now[b], target[b], r_best[b], d_best[b])) return false;
        c = cur[t] + (size_t)b * nn; d = best[t] + (size_t)b * nn;
        const uintptr_t a[2] = {(uintptr_t)c, (uintptr_t)d};
        s = span_of(nn, a);
        return true;
    }
    __device__ void one(size_t i) { d[i] = c[i]; }
    __device__ void four(size_t i) { *reinterpret_cast<float4*>(d + i) = *reinterpret_cast<const float4*>(c + i); }
};

__global__ __launch_bounds__(256) void select_state_kernel(const double* __restrict__ r_now, const double* __restrict__ d_now,
                                                           const double* __restrict__ target, double* __restrict__ r_best,
                                                           double* __restrict__ d_best, int B) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256)
        if (candidate_wins(r_now[b], d_now[b], target[b], r_best[b], d_best[b])) { r_best[b] = r_now[b]; d_best[b] = d_now[b]; }
}

__global__ __launch_bounds__(256) void mu_kernel(double* __restrict__ mu, const double* __restrict__ r_now, const double* __restrict__ target,
                                                 int B, double gain, double mu_min, double mu_max) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        const double r = r_now[b];
        if (r != r) continue;
        const double m = mu[b] * exp(gain * (r / target[b] - 1.0));
        mu[b] = fmin(fmax(m, mu_min), mu_max);
    }
}

// ---- seeds of J_b(mu): refine.hip's SeedOp with the pair's multiplier on the likelihood tensors (2..); the pictures (0, 1) as there
struct BudgetSeedOp {
    const float* a_[NT]; const float* b_[NT]; float* o_[NT]; size_t n[NT];
    const double* g; const double* mu; double s_pic, s_lik;
    const float* a; const float* x; float* o; float sc; bool lik;
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        const size_t off = (size_t)b * nn;
        lik = t >= 2;
        a = a_[t] + off; x = lik ? a : b_[t] + off; o = o_[t] + off;
        double gb = g ? g[b] : 1.0;
        if (lik && mu) gb = gb * mu[b];                          // * 1.0 is exact: mu of ones gives masic_refine_rd_seeds' bits
        sc = (float)(gb * (lik ? s_lik : s_pic));
        const uintptr_t ad[3] = {(uintptr_t)a, (uintptr_t)x, (uintptr_t)o};
        s = span_of(nn, ad);
        return true;
    }
    __device__ float f(float av, float xv) const { return lik ? sc / av : sc * (av - xv); }
    __device__ void one(size_t i) { o[i] = f(a[i], x[i]); }
    __device__ void four(size_t i) {
        const float4 av = *reinterpret_cast<const float4*>(a + i), xv = *reinterpret_cast<const float4*>(x + i);
        *reinterpret_cast<float4*>(o + i) = make_float4(f(av.x, xv.x), f(av.y, xv.y), f(av.z, xv.z), f(av.w, xv.w));
    }
};

bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

extern "C" int masic_budget_rd_seeds(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                                     const float* const* liks, const size_t* lik_n, int nliks, int B, double lmbda, double hw, const double* g,
                                     const double* mu, float* g1, float* g2, float* const* gl, void* stream) {
    MASIC_REQUIRE(x1_hat && x1 && x2_hat && x2 && g1 && g2 && n_pic > 0, MASIC_ERR_ARG, "budget_rd_seeds: null pointer or empty picture");
    MASIC_REQUIRE(nliks >= 0 && nliks <= 4 && (nliks == 0 || (liks && lik_n && gl)), MASIC_ERR_ARG, "budget_rd_seeds: 0..4 likelihood tensors");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "budget_rd_seeds: B = %d outside 1 .. %d", B, MAX_PAIRS);
    MASIC_REQUIRE(hw > 0.0, MASIC_ERR_ARG, "budget_rd_seeds: hw must be positive");
    BudgetSeedOp op{};
    op.a_[0] = x1_hat; op.b_[0] = x1; op.o_[0] = g1; op.a_[1] = x2_hat; op.b_[1] = x2; op.o_[1] = g2;
    op.n[0] = op.n[1] = n_pic;
    for (int k = 0; k < nliks; ++k) {
        MASIC_REQUIRE(liks[k] && gl[k] && lik_n[k] > 0, MASIC_ERR_ARG, "budget_rd_seeds: null or empty likelihood tensor");
        op.a_[2 + k] = liks[k]; op.b_[2 + k] = nullptr; op.o_[2 + k] = gl[k]; op.n[2 + k] = lik_n[k];
    }
    op.g = g; op.mu = mu;
    op.s_pic = 2.0 * lmbda * 255.0 * 255.0 / (double)n_pic;
    op.s_lik = -1.0 / (0.6931471805599453 * hw);
    launch_slices(op, 2 + nliks, B, (hipStream_t)stream);
    return masic_launch_status("budget_rd_seeds");
}

extern "C" int masic_budget_select(const float* const* cur, float* const* best, const size_t* n, int B, const double* r_now,
                                   const double* d_now, const double* target, double* r_best, double* d_best, void* stream) {
    MASIC_REQUIRE(four_ok((const void* const*)cur, n) && four_ok((const void* const*)best, n) && r_now && d_now && target && r_best && d_best,
                  MASIC_ERR_ARG, "budget_select: null pointer or empty tensor");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "budget_select: B = %d outside 1 .. %d", B, MAX_PAIRS);
    SelectOp op{};
    for (int k = 0; k < 4; ++k) { op.cur[k] = cur[k]; op.best[k] = best[k]; op.n[k] = n[k]; }
    op.r_now = r_now; op.d_now = d_now; op.target = target; op.r_best = r_best; op.d_best = d_best;
    hipStream_t st = (hipStream_t)stream;
    launch_slices(op, 4, B, st);
    hipLaunchKernelGGL(select_state_kernel, dim3((B + 255) / 256), dim3(256), 0, st, r_now, d_now, target, r_best, d_best, B);
    return masic_launch_status("budget_select");
}

extern "C" int masic_budget_mu(double* mu, const double* r_now, const double* target, int B, double gain, double mu_min, double mu_max,
                               void* stream) {
    MASIC_REQUIRE(mu && r_now && target, MASIC_ERR_ARG, "budget_mu: null pointer");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "budget_mu: B = %d outside 1 .. %d", B, MAX_PAIRS);
    MASIC_REQUIRE(positive_finite(gain) && positive_finite(mu_min) && positive_finite(mu_max) && mu_min <= mu_max, MASIC_ERR_ARG,
                  "budget_mu: gain, mu_min and mu_max must be finite and positive with mu_min <= mu_max");
    hipLaunchKernelGGL(mu_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, mu, r_now, target, B, gain, mu_min, mu_max);
    return masic_launch_status("budget_mu");
}
