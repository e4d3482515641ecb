// refine.hip -- the elementwise kernels of the encoder-side latent refinement (include/masic_refine.h; masic_amd/refine.py; DESIGN.md
// section 8.10): the noise of a step, the Adam step, keep-the-best-iterate and the seeds of the per-pair objective's backward.
//
// One shape for all of them (refine_slices.h): block (x, t, b) of a bounded grid walks pair b's slice of tensor t in 16-byte pieces with
// single floats at its head and tail.  No atomics, no grid-wide synchronisation, nothing read by the host.
#include "common.h"
#include "masic_refine.h"
#include "refine_slices.h"

namespace {

// ---- noise: Philox4x32-10 (Salmon et al. 2011), word 0 of the block
__device__ __forceinline__ unsigned philox_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

struct NoiseOp {
    float* out[NT]; size_t n[NT];
    const uint32_t* keys; const int32_t* step; uint32_t seed;
    float* p; unsigned key, tid, stp;                       // per block
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        p = out[t] + (size_t)b * nn;
        key = keys[b]; tid = (unsigned)t; stp = (unsigned)*step;
        const uintptr_t a[1] = {(uintptr_t)p};
        s = span_of(nn, a);
        return true;
    }
    __device__ float value(size_t i) const {
        const unsigned w = philox_word0((unsigned)(i & 0xffffffffull), tid, stp, (unsigned)(i >> 32), seed, key);
        return __fsub_rn(__fmul_rn((float)(w >> 8), 5.9604644775390625e-8f), 0.5f);
    }
    __device__ void one(size_t i) { p[i] = value(i); }
    __device__ void four(size_t i) { *reinterpret_cast<float4*>(p + i) = make_float4(value(i), value(i + 1), value(i + 2), value(i + 3)); }
};

// ---- Adam
struct AdamOp {
    float* p_[NT]; const float* g_[NT]; float* m_[NT]; float* v_[NT]; size_t n[NT];
    const int32_t* step; float lr;
    float* p; const float* g; float* m; float* v; float c1, c2;      // per block: 1 / (1 - beta^t)
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        const size_t o = (size_t)b * nn;
        p = p_[t] + o; g = g_[t] + o; m = m_[t] + o; v = v_[t] + o;
        const double tt = (double)*step;
        c1 = (float)(1.0 / (1.0 - pow(0.9, tt)));
        c2 = (float)(1.0 / (1.0 - pow(0.999, tt)));
        const uintptr_t a[4] = {(uintptr_t)p, (uintptr_t)g, (uintptr_t)m, (uintptr_t)v};
        s = span_of(nn, a);
        return true;
    }
    __device__ void upd(float& pp, float gg, float& mm, float& vv) const {
        mm = 0.9f * mm + 0.1f * gg;
        vv = 0.999f * vv + 0.001f * (gg * gg);
        pp = pp - lr * (mm * c1) / (sqrtf(vv * c2) + 1e-8f);
    }
    __device__ void one(size_t i) {
        float pp = p[i], mm = m[i], vv = v[i];
        upd(pp, g[i], mm, vv);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
    __device__ void four(size_t i) {
        float4 pp = *reinterpret_cast<float4*>(p + i), mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        upd(pp.x, gg.x, mm.x, vv.x); upd(pp.y, gg.y, mm.y, vv.y); upd(pp.z, gg.z, mm.z, vv.z); upd(pp.w, gg.w, mm.w, vv.w);
        *reinterpret_cast<float4*>(p + i) = pp; *reinterpret_cast<float4*>(m + i) = mm; *reinterpret_cast<float4*>(v + i) = vv;
    }
};

// ---- keep best
struct KeepOp {
    const float* cur[NT]; float* best[NT]; size_t n[NT];
    const double* j_now; const double* j_best;
    const float* c; float* d;
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        if (!(j_now[b] < j_best[b])) return false;
        c = cur[t] + (size_t)b * nn; d = best[t] + (size_t)b * nn;
        const uintptr_t a[2] = {(uintptr_t)c, (uintptr_t)d};
        s = span_of(nn, a);
        return true;
    }
    __device__ void one(size_t i) { d[i] = c[i]; }
    __device__ void four(size_t i) { *reinterpret_cast<float4*>(d + i) = *reinterpret_cast<const float4*>(c + i); }
};

__global__ __launch_bounds__(256) void keep_cost_kernel(const double* __restrict__ j_now, double* __restrict__ j_best, int B) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256)
        if (j_now[b] < j_best[b]) j_best[b] = j_now[b];
}

// ---- seeds of the per-pair objective: tensors 0, 1 the pictures, 2.. the likelihoods
struct SeedOp {
    const float* a_[NT]; const float* b_[NT]; float* o_[NT]; size_t n[NT];
    const double* g; double s_pic, s_lik;
    const float* a; const float* x; float* o; float sc; bool lik;
    __device__ bool begin(int t, int b, size_t nn, Span& s) {
        const size_t off = (size_t)b * nn;
        lik = t >= 2;
        a = a_[t] + off; x = lik ? a : b_[t] + off; o = o_[t] + off;
        sc = (float)((g ? g[b] : 1.0) * (lik ? s_lik : s_pic));
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

}  // namespace

extern "C" int masic_refine_noise(float* const* out, const size_t* n, int B, uint32_t seed, const uint32_t* pair_keys, const int32_t* step,
                                  void* stream) {
    MASIC_REQUIRE(four_ok((const void* const*)out, n) && pair_keys && step, MASIC_ERR_ARG, "refine_noise: null pointer or empty tensor");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "refine_noise: B = %d outside 1 .. %d", B, MAX_PAIRS);
    NoiseOp op{};
    for (int k = 0; k < 4; ++k) { op.out[k] = out[k]; op.n[k] = n[k]; }
    op.keys = pair_keys; op.step = step; op.seed = seed;
    launch_slices(op, 4, B, (hipStream_t)stream);
    return masic_launch_status("refine_noise");
}

extern "C" int masic_refine_adam(float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n, int B, double lr,
                                 const int32_t* step, void* stream) {
    MASIC_REQUIRE(four_ok((const void* const*)p, n) && four_ok((const void* const*)g, n) && four_ok((const void* const*)m, n) &&
                  four_ok((const void* const*)v, n) && step, MASIC_ERR_ARG, "refine_adam: null pointer or empty tensor");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "refine_adam: B = %d outside 1 .. %d", B, MAX_PAIRS);
    AdamOp op{};
    for (int k = 0; k < 4; ++k) { op.p_[k] = p[k]; op.g_[k] = g[k]; op.m_[k] = m[k]; op.v_[k] = v[k]; op.n[k] = n[k]; }
    op.step = step; op.lr = (float)lr;
    launch_slices(op, 4, B, (hipStream_t)stream);
    return masic_launch_status("refine_adam");
}

extern "C" int masic_refine_keep_best(const float* const* cur, float* const* best, const size_t* n, int B, const double* j_now, double* j_best,
                                      void* stream) {
    MASIC_REQUIRE(four_ok((const void* const*)cur, n) && four_ok((const void* const*)best, n) && j_now && j_best, MASIC_ERR_ARG,
                  "refine_keep_best: null pointer or empty tensor");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "refine_keep_best: B = %d outside 1 .. %d", B, MAX_PAIRS);
    KeepOp op{};
    for (int k = 0; k < 4; ++k) { op.cur[k] = cur[k]; op.best[k] = best[k]; op.n[k] = n[k]; }
    op.j_now = j_now; op.j_best = j_best;
    hipStream_t st = (hipStream_t)stream;
    launch_slices(op, 4, B, st);
    hipLaunchKernelGGL(keep_cost_kernel, dim3((B + 255) / 256), dim3(256), 0, st, j_now, j_best, B);
    return masic_launch_status("refine_keep_best");
}

extern "C" int masic_refine_rd_seeds(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                                     const float* const* liks, const size_t* lik_n, int nliks, int B, double lmbda, double hw, const double* g,
                                     float* g1, float* g2, float* const* gl, void* stream) {
    MASIC_REQUIRE(x1_hat && x1 && x2_hat && x2 && g1 && g2 && n_pic > 0, MASIC_ERR_ARG, "refine_rd_seeds: null pointer or empty picture");
    MASIC_REQUIRE(nliks >= 0 && nliks <= 4 && (nliks == 0 || (liks && lik_n && gl)), MASIC_ERR_ARG, "refine_rd_seeds: 0..4 likelihood tensors");
    MASIC_REQUIRE(B >= 1 && B <= MAX_PAIRS, MASIC_ERR_ARG, "refine_rd_seeds: B = %d outside 1 .. %d", B, MAX_PAIRS);
    MASIC_REQUIRE(hw > 0.0, MASIC_ERR_ARG, "refine_rd_seeds: hw must be positive");
    SeedOp op{};
    op.a_[0] = x1_hat; op.b_[0] = x1; op.o_[0] = g1; op.a_[1] = x2_hat; op.b_[1] = x2; op.o_[1] = g2;
    op.n[0] = op.n[1] = n_pic;
    for (int k = 0; k < nliks; ++k) {
        MASIC_REQUIRE(liks[k] && gl[k] && lik_n[k] > 0, MASIC_ERR_ARG, "refine_rd_seeds: null or empty likelihood tensor");
        op.a_[2 + k] = liks[k]; op.b_[2 + k] = nullptr; op.o_[2 + k] = gl[k]; op.n[2 + k] = lik_n[k];
    }
    op.g = g;
    op.s_pic = 2.0 * lmbda * 255.0 * 255.0 / (double)n_pic;
    op.s_lik = -1.0 / (0.6931471805599453 * hw);
    launch_slices(op, 2 + nliks, B, (hipStream_t)stream);
    return masic_launch_status("refine_rd_seeds");
}
