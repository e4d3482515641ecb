// align.hip -- weight-free homography estimation: coarse-to-fine photometric alignment of a grey patch pair in ONE launch
// (include/masic_align.h; restated in float64 by tests/align_ref.py).
//
// Workgroup i (512 lanes, 8 waves) handles pair i from its finite check to its eight offsets; nothing is shared between
// workgroups, so item i's bits depend on neither B nor its batch mates.  The current pyramid level of both patches is resident in
// LDS (2 * n * n floats, 128 KiB at n = 128); the coarser levels are built once by the workgroup into the caller's workspace and
// read back level by level.  Every loop has a fixed trip count; every sum has a fixed order: per lane in pixel order (float32),
// xor butterfly within the wave (float32), the 8 waves in wave order (float64).  The 8 x 8 normal equations are solved in float64
// by elimination without pivoting, one row per lane of the first wave; lane 0 applies the step and the guards.  No atomics, no fills, no host
// synchronisation.
#include <math.h>
#include "common.h"
#include "masic_align.h"

namespace {

constexpr int AL_LANES = 512;                // 8 waves: two per SIMD, so a lane may hold 256 registers (at 1024 lanes the 46 sums spill)
constexpr int AL_WAVES = AL_LANES / 64;
constexpr int AL_COARSE = 32;                 // the pyramid stops at 32 x 32
constexpr int AL_MAX_RADIUS = 15;             // (2 * 15 + 1)^2 = 961 shifts: the scan index fits the key's 10 bits
constexpr int AL_MAX_ITERS = 1000;
constexpr int AL_MAX_LDS = 2 * 128 * 128 * 4;  // dynamic LDS at P = 128
constexpr int AL_NJ = 36 + 8;                 // upper triangle of J^T J, then J^T r
constexpr int AL_SUMS = AL_NJ + 2;            // ... then the valid count and the sum of r^2

struct AlShared {
    double tot[AL_SUMS];                      // the workgroup's sums
    double hl[9];                             // the current level's matrix, h33 = 1
    double H[9];                              // the finest level's matrix
    double Hs[9];                             // the start value's matrix
    float red[AL_WAVES * AL_SUMS];            // per-wave sums
    float wcost[AL_WAVES];                    // per-wave winners of the search
    int wkey[AL_WAVES];
    int failed;                               // sticky: a guard fired
};

__device__ __forceinline__ bool al_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN
__device__ __forceinline__ bool al_finite(double v) { return fabs(v) <= 1.7976931348623157e+308; }

// out = T^-1 in T with T = [[s, 0, t], [0, s, t], [0, 0, 1]], renormalised to out[8] = 1
__device__ void al_conj(const double* in, double* out, double s, double t) {
    double m[9];
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = s * in[3 * r];
        m[3 * r + 1] = s * in[3 * r + 1];
        m[3 * r + 2] = t * (in[3 * r] + in[3 * r + 1]) + in[3 * r + 2];
    }
    for (int c = 0; c < 3; ++c) {
        out[c] = (m[c] - t * m[6 + c]) / s / m[8];
        out[3 + c] = (m[3 + c] - t * m[6 + c]) / s / m[8];
    }
    out[6] = m[6] / m[8];
    out[7] = m[7] / m[8];
    out[8] = 1.0;
}
__device__ void al_to_level(const double* H, double* hl, int level) {
    const double s = (double)(1 << level);
    al_conj(H, hl, s, (s - 1.0) * 0.5);
}
__device__ void al_from_level(const double* hl, double* H, int level) {
    const double s = (double)(1 << level);
    al_conj(hl, H, 1.0 / s, -((s - 1.0) * 0.5) / s);
}

// H with H(s_k) = s_k + d_k on the square of side P: the closed form of the square-to-quadrilateral map
__device__ void al_h_from_delta(const float* d, double P, double* H) {
    const double x0 = d[0], y0 = d[1], x1 = P + d[2], y1 = d[3], x2 = P + d[4], y2 = P + d[5], x3 = d[6], y3 = P + d[7];
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
    const double det = dx1 * dy2 - dx2 * dy1;
    const double g = (sx * dy2 - dx2 * sy) / det, h = (dx1 * sy - sx * dy1) / det;
    H[0] = (x1 - x0 + g * x1) / P; H[1] = (x3 - x0 + h * x3) / P; H[2] = x0;
    H[3] = (y1 - y0 + g * y1) / P; H[4] = (y3 - y0 + h * y3) / P; H[5] = y0;
    H[6] = g / P; H[7] = h / P; H[8] = 1.0;
}

// the four corners of the square under H, minus the square: out[8]; false if one leaves [-P/2, 3P/2] (or is not a number)
__device__ bool al_corners(const double* H, double P, double* out) {
    bool inside = true;
    for (int k = 0; k < 4; ++k) {
        const double x = (k == 1 || k == 2) ? P : 0.0, y = k >= 2 ? P : 0.0;
        const double D = H[6] * x + H[7] * y + H[8];
        const double X = (H[0] * x + H[1] * y + H[2]) / D, Y = (H[3] * x + H[4] * y + H[5]) / D;
        inside = inside && X >= -0.5 * P && X <= 1.5 * P && Y >= -0.5 * P && Y <= 1.5 * P;
        out[2 * k] = X - x;
        out[2 * k + 1] = Y - y;
    }
    return inside;
}

// One pixel of a level: the residual r = a(W(u)) - b(u) and, with JAC, its eight derivatives.  The coordinates are tested before
// anything becomes an index, and the index is clamped all the same.
template <bool JAC>
__device__ __forceinline__ bool al_pixel(const float* sa, const float* sb, int n, int i, int x, int y, const float (&h)[8], float& r,
                                         float (&J)[8]) {
    const float fx = (float)x, fy = (float)y;
    const float D = h[6] * fx + h[7] * fy + 1.0f;
    const float X = (h[0] * fx + h[1] * fy + h[2]) / D, Y = (h[3] * fx + h[4] * fy + h[5]) / D;
    const float hi = (float)(n - 1);
    if (!(X >= 0.0f && X <= hi && Y >= 0.0f && Y <= hi)) return false;
    const int x0 = min(max((int)floorf(X), 0), n - 2), y0 = min(max((int)floorf(Y), 0), n - 2);
    const float wx = X - (float)x0, wy = Y - (float)y0;
    const float* p = sa + y0 * n + x0;
    const float a00 = p[0], a10 = p[1], a01 = p[n], a11 = p[n + 1];
    const float val = (1.0f - wy) * ((1.0f - wx) * a00 + wx * a10) + wy * ((1.0f - wx) * a01 + wx * a11);
    r = val - sb[i];
    if (JAC) {
        const float gx = ((1.0f - wy) * (a10 - a00) + wy * (a11 - a01)) / D;
        const float gy = ((1.0f - wx) * (a01 - a00) + wx * (a11 - a10)) / D;
        const float q = -(gx * X + gy * Y);
        J[0] = gx * fx; J[1] = gx * fy; J[2] = gx;
        J[3] = gy * fx; J[4] = gy * fy; J[5] = gy;
        J[6] = q * fx; J[7] = q * fy;
    }
    return true;
}

// s[FIRST..AL_SUMS) of all lanes -> sh.tot[FIRST..AL_SUMS): butterfly within the wave, then the waves in wave order in float64.
// Ends with a barrier.
template <int FIRST>
__device__ __forceinline__ void al_reduce(float (&s)[AL_SUMS], AlShared& sh, int tid) {
#pragma unroll
    for (int k = FIRST; k < AL_SUMS; ++k) {
        float v = s[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        s[k] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = FIRST; k < AL_SUMS; ++k) sh.red[(tid >> 6) * AL_SUMS + k] = s[k];
    }
    __syncthreads();
    if (tid >= FIRST && tid < AL_SUMS) {
        double acc = 0.0;
        for (int w = 0; w < AL_WAVES; ++w) acc += (double)sh.red[w * AL_SUMS + tid];
        sh.tot[tid] = acc;
    }
    __syncthreads();
}

// Wave 0: (A + damping diag(A)) dp = g by Gaussian elimination without pivoting in float64, lane i (of the first eight; the others
// shadow them) holding row i of [A | g]; the pivots are those of the Cholesky factorisation.  dp is left in every lane's x; false on
// a non-positive (or NaN) pivot.  Every register index is static.
__device__ __forceinline__ bool al_solve(const AlShared& sh, double damping, int tid, double (&x)[8]) {
    const int i = tid & 7;
    double row[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int lo = min(i, k), hi = max(i, k);
        const double v = sh.tot[lo * 8 - lo * (lo - 1) / 2 + hi - lo];      // row-major upper triangle
        row[k] = k == i ? v + damping * v : v;
    }
    row[8] = sh.tot[36 + i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double pr[9];
#pragma unroll
        for (int k = j; k < 9; ++k) pr[k] = __shfl(row[k], j, 64);
        ok = ok && pr[j] > 0.0;
        const double f = i > j ? row[j] / pr[j] : 0.0;
#pragma unroll
        for (int k = j; k < 9; ++k) row[k] -= f * pr[k];
    }
#pragma unroll
    for (int j = 7; j >= 0; --j) {          // back substitution: lane j owns x[j]
        double v = row[8];
#pragma unroll
        for (int k = j + 1; k < 8; ++k) v -= row[k] * x[k];
        x[j] = __shfl(v / row[j], j, 64);
    }
    return ok;
}

// the workspace of one pair: levels 1 .. of a and b, (a_l, b_l) pairs from fine to coarse
__host__ __device__ inline size_t al_ws_floats(int P) { return P == 128 ? 2 * (64 * 64 + 32 * 32) : P == 64 ? 2 * 32 * 32 : 0; }

__global__ __launch_bounds__(AL_LANES) void align_patches_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ delta0, float* __restrict__ delta,
                                                                 float* __restrict__ info, float* __restrict__ ws, int P, int radius,
                                                                 int it0, int it1, int it2, float damping) {
    extern __shared__ float al_img[];         // a_l then b_l of the current level
    __shared__ AlShared sh;
    const int tid = threadIdx.x, pair = blockIdx.x;
    const int levels = P == 128 ? 3 : P == 64 ? 2 : 1;
    const float* ga = a + (size_t)pair * P * P;
    const float* gb = b + (size_t)pair * P * P;
    const float* gd0 = delta0 ? delta0 + (size_t)pair * 8 : nullptr;
    float* gws = ws + (size_t)pair * al_ws_floats(P);
    float* gdelta = delta + (size_t)pair * 8;
    float* ginfo = info + (size_t)pair * 4;

    // ---- a non-finite value anywhere: status 1 before anything is computed from it
    int bad = 0;
    for (int i = tid; i < P * P; i += AL_LANES) bad |= !al_finite(ga[i]) || !al_finite(gb[i]);
    if (gd0 && tid < 8) bad |= !al_finite(gd0[tid]);
    if (__syncthreads_or(bad)) {
        if (tid < 8) gdelta[tid] = gd0 ? gd0[tid] : 0.0f;
        if (tid < 4) ginfo[tid] = tid < 2 ? NAN : tid == 2 ? 0.0f : 1.0f;
        return;
    }

    // ---- the pyramid below the finest level, by 2 x 2 box means (level 2 as the mean of four level-1 means), into the workspace
    if (levels >= 2) {
        const int n1 = P / 2;
        for (int i = tid; i < n1 * n1; i += AL_LANES) {
            const int y = i / n1, x = i - y * n1;
            const float* pa = ga + (2 * y) * P + 2 * x;
            const float* pb = gb + (2 * y) * P + 2 * x;
            gws[i] = ((pa[0] + pa[1]) + (pa[P] + pa[P + 1])) * 0.25f;
            gws[n1 * n1 + i] = ((pb[0] + pb[1]) + (pb[P] + pb[P + 1])) * 0.25f;
        }
    }
    if (levels >= 3) {
        const int n2 = P / 4;
        float* w2 = gws + 2 * (P / 2) * (P / 2);
        for (int i = tid; i < n2 * n2; i += AL_LANES) {
            const int y = i / n2, x = i - y * n2;
            float m[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = (4 * y + 2 * (q >> 1)) * P + 4 * x + 2 * (q & 1);
                m[0][q] = ((ga[o] + ga[o + 1]) + (ga[o + P] + ga[o + P + 1])) * 0.25f;
                m[1][q] = ((gb[o] + gb[o + 1]) + (gb[o + P] + gb[o + P + 1])) * 0.25f;
            }
            w2[i] = ((m[0][0] + m[0][1]) + (m[0][2] + m[0][3])) * 0.25f;
            w2[n2 * n2 + i] = ((m[1][0] + m[1][1]) + (m[1][2] + m[1][3])) * 0.25f;
        }
    }
    __threadfence();                          // the workgroup reads the levels back below
    __syncthreads();

    // ---- the start value's matrix
    if (tid == 0) {
        sh.failed = 0;
        for (int k = 0; k < 9; ++k) sh.Hs[k] = (k % 4 == 0) ? 1.0 : 0.0;
        if (gd0) {
            float d0[8];
            for (int k = 0; k < 8; ++k) d0[k] = gd0[k];
            al_h_from_delta(d0, (double)P, sh.Hs);
            bool fin = true;
            for (int k = 0; k < 9; ++k) fin = fin && al_finite(sh.Hs[k]);
            if (!fin) {
                sh.failed = 1;
                for (int k = 0; k < 9; ++k) sh.Hs[k] = (k % 4 == 0) ? 1.0 : 0.0;
            }
        }
        for (int k = 0; k < 9; ++k) sh.H[k] = sh.Hs[k];
    }

#pragma unroll 1
    for (int level = levels - 1; level >= 0; --level) {
        const int n = P >> level, nn = n * n;
        const int lg = 5 + (levels - 1 - level);                   // log2(n)
        const int iters = level == 0 ? it2 : level == 1 ? it1 : it0;
        float* sa = al_img;
        float* sb = al_img + nn;
        // ---- this level of both patches into LDS
        {
            const float* la = ga;
            const float* lb = gb;
            if (level == 1) { la = gws; lb = gws + nn; }
            if (level == 2) { la = gws + 2 * (P / 2) * (P / 2); lb = la + nn; }
            __syncthreads();                  // the level before is no longer read
            for (int i = tid; i < nn; i += AL_LANES) {
                sa[i] = la[i];
                sb[i] = lb[i];
            }
            __syncthreads();
        }

        // ---- stage 1 on the coarsest level: shift k on lane k mod 512, the least cost by a total order (cost, |dx| + |dy|, scan index)
        if (level == levels - 1 && !gd0) {
            const int side = 2 * radius + 1, ncost = side * side;
            float cost = INFINITY;
            int key = (1 << 20) + tid;        // (|dx| + |dy|) << 10 | scan index; a lane without a shift loses every comparison
            for (int k = tid; k < ncost; k += AL_LANES) {
                const int dy = k / side - radius, dx = k - (k / side) * side - radius;
                float acc = 0.0f;
                for (int y = 0; y < AL_COARSE; ++y) {
                    const int yy = y + dy;
                    const bool yin = yy >= 0 && yy < AL_COARSE;
                    for (int x = 0; x < AL_COARSE; ++x) {
                        const int xx = x + dx;
                        const bool in = yin && xx >= 0 && xx < AL_COARSE;
                        const float d = sa[in ? yy * AL_COARSE + xx : 0] - sb[y * AL_COARSE + x];
                        acc += in ? d * d : 0.0f;
                    }
                }
                const int cnt = (AL_COARSE - abs(dx)) * (AL_COARSE - abs(dy));
                const float c = (4 * cnt >= AL_COARSE * AL_COARSE && al_finite(acc)) ? acc / (float)cnt : INFINITY;
                const int ck = ((abs(dx) + abs(dy)) << 10) | k;
                if (c < cost || (c == cost && ck < key)) { cost = c; key = ck; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float oc = __shfl_xor(cost, off, 64);
                const int ok = __shfl_xor(key, off, 64);
                if (oc < cost || (oc == cost && ok < key)) { cost = oc; key = ok; }
            }
            if ((tid & 63) == 0) { sh.wcost[tid >> 6] = cost; sh.wkey[tid >> 6] = key; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < AL_WAVES; ++w)
                    if (sh.wcost[w] < cost || (sh.wcost[w] == cost && sh.wkey[w] < key)) { cost = sh.wcost[w]; key = sh.wkey[w]; }
                const int k = key & 1023;
                const double scale = (double)(1 << (levels - 1));
                sh.H[2] = (double)(k - (k / side) * side - radius) * scale;
                sh.H[5] = (double)(k / side - radius) * scale;
            }
        }
        if (tid == 0) al_to_level(sh.H, sh.hl, level);
        __syncthreads();

        // ---- stage 2: forward-additive Gauss-Newton steps on this level
#pragma unroll 1
        for (int it = 0; it < iters; ++it) {
            float h[8], s[AL_SUMS];
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = (float)sh.hl[k];
#pragma unroll
            for (int k = 0; k < AL_SUMS; ++k) s[k] = 0.0f;
            for (int i = tid; i < nn; i += AL_LANES) {
                float r, J[8];
                if (al_pixel<true>(sa, sb, n, i, i & (n - 1), i >> lg, h, r, J)) {
                    int q = 0;
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int v = u; v < 8; ++v) s[q++] += J[u] * J[v];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s[36 + u] += J[u] * r;
                    s[AL_NJ] += 1.0f;
                    s[AL_NJ + 1] += r * r;
                }
            }
            al_reduce<0>(s, sh, tid);
            if (tid < 64) {
                double cand[9], Hf[9], c[8];
                bool ok = al_solve(sh, (double)damping, tid, c) && sh.tot[AL_NJ] >= 0.25 * (double)nn;
                if (tid == 0 && !sh.failed) {
                    for (int k = 0; k < 8; ++k) cand[k] = sh.hl[k] - c[k];
                    cand[8] = 1.0;
                    al_from_level(cand, Hf, level);
                    ok = al_corners(Hf, (double)P, c) && ok;          // (a NaN step fails here)
                    if (ok) {
                        for (int k = 0; k < 8; ++k) sh.hl[k] = cand[k];
                    } else {
                        sh.failed = 1;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) al_from_level(sh.hl, sh.H, level);
        __syncthreads();
    }

    // ---- the masked MSE at the start value and at the result, on the finest level (resident since the last level)
    float mse[2], frac[2];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const double* Hp = pass == 0 ? sh.Hs : sh.H;
        float h[8], s[AL_SUMS], J[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = (float)Hp[k];
        s[AL_NJ] = s[AL_NJ + 1] = 0.0f;
        for (int i = tid; i < P * P; i += AL_LANES) {
            float r;
            if (al_pixel<false>(al_img, al_img + P * P, P, i, i & (P - 1), i / P, h, r, J)) {
                s[AL_NJ] += 1.0f;
                s[AL_NJ + 1] += r * r;
            }
        }
        al_reduce<AL_NJ>(s, sh, tid);
        if (tid == 0) {
            mse[pass] = sh.tot[AL_NJ] > 0.0 ? (float)(sh.tot[AL_NJ + 1] / sh.tot[AL_NJ]) : INFINITY;
            frac[pass] = (float)(sh.tot[AL_NJ] / (double)(P * P));
        }
        __syncthreads();                      // tot is rewritten by the next pass
    }
    if (tid == 0) {
        double c[8];
        al_corners(sh.H, (double)P, c);                           // the offsets; the range was checked at every step
        bool ok = true;
        for (int k = 0; k < 8; ++k) ok = ok && al_finite(c[k]);
        const int status = (sh.failed || !ok || !(frac[1] >= 0.25f)) ? 1 : (mse[1] > mse[0] ? 2 : 0);
        for (int k = 0; k < 8; ++k) gdelta[k] = status == 0 ? (float)c[k] : (gd0 ? gd0[k] : 0.0f);
        ginfo[0] = status == 1 ? NAN : mse[0];                    // with status 2 the result IS the start value
        ginfo[1] = status == 1 ? NAN : mse[status == 2 ? 0 : 1];
        ginfo[2] = status == 1 ? 0.0f : frac[status == 2 ? 0 : 1];
        ginfo[3] = (float)status;
    }
}

bool al_supported(int B, int P) { return B >= 1 && B <= 65535 && (P == 32 || P == 64 || P == 128); }

}  // namespace

extern "C" size_t masic_align_workspace_bytes(int B, int P) {
    return al_supported(B, P) ? (size_t)B * al_ws_floats(P) * sizeof(float) : 0;
}

extern "C" int masic_align_patches(const float* a, const float* b, const float* delta0, float* delta, float* info, void* workspace,
                                   int B, int P, int search_radius, int it0, int it1, int it2, float damping, void* stream) {
    MASIC_REQUIRE(al_supported(B, P), MASIC_ERR_UNSUPPORTED, "align_patches: B = %d, P = %d (1 <= B <= 65535, P in {32, 64, 128})", B, P);
    MASIC_REQUIRE(a && b && delta && info, MASIC_ERR_ARG, "align_patches: null pointer");
    MASIC_REQUIRE(workspace || al_ws_floats(P) == 0, MASIC_ERR_ARG, "align_patches: P = %d needs a workspace of %zu bytes", P,
                  masic_align_workspace_bytes(B, P));
    MASIC_REQUIRE(search_radius >= 0 && search_radius <= AL_MAX_RADIUS, MASIC_ERR_ARG, "align_patches: search_radius %d not in [0, %d]",
                  search_radius, AL_MAX_RADIUS);
    MASIC_REQUIRE(it0 >= 0 && it1 >= 0 && it2 >= 0 && it0 <= AL_MAX_ITERS && it1 <= AL_MAX_ITERS && it2 <= AL_MAX_ITERS, MASIC_ERR_ARG,
                  "align_patches: iteration counts (%d, %d, %d) not in [0, %d]", it0, it1, it2, AL_MAX_ITERS);
    MASIC_REQUIRE(damping >= 0.0f && damping <= 3.402823466e+38f, MASIC_ERR_ARG, "align_patches: damping must be finite and >= 0");
    // the opt-in to more than 64 KiB of dynamic LDS, once: the finest level's 128 KiB beside the kernel's static 2.4 KiB (launch_lds
    // asks for all 160 KiB as dynamic, which a kernel with static LDS cannot have)
    static bool attr_set = false;
    if (!attr_set) {
        MASIC_REQUIRE(hipFuncSetAttribute((const void*)align_patches_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AL_MAX_LDS) == hipSuccess,
                      MASIC_ERR_LAUNCH, "align_patches: cannot reserve %d bytes of LDS", AL_MAX_LDS);
        attr_set = true;
    }
    hipLaunchKernelGGL(align_patches_kernel, dim3(B), dim3(AL_LANES), (size_t)2 * P * P * sizeof(float), (hipStream_t)stream, a, b, delta0,
                       delta, info, (float*)workspace, P, search_radius, it0, it1, it2, damping);
    return masic_launch_status("align_patches");
}
