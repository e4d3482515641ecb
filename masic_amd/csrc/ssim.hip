// ssim.hip -- SSIM and MS-SSIM of float32 NCHW images, forward and backward (pytorch-msssim 0.2.1 semantics).
//
// Replaces `pytorch_msssim.ms_ssim(x_hat, target, data_range=1, size_average=False)` of the reference drivers
// (coremasic/mywork/test3_real.py:102-103, newtrain_cqe_real.py:93-94) and `ssim`.  Per level:
//   mu = G(x), G = valid 11-tap separable Gaussian; sigma2 = G(x*x) - mu^2, sigma_xy = G(x*y) - mu_x*mu_y;
//   cs_map = (2 sigma_xy + C2) / (sigma_x^2 + sigma_y^2 + C2); ssim_map = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs_map;
//   the next level is avg_pool2d(., 2, padding=(H % 2, W % 2)) (count_include_pad, floor mode).
//
// Launches: forward = one ssim_fwd_level per level (tile partial sums + the pooled next level) + ssim_finish (fixed-order float64
// sums, relu / pow / product / means); backward = ssim_bwd_scalars (dL/dssim_nc, dL/dcs_nc per level and plane) + one
// ssim_bwd_level per level, coarsest first (moments recomputed, coefficient maps, transposed filter, pool adjoint of the coarser level).
// No atomics, no fills: every output element is written by exactly one thread, so results are bit-reproducible and capturable.
#include "common.h"

namespace {

constexpr int NT = 11;            // taps (the kernels are specialised for win_size 11)
constexpr int HALO = NT - 1;
constexpr int MAXL = 8;           // pyramid levels
constexpr int NTHR = 256;

// forward tile: 64 x 16 outputs of the valid domain
constexpr int FW = 64, FH = 16;
constexpr int FRW = 76;           // staged input columns (FW + HALO, rounded up to float4)
constexpr int FRH = FH + HALO;    // 26 staged input rows
// backward tile: 64 x 16 pixels of the level's input
constexpr int BW = 64, BH = 16;
constexpr int BCH = BH + HALO;    // 26 coefficient rows   (input rows iy0-10 .. iy0+15)
constexpr int BCW = 76;           // coefficient columns  (input cols ix0-10 .. ix0+65; 74 used)
constexpr int BRH = BCH + HALO;   // 36 staged input rows (iy0-10 .. iy0+25)
constexpr int BRW = 92;           // staged input columns ix0-12 .. ix0+79 (16-byte aligned origin)
constexpr int BVW = 88;           // vertical moments at staged columns 2 .. 89

struct Taps { float w[NT]; };

struct Level {
    int H, W, Ho, Wo;             // input and valid-output sizes
    int tiles_x, tiles;           // forward tiles (64 x 16 over Ho x Wo)
    long long part;               // offset of this level's partials (double2 units) in the partial slab
    long long pyr;                // offset of this level's X (and Y) planes in the pyramid (float units; level 0: unused)
};
struct Levels { Level l[MAXL]; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Stage rows [r0, r0 + nrows) x cols [c0, c0 + ncols) of one plane into LDS (row stride ncols, ncols % 4 == 0), zeros outside the image.
// vec: the plane base is 16-byte aligned, W % 4 == 0 and c0 % 4 == 0.
__device__ __forceinline__ void stage(const float* __restrict__ src, int H, int W, int r0, int c0, int nrows, int ncols, bool vec,
                                      float* __restrict__ dst) {
    const int q4 = ncols / 4, n = nrows * q4;
    for (int i = threadIdx.x; i < n; i += NTHR) {
        const int r = i / q4, q = i - r * q4;
        const int y = r0 + r, x = c0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < H) {
            const float* row = src + (size_t)y * W;
            if (vec && x >= 0 && x + 3 < W) {
                v = *reinterpret_cast<const float4*>(row + x);
            } else {
                if (x >= 0 && x < W) v.x = row[x];
                if (x + 1 >= 0 && x + 1 < W) v.y = row[x + 1];
                if (x + 2 >= 0 && x + 2 < W) v.z = row[x + 2];
                if (x + 3 >= 0 && x + 3 < W) v.w = row[x + 3];
            }
        }
        *reinterpret_cast<float4*>(dst + r * ncols + 4 * q) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward, one level
// grid (tiles, planes).  Xn / Yn (or null at the last level): the pooled next level [planes][Hn][Wn].
__global__ __launch_bounds__(NTHR) void ssim_fwd_level(const float* __restrict__ X, const float* __restrict__ Y, int H, int W, int Ho, int Wo,
                                                       int tiles_x, Taps tp, float C1, float C2, double2* __restrict__ part,
                                                       float* __restrict__ Xn, float* __restrict__ Yn, int Hn, int Wn) {
    __shared__ __attribute__((aligned(16))) float sx[FRH * FRW], sy[FRH * FRW];
    __shared__ __attribute__((aligned(16))) float hb[5][FRH * FW];      // W-filtered x, y, x*x, y*y, x*y
    __shared__ double red[2][NTHR / 64];
    const int plane = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy0 = ty * FH, ox0 = tx * FW;
    const size_t poff = (size_t)plane * H * W;
    const bool vec = (W % 4 == 0) && ((((size_t)X | (size_t)Y) & 15) == 0);
    stage(X + poff, H, W, oy0, ox0, FRH, FRW, vec, sx);
    stage(Y + poff, H, W, oy0, ox0, FRH, FRW, vec, sy);
    __syncthreads();

    // the pooled next level: pooled row i (first input row 2i - ph) belongs to the tile row whose 16 output rows hold 2i - ph
    // (tile row 0 also takes i = 0 when ph = 1; the last tile row takes the rest); the same for columns
    if (Xn) {
        const int ph = H & 1, pw = W & 1;
        const int ilo = ty == 0 ? 0 : (oy0 + ph + 1) / 2, ihi = (oy0 + FH >= Ho) ? Hn : (oy0 + FH + ph + 1) / 2;
        const int jlo = tx == 0 ? 0 : (ox0 + pw + 1) / 2, jhi = (ox0 + FW >= Wo) ? Wn : (ox0 + FW + pw + 1) / 2;
        const int nj = jhi - jlo, n = (ihi - ilo) * nj;
        const size_t noff = (size_t)plane * Hn * Wn;
        for (int k = threadIdx.x; k < n; k += NTHR) {
            const int i = ilo + k / nj, j = jlo + k % nj;
            const int r = 2 * i - ph - oy0, c = 2 * j - pw - ox0;     // staged coordinates of the window's first pixel (-1: the pad)
            float ax = 0.f, ay = 0.f;
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    const int rr = r + di, cc = c + dj;
                    if (rr >= 0 && cc >= 0) { ax += sx[rr * FRW + cc]; ay += sy[rr * FRW + cc]; }   // the pad counts as zero
                }
            Xn[noff + (size_t)i * Wn + j] = ax * 0.25f;
            Yn[noff + (size_t)i * Wn + j] = ay * 0.25f;
        }
    }

    // W pass: 26 rows x 16 quads of 4 output columns
    for (int it = threadIdx.x; it < FRH * (FW / 4); it += NTHR) {
        const int r = it / (FW / 4), q = it - r * (FW / 4);
        float vx[16], vy[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&sx[r * FRW + 4 * q + 4 * k]);
            const float4 b = *reinterpret_cast<const float4*>(&sy[r * FRW + 4 * q + 4 * k]);
            vx[4 * k] = a.x; vx[4 * k + 1] = a.y; vx[4 * k + 2] = a.z; vx[4 * k + 3] = a.w;
            vy[4 * k] = b.x; vy[4 * k + 1] = b.y; vy[4 * k + 2] = b.z; vy[4 * k + 3] = b.w;
        }
        float acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[m][k] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float w = tp.w[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = vx[k + t], b = vy[k + t];
                acc[0][k] = fmaf(w, a, acc[0][k]);
                acc[1][k] = fmaf(w, b, acc[1][k]);
                acc[2][k] = fmaf(w, a * a, acc[2][k]);
                acc[3][k] = fmaf(w, b * b, acc[3][k]);
                acc[4][k] = fmaf(w, a * b, acc[4][k]);
            }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
            *reinterpret_cast<float4*>(&hb[m][r * FW + 4 * q]) = make_float4(acc[m][0], acc[m][1], acc[m][2], acc[m][3]);
    }
    __syncthreads();

    // H pass: lane = output column, four rows per thread; then the maps and this thread's sums
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    float acc[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[m][k] = 0.f;
#pragma unroll
    for (int s = 0; s < 4 + HALO; ++s) {
        const int r = 4 * rg + s;
        float v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] = hb[m][r * FW + c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = s - k;
            if (t >= 0 && t < NT) {
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[m][k] = fmaf(tp.w[t], v[m], acc[m][k]);
            }
        }
    }
    float ssum = 0.f, csum = 0.f;
    const int ox = ox0 + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int oy = oy0 + 4 * rg + k;
        if (oy < Ho && ox < Wo) {
            const float mx = acc[0][k], my = acc[1][k];
            const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
            const float sxx = acc[2][k] - mx2, syy = acc[3][k] - my2, sxy = acc[4][k] - mxy;
            const float cs = (2.f * sxy + C2) / (sxx + syy + C2);
            const float sm = (2.f * mxy + C1) / (mx2 + my2 + C1) * cs;
            ssum += sm;
            csum += cs;
        }
    }
    const double ws = wave_sum((double)ssum), wc = wave_sum((double)csum);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ws; red[1][threadIdx.x >> 6] = wc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < NTHR / 64; ++w) { a += red[0][w]; b += red[1][w]; }
        part[(size_t)plane * gridDim.x + tile] = make_double2(a, b);
    }
}

// ---------------------------------------------------------------------------------------------------------------- finish
// One workgroup of 1024.  Per (level, plane), one wave: the tile partials summed in a fixed order in float64 -> stats[l][p] = (ssim_nc, cs_nc).
// Per plane the value pval[p] (ms: prod relu(m_i)^w_i; ssim: ssim_nc, relu'd if nonneg); then out[n] = its channel mean, or with
// size_average out[0] = the mean over every plane.
__global__ __launch_bounds__(1024) void ssim_finish(const double2* __restrict__ part, Levels lv, int L, int N, int C, Taps wt, int ms,
                                                    int size_average, int nonneg, double2* __restrict__ stats, double* __restrict__ pval,
                                                    float* __restrict__ out) {
    __shared__ double red[1024 / 64];
    const int P = N * C, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int job = wave; job < L * P; job += nw) {
        const int l = job / P, p = job - l * P;
        const int nt = lv.l[l].tiles;
        const double2* src = part + lv.l[l].part + (size_t)p * nt;
        double a = 0.0, b = 0.0;
        for (int i = lane; i < nt; i += 64) { const double2 v = src[i]; a += v.x; b += v.y; }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) {
            const double inv = 1.0 / ((double)lv.l[l].Ho * lv.l[l].Wo);
            stats[(size_t)l * P + p] = make_double2(a * inv, b * inv);
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        double v;
        if (ms) {
            v = 1.0;
            for (int l = 0; l < L; ++l) {
                const double2 s = stats[(size_t)l * P + p];
                v *= pow(fmax(l == L - 1 ? s.x : s.y, 0.0), (double)wt.w[l]);
            }
        } else {
            v = stats[p].x;
            if (nonneg) v = fmax(v, 0.0);
        }
        pval[p] = v;
    }
    __syncthreads();
    if (!size_average) {
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += pval[(size_t)n * C + c];
            out[n] = (float)(s / C);
        }
        return;
    }
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += blockDim.x) s += pval[p];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < nw; ++w) t += red[w];
        out[0] = (float)(t / P);
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// gsc[l][p] = (dL/dssim_nc, dL/dcs_nc) / (Ho_l * Wo_l): the upstream of every map pixel.  gout: [N] (size_average 0) or [1].
__global__ __launch_bounds__(NTHR) void ssim_bwd_scalars(const double2* __restrict__ stats, const float* __restrict__ gout, Levels lv, int L,
                                                         int N, int C, Taps wt, int ms, int size_average, int nonneg, float2* __restrict__ gsc) {
    const int P = N * C;
    for (int p = blockIdx.x * NTHR + threadIdx.x; p < P; p += gridDim.x * NTHR) {
        const double g = size_average ? (double)gout[0] / P : (double)gout[p / C] / C;
        if (!ms) {
            const double s = stats[p].x;
            const double gs = (nonneg && !(s > 0.0)) ? 0.0 : g;
            gsc[p] = make_float2((float)(gs / ((double)lv.l[0].Ho * lv.l[0].Wo)), 0.f);
            continue;
        }
        double raw[MAXL], t[MAXL];
        for (int l = 0; l < L; ++l) {
            const double2 s = stats[(size_t)l * P + p];
            raw[l] = l == L - 1 ? s.x : s.y;
            t[l] = pow(fmax(raw[l], 0.0), (double)wt.w[l]);
        }
        for (int l = 0; l < L; ++l) {
            // d prod / d t_l = product of the others; d t_l / d m_l = w m^(w-1); relu: zero where raw <= 0 (also through an inf of pow)
            double d = 0.0;
            if (raw[l] > 0.0 && wt.w[l] != 0.f) {
                double others = 1.0;
                for (int k = 0; k < L; ++k)
                    if (k != l) others *= t[k];
                d = g * others * (double)wt.w[l] * pow(raw[l], (double)wt.w[l] - 1.0);
            }
            const double inv = 1.0 / ((double)lv.l[l].Ho * lv.l[l].Wo);
            gsc[(size_t)l * P + p] = l == L - 1 ? make_float2((float)(d * inv), 0.f) : make_float2(0.f, (float)(d * inv));
        }
    }
}

// One level of the backward over a 64 x 16 tile of the level's input.  NM coefficient maps: DX && DY: (a_x, a_y, b, c), else (a, b, c).
//   dX = G^T(a_x) + 2 X G^T(b) + Y G^T(c),   dY = G^T(a_y) + 2 Y G^T(b) + X G^T(c),   plus 1/4 of the coarser level's gradient (pool adjoint).
// gxn / gyn (null at the coarsest level): that gradient [planes][Hn][Wn].
template <bool DX, bool DY>
__global__ __launch_bounds__(NTHR) void ssim_bwd_level(const float* __restrict__ X, const float* __restrict__ Y, int H, int W, int Ho, int Wo,
                                                       int tiles_x, Taps tp, float C1, float C2, const float2* __restrict__ gsc,
                                                       const float* __restrict__ gxn, const float* __restrict__ gyn, int Hn, int Wn,
                                                       float* __restrict__ gx, float* __restrict__ gy) {
    constexpr int NM = (DX && DY) ? 4 : 3;
    constexpr int SA = (2 * BRH * BRW > NM * BCH * BCW) ? 2 * BRH * BRW : NM * BCH * BCW;
    __shared__ __attribute__((aligned(16))) float sa[SA];            // staged x, y; then the coefficient maps
    __shared__ __attribute__((aligned(16))) float sv[5 * BCH * BVW]; // H-filtered moments; then the W-transposed maps
    float* sx = sa;
    float* sy = sa + BRH * BRW;
    const int plane = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int iy0 = ty * BH, ix0 = tx * BW;
    const size_t poff = (size_t)plane * H * W;
    const bool vec = (W % 4 == 0) && ((((size_t)X | (size_t)Y) & 15) == 0);
    stage(X + poff, H, W, iy0 - HALO, ix0 - 12, BRH, BRW, vec, sx);
    stage(Y + poff, H, W, iy0 - HALO, ix0 - 12, BRH, BRW, vec, sy);
    __syncthreads();

    // H pass of the moments: coefficient rows 0..25 (map rows iy0-10+r), staged columns 2..89, two rows per item
    for (int it = threadIdx.x; it < (BCH / 2) * BVW; it += NTHR) {
        const int r2 = it / BVW, cc = it - r2 * BVW;
        const int r = 2 * r2, col = cc + 2;
        float acc[5][2];
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[m][0] = acc[m][1] = 0.f;
#pragma unroll
        for (int s = 0; s < NT + 1; ++s) {
            const float a = sx[(r + s) * BRW + col], b = sy[(r + s) * BRW + col];
            const float aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int t = s - k;
                if (t >= 0 && t < NT) {
                    const float w = tp.w[t];
                    acc[0][k] = fmaf(w, a, acc[0][k]);
                    acc[1][k] = fmaf(w, b, acc[1][k]);
                    acc[2][k] = fmaf(w, aa, acc[2][k]);
                    acc[3][k] = fmaf(w, bb, acc[3][k]);
                    acc[4][k] = fmaf(w, ab, acc[4][k]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            sv[m * BCH * BVW + r * BVW + cc] = acc[m][0];
            sv[m * BCH * BVW + (r + 1) * BVW + cc] = acc[m][1];
        }
    }
    __syncthreads();

    // W pass of the moments -> the coefficient maps at map pixel (iy0-10+r, ix0-10+k), zero outside the valid domain
    float* cm = sa;
    const float2 g = gsc[plane];
    const float al = g.x, be = g.y;
    for (int it = threadIdx.x; it < BCH * (BCW / 4); it += NTHR) {
        const int r = it / (BCW / 4), q = it - r * (BCW / 4);
        float acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 a = *reinterpret_cast<const float4*>(&sv[m * BCH * BVW + r * BVW + 4 * q + 4 * k]);
                v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) s = fmaf(tp.w[t], v[k + t], s);
                acc[m][k] = s;
            }
        }
        const int oy = iy0 - HALO + r;
        float o[NM][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = ix0 - HALO + 4 * q + k;
            float ax = 0.f, ay = 0.f, b = 0.f, c = 0.f;
            if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo && 4 * q + k < BW + HALO) {
                const float mx = acc[0][k], my = acc[1][k];
                const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
                const float sxx = acc[2][k] - mx2, syy = acc[3][k] - my2, sxy = acc[4][k] - mxy;
                const float A1 = 2.f * mxy + C1, B1 = mx2 + my2 + C1, A2 = 2.f * sxy + C2, B2 = sxx + syy + C2;
                const float lum = A1 / B1, cs = A2 / B2;
                const float gcs = al * lum + be, gl = al * cs;
                b = -gcs * cs / B2;
                c = 2.f * gcs / B2;
                const float gb = 2.f * gl / B1;
                ax = gb * (my - lum * mx) - 2.f * b * mx - c * my;
                ay = gb * (mx - lum * my) - 2.f * b * my - c * mx;
            }
            if (DX && DY) { o[0][k] = ax; o[1][k] = ay; o[2][k] = b; o[3][k] = c; }
            else { o[0][k] = DX ? ax : ay; o[1][k] = b; o[2][k] = c; }
        }
        // (cm overlays the staged x, y: this pass reads sv only, and the last reader of x, y finished before the barrier above)
#pragma unroll
        for (int m = 0; m < NM; ++m)
            *reinterpret_cast<float4*>(&cm[m * BCH * BCW + r * BCW + 4 * q]) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
    }
    __syncthreads();

    // transposed W pass: input column j of the tile = sum_s w[10-s] map[j+s]; 26 rows x 16 quads -> sv as [NM][26][64]
    for (int it = threadIdx.x; it < BCH * (BW / 4); it += NTHR) {
        const int r = it / (BW / 4), q = it - r * (BW / 4);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 a = *reinterpret_cast<const float4*>(&cm[m * BCH * BCW + r * BCW + 4 * q + 4 * k]);
                v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
            }
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) s = fmaf(tp.w[NT - 1 - t], v[k + t], s);
                o[k] = s;
            }
            *reinterpret_cast<float4*>(&sv[m * BCH * BW + r * BW + 4 * q]) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    __syncthreads();

    // transposed H pass: lane = column, four rows per thread; then the gradient
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    float acc[NM][4];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[m][k] = 0.f;
#pragma unroll
    for (int s = 0; s < 4 + HALO; ++s) {
        const int r = 4 * rg + s;
        float v[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) v[m] = sv[m * BCH * BW + r * BW + c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = s - k;
            if (t >= 0 && t < NT) {
#pragma unroll
                for (int m = 0; m < NM; ++m) acc[m][k] = fmaf(tp.w[NT - 1 - t], v[m], acc[m][k]);
            }
        }
    }
    const int x = ix0 + c;
    if (x >= W) return;
    const int ph = H & 1, pw = W & 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = iy0 + 4 * rg + k;
        if (y >= H) break;
        const size_t i = poff + (size_t)y * W + x;
        const float xv = X[i], yv = Y[i];
        const size_t ni = gxn || gyn ? (size_t)plane * Hn * Wn + (size_t)((y + ph) >> 1) * Wn + ((x + pw) >> 1) : 0;
        if (DX) {
            const float ga = acc[0][k], gb = acc[NM - 2][k], gc = acc[NM - 1][k];
            float d = ga + 2.f * xv * gb + yv * gc;
            if (gxn) d += 0.25f * gxn[ni];
            gx[i] = d;
        }
        if (DY) {
            const float ga = acc[DX ? 1 : 0][k], gb = acc[NM - 2][k], gc = acc[NM - 1][k];
            float d = ga + 2.f * yv * gb + xv * gc;
            if (gyn) d += 0.25f * gyn[ni];
            gy[i] = d;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- host
namespace {

struct Plan {
    int L, P;
    Levels lv;
    size_t pyr_floats;                   // floats of one tensor's pyramid (levels 1 .. L-1); X's then Y's
    size_t part_off, stats_off, pval_off, fwd_bytes;
    size_t gsc_off, gpyr_off, bwd_bytes;
};

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// 0 on success; the level sizes follow avg_pool2d(2, padding=side % 2): side -> ceil(side / 2)
int make_plan(int N, int C, int H, int W, int levels, Plan* pl) {
    MASIC_REQUIRE(N > 0 && C > 0 && (long)N * C <= 65535, MASIC_ERR_SHAPE, "ssim: N * C = %ld planes (1 .. 65535)", (long)N * C);
    MASIC_REQUIRE(levels >= 1 && levels <= MAXL, MASIC_ERR_ARG, "ssim: %d levels (1 .. %d)", levels, MAXL);
    pl->L = levels;
    pl->P = N * C;
    size_t pyr = 0, part = 0;
    int h = H, w = W;
    for (int l = 0; l < levels; ++l) {
        MASIC_REQUIRE(h >= NT && w >= NT, MASIC_ERR_SHAPE, "ssim: level %d is %d x %d, smaller than the %d-tap window", l, h, w, NT);
        Level& v = pl->lv.l[l];
        v.H = h; v.W = w; v.Ho = h - HALO; v.Wo = w - HALO;
        v.tiles_x = ceil_div(v.Wo, FW);
        v.tiles = v.tiles_x * ceil_div(v.Ho, FH);
        v.part = (long long)part;
        part += (size_t)pl->P * v.tiles;
        v.pyr = (long long)pyr;
        if (l > 0) pyr += ((size_t)pl->P * h * w + 3) & ~(size_t)3;
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    pl->pyr_floats = pyr;
    pl->part_off = align16(2 * pyr * sizeof(float));
    pl->stats_off = align16(pl->part_off + part * sizeof(double2));
    pl->pval_off = align16(pl->stats_off + (size_t)levels * pl->P * sizeof(double2));
    pl->fwd_bytes = align16(pl->pval_off + (size_t)pl->P * sizeof(double));
    pl->gsc_off = 0;
    pl->gpyr_off = align16((size_t)levels * pl->P * sizeof(float2));
    pl->bwd_bytes = align16(pl->gpyr_off + 2 * pyr * sizeof(float));
    return MASIC_OK;
}

float* pyr_x(void* base, const Plan& pl, int l) { return (float*)base + pl.lv.l[l].pyr; }
float* pyr_y(void* base, const Plan& pl, int l) { return (float*)base + pl.pyr_floats + pl.lv.l[l].pyr; }

}  // namespace

extern "C" size_t masic_ssim_workspace_bytes(int N, int C, int H, int W, int levels, int backward) {
    Plan pl;
    if (make_plan(N, C, H, W, levels, &pl) != MASIC_OK) return 0;
    return backward ? pl.bwd_bytes : pl.fwd_bytes;
}

extern "C" int masic_ssim_fwd(const float* X, const float* Y, int N, int C, int H, int W, int levels, const float* taps, float C1, float C2,
                              void* ws, void* stream) {
    MASIC_REQUIRE(X && Y && taps && ws, MASIC_ERR_ARG, "ssim_fwd: null pointer");
    Plan pl;
    const int rc = make_plan(N, C, H, W, levels, &pl);
    if (rc != MASIC_OK) return rc;
    Taps tp;
    for (int t = 0; t < NT; ++t) tp.w[t] = taps[t];
    hipStream_t st = (hipStream_t)stream;
    double2* part = (double2*)((char*)ws + pl.part_off);
    for (int l = 0; l < pl.L; ++l) {
        const Level& v = pl.lv.l[l];
        const float* x = l == 0 ? X : pyr_x(ws, pl, l);
        const float* y = l == 0 ? Y : pyr_y(ws, pl, l);
        const bool pool = l + 1 < pl.L;
        float* xn = pool ? pyr_x(ws, pl, l + 1) : nullptr;
        float* yn = pool ? pyr_y(ws, pl, l + 1) : nullptr;
        const int hn = pool ? pl.lv.l[l + 1].H : 0, wn = pool ? pl.lv.l[l + 1].W : 0;
        hipLaunchKernelGGL(ssim_fwd_level, dim3(v.tiles, pl.P), dim3(NTHR), 0, st, x, y, v.H, v.W, v.Ho, v.Wo, v.tiles_x, tp, C1, C2,
                           part + v.part, xn, yn, hn, wn);
    }
    return masic_launch_status("ssim_fwd");
}

extern "C" int masic_ssim_finish(void* ws, int N, int C, int H, int W, int levels, const float* weights, int flags, float* out, void* stream) {
    MASIC_REQUIRE(ws && out, MASIC_ERR_ARG, "ssim_finish: null pointer");
    const int ms = (flags & MASIC_SSIM_MS) != 0;
    MASIC_REQUIRE(!ms || weights, MASIC_ERR_ARG, "ssim_finish: MS-SSIM needs the level weights");
    MASIC_REQUIRE(ms || levels == 1, MASIC_ERR_ARG, "ssim_finish: SSIM is one level");
    Plan pl;
    const int rc = make_plan(N, C, H, W, levels, &pl);
    if (rc != MASIC_OK) return rc;
    Taps wt = {};
    for (int l = 0; ms && l < levels; ++l) wt.w[l] = weights[l];
    hipLaunchKernelGGL(ssim_finish, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double2*)((char*)ws + pl.part_off), pl.lv, pl.L, N, C, wt,
                       ms, (flags & MASIC_SSIM_SIZE_AVERAGE) != 0, (flags & MASIC_SSIM_NONNEG) != 0,
                       (double2*)((char*)ws + pl.stats_off), (double*)((char*)ws + pl.pval_off), out);
    return masic_launch_status("ssim_finish");
}

extern "C" int masic_ssim_bwd(const float* X, const float* Y, const float* gout, int N, int C, int H, int W, int levels, const float* taps,
                              const float* weights, float C1, float C2, int flags, const void* ws, void* bws, float* dX, float* dY, void* stream) {
    MASIC_REQUIRE(X && Y && gout && taps && ws && bws, MASIC_ERR_ARG, "ssim_bwd: null pointer");
    MASIC_REQUIRE(dX || dY, MASIC_ERR_ARG, "ssim_bwd: neither dX nor dY requested");
    const int ms = (flags & MASIC_SSIM_MS) != 0;
    MASIC_REQUIRE(!ms || weights, MASIC_ERR_ARG, "ssim_bwd: MS-SSIM needs the level weights");
    MASIC_REQUIRE(ms || levels == 1, MASIC_ERR_ARG, "ssim_bwd: SSIM is one level");
    Plan pl;
    const int rc = make_plan(N, C, H, W, levels, &pl);
    if (rc != MASIC_OK) return rc;
    Taps tp, wt = {};
    for (int t = 0; t < NT; ++t) tp.w[t] = taps[t];
    for (int l = 0; ms && l < levels; ++l) wt.w[l] = weights[l];
    hipStream_t st = (hipStream_t)stream;
    float2* gsc = (float2*)((char*)bws + pl.gsc_off);
    void* gpyr = (char*)bws + pl.gpyr_off;
    hipLaunchKernelGGL(ssim_bwd_scalars, dim3(ceil_div(pl.P, NTHR)), dim3(NTHR), 0, st, (const double2*)((const char*)ws + pl.stats_off), gout,
                       pl.lv, pl.L, N, C, wt, ms, (flags & MASIC_SSIM_SIZE_AVERAGE) != 0, (flags & MASIC_SSIM_NONNEG) != 0, gsc);
    for (int l = pl.L - 1; l >= 0; --l) {
        const Level& v = pl.lv.l[l];
        const float* x = l == 0 ? X : pyr_x((void*)ws, pl, l);
        const float* y = l == 0 ? Y : pyr_y((void*)ws, pl, l);
        const bool coarser = l + 1 < pl.L;
        const float* gxn = coarser && dX ? pyr_x(gpyr, pl, l + 1) : nullptr;
        const float* gyn = coarser && dY ? pyr_y(gpyr, pl, l + 1) : nullptr;
        const int hn = coarser ? pl.lv.l[l + 1].H : 0, wn = coarser ? pl.lv.l[l + 1].W : 0;
        float* gx = dX ? (l == 0 ? dX : pyr_x(gpyr, pl, l)) : nullptr;
        float* gy = dY ? (l == 0 ? dY : pyr_y(gpyr, pl, l)) : nullptr;
        const int tiles_x = ceil_div(v.W, BW);
        const dim3 grid(tiles_x * ceil_div(v.H, BH), pl.P);
#define MASIC_SSIM_BWD(DXV, DYV) hipLaunchKernelGGL((ssim_bwd_level<DXV, DYV>), grid, dim3(NTHR), 0, st, x, y, v.H, v.W, v.Ho, v.Wo, tiles_x, tp, \
                                                    C1, C2, gsc + (size_t)l * pl.P, gxn, gyn, hn, wn, gx, gy)
        if (dX && dY) MASIC_SSIM_BWD(true, true);
        else if (dX) MASIC_SSIM_BWD(true, false);
        else MASIC_SSIM_BWD(false, true);
#undef MASIC_SSIM_BWD
    }
    return masic_launch_status("ssim_bwd");
}
