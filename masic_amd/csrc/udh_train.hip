// udh_train.hip -- the kernels that training the UDH homography net (udh/udh/train.py: Net + photometric_loss) needs beyond the
// inference schedule of udh.hip and the convolution backward of the codec path.  Float32 throughout (the per-pair 3 x 3 / 8 x 8
// algebra is float64 inside one thread), no float atomics anywhere: every sum has a fixed order -- a shuffle tree inside a wave, waves
// and workgroups in index order, partials plus a finishing pass across workgroups.
//
//   maxpool2_relu_bwd     g_y of MaxPool2d(2, 2) routed to the element max_pool2d's backward picks (first maximum in window scan
//                         order, NaN wins), times [x > 0] for the ReLU in front; one pass, one lane per window.
//   udh_conv1_wgrad       dW [Cout][2][3][3] and db of the first layer from the two patch tensors and dy: per-workgroup partials
//                         (4 output channels x 1024 pixels), a finishing kernel adds them in index order.
//   udh_fc_train_fwd      the two linear layers with the Dropout masks: x' = 2 m1 x, hidden = relu(x' W1^T + b1) through the
//                         inference kernels unchanged (masic_udh_fc_fwd), out = (2 m2 hidden) W2^T + b2.  The inference entry point
//                         also writes its own, unmasked `out`; the masked kernel overwrites it (B x 1024 x 8 of repeated work).
//   udh_fc_bwd            the linear backward.  A small kernel makes gW2, gb2, gb1 and g_h = (g_out W2) 2 m2 [hidden > 0] (stored
//                         transposed, [N][Bp], so that a wave reads the <= 32 values of a neuron with scalar loads); then ONE streaming
//                         pass over W1: a workgroup owns 256 columns of K for all N rows, keeps its columns of x' in registers, reads
//                         each W1 row piece once (16 bytes per lane), writes gW1's row piece once and accumulates gx in registers.
//                         gx needs no sum across workgroups, only across the four waves of one (through LDS, wave order).
//   udh_photo_matrix      S = inverse(N_dst inverse(h) N_src^-1), h = get_perspective_transform(corners - corners[:, :1],
//                         corners + delta): one lane per pair, float64; NaN where the system is exactly singular.
//                         udh_photo_matrix_bwd is its adjoint g_S -> g_delta.
//   udh_photo_loss        mean |warp_perspective(img_a, inverse(h), (h, w)) - patch_b| with warp.hip's coordinate arithmetic, and its
//                         backward to g_S (nine partial sums per workgroup, finished per pair in workgroup order).
#include "common.h"
#include "homography_math.h"

namespace {

// ------------------------------------------------------------------------------------------------ max-pool + ReLU backward
__global__ __launch_bounds__(256) void maxpool2_relu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx,
                                                                int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / Wo;                         // plane * Ho + r
    const int c = (int)(i - row * Wo);
    const size_t base = row * 2 * (size_t)(2 * Wo);
    const float2* p = reinterpret_cast<const float2*>(x + base) + c;
    const float2 t = p[0], u = p[Wo];
    const float raw[4] = {t.x, t.y, u.x, u.y};
    // the pooled tensor is relu(x): a NaN stays a NaN, anything else below zero is zero
    float m = raw[0] != raw[0] ? raw[0] : fmaxf(raw[0], 0.0f);
    int arg = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float v = raw[k] != raw[k] ? raw[k] : fmaxf(raw[k], 0.0f);
        if (v > m || v != v) { m = v; arg = k; }
    }
    const float g = gy[i];
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (k == arg && raw[k] > 0.0f) ? g : 0.0f;
    float2* q = reinterpret_cast<float2*>(gx + base) + c;
    q[0] = make_float2(o[0], o[1]);
    q[Wo] = make_float2(o[2], o[3]);
}

// ------------------------------------------------------------------------------------------------ first-layer weight gradient
constexpr int W1G_CO = 4;              // output channels per workgroup
constexpr int W1G_PIX = 1024;          // pixels per workgroup (4 per lane)
constexpr int W1G_V = 19;              // 18 taps + the bias

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void udh_conv1_wgrad_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ dy,
                                                                      float* __restrict__ part, int H, int W, int Cout) {
    __shared__ float red[4][W1G_CO * W1G_V];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int co0 = blockIdx.y * W1G_CO, img = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float* src[2] = {a + (size_t)img * plane, b + (size_t)img * plane};
    float acc[W1G_CO][W1G_V];
#pragma unroll
    for (int o = 0; o < W1G_CO; ++o)
#pragma unroll
        for (int t = 0; t < W1G_V; ++t) acc[o][t] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < W1G_PIX / 256; ++j) {
        const int pix = blockIdx.x * W1G_PIX + j * 256 + tid;
        if (pix >= H * W) continue;
        const int r = pix / W, c = pix - r * W;
        float v[W1G_V];
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int ih = r + kh - 1, iw = c + kw - 1;
                    const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
                    v[ci * 9 + kh * 3 + kw] = ok ? src[ci][(size_t)ih * W + iw] : 0.0f;
                }
        v[18] = 1.0f;
#pragma unroll
        for (int o = 0; o < W1G_CO; ++o) {
            const float g = dy[((size_t)img * Cout + co0 + o) * plane + pix];
#pragma unroll
            for (int t = 0; t < W1G_V; ++t) acc[o][t] = fmaf(g, v[t], acc[o][t]);
        }
    }
#pragma unroll
    for (int o = 0; o < W1G_CO; ++o)
#pragma unroll
        for (int t = 0; t < W1G_V; ++t) {
            const float s = wave_sum(acc[o][t]);
            if (lane == 0) red[wave][o * W1G_V + t] = s;
        }
    __syncthreads();
    if (tid < W1G_CO * W1G_V) {
        const float s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const size_t slot = (size_t)img * gridDim.x + blockIdx.x;
        part[(slot * Cout + co0) * W1G_V + tid] = s;
    }
}

__global__ __launch_bounds__(256) void udh_conv1_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                                     int slots, int Cout) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Cout * W1G_V) return;
    float s = 0.0f;
    for (int k = 0; k < slots; ++k) s += part[(size_t)k * Cout * W1G_V + i];
    const int co = i / W1G_V, t = i - co * W1G_V;
    if (t < 18) dw[co * 18 + t] = s; else db[co] = s;
}

// ------------------------------------------------------------------------------------------------ linear layers, training forward
__global__ __launch_bounds__(256) void udh_dropout_kernel(const float* __restrict__ x, const unsigned char* __restrict__ m, float* __restrict__ y, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const uchar4 k = reinterpret_cast<const uchar4*>(m)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(k.x ? 2.0f * v.x : 0.0f, k.y ? 2.0f * v.y : 0.0f, k.z ? 2.0f * v.z : 0.0f, k.w ? 2.0f * v.w : 0.0f);
}

// out[b][j] = sum_n (2 m2 hidden)[b][n] * w2[j][n] + b2[j]: the summation of udh_fc_finish_kernel on the dropped row
__global__ __launch_bounds__(512) void udh_fc2_masked_kernel(const float* __restrict__ hidden, const unsigned char* __restrict__ m2, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ out, int N, int M) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < M; j += 8) {
        float acc = 0.0f;
        for (int n = lane; n < N; n += 64) {
            const float h = m2[(size_t)b * N + n] ? 2.0f * hidden[(size_t)b * N + n] : 0.0f;
            acc = fmaf(h, w2[(size_t)j * N + n], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) out[(size_t)b * M + j] = acc + b2[j];
    }
}

// ------------------------------------------------------------------------------------------------ linear layers, backward
constexpr int FB_KCH = 256;            // columns of K per workgroup: one 16-byte piece per lane and row
constexpr int FB_NT = 4;               // W1 rows a wave has in flight
constexpr int FB_ROWS = 8;             // batch rows per row group
constexpr int FB_MAXG = 4;             // row groups per launch (the gx accumulators and x' live in registers)

// one lane per neuron n: g_h[b][n] = (sum_j g_out[b][j] w2[j][n]) * 2 m2[b][n] * [hidden[b][n] > 0] -> ghT[n][Bp] (zeros past B),
// gb1[n] = sum_b g_h, gW2[j][n] = sum_b g_out[b][j] * (2 m2 hidden)[b][n]; the first M lanes of workgroup 0 also make gb2.  b ascending.
__global__ __launch_bounds__(256) void udh_fc_bwd_head_kernel(const float* __restrict__ gout, const float* __restrict__ hidden, const unsigned char* __restrict__ m2,
                                                              const float* __restrict__ w2, float* __restrict__ ghT, float* __restrict__ gb1,
                                                              float* __restrict__ gw2, float* __restrict__ gb2, int B, int Bp, int N, int M) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) {
        float s1 = 0.0f;
        for (int b = 0; b < B; ++b) {
            float acc = 0.0f;
            for (int j = 0; j < M; ++j) acc = fmaf(gout[b * M + j], w2[(size_t)j * N + n], acc);
            const float h = hidden[(size_t)b * N + n];
            const float keep = m2 == nullptr ? 1.0f : (m2[(size_t)b * N + n] ? 2.0f : 0.0f);
            const float g = h > 0.0f ? acc * keep : 0.0f;
            ghT[(size_t)n * Bp + b] = g;
            s1 += g;
        }
        for (int b = B; b < Bp; ++b) ghT[(size_t)n * Bp + b] = 0.0f;
        gb1[n] = s1;
        for (int j = 0; j < M; ++j) {
            float s = 0.0f;
            for (int b = 0; b < B; ++b) {
                const float keep = m2 == nullptr ? 1.0f : (m2[(size_t)b * N + n] ? 2.0f : 0.0f);
                s = fmaf(gout[b * M + j], hidden[(size_t)b * N + n] * keep, s);
            }
            gw2[(size_t)j * N + n] = s;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < M) {
        float s = 0.0f;
        for (int b = 0; b < B; ++b) s += gout[b * M + threadIdx.x];
        gb2[threadIdx.x] = s;
    }
}

// The streaming pass.  Rows [b0, b0 + 8 NG) of the batch; ACC: gW1 already holds the sum over the rows before b0 and is added to.
template <int NG, bool ACC>
__global__ __launch_bounds__(256) void udh_fc1_bwd_kernel(const float* __restrict__ xd, const float* __restrict__ ghT, const unsigned char* __restrict__ m1,
                                                          const float* __restrict__ w, float* __restrict__ gw, float* __restrict__ gx,
                                                          int B, int Bp, int b0, int K, int N) {
    __shared__ float4 red[4][FB_ROWS][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t k0 = (size_t)blockIdx.x * FB_KCH + lane * 4;
    constexpr int R = NG * FB_ROWS;
    float4 xv[R], ga[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        xv[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        ga[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b0 + r < B) xv[r] = *reinterpret_cast<const float4*>(xd + (size_t)(b0 + r) * K + k0);
    }
    const int tiles = N / (4 * FB_NT);                  // per wave
    float4 wv[FB_NT], wn[FB_NT];
    {
        const int n0 = wave * FB_NT;
#pragma unroll
        for (int t = 0; t < FB_NT; ++t) wn[t] = *reinterpret_cast<const float4*>(w + (size_t)(n0 + t) * K + k0);
    }
#pragma unroll 1
    for (int it = 0; it < tiles; ++it) {
        const int n0 = (it * 4 + wave) * FB_NT;
#pragma unroll
        for (int t = 0; t < FB_NT; ++t) wv[t] = wn[t];
        if (it + 1 < tiles) {
            const int n1 = ((it + 1) * 4 + wave) * FB_NT;
#pragma unroll
            for (int t = 0; t < FB_NT; ++t) wn[t] = *reinterpret_cast<const float4*>(w + (size_t)(n1 + t) * K + k0);
        }
#pragma unroll
        for (int t = 0; t < FB_NT; ++t) {
            const float* gh = ghT + (size_t)(n0 + t) * Bp + b0;        // wave-uniform: scalar loads
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float* gp = gw + (size_t)(n0 + t) * K + k0;
            if (ACC) s = *reinterpret_cast<const float4*>(gp);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float g = gh[r];
                s.x = fmaf(g, xv[r].x, s.x); s.y = fmaf(g, xv[r].y, s.y); s.z = fmaf(g, xv[r].z, s.z); s.w = fmaf(g, xv[r].w, s.w);
                ga[r].x = fmaf(g, wv[t].x, ga[r].x); ga[r].y = fmaf(g, wv[t].y, ga[r].y);
                ga[r].z = fmaf(g, wv[t].z, ga[r].z); ga[r].w = fmaf(g, wv[t].w, ga[r].w);
            }
            *reinterpret_cast<float4*>(gp) = s;
        }
    }
    // gx: the four waves' sums over their neurons, added in wave order; wave w finishes rows 2w, 2w + 1 of each row group
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < FB_ROWS; ++r) red[wave][r][lane] = ga[g * FB_ROWS + r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = wave * 2 + q, b = b0 + g * FB_ROWS + r;
            if (b < B) {
                const float4 p0 = red[0][r][lane], p1 = red[1][r][lane], p2 = red[2][r][lane], p3 = red[3][r][lane];
                float4 s = make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z,
                                       ((p0.w + p1.w) + p2.w) + p3.w);
                if (m1 != nullptr) {
                    const uchar4 k = *reinterpret_cast<const uchar4*>(m1 + (size_t)b * K + k0);
                    s = make_float4(k.x ? 2.0f * s.x : 0.0f, k.y ? 2.0f * s.y : 0.0f, k.z ? 2.0f * s.z : 0.0f, k.w ? 2.0f * s.w : 0.0f);
                }
                *reinterpret_cast<float4*>(gx + (size_t)b * K + k0) = s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ photometric loss: the matrix
// (solve8, inv3, mul3, mul3_tn, mul3_nt: homography_math.h)
struct PhotoChain {
    double px[4], py[4];       // corners - corners[0] (float32 subtraction, as the reference forms it)
    double h[9], m[9], s[9];   // h, inverse(h), S
    double nd[9], nsi[9];      // N_dst, N_src^-1
};

// the 8 x 8 system of get_perspective_transform: [x y 1 0 0 0 -xu -yu] h = u, [0 0 0 x y 1 -xv -yv] h = v
__device__ void dlt_rows(const PhotoChain& c, const double* qx, const double* qy, double (&A)[8][9]) {
    for (int k = 0; k < 4; ++k) {
        double* rx = A[2 * k];
        double* ry = A[2 * k + 1];
        rx[0] = c.px[k]; rx[1] = c.py[k]; rx[2] = 1; rx[3] = 0; rx[4] = 0; rx[5] = 0; rx[6] = -c.px[k] * qx[k]; rx[7] = -c.py[k] * qx[k]; rx[8] = qx[k];
        ry[0] = 0; ry[1] = 0; ry[2] = 0; ry[3] = c.px[k]; ry[4] = c.py[k]; ry[5] = 1; ry[6] = -c.px[k] * qy[k]; ry[7] = -c.py[k] * qy[k]; ry[8] = qy[k];
    }
}

__device__ bool photo_chain(const float* corners, const float* delta, int Hs, int Ws, int Hd, int Wd, PhotoChain& c, double* qx, double* qy) {
    for (int k = 0; k < 4; ++k) {
        c.px[k] = (double)(corners[2 * k] - corners[0]);
        c.py[k] = (double)(corners[2 * k + 1] - corners[1]);
        qx[k] = (double)(corners[2 * k] + delta[2 * k]);                   // corners_hat is formed in float32
        qy[k] = (double)(corners[2 * k + 1] + delta[2 * k + 1]);
    }
    double A[8][9], x[8];
    dlt_rows(c, qx, qy, A);
    if (!solve8(A, x)) return false;
    for (int k = 0; k < 8; ++k) c.h[k] = x[k];
    c.h[8] = 1.0;
    if (!inv3(c.h, c.m)) return false;
    // N(h, w) = [[2/(w-1), 0, -1], [0, 2/(h-1), -1], [0, 0, 1]] (kornia: a size-1 axis divides by 1e-14)
    const double sxs = Ws == 1 ? 1e-14 : (double)(Ws - 1), sys = Hs == 1 ? 1e-14 : (double)(Hs - 1);
    const double sxd = Wd == 1 ? 1e-14 : (double)(Wd - 1), syd = Hd == 1 ? 1e-14 : (double)(Hd - 1);
    for (int k = 0; k < 9; ++k) c.nd[k] = c.nsi[k] = 0.0;
    c.nd[0] = 2.0 / sxd; c.nd[2] = -1.0; c.nd[4] = 2.0 / syd; c.nd[5] = -1.0; c.nd[8] = 1.0;
    c.nsi[0] = sxs / 2.0; c.nsi[2] = sxs / 2.0; c.nsi[4] = sys / 2.0; c.nsi[5] = sys / 2.0; c.nsi[8] = 1.0;
    double t[9], u[9];
    mul3(c.m, c.nsi, t);
    mul3(c.nd, t, u);
    return inv3(u, c.s);
}

__global__ __launch_bounds__(64) void udh_photo_matrix_kernel(const float* __restrict__ corners, const float* __restrict__ delta, float* __restrict__ S,
                                                              int B, int Hs, int Ws, int Hd, int Wd) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    PhotoChain c;
    double qx[4], qy[4];
    const bool ok = photo_chain(corners + (size_t)i * 8, delta + (size_t)i * 8, Hs, Ws, Hd, Wd, c, qx, qy);
    for (int k = 0; k < 9; ++k) S[(size_t)i * 9 + k] = ok ? (float)c.s[k] : __builtin_nanf("");
}

// g_S [B][slots][9] (the slots are added in index order) -> g_delta [B][4][2]
__global__ __launch_bounds__(64) void udh_photo_matrix_bwd_kernel(const float* __restrict__ corners, const float* __restrict__ delta, const float* __restrict__ gS,
                                                                  float* __restrict__ gdelta, int B, int slots, int Hs, int Ws, int Hd, int Wd) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    PhotoChain c;
    double qx[4], qy[4];
    bool ok = photo_chain(corners + (size_t)i * 8, delta + (size_t)i * 8, Hs, Ws, Hd, Wd, c, qx, qy);
    double gs[9];
    for (int k = 0; k < 9; ++k) {
        float s = 0.0f;
        for (int j = 0; j < slots; ++j) s += gS[((size_t)i * slots + j) * 9 + k];
        gs[k] = (double)s;
    }
    double lam[8];
    if (ok) {
        double t[9], gu[9], gm[9], gh[9];
        // S = inverse(U): g_U = -S^T g_S S^T
        mul3_tn(c.s, gs, t);
        mul3_nt(t, c.s, gu);
        for (int k = 0; k < 9; ++k) gu[k] = -gu[k];
        // U = N_dst M N_src^-1: g_M = N_dst^T g_U N_src^-T
        mul3_tn(c.nd, gu, t);
        mul3_nt(t, c.nsi, gm);
        // M = inverse(h): g_h = -M^T g_M M^T
        mul3_tn(c.m, gm, t);
        mul3_nt(t, c.m, gh);
        for (int k = 0; k < 9; ++k) gh[k] = -gh[k];
        // A x = b: lambda = A^-T g_x, g_A = -lambda x^T, g_b = lambda
        double A[8][9], At[8][9];
        dlt_rows(c, qx, qy, A);
        for (int r = 0; r < 8; ++r) {
            for (int k = 0; k < 8; ++k) At[r][k] = A[k][r];
            At[r][8] = gh[r];
        }
        ok = solve8(At, lam);
    }
    for (int k = 0; k < 4; ++k) {
        float gu = __builtin_nanf(""), gv = gu;
        if (ok) {
            // u enters row 2k through b and the entries -x u, -y u (columns 6, 7); v the same in row 2k + 1
            const double ga6u = -lam[2 * k] * c.h[6], ga7u = -lam[2 * k] * c.h[7];
            const double ga6v = -lam[2 * k + 1] * c.h[6], ga7v = -lam[2 * k + 1] * c.h[7];
            gu = (float)(lam[2 * k] - c.px[k] * ga6u - c.py[k] * ga7u);
            gv = (float)(lam[2 * k + 1] - c.px[k] * ga6v - c.py[k] * ga7v);
        }
        gdelta[(size_t)i * 8 + 2 * k] = gu;
        gdelta[(size_t)i * 8 + 2 * k + 1] = gv;
    }
}

// ------------------------------------------------------------------------------------------------ photometric loss: the sample
struct PhotoSample {
    float gx, gy, X, Y, scale;     // grid point, numerators, 1 / (Z + eps) (1 where |Z| <= eps)
    bool divides;                  // |Z| > eps
    float v, dvdx, dvdy;           // the sample and its derivative in source pixels (grid_sample's own: in-range neighbours only)
};

__device__ __forceinline__ PhotoSample photo_sample(const float* __restrict__ img, const float* __restrict__ m, int ox, int oy, int Hs, int Ws,
                                                    int Hd, int Wd, int align_corners) {
    PhotoSample o;
    // warp.hip: create_meshgrid(normalized) -> transform_points -> convert_points_from_homogeneous(eps = 1e-8) -> grid_sample
    o.gx = __fmul_rn(__fsub_rn(__fdiv_rn((float)ox, (float)(Wd - 1)), 0.5f), 2.0f);
    o.gy = __fmul_rn(__fsub_rn(__fdiv_rn((float)oy, (float)(Hd - 1)), 0.5f), 2.0f);
    o.X = __fadd_rn(__fadd_rn(__fmul_rn(o.gx, m[0]), __fmul_rn(o.gy, m[1])), m[2]);
    o.Y = __fadd_rn(__fadd_rn(__fmul_rn(o.gx, m[3]), __fmul_rn(o.gy, m[4])), m[5]);
    const float Z = __fadd_rn(__fadd_rn(__fmul_rn(o.gx, m[6]), __fmul_rn(o.gy, m[7])), m[8]);
    o.divides = fabsf(Z) > 1e-8f;
    o.scale = o.divides ? __fdiv_rn(1.0f, __fadd_rn(Z, 1e-8f)) : 1.0f;
    const float nx = __fmul_rn(o.X, o.scale), ny = __fmul_rn(o.Y, o.scale);
    const float fx = masic_grid_unnormalize(nx, Ws, align_corners);
    const float fy = masic_grid_unnormalize(ny, Hs, align_corners);
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx = __fsub_rn(fx, x0f), wy = __fsub_rn(fy, y0f);
    const float ex = __fsub_rn(1.0f, wx), ey = __fsub_rn(1.0f, wy);
    const float lim = 1.0e9f;
    const int x0 = (int)fminf(fmaxf(x0f, -lim), lim), y0 = (int)fminf(fmaxf(y0f, -lim), lim);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = x0 >= 0 && x0 < Ws, vx1 = x1 >= 0 && x1 < Ws;
    const bool vy0 = y0 >= 0 && y0 < Hs, vy1 = y1 >= 0 && y1 < Hs;
    o.v = o.dvdx = o.dvdy = 0.0f;
    if ((fx == fx) && (fy == fy)) {
        const float nw = (vx0 && vy0) ? img[(size_t)y0 * Ws + x0] : 0.0f;
        const float ne = (vx1 && vy0) ? img[(size_t)y0 * Ws + x1] : 0.0f;
        const float sw = (vx0 && vy1) ? img[(size_t)y1 * Ws + x0] : 0.0f;
        const float se = (vx1 && vy1) ? img[(size_t)y1 * Ws + x1] : 0.0f;
        float v = __fmul_rn(nw, __fmul_rn(ex, ey));
        v = __fadd_rn(v, __fmul_rn(ne, __fmul_rn(wx, ey)));
        v = __fadd_rn(v, __fmul_rn(sw, __fmul_rn(ex, wy)));
        v = __fadd_rn(v, __fmul_rn(se, __fmul_rn(wx, wy)));
        o.v = v;
        o.dvdx = (ne - nw) * ey + (se - sw) * wy;
        o.dvdy = (sw - nw) * ex + (se - ne) * wx;
    }
    return o;
}

// part[b * gridDim.x + block] = sum over the block's pixels of |sample - patch_b| (a shuffle tree, then the four waves in order)
__global__ __launch_bounds__(256) void udh_photo_loss_kernel(const float* __restrict__ img, const float* __restrict__ S, const float* __restrict__ pb,
                                                             float* __restrict__ part, int Hs, int Ws, int Hd, int Wd, int align_corners) {
    __shared__ float red[4];
    const int b = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    float d = 0.0f;
    if (pix < Hd * Wd) {
        const int oy = pix / Wd, ox = pix - oy * Wd;
        const PhotoSample s = photo_sample(img + (size_t)b * Hs * Ws, S + b * 9, ox, oy, Hs, Ws, Hd, Wd, align_corners);
        d = fabsf(s.v - pb[(size_t)b * Hd * Wd + pix]);
    }
    d = wave_sum(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void udh_photo_loss_finish_kernel(const float* __restrict__ part, float* __restrict__ loss, int n, double count) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / count);
}

// gS_part[b][block][9]: sum over the block's pixels of sign(diff) * g_loss / count * d sample / d S
__global__ __launch_bounds__(256) void udh_photo_loss_bwd_kernel(const float* __restrict__ img, const float* __restrict__ S, const float* __restrict__ pb,
                                                                 const float* __restrict__ gloss, float* __restrict__ gpart, int Hs, int Ws, int Hd, int Wd,
                                                                 int align_corners, float inv_count) {
    __shared__ float red[4][9];
    const int b = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    float g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = 0.0f;
    if (pix < Hd * Wd) {
        const int oy = pix / Wd, ox = pix - oy * Wd;
        const PhotoSample s = photo_sample(img + (size_t)b * Hs * Ws, S + b * 9, ox, oy, Hs, Ws, Hd, Wd, align_corners);
        const float diff = s.v - pb[(size_t)b * Hd * Wd + pix];
        const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : (diff == diff ? 0.0f : diff));
        const float c = sgn * (gloss[0] * inv_count);
        // source pixels per unit of the normalised coordinate
        const float ux = align_corners ? 0.5f * (float)(Ws - 1) : 0.5f * (float)Ws;
        const float uy = align_corners ? 0.5f * (float)(Hs - 1) : 0.5f * (float)Hs;
        const float gnx = c * s.dvdx * ux, gny = c * s.dvdy * uy;
        const float gX = gnx * s.scale, gY = gny * s.scale;
        const float gZ = s.divides ? -(gnx * s.X + gny * s.Y) * s.scale * s.scale : 0.0f;
        g[0] = gX * s.gx; g[1] = gX * s.gy; g[2] = gX;
        g[3] = gY * s.gx; g[4] = gY * s.gy; g[5] = gY;
        g[6] = gZ * s.gx; g[7] = gZ * s.gy; g[8] = gZ;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sum(g[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        gpart[((size_t)b * gridDim.x + blockIdx.x) * 9 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

}  // namespace

extern "C" int masic_maxpool2_relu_bwd(const float* x, const float* gy, float* gx, int planes, int H, int W, void* stream) {
    MASIC_REQUIRE(x && gy && gx, MASIC_ERR_ARG, "maxpool2_relu_bwd: null pointer");
    MASIC_REQUIRE(planes > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, MASIC_ERR_SHAPE, "maxpool2_relu_bwd: %d planes of %d x %d (even sizes only)", planes, H, W);
    MASIC_REQUIRE((((size_t)x | (size_t)gx) & 7) == 0, MASIC_ERR_ARG, "maxpool2_relu_bwd: x and gx must be 8-byte aligned");
    const size_t total = (size_t)planes * (H / 2) * (W / 2);
    MASIC_REQUIRE(total <= ((size_t)1 << 38), MASIC_ERR_SHAPE, "maxpool2_relu_bwd: %zu windows", total);
    hipLaunchKernelGGL(maxpool2_relu_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, gy, gx, W / 2, total);
    return masic_launch_status("maxpool2_relu_bwd");
}

extern "C" size_t masic_udh_conv1_wgrad_workspace_bytes(int B, int H, int W, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || (long)H * W > (1L << 30)) return 0;
    return (size_t)B * ceil_div(H * W, W1G_PIX) * Cout * W1G_V * sizeof(float);
}

extern "C" int masic_udh_conv1_wgrad(const float* a, const float* b, const float* dy, void* workspace, float* dw, float* db, int B, int H, int W,
                                     int Cout, void* stream) {
    MASIC_REQUIRE(a && b && dy && workspace && dw && db, MASIC_ERR_ARG, "udh_conv1_wgrad: null pointer");
    MASIC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W <= (1L << 30), MASIC_ERR_SHAPE, "udh_conv1_wgrad: B %d, %d x %d", B, H, W);
    MASIC_REQUIRE(Cout > 0 && Cout % W1G_CO == 0 && Cout / W1G_CO <= 65535, MASIC_ERR_SHAPE, "udh_conv1_wgrad: Cout %d is not a multiple of %d", Cout, W1G_CO);
    const int chunks = ceil_div(H * W, W1G_PIX);
    MASIC_REQUIRE((long)B * chunks <= (1L << 24), MASIC_ERR_SHAPE, "udh_conv1_wgrad: %ld partials", (long)B * chunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(udh_conv1_wgrad_partial_kernel, dim3(chunks, Cout / W1G_CO, B), dim3(256), 0, st, a, b, dy, (float*)workspace, H, W, Cout);
    hipLaunchKernelGGL(udh_conv1_wgrad_finish_kernel, dim3(ceil_div(Cout * W1G_V, 256)), dim3(256), 0, st, (const float*)workspace, dw, db, B * chunks, Cout);
    return masic_launch_status("udh_conv1_wgrad");
}

extern "C" int masic_udh_dropout_fwd(const float* x, const unsigned char* mask, float* y, size_t n, void* stream) {
    MASIC_REQUIRE(x && mask && y, MASIC_ERR_ARG, "udh_dropout_fwd: null pointer");
    MASIC_REQUIRE(n > 0 && n % 4 == 0 && n / 4 <= ((size_t)1 << 38), MASIC_ERR_SHAPE, "udh_dropout_fwd: %zu elements (multiples of 4)", n);
    MASIC_REQUIRE((((size_t)x | (size_t)y) & 15) == 0 && ((size_t)mask & 3) == 0, MASIC_ERR_ARG, "udh_dropout_fwd: misaligned pointer");
    hipLaunchKernelGGL(udh_dropout_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mask, y, n / 4);
    return masic_launch_status("udh_dropout_fwd");
}

extern "C" int masic_udh_fc_train_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const unsigned char* m2,
                                      void* workspace, float* hidden, float* out, int B, int K, int N, int M, void* stream) {
    MASIC_REQUIRE(hidden && m2, MASIC_ERR_ARG, "udh_fc_train_fwd: null pointer");
    const int rc = masic_udh_fc_fwd(x, w1, b1, w2, b2, workspace, hidden, out, B, K, N, M, stream);
    if (rc != MASIC_OK) return rc;
    hipLaunchKernelGGL(udh_fc2_masked_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, (const float*)hidden, m2, w2, b2, out, N, M);
    return masic_launch_status("udh_fc_train_fwd");
}

extern "C" size_t masic_udh_fc_bwd_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)N * round_up(B, FB_ROWS * FB_MAXG) * sizeof(float);
}

extern "C" int masic_udh_fc_bwd(const float* gout, const float* xd, const float* hidden, const unsigned char* m1, const unsigned char* m2,
                                const float* w1, const float* w2, void* workspace, float* gw1, float* gb1, float* gw2, float* gb2, float* gx,
                                int B, int K, int N, int M, void* stream) {
    MASIC_REQUIRE(gout && xd && hidden && w1 && w2 && workspace && gw1 && gb1 && gw2 && gb2 && gx, MASIC_ERR_ARG, "udh_fc_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && B <= (1 << 20), MASIC_ERR_SHAPE, "udh_fc_bwd: B %d", B);
    MASIC_REQUIRE(K > 0 && K % FB_KCH == 0, MASIC_ERR_SHAPE, "udh_fc_bwd: K %d is not a multiple of %d", K, FB_KCH);
    MASIC_REQUIRE(N > 0 && N % (4 * FB_NT) == 0, MASIC_ERR_SHAPE, "udh_fc_bwd: N %d is not a multiple of %d", N, 4 * FB_NT);
    MASIC_REQUIRE(M > 0 && M <= 256, MASIC_ERR_SHAPE, "udh_fc_bwd: M %d", M);
    MASIC_REQUIRE((((size_t)xd | (size_t)w1 | (size_t)gw1 | (size_t)gx) & 15) == 0 && ((size_t)m1 & 3) == 0, MASIC_ERR_ARG,
                  "udh_fc_bwd: x', w1, gw1 and gx must be 16-byte aligned, m1 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int slab = FB_ROWS * FB_MAXG, Bp = round_up(B, slab);
    float* ghT = (float*)workspace;
    hipLaunchKernelGGL(udh_fc_bwd_head_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, gout, hidden, m2, w2, ghT, gb1, gw2, gb2, B, Bp, N, M);
    const dim3 grid(K / FB_KCH);
    // <= 32 rows: one pass, gW1 written once.  Beyond: one pass per 32 rows on the same stream, each adding to gW1 in row order.
    for (int b0 = 0; b0 < B; b0 += slab) {
        const int groups = ceil_div((B - b0 < slab ? B - b0 : slab), FB_ROWS);
#define MASIC_FB(NG)                                                                                                                       \
    do {                                                                                                                                   \
        if (b0 == 0) hipLaunchKernelGGL((udh_fc1_bwd_kernel<NG, false>), grid, dim3(256), 0, st, xd, (const float*)ghT, m1, w1, gw1, gx, B, Bp, b0, K, N); \
        else hipLaunchKernelGGL((udh_fc1_bwd_kernel<NG, true>), grid, dim3(256), 0, st, xd, (const float*)ghT, m1, w1, gw1, gx, B, Bp, b0, K, N);          \
    } while (0)
        if (groups == 1) MASIC_FB(1); else if (groups == 2) MASIC_FB(2); else if (groups == 3) MASIC_FB(3); else MASIC_FB(4);
#undef MASIC_FB
    }
    return masic_launch_status("udh_fc_bwd");
}

extern "C" int masic_udh_photo_matrix(const float* corners, const float* delta, float* S, int B, int Hs, int Ws, int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(corners && delta && S, MASIC_ERR_ARG, "udh_photo_matrix: null pointer");
    MASIC_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, MASIC_ERR_SHAPE, "udh_photo_matrix: B %d, %d x %d -> %d x %d", B, Hs, Ws, Hd, Wd);
    hipLaunchKernelGGL(udh_photo_matrix_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, corners, delta, S, B, Hs, Ws, Hd, Wd);
    return masic_launch_status("udh_photo_matrix");
}

extern "C" int masic_udh_photo_matrix_bwd(const float* corners, const float* delta, const float* gS, float* gdelta, int B, int slots, int Hs, int Ws,
                                          int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(corners && delta && gS && gdelta, MASIC_ERR_ARG, "udh_photo_matrix_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && slots > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, MASIC_ERR_SHAPE, "udh_photo_matrix_bwd: B %d, %d slots", B, slots);
    hipLaunchKernelGGL(udh_photo_matrix_bwd_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, corners, delta, gS, gdelta, B, slots,
                       Hs, Ws, Hd, Wd);
    return masic_launch_status("udh_photo_matrix_bwd");
}

extern "C" int masic_udh_photo_slots(int Hd, int Wd) { return Hd > 0 && Wd > 0 && (long)Hd * Wd <= (1L << 30) ? ceil_div(Hd * Wd, 256) : 0; }

extern "C" int masic_udh_photo_loss_fwd(const float* img, const float* S, const float* patch_b, void* workspace, float* loss, int B, int Hs, int Ws,
                                        int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(img && S && patch_b && workspace && loss, MASIC_ERR_ARG, "udh_photo_loss_fwd: null pointer");
    const int slots = masic_udh_photo_slots(Hd, Wd);
    MASIC_REQUIRE(B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && slots > 0 && (long)Hs * Ws <= (1L << 30) && (long)B * slots <= (1L << 30), MASIC_ERR_SHAPE,
                  "udh_photo_loss_fwd: B %d, %d x %d -> %d x %d", B, Hs, Ws, Hd, Wd);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(udh_photo_loss_kernel, dim3(slots, B), dim3(256), 0, st, img, S, patch_b, (float*)workspace, Hs, Ws, Hd, Wd,
                       masic_warp_align_corners_value());
    hipLaunchKernelGGL(udh_photo_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, loss, B * slots, (double)B * Hd * Wd);
    return masic_launch_status("udh_photo_loss_fwd");
}

extern "C" int masic_udh_photo_loss_bwd(const float* img, const float* S, const float* patch_b, const float* gloss, float* gS_part, int B, int Hs, int Ws,
                                        int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(img && S && patch_b && gloss && gS_part, MASIC_ERR_ARG, "udh_photo_loss_bwd: null pointer");
    const int slots = masic_udh_photo_slots(Hd, Wd);
    MASIC_REQUIRE(B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && slots > 0 && (long)Hs * Ws <= (1L << 30) && (long)B * slots <= (1L << 30), MASIC_ERR_SHAPE,
                  "udh_photo_loss_bwd: B %d, %d x %d -> %d x %d", B, Hs, Ws, Hd, Wd);
    hipLaunchKernelGGL(udh_photo_loss_bwd_kernel, dim3(slots, B), dim3(256), 0, (hipStream_t)stream, img, S, patch_b, gloss, gS_part, Hs, Ws, Hd, Wd,
                       masic_warp_align_corners_value(), (float)(1.0 / ((double)B * Hd * Wd)));
    return masic_launch_status("udh_photo_loss_bwd");
}
