// lpips.hip -- what LPIPS on the AlexNet trunk (masic_amd/lpips.py; lpips 0.1.4's `LPIPS(net='alex')`) needs beyond the float32
// implicit-GEMM convolution of conv.hip, which runs layers 2-5 (masic_conv2d_fwd_ex, MASIC_ACT_RELU).  Everything is float32 with one
// summation order per sum, no float atomics and no fills; the two pictures of comparison n are images 2n and 2n + 1 of a batch.
//
//   lpips_conv1    Conv2d(3 -> 64, k11, s4, p2) + bias + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32, read from the two
//                  picture tensors with `normalize` and the scaling layer applied while staging (in-image pixels only: the padding
//                  is zero AFTER the scaling, so neither folds into the weights).  The input patch of a 4 x 32 output tile is
//                  staged in LDS de-interleaved by row and column mod 4: 48 planes (3 channels x 4 x 4) of 6 x 34 words, on which
//                  the layer is a 3 x 3 stride-1 walk -- K = 9 x 48 = 432, with zero weights where 4 t + r = 11 -- and the 32
//                  lanes of a B fragment read 32 consecutive words.  The plane pitch is 224 words (= 32 mod 64) so that the two
//                  half-waves of a fragment (planes 2q and 2q + 1) fall into disjoint banks.  43 KB of LDS, three workgroups per
//                  CU; the 110 KB weight image does not share LDS with the patch: it is stored in fragment order and streamed from
//                  L2 through registers (one coalesced 256-byte load per wave and k pair), the next tap's 24 fragments in flight
//                  while this tap's 48 MFMAs issue.  Wave w: output channels 32 (w & 1) .., tile rows 2 (w >> 1) and + 1.
//   maxpool3s2     MaxPool2d(3, 2), one output per lane, torch's scan (NaN propagates, the first of equal values stays).
//   lpips_dist     per pixel: the two channel norms first, then sum_c lin_c (a_c / na - b_c / nb)^2 of the normalised values (not
//                  the expanded form, which cancels when the pictures are close).  64 pixels per workgroup on the lanes, the
//                  channels dealt to the 4 waves (c = wave, wave + 4, ...); the four partial sums of a pixel are added in wave
//                  order, the 64 pixels in a fixed butterfly in float64, one double per workgroup.
//   lpips_finish   per picture: the chunks of a tap in a fixed order (float64), / (h w), the five taps in order (float32).
#include <math.h>

#include "common.h"

namespace {

constexpr int L1_TH = 4, L1_TW = 32;                  // output tile
constexpr int L1_PH = L1_TH + 2, L1_PW = L1_TW + 2;   // plane of the de-interleaved patch
constexpr int L1_PS = 224;                            // plane pitch in words (L1_PH * L1_PW = 204 used)
constexpr int L1_PLANES = 48;                         // ci * 16 + (row mod 4) * 4 + (column mod 4)
constexpr int L1_KPAIRS = 9 * L1_PLANES / 2;          // 216 k pairs: k = tap * 48 + plane
constexpr int L1_ROWS = 4 * L1_PH, L1_COLS = 4 * L1_PW;      // input rows / columns under a tile: 24 x 136
constexpr int L1_PACKED = L1_KPAIRS * 2 * 64;         // floats: [k pair][channel half][lane]
static_assert(L1_PH * L1_PW <= L1_PS && L1_PS % 64 == 32, "plane pitch");

__global__ void lpips_conv1_pack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L1_PACKED) return;
    const int kk = i >> 7, cob = (i >> 6) & 1, l = i & 63;
    const int co = cob * 32 + (l & 31), k = 2 * kk + (l >> 5);
    const int tap = k / L1_PLANES, plane = k - tap * L1_PLANES;
    const int kh = 4 * (tap / 3) + ((plane >> 2) & 3), kw = 4 * (tap % 3) + (plane & 3), ci = plane >> 4;
    wp[i] = (kh < 11 && kw < 11) ? w[((co * 3 + ci) * 11 + kh) * 11 + kw] : 0.0f;
}

__global__ __launch_bounds__(256) void lpips_conv1_kernel(const float* __restrict__ in0, const float* __restrict__ in1, const float* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ shift,
                                                          const float* __restrict__ scale, float* __restrict__ y, int H, int W, int Ho, int Wo,
                                                          int normalize) {
    __shared__ float patch[L1_PLANES * L1_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int img = blockIdx.z;
    const float* src = ((img & 1) ? in1 : in0) + (size_t)(img >> 1) * 3 * H * W;
    const int oy0 = blockIdx.y * L1_TH, ox0 = blockIdx.x * L1_TW;
    const int iy0 = 4 * oy0 - 2, ix0 = 4 * ox0 - 2;
    for (int i = tid; i < 3 * L1_ROWS * L1_COLS; i += 256) {
        const int c = i / (L1_ROWS * L1_COLS), r = i - c * (L1_ROWS * L1_COLS), pr = r / L1_COLS, pc = r - pr * L1_COLS;
        const int iy = iy0 + pr, ix = ix0 + pc;
        float v = 0.0f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = src[((size_t)c * H + iy) * W + ix];
            if (normalize) v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f);
            v = __fdiv_rn(__fsub_rn(v, shift[c]), scale[c]);
        }
        patch[((c * 4 + (pr & 3)) * 4 + (pc & 3)) * L1_PS + (pr >> 2) * L1_PW + (pc >> 2)] = v;
    }
    __syncthreads();

    const int cob = wave & 1, rp = wave >> 1;
    const float* wl = wp + cob * 64 + lane;
    const float* pb = patch + h * L1_PS + (2 * rp) * L1_PW + j;
    f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.0f;
    float a[L1_PLANES / 2], an[L1_PLANES / 2];
#pragma unroll
    for (int q = 0; q < L1_PLANES / 2; ++q) {
        a[q] = wl[q * 128];
        an[q] = 0.0f;
    }
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        if (tap < 8) {
#pragma unroll
            for (int q = 0; q < L1_PLANES / 2; ++q) an[q] = wl[((tap + 1) * (L1_PLANES / 2) + q) * 128];
        }
        const float* pt = pb + (tap / 3) * L1_PW + (tap % 3);
#pragma unroll
        for (int q = 0; q < L1_PLANES / 2; ++q) {
            const float b0 = pt[2 * q * L1_PS], b1 = pt[2 * q * L1_PS + L1_PW];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b1, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < L1_PLANES / 2; ++q) a[q] = an[q];
    }

    const int ox = ox0 + j;
    if (ox >= Wo) return;
    const size_t plane = (size_t)Ho * Wo;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int oy = oy0 + 2 * rp + n;
        if (oy >= Ho) continue;
        float* yo = y + (size_t)img * 64 * plane + (size_t)oy * Wo + ox;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = cob * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            yo[(size_t)co * plane] = fmaxf((n ? acc1[e] : acc0[e]) + bias[co], 0.0f);
        }
    }
}

__device__ __forceinline__ float max_nan(float m, float u) { return (u > m || u != u) ? u : m; }

__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Ho, int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / Wo, plane = row / Ho;
    const int c = (int)(i - row * Wo), r = (int)(row - plane * Ho);
    const float* p = x + (plane * H + 2 * r) * (size_t)W + 2 * c;
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) m = max_nan(m, p[(size_t)dy * W + dx]);
    y[i] = m;
}

constexpr int DIST_PX = 64;            // pixels per workgroup

__global__ __launch_bounds__(256) void lpips_dist_kernel(const float* __restrict__ f, const float* __restrict__ lin, double* __restrict__ part, int C, int HW) {
    __shared__ float sa[4][DIST_PX], sb[4][DIST_PX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * DIST_PX + lane, n = blockIdx.y;
    const bool ok = p < HW;
    const float* fa = f + (size_t)(2 * n) * C * HW + (ok ? p : 0);
    const float* fb = fa + (size_t)C * HW;
    float s0 = 0.0f, s1 = 0.0f;
    if (ok)
        for (int c = wave; c < C; c += 4) {
            const float u = fa[(size_t)c * HW], v = fb[(size_t)c * HW];
            s0 = fmaf(u, u, s0);
            s1 = fmaf(v, v, s1);
        }
    sa[wave][lane] = s0;
    sb[wave][lane] = s1;
    __syncthreads();
    const float na = sqrtf(((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane]) + 1e-10f;
    const float nb = sqrtf(((sb[0][lane] + sb[1][lane]) + sb[2][lane]) + sb[3][lane]) + 1e-10f;
    float t = 0.0f;
    if (ok)
        for (int c = wave; c < C; c += 4) {
            const float d = __fdiv_rn(fa[(size_t)c * HW], na) - __fdiv_rn(fb[(size_t)c * HW], nb);
            t = fmaf(lin[c], d * d, t);
        }
    __syncthreads();
    sa[wave][lane] = t;
    __syncthreads();
    if (wave != 0) return;
    double s = (double)(((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) part[(size_t)n * gridDim.x + blockIdx.x] = s;
}

struct FinishArgs {
    int nchunks[5], hw[5];
};

__global__ __launch_bounds__(256) void lpips_finish_kernel(const double* __restrict__ part, FinishArgs a, int N, float* __restrict__ out) {
    __shared__ double sd[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    size_t off = 0;
    float val = 0.0f;
    for (int t = 0; t < 5; ++t) {
        const double* p = part + off + (size_t)n * a.nchunks[t];
        double s = 0.0;
        for (int i = tid; i < a.nchunks[t]; i += 256) s += p[i];
        sd[tid] = s;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) {
            if (tid < m) sd[tid] += sd[tid + m];
            __syncthreads();
        }
        if (tid == 0) {
            const float v = (float)(sd[0] / (double)a.hw[t]);
            out[(size_t)(1 + t) * N + n] = v;
            val += v;
        }
        __syncthreads();
        off += (size_t)N * a.nchunks[t];
    }
    if (tid == 0) out[n] = val;
}

}  // namespace

extern "C" size_t masic_lpips_conv1_packed_bytes(void) { return (size_t)L1_PACKED * sizeof(float); }

extern "C" int masic_lpips_conv1_pack_weight(const float* w, float* w_packed, void* stream) {
    MASIC_REQUIRE(w && w_packed, MASIC_ERR_ARG, "lpips_conv1_pack_weight: null pointer");
    hipLaunchKernelGGL(lpips_conv1_pack_kernel, dim3(ceil_div(L1_PACKED, 256)), dim3(256), 0, (hipStream_t)stream, w, w_packed);
    return masic_launch_status("lpips_conv1_pack_weight");
}

extern "C" int masic_lpips_conv1_fwd(const float* in0, const float* in1, const float* w_packed, const float* bias, const float* shift,
                                     const float* scale, float* y, int N, int H, int W, int normalize, void* stream) {
    MASIC_REQUIRE(in0 && in1 && w_packed && bias && shift && scale && y, MASIC_ERR_ARG, "lpips_conv1_fwd: null pointer");
    MASIC_REQUIRE(N > 0 && 2 * (long)N <= 65535 && H >= 11 && W >= 11 && (long)H * W <= (1L << 28), MASIC_ERR_SHAPE,
                  "lpips_conv1_fwd: N %d, %d x %d", N, H, W);
    const int Ho = (H - 7) / 4 + 1, Wo = (W - 7) / 4 + 1;
    MASIC_REQUIRE(ceil_div(Ho, L1_TH) <= 65535, MASIC_ERR_SHAPE, "lpips_conv1_fwd: %d output rows", Ho);
    hipLaunchKernelGGL(lpips_conv1_kernel, dim3(ceil_div(Wo, L1_TW), ceil_div(Ho, L1_TH), 2 * N), dim3(256), 0, (hipStream_t)stream, in0, in1,
                       w_packed, bias, shift, scale, y, H, W, Ho, Wo, normalize);
    return masic_launch_status("lpips_conv1_fwd");
}

extern "C" int masic_maxpool3s2_fwd(const float* x, float* y, int planes, int H, int W, void* stream) {
    MASIC_REQUIRE(x && y, MASIC_ERR_ARG, "maxpool3s2_fwd: null pointer");
    MASIC_REQUIRE(planes > 0 && H >= 3 && W >= 3, MASIC_ERR_SHAPE, "maxpool3s2_fwd: %d planes of %d x %d", planes, H, W);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const size_t total = (size_t)planes * Ho * Wo;
    MASIC_REQUIRE(total <= ((size_t)1 << 38), MASIC_ERR_SHAPE, "maxpool3s2_fwd: %zu outputs", total);
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, Ho, Wo, total);
    return masic_launch_status("maxpool3s2_fwd");
}

extern "C" int masic_lpips_dist_chunks(int HW) { return HW > 0 ? ceil_div(HW, DIST_PX) : 0; }

extern "C" int masic_lpips_dist_fwd(const float* f, const float* lin, double* part, int N, int C, int HW, void* stream) {
    MASIC_REQUIRE(f && lin && part, MASIC_ERR_ARG, "lpips_dist_fwd: null pointer");
    MASIC_REQUIRE(N > 0 && N <= 65535 && C > 0 && HW > 0 && HW <= (1 << 30), MASIC_ERR_SHAPE, "lpips_dist_fwd: N %d, C %d, %d pixels", N, C, HW);
    hipLaunchKernelGGL(lpips_dist_kernel, dim3(ceil_div(HW, DIST_PX), N), dim3(256), 0, (hipStream_t)stream, f, lin, part, C, HW);
    return masic_launch_status("lpips_dist_fwd");
}

extern "C" int masic_lpips_finish(const double* part, const int* nchunks, const int* hw, int N, float* out, void* stream) {
    MASIC_REQUIRE(part && nchunks && hw && out, MASIC_ERR_ARG, "lpips_finish: null pointer");
    MASIC_REQUIRE(N > 0, MASIC_ERR_SHAPE, "lpips_finish: N %d", N);
    FinishArgs a;
    for (int t = 0; t < 5; ++t) {
        MASIC_REQUIRE(nchunks[t] > 0 && hw[t] > 0, MASIC_ERR_SHAPE, "lpips_finish: tap %d has %d chunks of %d pixels", t, nchunks[t], hw[t]);
        a.nchunks[t] = nchunks[t];
        a.hw[t] = hw[t];
    }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, part, a, N, out);
    return masic_launch_status("lpips_finish");
}
