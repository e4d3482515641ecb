// lpips_bwd.hip -- the input gradients of LPIPS on the AlexNet trunk (masic_amd/lpips.py): what the backward schedule needs beyond the
// float32 implicit-GEMM convolution of conv.hip, which runs the input gradients of layers 2-5 as the opposite layer kind.  The rules of
// lpips.hip hold: float32, one summation order per sum, no float atomics, no fills, no host synchronisation, and an image's result does
// not depend on what else shares the launch.  A chain runs on the images of one side (N images: only that picture requires grad) or on
// the 2N interleaved images of the forward (both do); the saved taps are always the forward's [2N] tensors.
//
//   lpips_dist_bwd   per pixel, with u = a / na, v = b / nb, d = u - v, Sa = sum_c lin_c d_c u_c, Sb = sum_c lin_c d_c v_c (all from the
//                    normalised values, as the forward's sum: the expanded form cancels when the pictures are close):
//                      dL/da_c = +(2 G / HW) (lin_c d_c / na - u_c Sa / sqrt(sum a^2)),  dL/db_c = -(2 G / HW) (lin_c d_c / nb - v_c Sb / ..)
//                    with the second term 0 where the pixel's squares sum to 0 (the forward's 0 / 1e-10 = 0 convention; lpips's own
//                    autograd is 0 / 0 there).  G = g_val[n] + g_res[n] is read on the device.  The gradient arriving from the layer
//                    above is added and the tap's ReLU mask applied, so what is written is the gradient of the pre-activation.  The
//                    forward's decomposition: 64 pixels per workgroup on the lanes, the channels dealt to the 4 waves, the four partial
//                    sums of a pixel added in wave order.  Three passes over the chunk's channels (norms, Sa / Sb, gradient).
//   maxpool3s2_bwd   a gather: an input pixel visits the at most 2 x 2 windows that cover it in row-major window order, finds each
//                    window's winner with the forward's scan (the first of equal values, the last NaN) and adds the window's gradient
//                    if it is the winner itself -- the order of torch's scatter, hence its bits.  Uncovered rows / columns get 0.
//                    A thread owns a 2 x 2 input block: its four pixels lie under the same four windows, scanned once.
//   lpips_conv1_bwd  the input gradient of Conv2d(3 -> 64, k11, s4, p2) with the scaling layer and `normalize` behind it.  With
//                    p = i + 2, q = p / 4, r = p % 4, input row i meets kernel rows r + 4 t of output rows q - t, t = 0 .. 2: on the
//                    4 x 4 input phases a 3 x 3 stride-1 walk over the output gradient, 64 channels in, 3 x 16 phase channels out.
//                    Plain FMAs: a lane owns one phase-grid pixel (qy, qx), a wave one row phase ry, so a thread keeps the 3 x 4
//                    results (channel, column phase) of that pixel in registers; the weights are wave-uniform (a repacked image
//                    [ry][co][tap][c][rx], read through the scalar cache), the output gradient comes from LDS, 16 channels of a
//                    (4 + 2) x (16 + 2) patch at a time, one word per 12 FMAs.  The taps with r + 4 t = 11 are skipped, not
//                    multiplied by zero.  The store does the depth-to-space, the crop to H x W, 1 / scale[c] (2 / scale[c] under
//                    normalize) and the split into the two pictures' gradient tensors; every pixel of the picture is written.
#include <math.h>

#include "common.h"

namespace {

constexpr int DIST_PX = 64;            // pixels per workgroup, as lpips_dist_kernel

__global__ __launch_bounds__(256) void lpips_dist_bwd_kernel(const float* __restrict__ f, const float* __restrict__ lin, const float* __restrict__ g_val,
                                                             const float* __restrict__ g_res, const float* g_in, float* g_pre, int C, int HW,
                                                             int sides) {
    __shared__ float sa[4][DIST_PX], sb[4][DIST_PX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * DIST_PX + lane, n = blockIdx.y;
    const bool ok = p < HW;
    const size_t img = (size_t)C * HW;
    const float* fa = f + (size_t)(2 * n) * img + (ok ? p : 0);
    const float* fb = fa + img;
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
    const float qa = sqrtf(((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane]);
    const float qb = sqrtf(((sb[0][lane] + sb[1][lane]) + sb[2][lane]) + sb[3][lane]);
    const float na = qa + 1e-10f, nb = qb + 1e-10f;
    float ta = 0.0f, tb = 0.0f;
    if (ok)
        for (int c = wave; c < C; c += 4) {
            const float u = __fdiv_rn(fa[(size_t)c * HW], na), v = __fdiv_rn(fb[(size_t)c * HW], nb);
            const float ld = lin[c] * (u - v);
            ta = fmaf(ld, u, ta);
            tb = fmaf(ld, v, tb);
        }
    __syncthreads();
    sa[wave][lane] = ta;
    sb[wave][lane] = tb;
    __syncthreads();
    if (!ok) return;
    const float Sa = ((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane];
    const float Sb = ((sb[0][lane] + sb[1][lane]) + sb[2][lane]) + sb[3][lane];
    const float ka = qa > 0.0f ? __fdiv_rn(Sa, qa) : 0.0f, kb = qb > 0.0f ? __fdiv_rn(Sb, qb) : 0.0f;
    const float coef = __fdiv_rn(2.0f * (g_val[n] + g_res[n]), (float)HW);
    const bool both = sides == 3;
    const size_t oa = (size_t)(both ? 2 * n : n) * img + p, ob = (size_t)(both ? 2 * n + 1 : n) * img + p;
    for (int c = wave; c < C; c += 4) {
        const float a = fa[(size_t)c * HW], b = fb[(size_t)c * HW];
        const float u = __fdiv_rn(a, na), v = __fdiv_rn(b, nb);
        const float ld = lin[c] * (u - v);
        if (sides & 1) {
            float g = coef * (__fdiv_rn(ld, na) - u * ka);
            if (g_in) g += g_in[oa + (size_t)c * HW];
            g_pre[oa + (size_t)c * HW] = a > 0.0f ? g : 0.0f;
        }
        if (sides & 2) {
            float g = -coef * (__fdiv_rn(ld, nb) - v * kb);
            if (g_in) g += g_in[ob + (size_t)c * HW];
            g_pre[ob + (size_t)c * HW] = b > 0.0f ? g : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, int C,
                                                             int H, int W, int Ho, int Wo, int img_stride, int img_off, int Hb, int Wb,
                                                             size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / Wb, plane = row / Hb, im = plane / C;
    const int b = (int)(i - row * Wb), a = (int)(row - plane * Hb), ch = (int)(plane - im * C);
    const float* xp = x + ((im * img_stride + img_off) * C + ch) * ((size_t)H * W);
    const float* gp = gy + plane * ((size_t)Ho * Wo);
    // the 2 x 2 input block (2a.., 2b..) lies under the windows (a - 1 + dr, b - 1 + dc) only: their winners (position 3 dy + dx in the
    // window, -1 where the window does not exist) and gradients
    int arg[2][2];
    float g[2][2];
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
            const int r = a - 1 + dr, c = b - 1 + dc;
            arg[dr][dc] = -1;
            g[dr][dc] = 0.0f;
            if (r < 0 || r >= Ho || c < 0 || c >= Wo) continue;
            const float* w = xp + (size_t)(2 * r) * W + 2 * c;
            float m = -INFINITY;
            int k = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float u = w[(size_t)dy * W + dx];
                    if (u > m || u != u) {
                        m = u;
                        k = dy * 3 + dx;
                    }
                }
            arg[dr][dc] = k;
            g[dr][dc] = gp[(size_t)r * Wo + c];
        }
    // pixel (2a + py, 2b + px) sits at (2 - 2 dr + py, 2 - 2 dc + px) of window (dr, dc); the windows are visited in row-major order
    float* op = gx + plane * ((size_t)H * W);
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            if (2 * a + py >= H || 2 * b + px >= W) continue;
            float s = 0.0f;
#pragma unroll
            for (int dr = py; dr < 2; ++dr)
#pragma unroll
                for (int dc = px; dc < 2; ++dc)
                    if (arg[dr][dc] == (2 - 2 * dr + py) * 3 + (2 - 2 * dc + px)) s += g[dr][dc];
            op[(size_t)(2 * a + py) * W + 2 * b + px] = s;
        }
}

constexpr int B1_TW = 16, B1_TH = 4;                  // phase-grid pixels of a workgroup: the 64 lanes (129 x 129 of them at 512 x 512)
constexpr int B1_PW = B1_TW + 2, B1_PH = B1_TH + 2;   // patch of the output gradient under them
constexpr int B1_CO = 16;                             // channels staged per step
constexpr int B1_PLANE = B1_PH * B1_PW;
static_assert(B1_TW * B1_TH == 64, "one phase-grid pixel per lane");
constexpr int B1_WCO = 9 * 12;                        // packed weights of one (row phase, output channel): [tap][c][rx]
constexpr int B1_PACKED = 4 * 64 * B1_WCO;            // floats: [ry][co][tap][c][rx]

__global__ void lpips_conv1_bwd_pack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B1_PACKED) return;
    const int rx = i & 3, c = (i >> 2) % 3, r = i / 12, tap = r % 9, co = (r / 9) & 63, ry = r / (9 * 64);
    const int kh = ry + 4 * (tap / 3), kw = rx + 4 * (tap % 3);
    wp[i] = (kh < 11 && kw < 11) ? w[((co * 3 + c) * 11 + kh) * 11 + kw] : 0.0f;
}

__global__ __launch_bounds__(256) void lpips_conv1_bwd_kernel(const float* __restrict__ g, const float* __restrict__ wp, const float* __restrict__ scale,
                                                              float* __restrict__ d0, float* __restrict__ d1, int H, int W, int Ho, int Wo,
                                                              int normalize) {
    __shared__ float patch[B1_CO * B1_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, lx = lane % B1_TW, ly = lane / B1_TW;
    const int ry = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.z, qy0 = blockIdx.y * B1_TH, qx0 = blockIdx.x * B1_TW;
    const size_t oplane = (size_t)Ho * Wo;
    const float* gi = g + (size_t)img * 64 * oplane;
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.0f;
#pragma unroll 1
    for (int co0 = 0; co0 < 64; co0 += B1_CO) {
        __syncthreads();
        for (int i = tid; i < B1_CO * B1_PLANE; i += 256) {
            const int cc = i / B1_PLANE, r = i - cc * B1_PLANE, pr = r / B1_PW, pc = r - pr * B1_PW;
            const int oy = qy0 - 2 + pr, ox = qx0 - 2 + pc;
            patch[i] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? gi[(size_t)(co0 + cc) * oplane + (size_t)oy * Wo + ox] : 0.0f;
        }
        __syncthreads();
        const float* wc = wp + (size_t)(ry * 64 + co0) * B1_WCO;
#pragma unroll 2
        for (int cc = 0; cc < B1_CO; ++cc) {
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) {
                if (ty == 2 && ry == 3) continue;            // kernel row 11
                const float* pr = patch + cc * B1_PLANE + (ly + 2 - ty) * B1_PW + lx + 2;
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    const float gv = pr[-tx];
                    const float* wt = wc + cc * B1_WCO + (ty * 3 + tx) * 12;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int rx = 0; rx < 4; ++rx)
                            if (rx + 4 * tx < 11) acc[c * 4 + rx] = fmaf(wt[c * 4 + rx], gv, acc[c * 4 + rx]);
                }
            }
        }
    }
    const int iy = 4 * (qy0 + ly) + ry - 2, ix0 = 4 * (qx0 + lx) - 2;
    if (iy < 0 || iy >= H) return;
    float* dst = (d0 && d1) ? ((img & 1) ? d1 : d0) + (size_t)(img >> 1) * 3 * H * W : (d0 ? d0 : d1) + (size_t)img * 3 * H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sc = scale[c];
#pragma unroll
        for (int rx = 0; rx < 4; ++rx) {
            const int ix = ix0 + rx;
            if (ix < 0 || ix >= W) continue;
            const float v = __fdiv_rn(acc[c * 4 + rx], sc);
            dst[((size_t)c * H + iy) * W + ix] = normalize ? 2.0f * v : v;
        }
    }
}

}  // namespace

extern "C" int masic_lpips_dist_bwd(const float* f, const float* lin, const float* g_val, const float* g_res, const float* g_in, float* g_pre,
                                    int N, int C, int HW, int sides, void* stream) {
    MASIC_REQUIRE(f && lin && g_val && g_res && g_pre, MASIC_ERR_ARG, "lpips_dist_bwd: null pointer");
    MASIC_REQUIRE(N > 0 && N <= 65535 && C > 0 && HW > 0 && HW <= (1 << 30) && sides >= 1 && sides <= 3, MASIC_ERR_SHAPE,
                  "lpips_dist_bwd: N %d, C %d, %d pixels, sides %d", N, C, HW, sides);
    hipLaunchKernelGGL(lpips_dist_bwd_kernel, dim3(ceil_div(HW, DIST_PX), N), dim3(256), 0, (hipStream_t)stream, f, lin, g_val, g_res, g_in, g_pre,
                       C, HW, sides);
    return masic_launch_status("lpips_dist_bwd");
}

extern "C" int masic_maxpool3s2_bwd(const float* x, const float* gy, float* gx, int B, int C, int H, int W, int img_stride, int img_off,
                                    void* stream) {
    MASIC_REQUIRE(x && gy && gx, MASIC_ERR_ARG, "maxpool3s2_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && img_stride >= 1 && img_off >= 0 && img_off < img_stride, MASIC_ERR_SHAPE,
                  "maxpool3s2_bwd: %d x %d planes of %d x %d, image stride %d offset %d", B, C, H, W, img_stride, img_off);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int Hb = (H + 1) / 2, Wb = (W + 1) / 2;          // 2 x 2 input blocks, one per thread
    const size_t total = (size_t)B * C * Hb * Wb;
    MASIC_REQUIRE(total <= ((size_t)1 << 38), MASIC_ERR_SHAPE, "maxpool3s2_bwd: %zu input blocks", total);
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, gy, gx, C, H, W, Ho, Wo,
                       img_stride, img_off, Hb, Wb, total);
    return masic_launch_status("maxpool3s2_bwd");
}

extern "C" size_t masic_lpips_conv1_bwd_packed_bytes(void) { return (size_t)B1_PACKED * sizeof(float); }

extern "C" int masic_lpips_conv1_bwd_pack_weight(const float* w, float* w_packed, void* stream) {
    MASIC_REQUIRE(w && w_packed, MASIC_ERR_ARG, "lpips_conv1_bwd_pack_weight: null pointer");
    hipLaunchKernelGGL(lpips_conv1_bwd_pack_kernel, dim3(ceil_div(B1_PACKED, 256)), dim3(256), 0, (hipStream_t)stream, w, w_packed);
    return masic_launch_status("lpips_conv1_bwd_pack_weight");
}

extern "C" int masic_lpips_conv1_bwd(const float* g, const float* w_packed, const float* scale, float* d0, float* d1, int B, int H, int W,
                                     int normalize, void* stream) {
    MASIC_REQUIRE(g && w_packed && scale && (d0 || d1), MASIC_ERR_ARG, "lpips_conv1_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && B <= 65535 && !(d0 && d1 && (B & 1)) && H >= 11 && W >= 11 && (long)H * W <= (1L << 28), MASIC_ERR_SHAPE,
                  "lpips_conv1_bwd: %d images, %d x %d", B, H, W);
    const int Ho = (H - 7) / 4 + 1, Wo = (W - 7) / 4 + 1;
    const int Hq = (H + 1) / 4 + 1, Wq = (W + 1) / 4 + 1;          // phase-grid pixels that hold a picture pixel
    MASIC_REQUIRE(ceil_div(Hq, B1_TH) <= 65535, MASIC_ERR_SHAPE, "lpips_conv1_bwd: %d rows", H);
    hipLaunchKernelGGL(lpips_conv1_bwd_kernel, dim3(ceil_div(Wq, B1_TW), ceil_div(Hq, B1_TH), B), dim3(256), 0, (hipStream_t)stream, g, w_packed,
                       scale, d0, d1, H, W, Ho, Wo, normalize);
    return masic_launch_status("lpips_conv1_bwd");
}
