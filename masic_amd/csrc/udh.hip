// udh.hip -- the layers of the UDH homography net (coremasic/mywork/model.py: Net) that the codec's convolution path does not
// already cover.  The net turns two grey p x p patches into the four corner offsets that masic_homography_from_corners makes
// h_matrix of; its matrix decides the warp masks, so every kernel here is float32 with a fixed accumulation order (no float
// atomics: DESIGN.md section 6) and a result row never depends on which other rows share the launch.
//
//   udh_conv1     Conv2d(2 -> 64, k3, p1) + bias + ReLU read from the two patch tensors (the torch.cat of model.py:94 never
//                 happens).  K = 18: one thread per pixel, 16 output channels per workgroup, the 288 weights of those channels
//                 in LDS (broadcast reads), an 18-step fmaf chain per output.
//   udh_maxpool2  MaxPool2d(2, 2) on NCHW planes, one output per lane from two 8-byte loads.
//   udh_fc1       relu(x[B,K] . W1^T + b1) -> [B,N] as pure weight streaming: W1 (134 MB at p = 128) is read once per group of
//                 <= 8 batch rows with 16-byte loads coalesced along K; a lane keeps its share of the group's activation rows of
//                 the workgroup's K chunk in registers.  K is split across workgroups (512 per chunk); each writes its partial sums and udh_fc_finish adds
//                 them in chunk order, then applies bias + ReLU and the N -> M second linear layer (M = 8).
// Layers 2-8 of the net are the float32 implicit-GEMM convolution of conv.hip (masic_conv2d_fwd_ex, MASIC_ACT_RELU).
#include "common.h"

namespace {

constexpr int C1_CO = 16;              // output channels per workgroup of the first layer

__global__ __launch_bounds__(256) void udh_conv1_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int H, int W, int Cout) {
    __shared__ __attribute__((aligned(16))) float ws[18 * C1_CO];      // [ci*9 + tap][co]
    __shared__ float bs[C1_CO];
    const int co0 = blockIdx.y * C1_CO, img = blockIdx.z;
    for (int i = threadIdx.x; i < 18 * C1_CO; i += 256) {
        const int t = i / C1_CO, o = i - t * C1_CO;
        ws[i] = w[(size_t)(co0 + o) * 18 + t];
    }
    if (threadIdx.x < C1_CO) bs[threadIdx.x] = bias[co0 + threadIdx.x];
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int r = pix / W, c = pix - r * W;
    const size_t plane = (size_t)H * W;
    const float* src[2] = {a + (size_t)img * plane, b + (size_t)img * plane};
    float v[18];
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
    float acc[C1_CO];
#pragma unroll
    for (int o = 0; o < C1_CO; ++o) acc[o] = 0.0f;
#pragma unroll
    for (int t = 0; t < 18; ++t) {
        const float4* wt = reinterpret_cast<const float4*>(ws + t * C1_CO);
#pragma unroll
        for (int q = 0; q < C1_CO / 4; ++q) {
            const float4 w4 = wt[q];
            acc[4 * q + 0] = fmaf(v[t], w4.x, acc[4 * q + 0]);
            acc[4 * q + 1] = fmaf(v[t], w4.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(v[t], w4.z, acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(v[t], w4.w, acc[4 * q + 3]);
        }
    }
    float* yo = y + ((size_t)img * Cout + co0) * plane + pix;
#pragma unroll
    for (int o = 0; o < C1_CO; ++o) yo[(size_t)o * plane] = fmaxf(acc[o] + bs[o], 0.0f);
}

// torch's max_pool2d propagates NaN; so does this
__device__ __forceinline__ float max_nan(float m, float u) { return (u > m || u != u) ? u : m; }

__global__ __launch_bounds__(256) void udh_maxpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int Ho, int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / Wo;                         // plane * Ho + r
    const int c = (int)(i - row * Wo);
    const float2* p = reinterpret_cast<const float2*>(x + row * 2 * (size_t)(2 * Wo)) + c;
    const float2 t = p[0], u = p[Wo];
    y[i] = max_nan(max_nan(max_nan(t.x, t.y), u.x), u.y);
}

// ---- linear 1: weight streaming
constexpr int FC_KCH = 512;            // K per workgroup: a lane keeps its 2 x 4 floats of each of the 8 activation rows in registers
constexpr int FC_NWG = 128;            // neurons per workgroup: 4 waves x 8 rounds x FC_NT
constexpr int FC_NT = 4;               // neurons a wave streams at once (8 loads of 16 bytes in flight per lane)
constexpr int FC_ROWS = 8;             // batch rows per weight pass
constexpr int FC_ST = FC_KCH / 256;    // 16-byte loads per lane and weight row

// One step of the transposing butterfly: the lanes of a pair (lane, lane ^ M) hold 2 * HALF values each; the lane with bit M clear
// keeps the lower HALF, the other the upper HALF, and each adds its partner's copy of what it keeps.
template <int HALF, int M>
__device__ __forceinline__ void fold(float (&v)[32], int lane) {
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = up ? v[i + HALF] : v[i];
        const float send = up ? v[i] : v[i + HALF];
        v[i] = keep + __shfl_xor(send, M, 64);
    }
}

__global__ __launch_bounds__(256) void udh_fc1_partial_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                              int B, int K, int N) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, b0 = blockIdx.z * FC_ROWS;
    const int rows = B - b0 < FC_ROWS ? B - b0 : FC_ROWS;
    const size_t k0 = (size_t)s * FC_KCH + lane * 4;
    float4 xv[FC_ST][FC_ROWS];                          // rows past the batch are zeros: their sums are computed and never stored
#pragma unroll
    for (int st = 0; st < FC_ST; ++st)
#pragma unroll
        for (int r = 0; r < FC_ROWS; ++r) {
            xv[st][r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < rows) xv[st][r] = *reinterpret_cast<const float4*>(x + (size_t)(b0 + r) * K + k0 + st * 256);
        }
#pragma unroll 1
    for (int it = 0; it < FC_NWG / (4 * FC_NT); ++it) {
        const int n0 = blockIdx.y * FC_NWG + wave * (FC_NWG / 4) + it * FC_NT;
        const float* wp = w + (size_t)n0 * K + k0;
        float4 wv[FC_ST][FC_NT];
#pragma unroll
        for (int st = 0; st < FC_ST; ++st)
#pragma unroll
            for (int nt = 0; nt < FC_NT; ++nt) wv[st][nt] = *reinterpret_cast<const float4*>(wp + (size_t)nt * K + st * 256);
        float v[32];                                    // [nt][row]
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = 0.0f;
#pragma unroll
        for (int st = 0; st < FC_ST; ++st)
#pragma unroll
            for (int nt = 0; nt < FC_NT; ++nt)
#pragma unroll
                for (int r = 0; r < FC_ROWS; ++r) {
                    float acc = v[nt * FC_ROWS + r];
                    acc = fmaf(wv[st][nt].x, xv[st][r].x, acc);
                    acc = fmaf(wv[st][nt].y, xv[st][r].y, acc);
                    acc = fmaf(wv[st][nt].z, xv[st][r].z, acc);
                    acc = fmaf(wv[st][nt].w, xv[st][r].w, acc);
                    v[nt * FC_ROWS + r] = acc;
                }
        // 32 sums per lane -> one per lane pair: value index (nt * 8 + row) = lane >> 1, summed over the 64 lanes in a fixed tree
        fold<16, 32>(v, lane);
        fold<8, 16>(v, lane);
        fold<4, 8>(v, lane);
        fold<2, 4>(v, lane);
        fold<1, 2>(v, lane);
        const float sum = v[0] + __shfl_xor(v[0], 1, 64);
        const int idx = lane >> 1, nt = idx >> 3, r = idx & 7;
        if ((lane & 1) == 0 && r < rows) part[((size_t)s * B + b0 + r) * N + n0 + nt] = sum;
    }
}

// hidden[b][n] = relu(sum_s part[s][b][n] + b1[n]) (chunk order), out[b][j] = sum_n hidden[b][n] * w2[j][n] + b2[j]
__global__ __launch_bounds__(1024) void udh_fc_finish_kernel(const float* __restrict__ part, const float* __restrict__ b1, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ hidden, float* __restrict__ out,
                                                             int B, int S, int N, int M) {
    extern __shared__ float hs[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int n = tid; n < N; n += 1024) {
        float acc = 0.0f;
        for (int s = 0; s < S; ++s) acc += part[((size_t)s * B + b) * N + n];
        const float h = fmaxf(acc + b1[n], 0.0f);
        hs[n] = h;
        if (hidden != nullptr) hidden[(size_t)b * N + n] = h;
    }
    __syncthreads();
    for (int j = wave; j < M; j += 16) {
        float acc = 0.0f;
        for (int n = lane; n < N; n += 64) acc = fmaf(hs[n], w2[(size_t)j * N + n], acc);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) out[(size_t)b * M + j] = acc + b2[j];
    }
}

__global__ void udh_shift_corners_kernel(const float* __restrict__ c, float* __restrict__ y, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = c[i] - c[(i >> 3) * 8 + (i & 1)];
}

}  // namespace

extern "C" int masic_udh_conv1_fwd(const float* a, const float* b, const float* w, const float* bias, float* y, int B, int H, int W, int Cout,
                                   void* stream) {
    MASIC_REQUIRE(a && b && w && bias && y, MASIC_ERR_ARG, "udh_conv1_fwd: null pointer");
    MASIC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W <= (1L << 30), MASIC_ERR_SHAPE, "udh_conv1_fwd: B %d, %d x %d", B, H, W);
    MASIC_REQUIRE(Cout > 0 && Cout % C1_CO == 0, MASIC_ERR_SHAPE, "udh_conv1_fwd: Cout %d is not a multiple of %d", Cout, C1_CO);
    hipLaunchKernelGGL(udh_conv1_kernel, dim3(ceil_div(H * W, 256), Cout / C1_CO, B), dim3(256), 0, (hipStream_t)stream, a, b, w, bias, y, H, W, Cout);
    return masic_launch_status("udh_conv1_fwd");
}

extern "C" int masic_maxpool2_fwd(const float* x, float* y, int planes, int H, int W, void* stream) {
    MASIC_REQUIRE(x && y, MASIC_ERR_ARG, "maxpool2_fwd: null pointer");
    MASIC_REQUIRE(planes > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, MASIC_ERR_SHAPE, "maxpool2_fwd: %d planes of %d x %d (even sizes only)", planes, H, W);
    MASIC_REQUIRE(((size_t)x & 7) == 0, MASIC_ERR_ARG, "maxpool2_fwd: input not 8-byte aligned");
    const size_t total = (size_t)planes * (H / 2) * (W / 2);
    MASIC_REQUIRE(total <= ((size_t)1 << 38), MASIC_ERR_SHAPE, "maxpool2_fwd: %zu outputs", total);
    hipLaunchKernelGGL(udh_maxpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, H / 2, W / 2, total);
    return masic_launch_status("maxpool2_fwd");
}

extern "C" size_t masic_udh_fc_workspace_bytes(int B, int K, int N) {
    if (B <= 0 || K <= 0 || N <= 0 || K % FC_KCH != 0) return 0;
    return (size_t)(K / FC_KCH) * B * N * sizeof(float);
}

extern "C" int masic_udh_fc_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, void* workspace,
                                float* hidden, float* out, int B, int K, int N, int M, void* stream) {
    MASIC_REQUIRE(x && w1 && b1 && w2 && b2 && workspace && out, MASIC_ERR_ARG, "udh_fc_fwd: null pointer");
    MASIC_REQUIRE(B > 0 && ceil_div(B, FC_ROWS) <= 65535, MASIC_ERR_SHAPE, "udh_fc_fwd: B %d", B);
    MASIC_REQUIRE(K > 0 && K % FC_KCH == 0, MASIC_ERR_SHAPE, "udh_fc_fwd: K %d is not a multiple of %d", K, FC_KCH);
    MASIC_REQUIRE(N > 0 && N % FC_NWG == 0 && N / FC_NWG <= 65535 && N <= 8192, MASIC_ERR_SHAPE, "udh_fc_fwd: N %d (multiples of %d up to 8192)", N, FC_NWG);
    MASIC_REQUIRE(M > 0 && M <= 4096, MASIC_ERR_SHAPE, "udh_fc_fwd: M %d", M);
    MASIC_REQUIRE((((size_t)x | (size_t)w1) & 15) == 0, MASIC_ERR_ARG, "udh_fc_fwd: x and w1 must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int S = K / FC_KCH;
    hipLaunchKernelGGL(udh_fc1_partial_kernel, dim3(S, N / FC_NWG, ceil_div(B, FC_ROWS)), dim3(256), 0, st, x, w1, (float*)workspace, B, K, N);
    hipLaunchKernelGGL(udh_fc_finish_kernel, dim3(B), dim3(1024), (size_t)N * sizeof(float), st, (const float*)workspace, b1, w2, b2, hidden, out,
                       B, S, N, M);
    return masic_launch_status("udh_fc_fwd");
}

extern "C" int masic_udh_shift_corners(const float* corners, float* out, int B, void* stream) {
    MASIC_REQUIRE(corners && out, MASIC_ERR_ARG, "udh_shift_corners: null pointer");
    MASIC_REQUIRE(B > 0 && B <= (1 << 27), MASIC_ERR_SHAPE, "udh_shift_corners: B %d", B);
    hipLaunchKernelGGL(udh_shift_corners_kernel, dim3(ceil_div(B * 8, 256)), dim3(256), 0, (hipStream_t)stream, corners, out, B * 8);
    return masic_launch_status("udh_shift_corners");
}
