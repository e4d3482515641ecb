// metrics.hip -- per-pair reductions of the test-split evaluation (include/masic_metrics.h; masic_amd/metrics.py).
//
// masic_rd_loss, masic_sse and masic_sum_log (misc.hip) return one value per BATCH.  An evaluation averages per-PAIR values -- the mean
// of per-pair PSNRs is not the PSNR of the mean MSE -- so these take a batch and return one row per pair:
//   pair_rd : the two squared errors and up to four sums of log-likelihoods of every image, in float64, each bit for bit what masic_sse /
//             masic_sum_log return for the image's slice alone;
//   u8_sse  : exact integer sums of squared byte differences of decoded 8-bit pictures against the originals.
// Both are a stage over blocks and a finishing launch; there are no atomics.
#include "common.h"
#include "masic_metrics.h"

namespace {

// ---- pair_rd.  RED_BLOCKS and grid_for are misc.hip's: the partition of a slice into blocks is part of the value.
constexpr int RED_BLOCKS = 1024;
constexpr int MAX_IMAGES = 65535;               // the image is gridDim.z (pair_rd) / gridDim.y (u8_sse)

int grid_for(size_t total, int cap) {
    size_t g = (total + 255) / 256;
    return (int)(g > (size_t)cap ? cap : (g == 0 ? 1 : g));
}

struct PairRdArgs {
    const float* a[6]; const float* b[6];      // tensors 0, 1: (x_hat, x) of the squared errors; 2..: likelihood tensors (b unused)
    unsigned long long n[6];                   // elements per image
    int g[6];                                   // stage-1 blocks per image of tensor t: grid_for(n[t], RED_BLOCKS)
    int nt;
};

// grid (max_t g[t], nt, B): block (x, t, img) is block x of reduce_stage1 run on image img's slice of tensor t
__global__ __launch_bounds__(256) void pair_rd_stage1(const PairRdArgs r, double* __restrict__ partial) {
    const int t = blockIdx.y, img = blockIdx.z;
    if ((int)blockIdx.x >= r.g[t]) return;
    __shared__ double red[256];
    const size_t n = r.n[t], stride = (size_t)r.g[t] * 256;
    const float* a = r.a[t] + (size_t)img * n;
    const float* b = t < 2 ? r.b[t] + (size_t)img * n : nullptr;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        if (t >= 2) acc += (double)logf(a[i]);
        else { const float d = a[i] - b[i]; acc += (double)(d * d); }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[((size_t)img * 6 + t) * RED_BLOCKS + blockIdx.x] = red[0];
}

// grid (6, B): block (t, img) is reduce_stage2 over the g[t] partials of (img, t); absent tensors give 0
__global__ __launch_bounds__(256) void pair_rd_finish(const PairRdArgs r, const double* __restrict__ partial, double* __restrict__ out) {
    const int t = blockIdx.x, img = blockIdx.y;
    if (t >= r.nt) {
        if (threadIdx.x == 0) out[(size_t)img * 6 + t] = 0.0;
        return;
    }
    __shared__ double red[256];
    const double* p = partial + ((size_t)img * 6 + t) * RED_BLOCKS;
    double acc = 0.0;
    for (int i = threadIdx.x; i < r.g[t]; i += 256) acc += p[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)img * 6 + t] = red[0];
}

// ---- u8_sse
constexpr int U8_BLOCKS = 256;                  // stage-1 blocks per picture at most
constexpr int U8_PIECE = 16;                    // bytes a lane reads at once

__device__ __forceinline__ unsigned sq_diff4(unsigned x, unsigned y) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((x >> k) & 255u) - (int)((y >> k) & 255u);
        s += (unsigned)(d * d);
    }
    return s;
}

// grid (g, P).  Picture p's bytes [0, n) are split into a head of single bytes up to a's next 16-byte boundary, nvec 16-byte pieces and
// a tail of single bytes; where b is not aligned as a is, the head is the whole picture.  A piece adds at most 16 * 255^2 < 2^21 to a
// lane's uint64 sum.
__global__ __launch_bounds__(256) void u8_sse_stage1(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t n,
                                                     unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long red[256];
    const uint8_t* pa = a + (size_t)blockIdx.y * n;
    const uint8_t* pb = b + (size_t)blockIdx.y * n;
    size_t head = (size_t)((U8_PIECE - ((uintptr_t)pa & (U8_PIECE - 1))) & (U8_PIECE - 1));
    if (head > n || (((uintptr_t)pb + head) & (U8_PIECE - 1)) != 0) head = n;
    const size_t nvec = (n - head) / U8_PIECE, tail0 = head + nvec * U8_PIECE;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    unsigned long long acc = 0;
    const uint4* va = reinterpret_cast<const uint4*>(pa + head);
    const uint4* vb = reinterpret_cast<const uint4*>(pb + head);
    for (size_t i = first; i < nvec; i += stride) {
        const uint4 x = va[i], y = vb[i];
        acc += sq_diff4(x.x, y.x) + sq_diff4(x.y, y.y) + sq_diff4(x.z, y.z) + sq_diff4(x.w, y.w);
    }
    for (size_t i = first; i < head; i += stride) {
        const int d = (int)pa[i] - (int)pb[i];
        acc += (unsigned)(d * d);
    }
    for (size_t i = tail0 + first; i < n; i += stride) {
        const int d = (int)pa[i] - (int)pb[i];
        acc += (unsigned)(d * d);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * U8_BLOCKS + blockIdx.x] = red[0];
}

// grid (P): U8_BLOCKS == the block's 256 lanes, one partial per lane
__global__ __launch_bounds__(256) void u8_sse_finish(const unsigned long long* __restrict__ partial, int g, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[256];
    red[threadIdx.x] = (int)threadIdx.x < g ? partial[(size_t)blockIdx.x * U8_BLOCKS + threadIdx.x] : 0ull;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}
static_assert(U8_BLOCKS <= 256, "u8_sse_finish reads one partial per lane");

}  // namespace

extern "C" size_t masic_metrics_pair_rd_workspace_bytes(int B) {
    return B >= 1 && B <= MAX_IMAGES ? (size_t)B * 6 * RED_BLOCKS * sizeof(double) : 0;
}

extern "C" int masic_metrics_pair_rd(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                                     const float* const* liks, const size_t* lik_n, int nliks, int B, double* out, void* workspace,
                                     void* stream) {
    MASIC_REQUIRE(x1_hat && x1 && x2_hat && x2 && out && workspace, MASIC_ERR_ARG, "metrics_pair_rd: null pointer");
    MASIC_REQUIRE(nliks >= 0 && nliks <= 4 && (nliks == 0 || (liks && lik_n)), MASIC_ERR_ARG, "metrics_pair_rd: 0..4 likelihood tensors");
    MASIC_REQUIRE(B >= 1 && B <= MAX_IMAGES, MASIC_ERR_ARG, "metrics_pair_rd: B = %d outside 1 .. %d", B, MAX_IMAGES);
    PairRdArgs r{};
    r.a[0] = x1_hat; r.b[0] = x1; r.a[1] = x2_hat; r.b[1] = x2;
    r.n[0] = r.n[1] = n_pic;
    for (int k = 0; k < nliks; ++k) {
        MASIC_REQUIRE(liks[k], MASIC_ERR_ARG, "metrics_pair_rd: null likelihood tensor");
        r.a[2 + k] = liks[k]; r.b[2 + k] = nullptr; r.n[2 + k] = lik_n[k];
    }
    r.nt = 2 + nliks;
    int gmax = 1;
    for (int t = 0; t < r.nt; ++t) { r.g[t] = grid_for(r.n[t], RED_BLOCKS); gmax = r.g[t] > gmax ? r.g[t] : gmax; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pair_rd_stage1, dim3(gmax, r.nt, B), dim3(256), 0, st, r, (double*)workspace);
    hipLaunchKernelGGL(pair_rd_finish, dim3(6, B), dim3(256), 0, st, r, (const double*)workspace, out);
    return masic_launch_status("metrics_pair_rd");
}

extern "C" size_t masic_metrics_u8_sse_workspace_bytes(int P) {
    return P >= 1 && P <= MAX_IMAGES ? (size_t)P * U8_BLOCKS * sizeof(unsigned long long) : 0;
}

extern "C" int masic_metrics_u8_sse(const uint8_t* a, const uint8_t* b, size_t n, int P, uint64_t* out, void* workspace, void* stream) {
    MASIC_REQUIRE(a && b && out && workspace, MASIC_ERR_ARG, "metrics_u8_sse: null pointer");
    MASIC_REQUIRE(n >= 1, MASIC_ERR_ARG, "metrics_u8_sse: empty pictures");
    MASIC_REQUIRE(P >= 1 && P <= MAX_IMAGES, MASIC_ERR_ARG, "metrics_u8_sse: P = %d outside 1 .. %d", P, MAX_IMAGES);
    const int g = grid_for((n + U8_PIECE - 1) / U8_PIECE, U8_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(u8_sse_stage1, dim3(g, P), dim3(256), 0, st, a, b, n, (unsigned long long*)workspace);
    hipLaunchKernelGGL(u8_sse_finish, dim3(P), dim3(256), 0, st, (const unsigned long long*)workspace, g, (unsigned long long*)out);
    return masic_launch_status("metrics_u8_sse");
}
