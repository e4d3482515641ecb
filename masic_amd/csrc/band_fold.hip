// band_fold.hip -- the row bands of a latent as a batch of images, and back (include/masic_bandfold.h; masic_amd/bandfold.py; DESIGN.md
// section 8.1 "Row bands in the model").
//
//   fold     float32 NCHW [B, C, h, w] -> [B T, C, S, w], T = ceil(h / S); the rows a short last band lacks are written as +0.0
//   unfold   [B T, C, S, w] -> [B, C, h, w] (padding rows dropped), optionally * gate[b, gate_c], into a channel slice of a float32 NCHW
//            buffer or of an F16K one
//
// Pure data movement at latent resolution.  A band of a (b, c) plane is ONE contiguous run of min(S, h - t S) w floats on both sides, and
// a vector of V floats never straddles a band when V divides S w and h w: the float32 kernels move V = 4 floats (16 bytes) per lane where
// the shape and the bases allow it, V = 2 where only that holds (w = 2 (mod 4) with odd S), single floats otherwise (odd w).  Consecutive
// lanes take consecutive vectors of the destination, whose source addresses are consecutive within a run.  The F16K form takes
// nchw_to_f16k_view_kernel's shape: one lane per (pixel, 8-channel half record), 8 loads each coalesced across the lanes' pixels, one
// 16-byte store.  No atomics, no shared memory, nothing read by the host: capturable, and the same bits every run.
#include "common.h"
#include "masic_bandfold.h"

namespace {

constexpr int MAX_BLOCKS = 1024;          // of 256 lanes; the lanes loop past it (masic_bandfold_max_blocks)

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<2> { typedef float2 T; };
template <> struct Vec<4> { typedef float4 T; };

__device__ __forceinline__ float zero_of(float) { return 0.0f; }
__device__ __forceinline__ float2 zero_of(float2) { return make_float2(0.0f, 0.0f); }
__device__ __forceinline__ float4 zero_of(float4) { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float mul(float a, float g) { return a * g; }
__device__ __forceinline__ float2 mul(float2 a, float2 g) { return make_float2(a.x * g.x, a.y * g.y); }
__device__ __forceinline__ float4 mul(float4 a, float4 g) { return make_float4(a.x * g.x, a.y * g.y, a.z * g.z, a.w * g.w); }

// one lane per vector of dst; run = S w / V vectors of one (image, channel) plane of dst, plane = h w / V vectors of one of src
template <int V>
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t total, int C, int T, int h, int w,
                                                   int S, int run, int plane) {
    typedef typename Vec<V>::T vec;
    const vec* s = reinterpret_cast<const vec*>(src);
    vec* d = reinterpret_cast<vec*>(dst);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)run;                  // (b T + t) C + c
        const int k = (int)(i - r * (size_t)run);
        const size_t bt = r / (size_t)C;
        const int c = (int)(r - bt * (size_t)C);
        const size_t b = bt / (size_t)T;
        const int t = (int)(bt - b * (size_t)T);
        const int rows = min(S, h - t * S);
        const int valid = rows * w / V;                    // vectors of the band that exist in src
        d[i] = k < valid ? s[(b * (size_t)C + c) * (size_t)plane + (size_t)t * run + k] : zero_of(vec());
    }
}

// one lane per vector of the C h w values of dst's slice
template <int V, bool GATE>
__global__ __launch_bounds__(256) void unfold_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ gate,
                                                     size_t total, int C, int T, int run, int plane, int dst_ctot, int dst_coff, int gate_ctot,
                                                     int gate_c) {
    typedef typename Vec<V>::T vec;
    const vec* s = reinterpret_cast<const vec*>(src);
    const vec* g = reinterpret_cast<const vec*>(gate);
    vec* d = reinterpret_cast<vec*>(dst);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t p = i / (size_t)plane;                // b C + c
        const int e = (int)(i - p * (size_t)plane);        // vector of the plane
        const size_t b = p / (size_t)C;
        const int c = (int)(p - b * (size_t)C);
        const int t = e / run, k = e - t * run;
        vec v = s[((b * (size_t)T + t) * (size_t)C + c) * (size_t)run + k];
        if (GATE) v = mul(v, g[(b * (size_t)gate_ctot + gate_c) * (size_t)plane + e]);
        d[(b * (size_t)dst_ctot + dst_coff + c) * (size_t)plane + e] = v;
    }
}

__device__ __forceinline__ unsigned pack2(float lo, float hi) {          // f16k_ops.hip's
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// nchw_to_f16k_view_kernel with the source read through the band map: lane = (pixel p, half record c8) of picture blockIdx.z
__global__ __launch_bounds__(256) void unfold_f16k_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, const float* __restrict__ gate,
                                                          int C, int T, int HW, int SW, int dst_ctot, int dst_coff, int gate_ctot, int gate_c) {
    const int b = blockIdx.z, c8 = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int t = p / SW, k = p - t * SW;
    const float* xb = src + (((size_t)b * T + t) * C) * SW + k;
    const float gv = gate != nullptr ? gate[((size_t)b * gate_ctot + gate_c) * HW + p] : 1.0f;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = c8 * 8 + i;
        v[i] = c < C ? xb[(size_t)c * SW] * gv : 0.0f;
    }
    uint4 q;
    q.x = pack2(v[0], v[1]); q.y = pack2(v[2], v[3]); q.z = pack2(v[4], v[5]); q.w = pack2(v[6], v[7]);
    const int dc8 = (dst_coff >> 3) + c8;
    reinterpret_cast<uint4*>(dst + (((size_t)b * (dst_ctot >> 4) + (dc8 >> 1)) * HW) * 16)[2 * (size_t)p + (dc8 & 1)] = q;
}

// the widest vector that divides both a band's run and a plane and at which every base is aligned
int vector_width(int h, int w, int S, const void* a, const void* b, const void* c) {
    const size_t sw = (size_t)S * w, hw = (size_t)h * w;
    const uintptr_t bases = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
    if (sw % 4 == 0 && hw % 4 == 0 && (bases & 15) == 0) return 4;
    if (sw % 2 == 0 && hw % 2 == 0 && (bases & 7) == 0) return 2;
    return 1;
}

unsigned blocks_of(size_t total) {
    const size_t nb = (total + 255) / 256;
    return nb > (size_t)MAX_BLOCKS ? (unsigned)MAX_BLOCKS : (unsigned)nb;
}

int check_shape(const char* who, int B, int C, int h, int w, int S) {
    MASIC_REQUIRE(B >= 1 && C >= 1 && h >= 1 && w >= 1, MASIC_ERR_ARG, "%s: B, C, h, w = %d, %d, %d, %d must be positive", who, B, C, h, w);
    MASIC_REQUIRE(S >= 1, MASIC_ERR_ARG, "%s: band_rows = %d must be at least 1", who, S);
    // a plane and a folded image are indexed with int
    MASIC_REQUIRE((size_t)h * w < ((size_t)1 << 30) && (size_t)S * w < ((size_t)1 << 30), MASIC_ERR_ARG, "%s: h w or S w does not fit", who);
    return MASIC_OK;
}

int check_gate(const char* who, const float* gate, int gate_ctot, int gate_c) {
    MASIC_REQUIRE(gate == nullptr || (gate_c >= 0 && gate_c < gate_ctot), MASIC_ERR_SHAPE, "%s: gate channel %d outside 0 .. %d", who, gate_c, gate_ctot - 1);
    return MASIC_OK;
}

}  // namespace

extern "C" int masic_bandfold_max_blocks(void) { return MAX_BLOCKS; }

extern "C" int masic_bandfold_fold(const float* src, float* dst, int B, int C, int h, int w, int S, void* stream) {
    MASIC_REQUIRE(src && dst, MASIC_ERR_ARG, "bandfold_fold: null pointer");
    if (int rc = check_shape("bandfold_fold", B, C, h, w, S)) return rc;
    const int T = ceil_div(h, S);
    const int V = vector_width(h, w, S, src, dst, nullptr);
    const int run = (int)((size_t)S * w / V), plane = (int)((size_t)h * w / V);
    const size_t total = (size_t)B * T * C * run;
    const dim3 grid(blocks_of(total));
    hipStream_t st = (hipStream_t)stream;
    if (V == 4) hipLaunchKernelGGL(fold_kernel<4>, grid, dim3(256), 0, st, src, dst, total, C, T, h, w, S, run, plane);
    else if (V == 2) hipLaunchKernelGGL(fold_kernel<2>, grid, dim3(256), 0, st, src, dst, total, C, T, h, w, S, run, plane);
    else hipLaunchKernelGGL(fold_kernel<1>, grid, dim3(256), 0, st, src, dst, total, C, T, h, w, S, run, plane);
    return masic_launch_status("bandfold_fold");
}

extern "C" int masic_bandfold_unfold(const float* src, float* dst, int B, int C, int h, int w, int S, int dst_ctot, int dst_coff,
                                     const float* gate, int gate_ctot, int gate_c, void* stream) {
    MASIC_REQUIRE(src && dst, MASIC_ERR_ARG, "bandfold_unfold: null pointer");
    if (int rc = check_shape("bandfold_unfold", B, C, h, w, S)) return rc;
    MASIC_REQUIRE(dst_coff >= 0 && dst_coff <= dst_ctot - C, MASIC_ERR_SHAPE, "bandfold_unfold: channels [%d, %d) outside a buffer of %d", dst_coff,
                  dst_coff + C, dst_ctot);
    if (int rc = check_gate("bandfold_unfold", gate, gate_ctot, gate_c)) return rc;
    const int T = ceil_div(h, S);
    const int V = vector_width(h, w, S, src, dst, gate);
    const int run = (int)((size_t)S * w / V), plane = (int)((size_t)h * w / V);
    const size_t total = (size_t)B * C * plane;
    const dim3 grid(blocks_of(total));
    hipStream_t st = (hipStream_t)stream;
#define MASIC_UNFOLD(VV, GG) \
    hipLaunchKernelGGL((unfold_kernel<VV, GG>), grid, dim3(256), 0, st, src, dst, gate, total, C, T, run, plane, dst_ctot, dst_coff, gate_ctot, gate_c)
    if (gate) { if (V == 4) MASIC_UNFOLD(4, true); else if (V == 2) MASIC_UNFOLD(2, true); else MASIC_UNFOLD(1, true); }
    else { if (V == 4) MASIC_UNFOLD(4, false); else if (V == 2) MASIC_UNFOLD(2, false); else MASIC_UNFOLD(1, false); }
#undef MASIC_UNFOLD
    return masic_launch_status("bandfold_unfold");
}

extern "C" int masic_bandfold_unfold_f16k(const float* src, void* dst, int B, int C, int h, int w, int S, int dst_ctot, int dst_coff,
                                          const float* gate, int gate_ctot, int gate_c, void* stream) {
    MASIC_REQUIRE(src && dst, MASIC_ERR_ARG, "bandfold_unfold_f16k: null pointer");
    if (int rc = check_shape("bandfold_unfold_f16k", B, C, h, w, S)) return rc;
    MASIC_REQUIRE(dst_ctot % 16 == 0 && dst_coff % 16 == 0 && dst_coff >= 0 && dst_coff <= dst_ctot - C, MASIC_ERR_SHAPE,
                  "bandfold_unfold_f16k: channels [%d, %d) misaligned or outside a buffer of %d", dst_coff, dst_coff + C, dst_ctot);
    if (int rc = check_gate("bandfold_unfold_f16k", gate, gate_ctot, gate_c)) return rc;
    MASIC_REQUIRE(B <= 65535 && ceil_div(C, 8) <= 65535, MASIC_ERR_ARG, "bandfold_unfold_f16k: B = %d or C = %d exceeds the grid", B, C);
    const int T = ceil_div(h, S), HW = h * w;
    // a lane past a band's S w values of a short last band does not exist: p < HW, and p / SW < T with k inside the rows src holds
    hipLaunchKernelGGL(unfold_f16k_kernel, dim3(ceil_div(HW, 256), ceil_div(C, 8), B), dim3(256), 0, (hipStream_t)stream, src,
                       (unsigned short*)dst, gate, C, T, HW, S * w, dst_ctot, dst_coff, gate_ctot, gate_c);
    return masic_launch_status("bandfold_unfold_f16k");
}
