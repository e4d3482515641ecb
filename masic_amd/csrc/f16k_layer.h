// f16k_layer.h -- what the kernels that own one fixed 128 -> 128 5x5 stride-2 layer with a fused one-product (I)GDN share
// (deconv_igdn.hip, conv_s2_gdn.hip): on the device the block map, the buffer resources, the beta^ / bias copy into
// LDS, the accumulators' start from it and the ring-slot advance; on the host the shape limit of their extern "C" entry points.  The K
// loops and epilogues are each kernel's own.  Every piece here is text the two kernels held twice, and a piece lives here only where
// moving it leaves the kernels' code objects as they were (profiles/layer_kernels_codeobj.txt): conv_s2_gdn_f16k starts its accumulators
// in its own text, and the four-block F16K store loop stays in both files, because the shared form changed their code.
#pragma once
#include "f16k_device.h"

namespace {

constexpr int LAYER_OOB = 0x7ffffff0;                           // a buffer offset past every resource: the DMA writes zeros

// blockIdx.x, .z -> (tile, image): conv_f16k's maps -- with a multiple of 8 images, image 8 slot + k is walked tile by tile on XCD k
// (block ids go round-robin over the XCDs, gridDim.x is a multiple of 8), else tile = blockIdx.x, image = blockIdx.z.  The workgroups
// of a tile (blockIdx.y, where a kernel has more than one) are gridDim.x block ids apart: on one XCD and close in time, so their
// interleaved output pixels meet in one L2.  The caller returns where tile is past its last one (the grid is rounded up to the XCDs).
__device__ __forceinline__ void layer_block_map(int xcd_images, int& tile, int& b) {
    if (xcd_images) {
        const int idx = (blockIdx.x >> 3) + (gridDim.x >> 3) * blockIdx.z;
        const int slot = idx / (int)gridDim.x;
        tile = idx - slot * (int)gridDim.x;
        b = slot * 8 + (blockIdx.x & 7);
    } else {
        tile = blockIdx.x;
        b = blockIdx.z;
    }
}

// a raw buffer resource over `bytes` bytes at p: a DMA or load past its end returns zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t layer_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
}
constexpr int LAYER_GDN_BYTES = 65536 + 512;                    // gdn_pack_f16k_kernel's image: 64 KiB of gamma^ pieces, then beta^[128]

// beta^ (behind the gamma^ pieces of the packed GDN) and the bias (zeros without one) into their 512 B of LDS: threads 0 .. 127, in
// the prologue, in front of its barrier
__device__ __forceinline__ void layer_beta_bias_to_lds(float* beta_lds, float* bias_lds, const unsigned char* gdn, const float* bias, int tid) {
    if (tid < 128) {
        beta_lds[tid] = reinterpret_cast<const float*>(gdn + 65536)[tid];
        bias_lds[tid] = bias != nullptr ? bias[tid] : 0.0f;
    }
}

// The accumulators of a wave's NP pixel sub-tiles (all 128 output channels each: conv_f16k's layout: the GDN finds a pixel's channels in
// the wave's registers) start at the bias: from the LDS copy instead of 64 scalar loads per lane.  h: the lane's half (lane >> 5).
template <int NP>
__device__ __forceinline__ void layer_acc_from_bias(f32x16 (*acc)[4], const float* bias_lds, int h) {
    const float* bp = bias_lds + 4 * h;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bv = *reinterpret_cast<const float4*>(bp + m * 32 + 8 * q);
#pragma unroll
            for (int n = 0; n < NP; ++n) { acc[n][m][4 * q + 0] = bv.x; acc[n][m][4 * q + 1] = bv.y; acc[n][m][4 * q + 2] = bv.z; acc[n][m][4 * q + 3] = bv.w; }
        }
}

// the byte offset of the weight ring's slot after `slot`: NWS slots of WST bytes
template <int NWS, int WST>
__device__ __forceinline__ int layer_ring_next(int slot) { return slot + WST == NWS * WST ? 0 : slot + WST; }

// ---- host: the shapes the extern "C" entry points take
// 32-bit offsets: the larger of an image's input and output (bytes_per_input_pixel: 256 where it is the input, 4 x 256 for the output
// of a transposed layer) is one buffer resource; grid limits
inline bool layer_shape_ok(int B, int Hi, int Wi, int bytes_per_input_pixel) {
    return B >= 1 && B <= 65535 && Hi >= 1 && Wi >= 1 && (long long)Hi * Wi * bytes_per_input_pixel < (1ll << 31);
}

}  // namespace
