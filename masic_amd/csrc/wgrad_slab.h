// wgrad_slab.h -- the finishing pass of the deterministic weight gradients (conv_wgrad.hip, wgrad_f16k.hip).
#pragma once
#include "common.h"

// slabs [nsplit][T][AQ] -> dw [AQ][T], dw = slab 0 + slab 1 + ... in split order (float32); T = 1: the plain sum of [nsplit][AQ] slabs.
// Threads walk the slab layout (coalesced reads) and keep 8 slab loads in flight; the adds stay in split order.  Slab contents are
// left as they are (the deterministic workspace is irrelevant on entry and exit).
__global__ __launch_bounds__(256) static void wgrad_slab_transpose_kernel(const float* __restrict__ ws, float* __restrict__ dw, int T, int AQ, int nsplit) {
    const size_t total = (size_t)T * AQ;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i / AQ);
        const size_t aq = i - (size_t)t * AQ;
        const float* src = ws + i;
        float s = 0.0f;
        int z = 0;
        for (; z + 8 <= nsplit; z += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = src[(size_t)(z + k) * total];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; z < nsplit; ++z) s += src[(size_t)z * total];
        dw[aq * T + t] = s;
    }
}
