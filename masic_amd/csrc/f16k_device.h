// f16k_device.h -- device helpers the F16K kernel families share (conv_f16k.hip, conv_a.hip, gemm_f16k.hip, conv3x3_resident.hip; the
// typedefs, static_for and pack2bf also serve skinny.hip, wgrad_f16k.hip, gemm_bf16.hip, conv.hip and gdn_bwd.hip): vector typedefs, LDS reads
// and counted waits the compiler does not see, the fp8 MFMA, bf16 / fp8 packing, the LDS swizzle, the F16K / F8K tile epilogues, the
// buffer -> LDS DMA and the (inverse) GDN on accumulators.  A helper that one family alone uses stays in that family's file.
#pragma once
#include "common.h"
#include <type_traits>

// host side: the diagnostics buffer of masic_conv_f16k_set_stamps (defined beside it in conv_f16k.hip), which the launchers of conv_f16k
// and of the first analysis layer (conv_a.hip) hand to their kernels
extern __attribute__((visibility("hidden"))) unsigned long long* g_f16k_stamps;

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// LDS reads / waits the compiler does not see (see the K loop of conv_f16k)
template <int OFF>
__device__ __forceinline__ void ds_read128(v4u& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c, v4u& d, v4u& e) {
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c, v4u& d, v4u& e, v4u& f) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c, v4u& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c, v4u& d, v4u& e, v4u& f, v4u& g, v4u& h) {
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait(v4u& a, v4u& b, v4u& c, v4u& d, v4u& e, v4u& f, v4u& g, v4u& h, v4u& i, v4u& j) {
    asm volatile("s_waitcnt lgkmcnt(%10)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j) : "n"(N) : "memory");
}

// ---- fp8 (OCP e4m3fn) operands: v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (E8M0 127) = a plain fp8 MFMA at
// twice the bf16 rate (MI355X_MICROARCH.md, Matrix cores).  A lane's operand is 32 consecutive k (two ds_read_b128 that the
// register coalescer places in one 8-register tuple); lanes 0-31 / 32-63 hold the two 32-k halves of the instruction's K = 64.
typedef int v8i __attribute__((ext_vector_type(8)));
__device__ __forceinline__ v8i cat8(const v4u& lo, const v4u& hi) {
    return __builtin_bit_cast(v8i, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ f32x16 mfma_f8(const v8i& a, const v8i& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
__device__ __forceinline__ unsigned pack4f8(float a, float b, float c, float d, float inv) {
    // saturating: e4m3fn has no infinity, its largest finite value is 448
    a = __builtin_amdgcn_fmed3f(a * inv, -448.0f, 448.0f);
    b = __builtin_amdgcn_fmed3f(b * inv, -448.0f, 448.0f);
    c = __builtin_amdgcn_fmed3f(c * inv, -448.0f, 448.0f);
    d = __builtin_amdgcn_fmed3f(d * inv, -448.0f, 448.0f);
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (unsigned)v;
}

__device__ __forceinline__ int swz(int slot) { return slot ^ ((slot >> 4) & 3); }

__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// residual add in float32 BEFORE the rounding to bf16: lane (j, h) holds channels 8q + 4h + i of tile t, i.e. 4 consecutive
// bf16 (8 bytes) at element offset 8(q & 1) + 4h of record q >> 1 of the residual's tile.  res: address of the lane's pixel in
// the first record of the tile (element units), + 4h.
__device__ __forceinline__ void add_f16k_residual(f32x16& t, const unsigned short* res, unsigned rec_stride) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint2 r = *reinterpret_cast<const uint2*>(res + (size_t)(q >> 1) * rec_stride + 8 * (q & 1));
        t[4 * q + 0] += __builtin_bit_cast(float, r.x << 16);
        t[4 * q + 1] += __builtin_bit_cast(float, r.x & 0xffff0000u);
        t[4 * q + 2] += __builtin_bit_cast(float, r.y << 16);
        t[4 * q + 3] += __builtin_bit_cast(float, r.y & 0xffff0000u);
    }
}
// t *= act'(mask): the backward of ReLU / LeakyReLU(0.01) as an epilogue of the input-gradient convolution -- mask = the forward
// activation's OUTPUT in F16K (its sign is the pre-activation's), addressed like a residual tensor
__device__ __forceinline__ void mul_f16k_actmask(f32x16& t, const unsigned short* mask, unsigned rec_stride, float slope) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint2 r = *reinterpret_cast<const uint2*>(mask + (size_t)(q >> 1) * rec_stride + 8 * (q & 1));
        t[4 * q + 0] *= __builtin_bit_cast(float, r.x << 16) > 0.0f ? 1.0f : slope;
        t[4 * q + 1] *= __builtin_bit_cast(float, r.x & 0xffff0000u) > 0.0f ? 1.0f : slope;
        t[4 * q + 2] *= __builtin_bit_cast(float, r.y << 16) > 0.0f ? 1.0f : slope;
        t[4 * q + 3] *= __builtin_bit_cast(float, r.y & 0xffff0000u) > 0.0f ? 1.0f : slope;
    }
}
// F16K store of the 32 channels of accumulator tile `t` (lane (j, h) holds channels 4h + 8q + i, q, i < 4, of pixel j):
// the two halves of the wave swap their middle quarters (v_permlane32_swap) so that lane (j, h) ends up with the 8
// consecutive channels 8h .. 8h+7 of each 16-channel record and writes it with one 16-byte store -- the wave writes
// whole 32-byte records (full sectors; 1 KiB contiguous when the pixels are adjacent) instead of scattered 8-byte pieces.
// rec: address of the lane's pixel in the first of the two records, + 8h elements; rec_stride: elements between records.
__device__ __forceinline__ void store_f16k_tile(const f32x16& t, unsigned short* rec, unsigned rec_stride) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned a0 = pack2bf(t[8 * r + 0], t[8 * r + 1]), a1 = pack2bf(t[8 * r + 2], t[8 * r + 3]);   // channels 4h .. 4h+3
        const unsigned b0 = pack2bf(t[8 * r + 4], t[8 * r + 5]), b1 = pack2bf(t[8 * r + 6], t[8 * r + 7]);   // channels 8 + 4h ..
        const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        uint4 st;
        st.x = s0[0]; st.y = s1[0]; st.z = s0[1]; st.w = s1[1];
        *reinterpret_cast<uint4*>(rec + (size_t)r * rec_stride) = st;
    }
}

// the same through a buffer resource: voff = byte offset of the lane's pixel in the first record + 16h, or any offset >= the resource's
// size for a lane that has nothing to store (dropped by the range check) -- the instruction is issued unconditionally, so the number
// of store instructions a wave has in flight is known at compile time (counted s_waitcnt vmcnt in conv_a_gdn_f16k)
__device__ __forceinline__ void store_f16k_tile_buf(const f32x16& t, __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned rec_stride_bytes) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned a0 = pack2bf(t[8 * r + 0], t[8 * r + 1]), a1 = pack2bf(t[8 * r + 2], t[8 * r + 3]);
        const unsigned b0 = pack2bf(t[8 * r + 4], t[8 * r + 5]), b1 = pack2bf(t[8 * r + 6], t[8 * r + 7]);
        const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        v4u st = {s0[0], s1[0], s0[1], s1[1]};
        __builtin_amdgcn_raw_buffer_store_b128(st, rs, (int)(voff + r * rec_stride_bytes), 0, 0);
    }
}

// F8K store (fp8 activations [B][C/32][H*W][32]: a pixel's 32 channels are one 32-byte record) of accumulator tile `t` = one
// whole record per pixel: lane (j, h) holds channels 8q + 4h + i; after two v_permlane32_swap it holds the 16 consecutive
// channels 16h .. 16h+15 and writes them with one 16-byte store.  rec: address of the lane's pixel record + 16h bytes.
__device__ __forceinline__ void store_f8k_tile(const f32x16& t, unsigned char* rec, float inv) {
    unsigned q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = pack4f8(t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3], inv);
    const auto s0 = __builtin_amdgcn_permlane32_swap(q[0], q[2], false, false);     // h = 0: channels 0-3, 4-7;   h = 1: 16-19, 20-23
    const auto s1 = __builtin_amdgcn_permlane32_swap(q[1], q[3], false, false);     // h = 0: 8-11, 12-15;         h = 1: 24-27, 28-31
    uint4 st;
    st.x = s0[0]; st.y = s0[1]; st.z = s1[0]; st.w = s1[1];
    *reinterpret_cast<uint4*>(rec) = st;
}

__device__ __forceinline__ void dma_buf16(__amdgpu_buffer_rsrc_t r, unsigned char* lds_wave_base, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voffset, soffset, 0, 0);
}

// (Inverse) GDN over the 128 channels a wave holds for its 32 pixels (accumulator layout of four 32x32 MFMA tiles):
//   y_i = x_i * rsqrt(beta^_i + sum_j gamma^_ij x_j^2)  (inverse: * sqrt), compressai/layers/gdn.py:77-92.
// The 128 x 128 contraction runs on the matrix cores with gamma^ and x^2 each split into bf16 hi + lo (three products:
// error ~2^-16 of a term).  k-step s covers channels 32(s>>1) + 16(s&1) + 8(c>>2) + 4hh + (c&3), c = 0..7 -- exactly the
// 8 accumulator registers acc[s>>1][8(s&1) + c] the lane already holds for its pixel, so the B operand needs no data
// movement; the gamma^ fragments lie in LDS pre-arranged in that order (gdn.hip: gdn_pack_f16k_kernel).
// gimg: LDS address of the fragment image + lane * 16;  bet: LDS address of beta^[128] + 4h (read late: no registers held).
// X3 = false: one product (bf16 gamma^ x bf16 x^2, error ~2^-10 of the result -- the order of the bf16 rounding the result gets
// anyway when it is stored as F16K / fed to a bf16-operand layer): a third of the MFMAs, half the fragment reads, no lo split.
// PS: bytes between the hi pieces of consecutive (m, k-step) pairs -- 2048 for the image as gdn_pack_f16k_kernel lays it out (hi and lo
// pieces alternate), 1024 for a copy that holds the hi pieces alone (one-product form only).
template <bool X3, int PS = 2048>
__device__ __forceinline__ void gdn_in_registers(f32x16 (&acc)[4], const unsigned char* gimg, const float* bet, int inverse) {
    static_assert(PS == 2048 || (PS == 1024 && !X3), "a hi-only image serves the one-product form");
    f32x16 nrm[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) nrm[m][e] = 0.0f;
#pragma unroll
    for (int sx = 0; sx < 8; ++sx) {
        bf16x8 bh, blo;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            const float xv = acc[sx >> 1][8 * (sx & 1) + cc];
            const float sq = __fmul_rn(xv, xv);
            const __bf16 hi = (__bf16)sq;
            bh[cc] = hi;
            if constexpr (X3) blo[cc] = (__bf16)(sq - (float)hi);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bf16x8 gh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(gimg + (m * 8 + sx) * PS));
            if constexpr (X3) {
                const bf16x8 gl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(gimg + (m * 8 + sx) * PS + 1024));
                nrm[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl, bh, nrm[m], 0, 0, 0);
                nrm[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, blo, nrm[m], 0, 0, 0);
            }
            nrm[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, bh, nrm[m], 0, 0, 0);
        }
    }
    // v_sqrt_f32 / v_rsq_f32 (1 ulp): the result is rounded to bf16 or feeds a bf16-operand convolution anyway.  `inverse` is uniform:
    // a BRANCH, not a select -- as `inverse ? sqrt : rsq` the compiler evaluated both for every element (128 quarter-rate instructions
    // and 64 selects per lane where 64 + 0 do)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 be = *reinterpret_cast<const float4*>(bet + m * 32 + 8 * q);
            nrm[m][4 * q + 0] += be.x; nrm[m][4 * q + 1] += be.y; nrm[m][4 * q + 2] += be.z; nrm[m][4 * q + 3] += be.w;
        }
    if (inverse) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] *= __builtin_amdgcn_sqrtf(nrm[m][e]);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] *= __builtin_amdgcn_rsqf(nrm[m][e]);
    }
}
}  // namespace
