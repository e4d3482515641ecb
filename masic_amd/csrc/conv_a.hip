// conv_a.hip -- the first analysis layer on the matrix cores, (I)GDN fused, F16K out (gfx950 / MI355X).
//
// g_a_conv1 + g_a_gdn1 (MASIC.py:515-516, :563-564): Conv2d(3 -> 128, k5, s2, p2) on the float32 NCHW image followed by
// GDN, written as F16K for the next convolution.  K = 75 (padded to 80 = 5 MFMA k-steps), so the layer is bound by its
// output (B x 128 x H/2 x W/2) and by the GDN contraction, not by the convolution: persistent workgroups (8 waves, one
// 8 x 32 output tile per iteration, wave w = row w) keep the gamma^ image (64 KiB), the weight fragments (20 KiB), bias
// and beta^ in LDS for all their tiles; the 3 x 19 x 67 input patch of the next tile is fetched into registers while the
// current one is contracted.  k = tap * 3 + ci; a lane's B fragment is 8 two-byte LDS reads of the bf16 patch.
//
// Device helpers shared with the other F16K families (gdn_in_registers, the tile stores, ...): f16k_device.h.  The launcher hands
// g_f16k_stamps (masic_conv_f16k_set_stamps, conv_f16k.hip) to its kernels.
#include "f16k_device.h"

namespace {
struct ConvAArgs {
    const float* x;               // float32 NCHW [B][in_ctot][Hi][Wi], channels in_coff .. in_coff+2
    const uint4* wimg;            // [m 4][s 6][lane 64] x 8 bf16: W[32m + (lane & 31)][k-slot (s, lane >> 5, c)], pack_conv_a_kernel
    const float* bias;            // [128] or null
    const uint4* gdn_img;         // gdn_pack_f16k_kernel image, then beta^[128]
    unsigned short* y16;          // F16K [B][8][Ho*Wo][16]
    int gdn_inverse, Hi, Wi, in_ctot, in_coff, Ho, Wo, tiles_w, tiles_per_img, ntiles;
    unsigned char* y8;            // instead of y16: F8K [B][4][Ho*Wo][32] fp8, quantised with out_inv_scale
    float out_inv_scale;
    unsigned short* y16_pre;      // also store conv + bias before the GDN (F16K), or null
    unsigned long long* stamps;   // diagnostics: s_memrealtime (100 MHz) at 6 points of every tile of workgroup 0 / wave 0, or null
};

#ifndef CONVA_ABLATE
#define CONVA_ABLATE 0     // timing experiments only: 1 no GDN math, 2 no convolution, 3 no patch fetch / stash after the first tile, 4 no stores
#endif
constexpr int CA_PH = 19, CA_PW = 67, CA_NEL = 3 * CA_PH * CA_PW;                     // patch of an 8 x 32 tile, stride 2, 5 x 5: [ci][row][col], float32
constexpr int CA_NPT = (CA_NEL + 511) / 512;                                          // patch elements (= 4-byte DMA pieces) per thread
constexpr int CA_KSTEPS = 6, CA_WIMG_BYTES = 4 * CA_KSTEPS * 1024;                    // k-steps of the convolution (see pack_conv_a_kernel); weight fragment image
constexpr int CA_PATCH_BYTES = CA_NPT * 2048;                                         // 3 * 19 * 67 * 4 = 15276, padded to whole wave-instructions

// k order of the first layer's contraction: k-step s = 2p + q covers the kernel-row pair (2p, 2p + 1) -- lane half h = the row within the
// pair -- and the (ci, kw) pairs 8q .. 8q + 7 of the 15 a row has (pair = 5 ci + kw; pair 15 and kernel row 5 are zero-weight padding):
// k = 96 slots for K = 75.  With this order the LDS offset of a lane's operand element is (ci * 19 + 2p + h) * 67 + kw: the only
// per-lane part, h * 67, goes into the lane's base address and every read takes a compile-time immediate offset (the k = tap * 3 + ci
// order of round 2 needed 40 per-lane offsets: 40 VGPRs the compiler kept live across the whole tile loop).
__global__ void pack_conv_a_kernel(const float* __restrict__ w, uint4* __restrict__ wimg) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * CA_KSTEPS * 64) return;
    const int ms = idx >> 6, l = idx & 63, m = ms / CA_KSTEPS, sx = ms - m * CA_KSTEPS, r = l & 31, hh = l >> 5;
    const int kh = 2 * (sx >> 1) + hh;
    bf16x8 v;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int pair = 8 * (sx & 1) + c, ci = pair / 5, kw = pair - 5 * ci;
        v[c] = (__bf16)((pair < 15 && kh < 5) ? w[((size_t)(32 * m + r) * 3 + ci) * 25 + kh * 5 + kw] : 0.0f);
    }
    wimg[idx] = __builtin_bit_cast(uint4, v);
}

// The one-product GDN of gdn_in_registers and the per-channel vector add, with LDS reads the compiler does NOT see (inline asm, counted
// lgkmcnt): while a global -> LDS DMA is in flight hipcc puts `s_waitcnt vmcnt(0)` in front of every ds_read it knows about (the DMA might
// alias it), which here would end the next patch's flight -- and wait for the previous tile's output stores -- right after the convolution.
// gaddr: LDS byte address of the gamma^ fragment image + lane * 16;  baddr: LDS byte address of the [128] float vector + 16 h.
template <int OP>      // 0: acc[m] += vec   1: acc[m] *= rsqrt(nrm[m] + vec)   2: acc[m] *= sqrt(nrm[m] + vec)
__device__ __forceinline__ void vec_apply_hidden(f32x16 (&acc)[4], const f32x16 (&nrm)[4], unsigned baddr) {
    static_for<0, 2>([&](auto HALF) {
        constexpr int half = decltype(HALF)::value;
        v4u v[8];
        static_for<0, 8>([&](auto I) {
            constexpr int i = decltype(I)::value, m = 2 * half + (i >> 2), q = i & 3;
            ds_read128<(m * 32 + 8 * q) * 4>(v[i], baddr);
        });
        lgkm_wait<0>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        static_for<0, 8>([&](auto I) {
            constexpr int i = decltype(I)::value, m = 2 * half + (i >> 2), q = i & 3;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned u = v[i][e];            // (a copy first: __builtin_bit_cast on a vector-ELEMENT lvalue reads element 0 whatever e is)
                const float b = __builtin_bit_cast(float, u);
                if constexpr (OP == 0) acc[m][4 * q + e] += b;
                else if constexpr (OP == 1) acc[m][4 * q + e] *= __builtin_amdgcn_rsqf(nrm[m][4 * q + e] + b);
                else acc[m][4 * q + e] *= __builtin_amdgcn_sqrtf(nrm[m][4 * q + e] + b);
            }
        });
    });
}
__device__ __forceinline__ void gdn_in_registers_hidden(f32x16 (&acc)[4], unsigned gaddr, unsigned baddr, int inverse) {
    // the accumulators of the contraction start at beta^ (read straight into them: no add afterwards)
    f32x16 nrm[4];
    {
        v4u vb[16];
        static_for<0, 16>([&](auto I) { constexpr int i = decltype(I)::value; ds_read128<((i >> 2) * 32 + 8 * (i & 3)) * 4>(vb[i], baddr); });
        lgkm_wait<0>(vb[0], vb[1], vb[2], vb[3], vb[4], vb[5], vb[6], vb[7]);
        lgkm_wait<0>(vb[8], vb[9], vb[10], vb[11], vb[12], vb[13], vb[14], vb[15]);
        static_for<0, 4>([&](auto M) {
            constexpr int m = decltype(M)::value;
            typedef float f32x4v __attribute__((ext_vector_type(4)));
            const f32x4v q0 = __builtin_bit_cast(f32x4v, vb[4 * m]), q1 = __builtin_bit_cast(f32x4v, vb[4 * m + 1]);
            const f32x4v q2 = __builtin_bit_cast(f32x4v, vb[4 * m + 2]), q3 = __builtin_bit_cast(f32x4v, vb[4 * m + 3]);
            nrm[m] = __builtin_shufflevector(__builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(q2, q3, 0, 1, 2, 3, 4, 5, 6, 7),
                                             0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
        });
    }
    v4u g[2][4];
    static_for<0, 4>([&](auto M) { constexpr int m = decltype(M)::value; ds_read128<((m * 8 + 0) * 2) * 1024>(g[0][m], gaddr); });
    static_for<0, 8>([&](auto SX) {
        constexpr int sx = decltype(SX)::value, cur = sx & 1;
        if constexpr (sx + 1 < 8)
            static_for<0, 4>([&](auto M) { constexpr int m = decltype(M)::value; ds_read128<((m * 8 + sx + 1) * 2) * 1024>(g[cur ^ 1][m], gaddr); });
        v4u bq;                          // x^2 of the 8 channels of this k-step, packed pair by pair (one v_pk_mul + one v_cvt_pk per pair)
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) {
            const float x0 = acc[sx >> 1][8 * (sx & 1) + 2 * cp], x1 = acc[sx >> 1][8 * (sx & 1) + 2 * cp + 1];
            bq[cp] = pack2bf(__fmul_rn(x0, x0), __fmul_rn(x1, x1));
        }
        const bf16x8 bh = __builtin_bit_cast(bf16x8, bq);
        lgkm_wait<(sx + 1 < 8 ? 4 : 0)>(g[cur][0], g[cur][1], g[cur][2], g[cur][3]);
        static_for<0, 4>([&](auto M) {
            constexpr int m = decltype(M)::value;
            nrm[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, g[cur][m]), bh, nrm[m], 0, 0, 0);
        });
    });
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

// X3: three-product GDN contraction; OUT: 0 F16K, 1 F8K (fp8), 2 F16K + the pre-GDN result (training), 3 F16K WITHOUT the GDN (the
// plain Conv2d(3 -> 128, k5, s2): the input gradient of g_s_conv4 = ConvTranspose2d(128 -> 3), MASIC.py:550, in the training step --
// no gamma^ image is loaded).  Compile-time variants: with
// the choices as run-time branches both GDN forms were inlined and the kernel spilled 68 VGPRs in its tile loop (129 us per launch
// at 8x512x512 against 80 for the round-1 kernel).
template <bool X3, int OUT>
__global__ __launch_bounds__(512, 1) void conv_a_gdn_f16k(const ConvAArgs a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    constexpr int WIMG = 65536, VEC = WIMG + CA_WIMG_BYTES, PATCH = VEC + 1024;      // LDS map: gamma image | weights | bias, beta^ | 2 patches
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;   // LDS byte address of lds[0]

    // ---- once per workgroup: fragment images by DMA, bias / beta^ by plain stores
    {
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)a.gdn_img, 0, 65536 + 512, 0x00020000);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.wimg, 0, CA_WIMG_BYTES, 0x00020000);
        if constexpr (OUT != 3) {
#pragma unroll
            for (int k = 0; k < 8; ++k) dma_buf16(rg, lds + (wave * 8 + k) * 1024, lane * 16, (wave * 8 + k) * 1024);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dma_buf16(rw, lds + WIMG + (wave * 3 + k) * 1024, lane * 16, (wave * 3 + k) * 1024);            // 8 waves x 3 KiB = 24 KiB
        float* vec = reinterpret_cast<float*>(lds + VEC);
        if (tid < 128) {
            vec[tid] = a.bias != nullptr ? a.bias[tid] : 0.0f;
            if constexpr (OUT != 3) vec[128 + tid] = reinterpret_cast<const float*>(a.gdn_img + 4 * 8 * 2 * 64)[tid];
        }
    }
    // ---- patch element map of this thread (tile independent): element el = tid + 512 i -> (ci, row, col) of the float32 LDS patch
    // [ci][row 19][col 67]; the patch is filled by 4-byte global -> LDS DMA (wave-instruction i of wave w lands at dwords 512 i + 64 w ..),
    // so it costs no registers and no conversion pass, and elements outside the image come back as zeros from the buffer range check.
    // (Round 2 staged it through registers with a padding select right behind the loads: the compiler put `s_waitcnt vmcnt(0)` there, at
    // the TOP of the tile loop, which waited for the loads' full latency AND -- vmcnt retires in order -- for the previous tile's 64 KiB of
    // output stores before the first MFMA of every tile: load latency + store drain + compute in series, 8.5 us per tile for 1.7 us of MFMAs.)
    const size_t plane = (size_t)a.Hi * a.Wi;
    unsigned offrel[CA_NPT], rc[CA_NPT];       // byte offset of the element relative to the patch origin; row | col << 8 | valid << 16
#pragma unroll
    for (int i = 0; i < CA_NPT; ++i) {
        const int el = tid + 512 * i;
        const int ci = el / (CA_PH * CA_PW), rem = el - ci * (CA_PH * CA_PW);
        const int row = rem / CA_PW, col = rem - row * CA_PW;
        offrel[i] = (unsigned)(((size_t)ci * plane + (size_t)row * a.Wi + col) * 4);
        rc[i] = (unsigned)row | ((unsigned)col << 8) | (el < CA_NEL ? 1u << 16 : 0u);
    }
    auto fetch = [&](int tile, int buf) {           // global -> LDS, left in flight
        const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
        const int ih0 = (t / a.tiles_w) * 16 - 2, iw0 = (t % a.tiles_w) * 64 - 2;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane), 0,
                                                                            (int)(3 * plane * 4), 0x00020000);
        const unsigned origin = (unsigned)((ih0 * a.Wi + iw0) * 4);
        unsigned char* dst = lds + PATCH + buf * CA_PATCH_BYTES + wave * 256;
#pragma unroll
        for (int i = 0; i < CA_NPT; ++i) {
            const int ih = ih0 + (int)(rc[i] & 255u), iw = iw0 + (int)((rc[i] >> 8) & 255u);
            const unsigned ok = (rc[i] >> 16) & (unsigned)(ih >= 0) & (unsigned)(ih < a.Hi) & (unsigned)(iw >= 0) & (unsigned)(iw < a.Wi);
            const unsigned off = ok ? offrel[i] + origin : 0xC0000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + i * 2048), 4, (int)off, 0, 0, 0);
        }
    };

    // Memory schedule of the tile loop (OUT == 0; the other forms wait for everything, vmcnt(0)).  Per tile t, in this order:
    //   convolution + GDN on patch buffer t & 1  ->  s_waitcnt vmcnt(8)  ->  s_barrier  ->  issue the patch DMA of tile t + 2 into buffer
    //   t & 1 (every wave is done reading it)  ->  issue the 8 output stores of tile t.
    // vmcnt retires in order, so at the wait of tile t + 1 the queue holds [DMA(t + 2)][8 stores of t]: vmcnt(8) waits for the patch and
    // for everything older, and leaves the 8 stores IN FLIGHT across the barrier -- there is always a tile of stores (64 KiB per CU)
    // draining while the next tile computes, and the HBM pipe never idles between two tiles' bursts (with the stores issued before the
    // DMA, or vmcnt(0), each round of 256 tiles paid its drain in full: 60 us per launch for 15 us of arithmetic and 21 us of stores).
    // The stores go through a buffer resource with out-of-range offsets for lanes outside the picture: always exactly 8 instructions.
    constexpr bool COUNTED = OUT == 0;
    int tile = blockIdx.x;
    if (tile < a.ntiles) fetch(tile, 0);
    if (COUNTED && tile + (int)gridDim.x < a.ntiles) fetch(tile + gridDim.x, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // The bias rides in the contraction: k-slot (k-step 1, element 7) is the 16th, unused (ci, kw) pair of kernel rows 0 / 1 -- its B operand
    // is set to 1 and its weight to bias_hi (lane half 0) / bias_lo (lane half 1), a bf16 split with 2^-17 relative error: no 64 adds and
    // 16 LDS reads per lane and tile.  The weight image arrived by DMA without it; it is patched here, once per workgroup.
    if (tid < 256) {
        const int co = tid & 127, hh = tid >> 7;
        const float bv = reinterpret_cast<const float*>(lds + VEC)[co];
        const __bf16 hi = (__bf16)bv;
        const __bf16 val = hh == 0 ? hi : (__bf16)(bv - (float)hi);
        reinterpret_cast<__bf16*>(lds + WIMG + (((co >> 5) * CA_KSTEPS + 1) * 64 + (co & 31) + 32 * hh) * 16)[7] = val;
    }
    __syncthreads();
    const unsigned char* gimg = lds + lane * 16;
    const float* vec = reinterpret_cast<const float*>(lds + VEC);
    const size_t oplane = (size_t)a.Ho * a.Wo;
    int buf = 0;
    unsigned long long* stamp = (a.stamps != nullptr && blockIdx.x == 0 && tid == 0) ? a.stamps : nullptr;
    for (; tile < a.ntiles; tile += gridDim.x, buf ^= 1) {
        const int next = tile + gridDim.x;
        if (stamp) stamp[0] = __builtin_amdgcn_s_memrealtime();
        if (!COUNTED && next < a.ntiles && CONVA_ABLATE != 3) fetch(next, buf ^ 1);   // in flight during this tile's contraction and GDN
        // ---- convolution: 5 k-steps x 4 channel blocks
        const float* pl = reinterpret_cast<const float*>(lds + PATCH + buf * CA_PATCH_BYTES) + (2 * wave + h) * CA_PW + 2 * j;
        f32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] = 0.0f;
#pragma unroll
        for (int sx = 0; sx < (CONVA_ABLATE == 2 ? 0 : CA_KSTEPS); ++sx) {
            bf16x8 bfr;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int pair = 8 * (sx & 1) + c, ci = pair < 15 ? pair / 5 : 0, kw = pair < 15 ? pair % 5 : 0;
                if (sx == 1 && c == 7) bfr[c] = (__bf16)1.0f;                              // the bias slot (see above)
                else bfr[c] = (__bf16)pl[(ci * CA_PH + 2 * (sx >> 1)) * CA_PW + kw];      // (+ h rows: in the lane's base; kernel row 5 / pair 15: zero weights)
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const bf16x8 af = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + WIMG + (m * CA_KSTEPS + sx) * 1024 + lane * 16));
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[m], 0, 0, 0);
            }
        }
        if (stamp) stamp[1] = __builtin_amdgcn_s_memrealtime();
        // ---- GDN, F16K store (LDS reads hidden from the compiler: the next patch's DMA is in flight)
        if constexpr (OUT == 2) {
            const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
            const int oh = (t / a.tiles_w) * 8 + wave, ow = (t % a.tiles_w) * 32 + j;
            if (oh < a.Ho && ow < a.Wo) {
                unsigned short* yp = a.y16_pre + (((size_t)b * 8) * oplane + (size_t)oh * a.Wo + ow) * 16 + 8 * h;
                const unsigned op16 = (unsigned)oplane * 16;
#pragma unroll
                for (int m = 0; m < 4; ++m) store_f16k_tile(acc[m], yp + (size_t)(2 * m) * op16, op16);
            }
        }
        if constexpr (OUT != 3) {
            if (CONVA_ABLATE != 1) {
                if constexpr (X3) gdn_in_registers<true>(acc, gimg, vec + 128 + 4 * h, a.gdn_inverse & 1);
                else gdn_in_registers_hidden(acc, ldsb + lane * 16, ldsb + VEC + 512 + 16 * h, a.gdn_inverse & 1);
            }
        }
        // the next tile's patch has had the whole convolution + GDN to land: wait for it (vmcnt(0): that is also the PREVIOUS tile's output
        // stores, issued a full tile of MFMA work ago), the workgroup barrier, and only THEN this tile's stores -- nothing waits for them
        // until the end of the next tile.  The stores are the kernel's HBM floor (134 MB per launch at 8 x 512 x 512); they drain UNDER
        // the next tile's MFMAs.
        if (stamp) stamp[2] = __builtin_amdgcn_s_memrealtime();
        if constexpr (COUNTED) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (stamp) stamp[3] = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (stamp) stamp[4] = __builtin_amdgcn_s_memrealtime();
        if constexpr (COUNTED) {
            if (next + (int)gridDim.x < a.ntiles && CONVA_ABLATE != 3) fetch(next + gridDim.x, buf);
            const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
            const int oh = (t / a.tiles_w) * 8 + wave, ow = (t % a.tiles_w) * 32 + j;
            const unsigned rec_bytes = (unsigned)oplane * 32;
            const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(a.y16 + (size_t)b * 8 * oplane * 16), 0, (int)(8 * rec_bytes), 0x00020000);
            const unsigned voff = (oh < a.Ho && ow < a.Wo && CONVA_ABLATE != 4) ? ((unsigned)oh * a.Wo + ow) * 32 + 16 * h : 0xC0000000u;
#pragma unroll
            for (int m = 0; m < 4; ++m) store_f16k_tile_buf(acc[m], ry, voff + (unsigned)(2 * m) * rec_bytes, rec_bytes);
            if (stamp) { stamp[5] = __builtin_amdgcn_s_memrealtime(); stamp += 6; }
        } else if (CONVA_ABLATE != 4) {
            const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
            const int oh = (t / a.tiles_w) * 8 + wave, ow = (t % a.tiles_w) * 32 + j;
            if (oh < a.Ho && ow < a.Wo) {
                if constexpr (OUT == 1) {
                    unsigned char* yb = a.y8 + (((size_t)b * 4) * oplane + (size_t)oh * a.Wo + ow) * 32 + 16 * h;
#pragma unroll
                    for (int m = 0; m < 4; ++m) store_f8k_tile(acc[m], yb + (size_t)m * oplane * 32, a.out_inv_scale);
                } else {
                    unsigned short* yb = a.y16 + (((size_t)b * 8) * oplane + (size_t)oh * a.Wo + ow) * 16 + 8 * h;
                    const unsigned op16 = (unsigned)oplane * 16;
#pragma unroll
                    for (int m = 0; m < 4; ++m) store_f16k_tile(acc[m], yb + (size_t)(2 * m) * op16, op16);
                }
            }
        }
    }
}

// The inference form of the first layer (one-product GDN, F16K out, Wi % 4 == 0) with WAVE-PRIVATE patches and no barrier in the tile loop.
// Wave w of the workgroup owns output row w of the 8 x 32 tile: its own [15 rows = (ci, kh)][72 floats] float32 patch (4 320 bytes, two
// buffers) is filled by 16-byte global -> LDS DMA -- 270 pieces = 5 wave-instructions, against 8 of the 64 four-byte instructions per
// workgroup and tile of the shared patch, whose issue (~80 cycles each on the CU's one address path) cost more than the tile's MFMAs --
// and read by that wave alone, so the waves of a workgroup never wait for each other: they drift out of phase, and one wave's MFMAs run
// under the other's VALU work on the same SIMD (in lock step both waves of a SIMD were in the VALU-heavy epilogue at the same time).
// Memory schedule per wave and tile k:   s_waitcnt vmcnt(21) -> convolution on buffer k & 1 -> DMA of tile k + 2 into that buffer ->
// GDN -> 8 output stores.  Every iteration issues exactly 5 DMA + 8 store instructions (lanes / tiles with nothing to move get
// out-of-range offsets: loads write zeros, stores are dropped), so at the top of tile k the instructions younger than the DMA of tile k
// are [8 stores of k-2][5 DMA of k+1][8 stores of k-1] = 21: vmcnt(21) is exact, and two tiles of stores stay in flight.
constexpr int CW_PCS = 18, CW_ROWS = 15, CW_NP = CW_ROWS * CW_PCS, CW_NI = (CW_NP + 63) / 64, CW_BYTES = CW_NP * 16, CW_PITCH = CW_PCS * 4;
static_assert(CW_NI == 5 && CW_BYTES == 4320, "vmcnt(21) below counts 5 DMA instructions per tile");
// One zeroed patch row behind the last wave's second buffer: the zero-weight kernel row 5 of ci = 2 reads row 15 of a patch, i.e. the first
// row of whatever follows it.  For waves 0..6 and for wave 7's first buffer that is another patch (finite floats); for wave 7 on every tile
// it computes from its SECOND buffer (a workgroup's 2nd, 4th, ... tile) it was past the allocation, where LDS holds what the last kernel on
// the CU left: a NaN or Inf pattern there times the zero weight made a NaN output pixel.
constexpr int CW_TAIL_BYTES = CW_PITCH * 4;
constexpr int CW_LDS = 65536 + CA_WIMG_BYTES + 1024 + 16 * CW_BYTES + CW_TAIL_BYTES;
static_assert(CW_LDS <= 160 * 1024, "LDS");
__global__ __launch_bounds__(512, 1) void conv_a_gdn_f16k_w(const ConvAArgs a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    constexpr int WIMG = 65536, VEC = WIMG + CA_WIMG_BYTES, PATCH = VEC + 1024;      // LDS map: gamma image | weights | bias, beta^ | 8 x 2 patches
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    unsigned long long* const pst = (a.stamps != nullptr && tid == 0 && (blockIdx.x == 0 || blockIdx.x + 1 == gridDim.x)) ? a.stamps + 48 + (blockIdx.x == 0 ? 0 : 8) : nullptr;
    if (pst) pst[0] = __builtin_amdgcn_s_memrealtime();
    {
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)a.gdn_img, 0, 65536 + 512, 0x00020000);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.wimg, 0, CA_WIMG_BYTES, 0x00020000);
#pragma unroll
        for (int k = 0; k < 8; ++k) dma_buf16(rg, lds + (wave * 8 + k) * 1024, lane * 16, (wave * 8 + k) * 1024);
#pragma unroll
        for (int k = 0; k < 3; ++k) dma_buf16(rw, lds + WIMG + (wave * 3 + k) * 1024, lane * 16, (wave * 3 + k) * 1024);
        float* vec = reinterpret_cast<float*>(lds + VEC);
        if (tid < 128) {
            vec[tid] = a.bias != nullptr ? a.bias[tid] : 0.0f;
            vec[128 + tid] = reinterpret_cast<const float*>(a.gdn_img + 4 * 8 * 2 * 64)[tid];
        }
        if (tid < CW_PITCH) reinterpret_cast<float*>(lds + PATCH + 16 * CW_BYTES)[tid] = 0.0f;      // (visible after the barriers below)
    }
    // piece map of this lane (tile independent): piece p = lane + 64 i -> patch row r = p / 18 = 5 ci + kh, 16-byte column piece pc = p % 18
    const size_t plane = (size_t)a.Hi * a.Wi;
    unsigned offrel[CW_NI], rc[CW_NI];          // byte offset relative to the patch origin; kh | pc << 8 | valid << 16
#pragma unroll
    for (int i = 0; i < CW_NI; ++i) {
        const int p = lane + 64 * i, r = p / CW_PCS, pc = p - r * CW_PCS, ci = r / 5, kh = r - 5 * ci;
        offrel[i] = (unsigned)(((size_t)ci * plane + (size_t)kh * a.Wi + 4 * pc) * 4);
        rc[i] = (unsigned)kh | ((unsigned)pc << 8) | (p < CW_NP ? 1u << 16 : 0u);
    }
    unsigned char* const mypatch = lds + PATCH + wave * (2 * CW_BYTES);
    auto fetch = [&](int tile, int buf) {           // always CW_NI instructions; a tile past the end / a row below the picture loads zeros
        const bool live = tile < a.ntiles;
        const int tl = live ? tile : 0;
        const int b = tl / a.tiles_per_img, t = tl - b * a.tiles_per_img;
        const int oh = (t / a.tiles_w) * 8 + wave;
        const int ih0 = 2 * oh - 2, iw0 = (t % a.tiles_w) * 64 - 4;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane), 0,
                                                                            (int)(3 * plane * 4), 0x00020000);
        const unsigned origin = (unsigned)((ih0 * a.Wi + iw0) * 4);
        const unsigned rowok = (unsigned)(live && oh < a.Ho);
        unsigned char* dst = mypatch + buf * CW_BYTES;
#pragma unroll
        for (int i = 0; i < CW_NI; ++i) {
            const int ih = ih0 + (int)(rc[i] & 255u), iw = iw0 + 4 * (int)((rc[i] >> 8) & 255u);
            const unsigned ok = rowok & (rc[i] >> 16) & (unsigned)(ih >= 0) & (unsigned)(ih < a.Hi) & (unsigned)(iw >= 0) & (unsigned)(iw < a.Wi);
            const unsigned off = ok ? offrel[i] + origin : 0xC0000000u;
            if (i + 1 < CW_NI || lane < CW_NP - 64 * (CW_NI - 1))      // the last instruction covers 14 pieces: the other lanes are masked off (EXEC)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, (int)off, 0, 0, 0);
        }
    };
    int tile = blockIdx.x;
    fetch(tile, 0);
    fetch(tile + gridDim.x, 1);
    if (pst) pst[1] = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (pst) pst[2] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
    if (pst) pst[3] = __builtin_amdgcn_s_memrealtime();
    if (tid < 256) {                // the bias as a k-slot of the contraction (see conv_a_gdn_f16k)
        const int co = tid & 127, hh = tid >> 7;
        const float bv = reinterpret_cast<const float*>(lds + VEC)[co];
        const __bf16 hi = (__bf16)bv;
        const __bf16 val = hh == 0 ? hi : (__bf16)(bv - (float)hi);
        reinterpret_cast<__bf16*>(lds + WIMG + (((co >> 5) * CA_KSTEPS + 1) * 64 + (co & 31) + 32 * hh) * 16)[7] = val;
    }
    __syncthreads();
    const size_t oplane = (size_t)a.Ho * a.Wo;
    const unsigned rec_bytes = (unsigned)oplane * 32;
    int buf = 0;
    unsigned long long* stamp = (a.stamps != nullptr && blockIdx.x == 0 && tid == 0) ? a.stamps : nullptr;
    for (; tile < a.ntiles; tile += gridDim.x, buf ^= 1) {
        if (stamp) stamp[0] = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt vmcnt(21)" ::: "memory");
        if (stamp) stamp[1] = __builtin_amdgcn_s_memrealtime();
        // ---- convolution: 6 k-steps x 4 channel blocks; patch element (ci, kh = 2p + h, column 2 j + kw - 2) = row 5 ci + kh, float 2 j + kw + 2
        const float* pl = reinterpret_cast<const float*>(mypatch + buf * CW_BYTES) + h * CW_PITCH + 2 * j + 2;
        f32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] = 0.0f;
#pragma unroll
        for (int sx = 0; sx < CA_KSTEPS; ++sx) {
            bf16x8 bfr;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int pair = 8 * (sx & 1) + c, ci = pair < 15 ? pair / 5 : 0, kw = pair < 15 ? pair % 5 : 0;
                // (kernel row 5 -- k-steps 4, 5, lane half 1 -- has zero weights and reads row 0 of the next ci / the 288 bytes behind this
                // buffer: the wave's other buffer, the next wave's, or the zeroed tail row (CW_TAIL_BYTES) -- all filled with finite floats
                // before the first tile)
                if (sx == 1 && c == 7) bfr[c] = (__bf16)1.0f;
                else bfr[c] = (__bf16)pl[(ci * 5 + 2 * (sx >> 1)) * CW_PITCH + kw];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const bf16x8 af = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + WIMG + (m * CA_KSTEPS + sx) * 1024 + lane * 16));
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[m], 0, 0, 0);
            }
        }
        if (stamp) stamp[2] = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this wave's reads of the buffer are done: refill it for the tile after next
        fetch(tile + 2 * (int)gridDim.x, buf);
        if (stamp) stamp[3] = __builtin_amdgcn_s_memrealtime();
        gdn_in_registers_hidden(acc, ldsb + lane * 16, ldsb + VEC + 512 + 16 * h, a.gdn_inverse & 1);
        if (stamp) stamp[4] = __builtin_amdgcn_s_memrealtime();
        {
            const int b = tile / a.tiles_per_img, t = tile - b * a.tiles_per_img;
            const int oh = (t / a.tiles_w) * 8 + wave, ow = (t % a.tiles_w) * 32 + j;
            const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(a.y16 + (size_t)b * 8 * oplane * 16), 0, (int)(8 * rec_bytes), 0x00020000);
            const unsigned voff = (oh < a.Ho && ow < a.Wo) ? ((unsigned)oh * a.Wo + ow) * 32 + 16 * h : 0xC0000000u;
#pragma unroll
            for (int m = 0; m < 4; ++m) store_f16k_tile_buf(acc[m], ry, voff + (unsigned)(2 * m) * rec_bytes, rec_bytes);
        }
        if (stamp) { stamp[5] = __builtin_amdgcn_s_memrealtime(); stamp += 6; }
    }
    if (pst) pst[4] = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (pst) pst[5] = __builtin_amdgcn_s_memrealtime();
}
}  // namespace

// First analysis layer: Conv2d(3 -> 128, k5, s2, p2) + GDN -> F16K (conv_a_gdn_f16k above).  x: float32 NCHW channel view.
extern "C" size_t masic_conv_a_packed_bytes(void) { return CA_WIMG_BYTES; }
extern "C" int masic_conv_a_pack_weight(const float* w, void* w_packed, void* stream) {
    MASIC_REQUIRE(w && w_packed, MASIC_ERR_ARG, "conv_a_pack_weight: null pointer");
    hipLaunchKernelGGL(pack_conv_a_kernel, dim3(4 * CA_KSTEPS * 64 / 256), dim3(256), 0, (hipStream_t)stream, w, (uint4*)w_packed);
    return masic_launch_status("conv_a_pack_weight");
}
namespace {
// One row per compiled kernel; plan_conv_a picks the row, the grid and the LDS bytes for the launcher and for masic_conv_a_plan_name.
typedef void (*ConvALaunchFn)(dim3 grid, size_t lds, hipStream_t st, const ConvAArgs& a);
template <auto K>
void conv_a_run(dim3 grid, size_t lds, hipStream_t st, const ConvAArgs& a) { launch_lds<K>(grid, 512, lds, st, a); }
struct ConvARow { const char* name; ConvALaunchFn launch; };
#define CONV_A_ROW(X3, OUT) {"conv_a_gdn_f16k<" #X3 ", " #OUT ">", conv_a_run<conv_a_gdn_f16k<X3, OUT>>}
const ConvARow CONV_A_ROWS[] = {{"conv_a_gdn_f16k_w", conv_a_run<conv_a_gdn_f16k_w>},
                                CONV_A_ROW(false, 0), CONV_A_ROW(false, 1), CONV_A_ROW(false, 2), CONV_A_ROW(false, 3),
                                CONV_A_ROW(true, 0), CONV_A_ROW(true, 1), CONV_A_ROW(true, 2)};
constexpr int CONV_A_MAX_WGS = 256;         // persistent workgroups: one per CU
struct ConvAPlan { const ConvARow* row; dim3 grid; size_t lds; int Ho, Wo, tiles_w, tiles_per_img, ntiles; };

// x_aligned16: the first input plane starts on a 16-byte boundary; gdn: a GDN follows; x3: its three-product form; out: 0 F16K, 1 fp8, 2 F16K
// plus the pre-GDN result
int plan_conv_a(int B, int Hi, int Wi, bool x_aligned16, bool gdn, bool x3, int out, ConvAPlan* p) {
    MASIC_REQUIRE(out >= 0 && out <= 2 && (gdn || (out == 0 && !x3)), MASIC_ERR_ARG, "conv_a_fwd: without a GDN the output is one F16K tensor");
    MASIC_REQUIRE(B > 0 && Hi > 0 && Wi > 0, MASIC_ERR_SHAPE, "conv_a_gdn_fwd: bad shape");
    p->Ho = (Hi + 4 - 5) / 2 + 1, p->Wo = (Wi + 4 - 5) / 2 + 1;
    p->tiles_w = ceil_div(p->Wo, 32), p->tiles_per_img = p->tiles_w * ceil_div(p->Ho, 8), p->ntiles = p->tiles_per_img * B;
    p->grid = dim3(p->ntiles < CONV_A_MAX_WGS ? p->ntiles : CONV_A_MAX_WGS);
    // the wave-private kernel where it applies; the shared-patch kernel for the rest (no GDN, x3, fp8 or pre-GDN outputs, unaligned input)
    const bool w = gdn && !x3 && out == 0 && Wi % 4 == 0 && x_aligned16 && ((size_t)Hi * Wi) % 4 == 0;
    p->row = &CONV_A_ROWS[w ? 0 : (!gdn ? 4 : (x3 ? 5 : 1) + out)];
    p->lds = w ? (size_t)CW_LDS : 65536 + CA_WIMG_BYTES + 1024 + (size_t)2 * CA_PATCH_BYTES;
    return MASIC_OK;
}

int conv_a_launch(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse, void* y_f16k, void* y_f8k,
                  float out_inv_scale, void* y_pre, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream) {
    MASIC_REQUIRE(x && w_packed && ((y_f16k != nullptr) != (y_f8k != nullptr)), MASIC_ERR_ARG, "conv_a_gdn_fwd: null pointer / exactly one output");
    MASIC_REQUIRE(gdn_packed != nullptr || (y_f16k != nullptr && y_pre == nullptr), MASIC_ERR_ARG, "conv_a_fwd: without a GDN the output is one F16K tensor");
    MASIC_REQUIRE(y_f8k == nullptr || out_inv_scale > 0.0f, MASIC_ERR_ARG, "conv_a_gdn_fwd: an fp8 output needs out_inv_scale > 0");
    MASIC_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && in_coff >= 0 && in_coff + 3 <= in_ctot, MASIC_ERR_SHAPE, "conv_a_gdn_fwd: bad shape");
    const bool gdn = gdn_packed != nullptr;
    ConvAPlan p;
    const int rc = plan_conv_a(B, Hi, Wi, ((size_t)x & 15) == 0, gdn, gdn && (gdn_inverse & 2) != 0, y_f8k != nullptr ? 1 : (y_pre != nullptr ? 2 : 0), &p);
    if (rc != MASIC_OK) return rc;
    ConvAArgs a{x, (const uint4*)w_packed, bias, (const uint4*)gdn_packed, (unsigned short*)y_f16k, gdn_inverse, Hi, Wi, in_ctot, in_coff,
                p.Ho, p.Wo, p.tiles_w, p.tiles_per_img, p.ntiles, (unsigned char*)y_f8k, out_inv_scale, (unsigned short*)y_pre, g_f16k_stamps};
    p.row->launch(p.grid, p.lds, (hipStream_t)stream, a);
    return masic_launch_status("conv_a_gdn_fwd");
}
}  // namespace
// the launch of the first-layer call that the form arguments name (include/masic_hip.h); the integers: ntiles tiles_w tiles_per_img Ho Wo
extern "C" int masic_conv_a_plan_name(int B, int Hi, int Wi, int x_aligned16, int gdn, int products, int out, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0, MASIC_ERR_ARG, "conv_a_plan_name: no buffer");
    buf[0] = 0;
    MASIC_REQUIRE(products == 1 || products == 3, MASIC_ERR_ARG, "conv_a_plan_name: products %d (1 or 3)", products);
    ConvAPlan p;
    const int rc = plan_conv_a(B, Hi, Wi, x_aligned16 != 0, gdn != 0, products == 3, out, &p);
    if (rc != MASIC_OK) return rc;
    const int v[5] = {p.ntiles, p.tiles_w, p.tiles_per_img, p.Ho, p.Wo};
    const bool ok = masic_plan_line_ints(buf, n, p.row->name, p.grid, 512, p.lds, v, 5);
    if (!ok) buf[0] = 0;
    MASIC_REQUIRE(ok, MASIC_ERR_ARG, "conv_a_plan_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}
// the same with the result optionally written as F8K fp8 (y_f8k, quantised with out_inv_scale) for an fp8-operand second layer
extern "C" int masic_conv_a_gdn_fwd_ex(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                                       void* y_f16k, void* y_f8k, float out_inv_scale, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream) {
    return conv_a_launch(x, w_packed, bias, gdn_packed, gdn_inverse, y_f16k, y_f8k, out_inv_scale, nullptr, B, Hi, Wi, in_ctot, in_coff, stream);
}
extern "C" int masic_conv_a_gdn_fwd(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                                    void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream) {
    return conv_a_launch(x, w_packed, bias, gdn_packed, gdn_inverse, y_f16k, nullptr, 0.0f, nullptr, B, Hi, Wi, in_ctot, in_coff, stream);
}
// training-mode form: F16K output plus the pre-GDN result (see masic_conv_f16k_gdn_dual_fwd)
extern "C" int masic_conv_a_gdn_dual_fwd(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                                         void* y_pre_f16k, void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream) {
    MASIC_REQUIRE(y_pre_f16k && y_f16k, MASIC_ERR_ARG, "conv_a_gdn_dual_fwd: null pointer");
    return conv_a_launch(x, w_packed, bias, gdn_packed, gdn_inverse, y_f16k, nullptr, 0.0f, y_pre_f16k, B, Hi, Wi, in_ctot, in_coff, stream);
}
// the convolution alone (no GDN), F16K out: Conv2d(3 -> 128, k5, s2, p2) on a float32 NCHW channel view
extern "C" int masic_conv_a_fwd(const float* x, const void* w_packed, const float* bias, void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff,
                                void* stream) {
    MASIC_REQUIRE(y_f16k != nullptr, MASIC_ERR_ARG, "conv_a_fwd: null pointer");
    return conv_a_launch(x, w_packed, bias, nullptr, 0, y_f16k, nullptr, 0.0f, nullptr, B, Hi, Wi, in_ctot, in_coff, stream);
}
