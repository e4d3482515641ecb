// gemm_f16k.hip -- 1x1 layers as DMA-staged GEMMs on F16K / F8K activations (gfx950 / MI355X).
// The nine 1x1 (transposed) convolutions of each GMM head (MASIC.py:330-468) with the K-loop machinery of conv_f16k: the
// register-streamed kernel of gemm_bf16.hip waits an L2 round trip every other k-step; here both operands are staged by
// buffer_load ... lds three 64-channel chunks deep, with counted vmcnt and inline-asm LDS reads.
//   tile 128 co x 256 px, 8 waves, wave w = all 128 co of pixels 32w .. 32w+31 (4 accumulator tiles)
//   stage (48 KiB) = weights [k16 4][hh][co 128][8] (16 KiB, a linear copy of the packed stream) | activations [k16 4][hh][px 256][8]
//   waves 0-3 fetch the weights (4 wave-instructions per chunk each), waves 4-7 the activations (8 each)
//
// Device helpers shared with the other F16K families (dma_buf16, ds_read128, lgkm_wait, mfma_f8, the tile stores): f16k_device.h.
#include "f16k_device.h"

namespace {

struct GemmF16kArgs {
    const unsigned short* x;      // F16K [B][Cin16][HW][16]
    const unsigned short* w;      // per 128-co block: [chunk][k16 4][hh][co 128][8]
    const float* bias;
    unsigned short* y16;          // F16K [B][out_ctot/16][HW][16] or null
    float* y32;                   // float32 NCHW view or null
    int Cin16, nchunks, Cout, HW, out_ctot, out_coff, act;
    const float* wscale;          // fp8 operands: per-output-channel dequantisation factor, else null
    unsigned char* y8;            // F8K output [B][out_ctot/32][HW][32] (quantised with out_inv_scale) or null
    float out_inv_scale;
};

// Up to three independent GEMMs over the same pixels in ONE launch (masic_gemm_f16k_group_fwd): the three entropy-parameter stacks
// of a GMM head (MASIC.py:330-468) are three 3-layer chains of 6 / 8 / 9 co-blocks x 32 pixel tiles each at 8 x 32 x 32 latents --
// 192 ... 288 workgroups on 256 CUs per launch, most of whose time is launch ramp, prologue and tail.  Layer i of the three stacks
// as one grid (blockIdx.y walks the co-blocks of group 0, then 1, then 2) is 20 ... 27 co-blocks = 640 ... 864 workgroups.
constexpr int GEMM_MAXG = 3;
struct GemmGroupArgs {
    GemmF16kArgs g[GEMM_MAXG];
    int cb_end[GEMM_MAXG];        // first co-block (blockIdx.y) past group i
    int n;
};

// fp8 operands: [co block][k32][hh][co 128][16 fp8] with per-output-channel scales ws[co] = max|W[co]| / 448
__global__ void wscale_gemm_f8k_kernel(const float* __restrict__ w, float* __restrict__ ws, int Cin, int Cout, int transposed) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= Cout) return;
    float m = 0.0f;
    for (int ci = 0; ci < Cin; ++ci) m = fmaxf(m, fabsf(transposed ? w[(size_t)ci * Cout + co] : w[(size_t)co * Cin + ci]));
    ws[co] = m > 0.0f ? m / 448.0f : 1.0f;
}
__global__ void pack_gemm_f8k_kernel(const float* __restrict__ w, const float* __restrict__ ws, unsigned char* __restrict__ wp, int Cin, int Cout,
                                     int nk32, int ncb, int transposed) {
    const size_t total = (size_t)ncb * nk32 * 4096;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int e = (int)(r & 15); r >>= 4;
        const int co = (int)(r & 127); r >>= 7;
        const int hh = (int)(r & 1); r >>= 1;
        const int k32 = (int)(r % nk32);
        const int cb = (int)(r / nk32);
        const int ci = k32 * 32 + hh * 16 + e, cog = cb * 128 + co;
        float v = 0.0f;
        if (ci < Cin && cog < Cout) v = (transposed ? w[(size_t)ci * Cout + cog] : w[(size_t)cog * Cin + ci]) / ws[cog];
        wp[i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.0f, 0, false) & 0xff);
    }
}

__global__ void pack_gemm_f16k_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int Cin, int Cout, int nk16,
                                      int ncb, int transposed) {
    // [co block][k16][hh][co 128][8]: chunks of any KC consecutive k16 blocks are contiguous
    const int nchunks = nk16;
    const size_t total = (size_t)ncb * nk16 * 2048;                          // bf16 elements
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int e = (int)(r & 7); r >>= 3;
        const int co = (int)(r & 127); r >>= 7;
        const int hh = (int)(r & 1); r >>= 1;
        const int k16 = (int)(r % nchunks);
        const int cb = (int)(r / nchunks);
        const int ci = k16 * 16 + hh * 8 + e, cog = cb * 128 + co;
        float v = 0.0f;
        if (ci < Cin && cog < Cout) v = transposed ? w[(size_t)ci * Cout + cog] : w[(size_t)cog * Cin + ci];
        const __bf16 bv = (__bf16)v;
        wp[i] = __builtin_bit_cast(unsigned short, bv);
    }
}

// KC: 16-channel blocks per chunk.  KC = 2 keeps a stage at 24 KiB: two workgroups per CU, which is what a grid of
// 288 workgroups (nine 128-channel blocks x 32 pixel tiles) on 256 CUs needs.
// F8: fp8 operands (F8K input, 32-channel blocks; one MFMA = two consecutive blocks of the chunk, one per lane half)
template <int KC, bool F8 = false>
__global__ __launch_bounds__(512, KC == 2 ? 2 : 1) void gemm_f16k(const GemmGroupArgs ga) {
    static_assert(!F8 || KC % 2 == 0, "fp8 operands consume channel blocks in pairs");
    // group of this workgroup (uniform: scalar selects on blockIdx.y)
    GemmF16kArgs a = ga.g[0];
    int cb0 = 0;
    if (ga.n > 1 && (int)blockIdx.y >= ga.cb_end[0]) { a = ga.g[1]; cb0 = ga.cb_end[0]; }
    if (ga.n > 2 && (int)blockIdx.y >= ga.cb_end[1]) { a = ga.g[2]; cb0 = ga.cb_end[1]; }
    const int cblk = (int)blockIdx.y - cb0;                                  // co-block inside the group
    constexpr int ACT0 = KC * 4096, STAGE = KC * 12288, NS = 3;
    constexpr int WPW = KC, APW = 2 * KC;                                    // weight / activation DMA pieces per wave per chunk
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const bool wrole = wave < 4;
    const int wq = wave & 3;
    const int p0 = blockIdx.x * 256, m0 = cblk * 128, b = blockIdx.z;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + (size_t)b * a.Cin16 * a.HW * 16), 0, a.Cin16 * a.HW * 32, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.w + (size_t)cblk * a.nchunks * (KC * 2048)), 0, a.nchunks * (KC * 4096), 0x00020000);
    // activation pieces of this wave: piece I = k*4 + wq, k < 8: k16 = I >> 3, hh = (I >> 2) & 1, pixel block = I & 3 = wq
    const int px = wq * 64 + lane;
    const int avoff = p0 + px < a.HW ? px * 32 : 0x7ffffff0;                  // + hh*16 per piece
    auto issue = [&](int c, int stage) {
        unsigned char* st = lds + stage * STAGE;
        if (wrole) {
#pragma unroll
            for (int k = 0; k < WPW; ++k) dma_buf16(rw, st + (k * 4 + wq) * 1024, lane * 16, c * (KC * 4096) + (k * 4 + wq) * 1024);
        } else {
#pragma unroll
            for (int k = 0; k < APW; ++k) {
                const int k16 = k >> 1, hh = k & 1;                           // I = k*4 + wq -> (I >> 3, (I >> 2) & 1)
                dma_buf16(rx, st + ACT0 + k16 * 8192 + hh * 4096 + wq * 1024, avoff + hh * 16, ((c * KC + k16) * a.HW + p0) * 32);
            }
        }
    };
    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = 0.0f;
    issue(0, 0);
    issue(1, 1);
    if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APW) : "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned al = ldsb + (F8 ? j * 16 + h * 4096 : (h * 128 + j) * 16);
    const unsigned bl = ldsb + ACT0 + (F8 ? (wave * 32 + j) * 16 + h * 8192 : (h * 256 + wave * 32 + j) * 16);
    int cs = 0, ps = 2;                                                      // consumer / producer stage
    for (int c = 0; c < a.nchunks; ++c) {
        issue(c + 2, ps);                                                     // past the end: reads as zeros into a free stage
        ps = ps == NS - 1 ? 0 : ps + 1;
        const unsigned wa = al + cs * STAGE, ba = bl + cs * STAGE;
        constexpr int NQ = F8 ? 2 : 1, NKS = F8 ? KC / 2 : KC;
        v4u af[2][4][NQ], bfr[2][NQ];
        auto request = [&](auto ic, auto bc) {
            constexpr int i = decltype(ic)::value, buf = decltype(bc)::value;
            if constexpr (F8) {
                ds_read128<i * 16384>(bfr[buf][0], ba);
                ds_read128<i * 16384 + 4096>(bfr[buf][1], ba);
                static_for<0, 4>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    ds_read128<i * 8192 + m * 512>(af[buf][m][0], wa);
                    ds_read128<i * 8192 + m * 512 + 2048>(af[buf][m][1], wa);
                });
            } else {
                ds_read128<i * 8192>(bfr[buf][0], ba);
                static_for<0, 4>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    ds_read128<i * 4096 + m * 512>(af[buf][m][0], wa);
                });
            }
        };
        request(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        static_for<0, NKS>([&](auto ic) {
            constexpr int i = decltype(ic)::value, buf = i & 1;
            if constexpr (i + 1 < NKS) request(std::integral_constant<int, i + 1>{}, std::integral_constant<int, (i + 1) & 1>{});
            if constexpr (F8) {
                lgkm_wait<(i + 1 < NKS ? 10 : 0)>(bfr[buf][0], bfr[buf][1], af[buf][0][0], af[buf][0][1], af[buf][1][0], af[buf][1][1],
                                                   af[buf][2][0], af[buf][2][1], af[buf][3][0], af[buf][3][1]);
                const v8i b8 = cat8(bfr[buf][0], bfr[buf][1]);
                static_for<0, 4>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    acc[m] = mfma_f8(cat8(af[buf][m][0], af[buf][m][1]), b8, acc[m]);
                });
            } else {
                lgkm_wait<(i + 1 < NKS ? 5 : 0)>(bfr[buf][0], af[buf][0][0], af[buf][1][0], af[buf][2][0], af[buf][3][0]);
                static_for<0, 4>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[buf][m][0]), __builtin_bit_cast(bf16x8, bfr[buf][0]), acc[m], 0, 0, 0);
                });
            }
        });
        cs = cs == NS - 1 ? 0 : cs + 1;
        if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WPW) : "memory");   // chunk c+1 has landed, chunk c+2 may stay in flight
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APW) : "memory");
        __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- epilogue: (dequantisation) + bias + activation -> F16K, F8K or float32 NCHW view
    if constexpr (F8) {
        const float* sp = a.wscale + m0 + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][e] *= sp[m * 32 + (e & 3) + 8 * (e >> 2)];
            }
    }
    if (a.bias != nullptr) {
        const float* bp = a.bias + m0 + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) {
                float bv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) bv[e] = bp[m * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][e] += bv[e];
            }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = apply_act(acc[m][e], a.act);
    const int p = p0 + wave * 32 + j;
    if (p >= a.HW) return;
    if (a.y32 != nullptr) {
        float* yb = a.y32 + ((size_t)b * a.out_ctot + a.out_coff + m0 + 4 * h) * a.HW + p;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) {
#pragma unroll
                for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * (unsigned)a.HW] = acc[m][e];
            }
    } else if (a.y8 != nullptr) {
        const int c32 = (a.out_coff + m0) >> 5;
        unsigned char* yb = a.y8 + (((size_t)b * (a.out_ctot >> 5) + c32) * a.HW + p) * 32 + 16 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) store_f8k_tile(acc[m], yb + (size_t)m * a.HW * 32, a.out_inv_scale);
    } else {
        const int c16 = (a.out_coff + m0) >> 4;
        unsigned short* yb = a.y16 + (((size_t)b * (a.out_ctot >> 4) + c16) * a.HW + p) * 16 + 8 * h;
        const unsigned op16 = (unsigned)a.HW * 16;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) store_f16k_tile(acc[m], yb + (size_t)(2 * m) * op16, op16);
    }
}


// ---- gemm_f16k2: the same GEMMs with 128 co x 64 px per WAVE (8 accumulator tiles) and the activations NOT staged through LDS.
// In gemm_f16k every wave owns all 128 output channels of only 32 pixels: each of its MFMAs needs a fresh weight fragment from LDS, so a
// k-step is 5 ds_read_b128 for 4 MFMAs -- 320 LDS cycles against 256 MFMA cycles per CU and k-step: the kernel was bound by its LDS reads
// (0.54 PFLOP/s alone), and a 32-channel chunk was only 8 MFMAs per wave and barrier.  Here:
//   * a wave holds 4 (co) x 2 (px) tiles: 4 weight fragments feed 8 MFMAs;
//   * its activation operand is a pixel's own F16K half-record -- 16 contiguous bytes per lane, 1 KiB per wave-instruction, nothing another
//     wave of the workgroup needs (all four waves share the CO block, not the pixels): it is loaded straight into registers
//     (buffer_load_dwordx4, one 64-channel chunk ahead), so LDS holds the weight ring only (3 x 16 KiB) and carries 4 reads per 8 MFMAs;
//   * a chunk is 64 channels = 32 MFMAs per wave and barrier; workgroup = 4 waves = 128 co x 256 px, two workgroups per CU (independent
//     barriers: one's prologue / epilogue under the other's K loop);
//   * per-iteration issue order [8 activation loads of chunk c+1][4 weight DMA pieces of chunk c+2], then s_waitcnt vmcnt(4): the
//     activations of the next chunk and the weights issued an iteration earlier have landed, the newest weight pieces stay in flight;
//   * workgroup n runs on XCD n % 8 (hardware round-robin): image b = n % 8 (+ 8 per pass), so an image's activations are fetched into ONE
//     XCD's L2, and inside an image the pixel tile is the fastest index: the workgroups resident together share few weight blocks.
constexpr int G2_KC = 4, G2_STAGE = G2_KC * 4096, G2_NS = 3;
template <int N>
__device__ __forceinline__ void vm_wait(v4u& a, v4u& b, v4u& c, v4u& d, v4u& e, v4u& f, v4u& g, v4u& h) {
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(N) : "memory");
}
__device__ __forceinline__ void buf_load128(v4u& dst, unsigned voff, v4u rsrc, unsigned soff) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__global__ __launch_bounds__(256, 2) void gemm_f16k2(const GemmGroupArgs ga, int B, int npx, int tiles_per_img) {
    // workgroup -> (image, co-block over all groups, pixel tile): workgroup n runs on XCD n % 8 (hardware round-robin), image b = n % 8 (+ 8
    // per pass), so an image's activations are fetched into ONE XCD's L2; inside an image the pixel tile is the fastest index.  Measured
    // (PMC FETCH_SIZE x 2, the 768 -> 3 x 1152 layer at 8 x 32 x 32): 97 MB fetched per launch against 204 MB for gemm_f16k's blockIdx.y-major
    // order (operands: 18 MB).  A 4 x 2 XCD grid (pixel quarter x co-block half, half of the weights resident per L2) fetched 109 MB and ran
    // within 3 % of this order: the launch is not bound by its fabric traffic.
    // (Fewer than 8 images -- the bitstream coder runs one: plain order, every workgroup live; the XCD order would park B of 8 XCDs' worth.)
    const int n = blockIdx.x, kx = B >= 8 ? n >> 3 : n % tiles_per_img;
    const int b = B >= 8 ? (n & 7) + 8 * ((n >> 3) / tiles_per_img) : n / tiles_per_img;
    if (b >= B) return;
    const int t = kx % tiles_per_img, pxt = t % npx, cbg = t / npx;
    GemmF16kArgs a = ga.g[0];
    int cb0 = 0;
    if (ga.n > 1 && cbg >= ga.cb_end[0]) { a = ga.g[1]; cb0 = ga.cb_end[0]; }
    if (ga.n > 2 && cbg >= ga.cb_end[1]) { a = ga.g[2]; cb0 = ga.cb_end[1]; }
    const int cblk = cbg - cb0;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int p0 = pxt * 256, m0 = cblk * 128;
    const int nchunks = a.nchunks;                                                 // 64-channel chunks (Cin padded to a multiple of 64 by the pack)
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(a.w + (size_t)cblk * nchunks * (G2_KC * 2048)), 0, nchunks * G2_STAGE, 0x00020000);
    // activation descriptor by hand (inline-asm loads take it as four SGPRs): base, stride 0, bytes, the flags make_buffer_rsrc is given above
    const unsigned long long xb = (unsigned long long)(a.x + (size_t)b * a.Cin16 * a.HW * 16);
    v4u rx;
    rx[0] = __builtin_amdgcn_readfirstlane((unsigned)xb);
    rx[1] = __builtin_amdgcn_readfirstlane((unsigned)(xb >> 32) & 0xffffu);
    rx[2] = __builtin_amdgcn_readfirstlane((unsigned)(a.Cin16 * a.HW * 32));
    rx[3] = 0x00020000u;
    unsigned bvoff[2];                                                             // the lane's half-record in k16 block 0, per pixel sub-tile
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = p0 + wave * 64 + q * 32 + j;
        bvoff[q] = p < a.HW ? (unsigned)p * 32u + 16u * h : 0xC0000000u;
    }
    const unsigned kstride = (unsigned)a.HW * 32u;                                 // bytes between k16 blocks
    auto issue_w = [&](int c) {                                                    // 16 KiB of weights: 4 pieces per wave
        unsigned char* st = lds + (c % G2_NS) * G2_STAGE;
#pragma unroll
        for (int k = 0; k < 4; ++k) dma_buf16(rw, st + (k * 4 + wave) * 1024, lane * 16, c * G2_STAGE + (k * 4 + wave) * 1024);
    };
    v4u bq[2][G2_KC][2];                                                            // [parity][k16 of the chunk][pixel sub-tile]
    auto issue_b = [&](auto PC, int c) {
        constexpr int pc = decltype(PC)::value;
        static_for<0, G2_KC>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)(c * G2_KC + i) * kstride);
            buf_load128(bq[pc][i][0], bvoff[0], rx, so);
            buf_load128(bq[pc][i][1], bvoff[1], rx, so);
        });
    };
    f32x16 acc[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][m][e] = 0.0f;
    // prologue: activations of chunk 0, weights of chunks 0 and 1
    issue_b(std::integral_constant<int, 0>{}, 0);
    issue_w(0);
    issue_w(1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                              // (the activation registers are claimed by the first body's wait below)
    __builtin_amdgcn_s_barrier();
    const unsigned al = ldsb + (h * 128 + j) * 16;
    auto body = [&](auto PC, int c) {
        constexpr int pc = decltype(PC)::value;
        issue_b(std::integral_constant<int, pc ^ 1>{}, c + 1);                     // past the end: out of range, reads as zeros
        issue_w(c + 2);
        const unsigned wa = al + (c % G2_NS) * G2_STAGE;
        v4u af[2][4];
        static_for<0, 4>([&](auto M) { constexpr int m = decltype(M)::value; ds_read128<m * 512>(af[0][m], wa); });
        static_for<0, G2_KC>([&](auto I) {
            constexpr int i = decltype(I)::value, fb = i & 1;
            if constexpr (i + 1 < G2_KC)
                static_for<0, 4>([&](auto M) { constexpr int m = decltype(M)::value; ds_read128<(i + 1) * 4096 + m * 512>(af[fb ^ 1][m], wa); });
            lgkm_wait<(i + 1 < G2_KC ? 4 : 0)>(af[fb][0], af[fb][1], af[fb][2], af[fb][3]);
            static_for<0, 2>([&](auto Q) {
                constexpr int q = decltype(Q)::value;
                const bf16x8 bv = __builtin_bit_cast(bf16x8, bq[pc][i][q]);
                static_for<0, 4>([&](auto M) {
                    constexpr int m = decltype(M)::value;
                    acc[q][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[fb][m]), bv, acc[q][m], 0, 0, 0);
                });
            });
        });
        // chunk c+1: its activations (issued above, the 8 oldest of this iteration) and its weights (issued one iteration ago) have landed when at
        // most the 4 newest weight pieces are still in flight
        vm_wait<4>(bq[pc ^ 1][0][0], bq[pc ^ 1][0][1], bq[pc ^ 1][1][0], bq[pc ^ 1][1][1], bq[pc ^ 1][2][0], bq[pc ^ 1][2][1], bq[pc ^ 1][3][0], bq[pc ^ 1][3][1]);
        __builtin_amdgcn_s_barrier();
    };
    {
        // claim chunk 0's activation registers (their loads completed with the prologue's wait: they are older than the weight pieces)
        vm_wait<4>(bq[0][0][0], bq[0][0][1], bq[0][1][0], bq[0][1][1], bq[0][2][0], bq[0][2][1], bq[0][3][0], bq[0][3][1]);
    }
    int c = 0;
    for (; c + 1 < nchunks; c += 2) {
        body(std::integral_constant<int, 0>{}, c);
        body(std::integral_constant<int, 1>{}, c + 1);
    }
    if (c < nchunks) body(std::integral_constant<int, 0>{}, c);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- epilogue: bias + activation -> F16K or float32 NCHW view
    if (a.bias != nullptr) {
        const float* bp = a.bias + m0 + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m0 + m * 32 < a.Cout) {
                float bv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) bv[e] = bp[m * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[q][m][e] += bv[e];
            }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][m][e] = apply_act(acc[q][m][e], a.act);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = p0 + wave * 64 + q * 32 + j;
        if (p >= a.HW) continue;
        if (a.y32 != nullptr) {
            float* yb = a.y32 + ((size_t)b * a.out_ctot + a.out_coff + m0 + 4 * h) * a.HW + p;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m0 + m * 32 < a.Cout) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * (unsigned)a.HW] = acc[q][m][e];
                }
        } else {
            const int c16 = (a.out_coff + m0) >> 4;
            unsigned short* yb = a.y16 + (((size_t)b * (a.out_ctot >> 4) + c16) * a.HW + p) * 16 + 8 * h;
            const unsigned op16 = (unsigned)a.HW * 16;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m0 + m * 32 < a.Cout) store_f16k_tile(acc[q][m], yb + (size_t)(2 * m) * op16, op16);
        }
    }
}

}  // namespace

// Up to 18 weight packs in one launch (blockIdx.y = job): the nine 1x1 layers of an entropy-parameter head, each for the forward GEMM
// and -- transposed -- for the input-gradient GEMM of the training step, whose weights change with every optimizer step (one launch per
// pack was 36 launches of ~5 us per head pair and step).
namespace {
constexpr int GEMM_PACK_MAXJ = 18;
struct GemmPackJobs {
    const float* w[GEMM_PACK_MAXJ];
    unsigned short* wp[GEMM_PACK_MAXJ];
    int Cin[GEMM_PACK_MAXJ], Cout[GEMM_PACK_MAXJ], transposed[GEMM_PACK_MAXJ];
};
__global__ void pack_gemm_f16k_multi_kernel(const GemmPackJobs J) {
    const int jb = blockIdx.y;
    const float* __restrict__ w = J.w[jb];
    unsigned short* __restrict__ wp = J.wp[jb];
    const int Cin = J.Cin[jb], Cout = J.Cout[jb], transposed = J.transposed[jb];
    const int nk16 = ((Cin + 15) / 16 + 3) / 4 * 4, ncb = (Cout + 127) / 128;
    const size_t total = (size_t)ncb * nk16 * 2048;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int e = (int)(r & 7); r >>= 3;
        const int co = (int)(r & 127); r >>= 7;
        const int hh = (int)(r & 1); r >>= 1;
        const int k16 = (int)(r % nk16);
        const int cb = (int)(r / nk16);
        const int ci = k16 * 16 + hh * 8 + e, cog = cb * 128 + co;
        float v = 0.0f;
        if (ci < Cin && cog < Cout) v = transposed ? w[(size_t)ci * Cout + cog] : w[(size_t)cog * Cin + ci];
        const __bf16 bv = (__bf16)v;
        wp[i] = __builtin_bit_cast(unsigned short, bv);
    }
}
}  // namespace

// jobs: n (<= 18) packs as masic_gemm_f16k_pack_weight would make them, one launch: w[i] / wp[i] / Cin[i] / Cout[i] / transposed[i]
extern "C" int masic_gemm_f16k_pack_weights(const float* const* w, void* const* wp, const int* Cin, const int* Cout, const int* transposed, int n, void* stream) {
    MASIC_REQUIRE(w && wp && Cin && Cout && transposed && n >= 1 && n <= GEMM_PACK_MAXJ, MASIC_ERR_ARG, "gemm_f16k_pack_weights: 1 ... %d jobs", GEMM_PACK_MAXJ);
    GemmPackJobs J{};
    size_t most = 0;
    for (int i = 0; i < n; ++i) {
        MASIC_REQUIRE(w[i] && wp[i] && Cin[i] > 0 && Cout[i] > 0, MASIC_ERR_ARG, "gemm_f16k_pack_weights: bad job %d", i);
        J.w[i] = w[i]; J.wp[i] = (unsigned short*)wp[i]; J.Cin[i] = Cin[i]; J.Cout[i] = Cout[i]; J.transposed[i] = transposed[i];
        const size_t total = (size_t)ceil_div(Cout[i], 128) * round_up(ceil_div(Cin[i], 16), 4) * 2048;
        most = most > total ? most : total;
    }
    int nb = (int)((most + 255) / 256);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(pack_gemm_f16k_multi_kernel, dim3(nb, n), dim3(256), 0, (hipStream_t)stream, J);
    return masic_launch_status("gemm_f16k_pack_weights");
}

extern "C" size_t masic_gemm_f16k_packed_bytes(int Cin, int Cout) {
    return (size_t)ceil_div(Cout, 128) * round_up(ceil_div(Cin, 16), 4) * 4096;
}

extern "C" int masic_gemm_f16k_pack_weight(const float* w, void* wp, int Cin, int Cout, int transposed, void* stream) {
    MASIC_REQUIRE(w && wp && Cin > 0 && Cout > 0, MASIC_ERR_ARG, "gemm_f16k_pack_weight: bad argument");
    const int nchunks = round_up(ceil_div(Cin, 16), 4), ncb = ceil_div(Cout, 128);          // k16 blocks, padded to a multiple of 4
    const size_t total = (size_t)ncb * nchunks * 2048;
    int nb = (int)((total + 255) / 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(pack_gemm_f16k_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)wp, Cin, Cout, nchunks, ncb, transposed);
    return masic_launch_status("gemm_f16k_pack_weight");
}

// y = act(W x + b), x in F16K with Cin a multiple of 16; output F16K (y_f16k: out_ctot channels, written at out_coff) or a
// float32 NCHW channel view (y_nchw).  Cout must be a multiple of 32.
extern "C" int masic_gemm_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, void* y_f16k, float* y_nchw,
                                   int B, int Cin, int Cout, int HW, int out_ctot, int out_coff, int act, void* stream) {
    const masic_gemm_group_t g{x_f16k, w_packed, nullptr, bias, y_f16k, nullptr, y_nchw, 0.0f, Cin, Cout, out_ctot, out_coff, act};
    return masic_gemm_f16k_group_fwd(&g, 1, B, HW, stream);
}

// Up to three such layers over the same B x HW pixels in one launch (GemmGroupArgs above).  All groups bf16 operands (wscale NULL
// everywhere: x is F16K, Cin % 16 == 0) or all fp8 (wscale set everywhere: x is F8K, Cin % 32 == 0, weights from
// masic_gemm_f8k_pack_weight); per group exactly one of y_f16k / y_f8k / y_nchw.  Results are those of the single-layer calls, bit for bit.
extern "C" int masic_gemm_f16k_group_fwd(const masic_gemm_group_t* groups, int ngroups, int B, int HW, void* stream) {
    MASIC_REQUIRE(groups != nullptr && ngroups >= 1 && ngroups <= GEMM_MAXG, MASIC_ERR_ARG, "gemm_f16k_group_fwd: 1 ... %d groups", GEMM_MAXG);
    MASIC_REQUIRE(B > 0 && HW > 0, MASIC_ERR_SHAPE, "gemm_f16k_group_fwd: non-positive size");
    const bool f8 = groups[0].wscale != nullptr;
    const int cblk = f8 ? 32 : 16;
    GemmGroupArgs ga{};
    int ncb = 0;
    for (int i = 0; i < ngroups; ++i) {
        const masic_gemm_group_t& g = groups[i];
        MASIC_REQUIRE((g.wscale != nullptr) == f8, MASIC_ERR_ARG, "gemm_f16k_group_fwd: bf16 and fp8 groups cannot share a launch");
        MASIC_REQUIRE(g.x && g.w_packed && ((g.y_f16k != nullptr) + (g.y_f8k != nullptr) + (g.y_nchw != nullptr) == 1), MASIC_ERR_ARG,
                      "gemm_f16k_fwd: need input, weights and exactly one output");
        MASIC_REQUIRE(g.Cin > 0 && g.Cin % cblk == 0 && g.Cout > 0 && g.Cout % 32 == 0, MASIC_ERR_UNSUPPORTED,
                      "gemm_f16k_fwd: needs Cin %% %d == 0 and Cout %% 32 == 0", cblk);
        const int oalign = f8 ? 32 : 16;
        MASIC_REQUIRE(g.out_coff >= 0 && g.out_coff + g.Cout <= g.out_ctot && (g.y_nchw != nullptr || (g.out_ctot % oalign == 0 && g.out_coff % oalign == 0)),
                      MASIC_ERR_SHAPE, "gemm_f16k_fwd: output channel view");
        MASIC_REQUIRE(g.y_f8k == nullptr || g.out_inv_scale > 0.0f, MASIC_ERR_ARG, "gemm_f8k_fwd: an fp8 output needs out_inv_scale > 0");
        MASIC_REQUIRE((long)(g.Cin / cblk) * HW * 32 < (1l << 31), MASIC_ERR_UNSUPPORTED, "gemm_f16k_fwd: activation plane too large for 32-bit offsets");
        ncb += ceil_div(g.Cout, 128);
        ga.cb_end[i] = ncb;
    }
    ga.n = ngroups;
    bool f8_out = false;
    for (int i = 0; i < ngroups; ++i) f8_out = f8_out || groups[i].y_f8k != nullptr;
    // bf16 operands, no fp8 output: gemm_f16k2 (64-channel chunks).  Otherwise gemm_f16k: bf16 operands in 32-channel chunks, 72 KiB of
    // LDS -- two workgroups per CU, or one next to a workgroup of another stream's kernel.  (The 64-channel form, 144 KiB, a CU to itself,
    // was as fast when the launch had the chip to itself, but inside the three-stream forward it shut the other streams' kernels out of
    // its CUs: 2.54 -> 2.41 ms per step at 8 x 512 x 512 with KC = 2 everywhere, A/B on one box, 100 replays each, twice.)  fp8
    // operands: 128-channel chunks only.
    const int kc = f8 ? 4 : (f8_out ? 2 : G2_KC);
    for (int i = 0; i < ngroups; ++i) {
        const masic_gemm_group_t& g = groups[i];
        const int cin_b = g.Cin / cblk, nkb = round_up(cin_b, 4);
        ga.g[i] = GemmF16kArgs{(const unsigned short*)g.x, (const unsigned short*)g.w_packed, g.bias, (unsigned short*)g.y_f16k, g.y_nchw,
                               cin_b, nkb / kc, g.Cout, HW, g.out_ctot, g.out_coff, g.act, g.wscale, (unsigned char*)g.y_f8k, g.out_inv_scale};
    }
    if (!f8 && !f8_out) {
        const int npx = ceil_div(HW, 256), tiles_per_img = npx * ncb;
        launch_lds<gemm_f16k2>(dim3(B >= 8 ? 8 * tiles_per_img * ceil_div(B, 8) : B * tiles_per_img), 256, G2_NS * G2_STAGE, (hipStream_t)stream, ga, B, npx, tiles_per_img);
        return masic_launch_status("gemm_f16k_fwd");
    }
    const dim3 grid(ceil_div(HW, 256), ncb, B);
    if (f8) launch_lds<gemm_f16k<4, true>>(grid, 512, 3 * 4 * 12288, (hipStream_t)stream, ga);
    else launch_lds<gemm_f16k<2>>(grid, 512, 3 * 2 * 12288, (hipStream_t)stream, ga);
    return masic_launch_status("gemm_f16k_fwd");
}

// fp8 (e4m3) operand form of masic_gemm_f16k_*: x in F8K (Cin % 32 == 0), weights from masic_gemm_f8k_pack_weight (which also
// writes the per-output-channel weight scales); wscale[Cout] = those scales x the input tensor's scale.  Exactly one output:
// y_f16k (bf16, next layer runs bf16 operands), y_f8k (fp8, quantised with out_inv_scale) or y_nchw (float32 view).
extern "C" size_t masic_gemm_f8k_packed_bytes(int Cin, int Cout) {
    return (size_t)ceil_div(Cout, 128) * round_up(ceil_div(Cin, 32), 4) * 4096;
}

extern "C" int masic_gemm_f8k_pack_weight(const float* w, void* wp, float* wscale, int Cin, int Cout, int transposed, void* stream) {
    MASIC_REQUIRE(w && wp && wscale && Cin > 0 && Cout > 0, MASIC_ERR_ARG, "gemm_f8k_pack_weight: bad argument");
    const int nk32 = round_up(ceil_div(Cin, 32), 4), ncb = ceil_div(Cout, 128);
    hipLaunchKernelGGL(wscale_gemm_f8k_kernel, dim3(ceil_div(Cout, 128)), dim3(128), 0, (hipStream_t)stream, w, wscale, Cin, Cout, transposed);
    const size_t total = (size_t)ncb * nk32 * 4096;
    int nb = (int)((total + 255) / 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(pack_gemm_f8k_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, w, (const float*)wscale, (unsigned char*)wp, Cin, Cout, nk32, ncb, transposed);
    return masic_launch_status("gemm_f8k_pack_weight");
}

extern "C" int masic_gemm_f8k_fwd(const void* x_f8k, const void* w_packed, const float* wscale, const float* bias, void* y_f16k, void* y_f8k,
                                  float* y_nchw, float out_inv_scale, int B, int Cin, int Cout, int HW, int out_ctot, int out_coff, int act, void* stream) {
    MASIC_REQUIRE(wscale != nullptr, MASIC_ERR_ARG, "gemm_f8k_fwd: need input, weights, scales and exactly one output");
    const masic_gemm_group_t g{x_f8k, w_packed, wscale, bias, y_f16k, y_f8k, y_nchw, out_inv_scale, Cin, Cout, out_ctot, out_coff, act};
    return masic_gemm_f16k_group_fwd(&g, 1, B, HW, stream);
}
