// conv3x3_resident.hip -- 3x3 layers with LDS-resident weights on F16K activations (gfx950 / MI355X).
// Conv2d(CI -> CO, k3, s1, p1) (or its input gradient) on F16K for CI in {16, 32, 64} (16: a 3- or 6-channel picture zero-padded to
// one record per pixel), CO in {32, 64}: the 32- and 64-channel stages of Independent_EN and its two input layers (reference
// MASIC.py:149-164, 1456-1482 -- 28 of its 40 convolutions, and the input gradients of 24 of them in training).  K = 288 is 18 MFMA k-steps: on
// conv_f16k such a layer is three quarters per-workgroup prologue / epilogue (171 us per launch at 8 x 512^2 against an HBM floor of
// ~45).  Here the whole weight tensor (18 KiB of bf16 fragments) stays in LDS for the life of a PERSISTENT workgroup that walks
// over 16 x 32-pixel tiles of one XCD's share of the images:
//   * waves 8-11 are loaders: per tile they issue the 39 `buffer_load ... lds` pieces of the (18 x 34 pixel x 32 channel) patch two
//     tiles ahead into a ring of three buffers (10 pieces each: a single wave needs 60-185 cycles per piece, 121 -> see DESIGN.md us
//     per launch with one loader) and wait -- with a counted vmcnt, nothing else is on their counter -- for the patch of the
//     NEXT tile; padding pixels are out-of-range buffer offsets (zero fill);
//   * waves 0-7 own two image rows of the tile each: 18 k-steps x (1 weight + 2 patch fragments by ds_read_b128, 2 MFMAs), then
//     the F16K epilogue of conv_f16k (bias, activation, act'(mask), pre-residual copy, residual adds, 16-byte stores);
//   * ONE barrier per tile hands the landed patch to the compute waves and the drained buffer back to the loader.
// HBM-bound by design: 39 KiB in + 32 KiB out (+ residuals) per tile against 36 MFMAs per wave.
//
// Device helpers shared with the other F16K families (dma_buf16, ds_read128, lgkm_wait, pack2bf, the tile epilogues): f16k_device.h.
#include "f16k_device.h"

struct C3Args {
    const unsigned short* x; const unsigned short* w; const float* bias;
    const unsigned short* res1; const unsigned short* res2; const unsigned short* mask16; unsigned short* y_pre; unsigned short* y16;
    int B, H, W, in_ctot16, in_c16off, out_ctot, out_coff, res_ctot, act;
    float mask_slope;
    int tiles_w, tiles_per_image, ntiles;
    // backward chains of a residual block (masic_amd/autograd.py: EnhancementBlockFn): a SECOND output y2 = y * act'(mask2) -- the next
    // layer's dy, which a separate elementwise pass used to make -- and per-channel sums (the bias gradient) of the value before the
    // residual adds (sum_of = 1) or of y2 (sum_of = 2), bf16-rounded as stored, as per-wave partials [gridDim.x * 8][32]
    const unsigned short* mask2; unsigned short* y2; float mask2_slope;
    float* sum_part; int sum_of;
};

namespace {

// s_barrier that the compiler does not move LDS accesses across (the intrinsic alone is "no memory"); no hardware wait is added:
// what crosses it here was waited for explicitly (the loader's vmcnt) or consumed by MFMAs (the compute waves' fragment reads)
__device__ __forceinline__ void wg_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int CI, int C, bool EX = false>      // input channels (a multiple of 16), output channels; EX: the second output / channel sums of C3Args
__global__ __launch_bounds__(768, 1) void conv3x3_resident_f16k(const C3Args a) {
    constexpr int KB = CI / 16;                        // 16-channel blocks = 32-byte records per input pixel
    constexpr int NM = C / 32;                         // 32-channel accumulator tiles per pixel; a wave owns one of them for two image rows
    constexpr int TH = 16 / NM, TW = 32, PWd = TW + 2, NPIX = (TH + 2) * PWd;
    constexpr int PREC = KB * 2 * NPIX;                // 16-byte records of a patch: [kb][k-half][pixel]
    constexpr int NI = (PREC + 63) / 64;               // DMA wave-instructions per patch
    constexpr int PBYTES = NI * 1024;
    constexpr int SLAB = 2 * C * 16;                   // one (tap, kb) weight slab: [k-half][co]
    constexpr int WBYTES = 9 * KB * SLAB;
    constexpr int NWI = WBYTES / 1024;
    constexpr int NBUF = WBYTES + 3 * PBYTES + 1024 <= 160 * 1024 ? 3 : 2;   // patch ring (64 -> 64: 72 KiB of weights leave room for two 43-KiB patches)
    constexpr int PD = NBUF - 1;                       // tiles of look-ahead
    constexpr int NLW = 4;                             // loader waves (8 .. 11): one wave issues a 1-KiB piece every 60-185 cycles
    constexpr int NIW = (NI + NLW - 1) / NLW;          // pieces per loader wave and patch (the last wave pads with sink pieces)
    constexpr int NWW = (NWI + NLW - 1) / NLW;         // weight pieces per loader wave
    constexpr int SINK = WBYTES + NBUF * PBYTES;       // 1 KiB that padding pieces write zeros to
    static_assert((C == 32 || C == 64) && (CI == 16 || CI == 32 || CI == 64), "8 compute waves = (16 / NM row pairs) x NM channel tiles");
    static_assert(PD * NIW + NWW <= 60 && WBYTES % 1024 == 0 && SINK + 1024 <= 160 * 1024, "vmcnt is 6 bits; whole DMA pieces; LDS");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];      // [weights][NBUF patches][sink]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    // tiles of XCD k (workgroup ids go round-robin over the 8 XCDs) are one contiguous eighth of the tile list -- whole images when
    // B % 8 == 0 -- so the halos neighbouring tiles share are re-read from that XCD's L2
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const int per = (a.ntiles + 7) >> 3;
    const int t_end = (xcd + 1) * per < a.ntiles ? (xcd + 1) * per : a.ntiles;
    const int t_first = xcd * per + slot;
    const int n_my = t_first < t_end ? (t_end - t_first + nslot - 1) / nslot : 0;
    if (n_my == 0) {
        if (EX && a.sum_part != nullptr && wave < 8 && lane < 32) a.sum_part[((size_t)blockIdx.x * 8 + wave) * 32 + lane] = 0.0f;
        return;
    }
    const int HW = a.H * a.W;
    const int plane_bytes = HW * 32;

    if (wave >= 8) {
        // ---- loaders: wave 8 + lw takes pieces lw, lw + 4, ... of every patch
        const int lw = wave - 8;
        int packed[NIW];                               // plane << 16 | patch row << 8 | patch column of this lane's record in piece I
#pragma unroll
        for (int k = 0; k < NIW; ++k) {
            const int q = (k * NLW + lw) * 64 + lane;
            const int plane = q / NPIX, p = q - plane * NPIX;
            const int pr = p / PWd, pc = p - pr * PWd;
            packed[k] = q < PREC ? (plane << 16 | pr << 8 | pc) : -1;
        }
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, WBYTES, 0x00020000);
#pragma unroll
        for (int k = 0; k < NWW; ++k) {
            const int piece = k * NLW + lw;
            dma_buf16(rw, lds + (piece < NWI ? piece * 1024 : SINK), piece < NWI ? lane * 16 : 0x7ffffff0, piece < NWI ? piece * 1024 : 0);
        }
        auto issue = [&](int i) {
            const int tile = t_first + i * nslot;
            const int b = tile / a.tiles_per_image, rem = tile - b * a.tiles_per_image;
            const int th_i = rem / a.tiles_w, tw_i = rem - th_i * a.tiles_w;
            const int ih0 = th_i * TH - 1, iw0 = tw_i * TW - 1;
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(a.x + ((size_t)b * a.in_ctot16 + a.in_c16off) * (size_t)HW * 16), 0, KB * plane_bytes, 0x00020000);
            unsigned char* dst = lds + WBYTES + (i % NBUF) * PBYTES;
#pragma unroll
            for (int k = 0; k < NIW; ++k) {
                const int pk = packed[k], piece = k * NLW + lw;
                const int ih = ih0 + ((pk >> 8) & 0xff), iw = iw0 + (pk & 0xff);
                const bool ok = pk >= 0 && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
                const int plane = pk >> 16;
                const int voff = ok ? (plane >> 1) * plane_bytes + (ih * a.W + iw) * 32 + (plane & 1) * 16 : 0x7ffffff0;
                dma_buf16(rx, piece < NI ? dst + piece * 1024 : lds + SINK, voff, 0);
            }
        };
        issue(0);
        if (PD == 2 && n_my > 1) {
            issue(1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NIW) : "memory");       // weights + tile 0 have landed, tile 1 may be in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        wg_barrier();
        for (int i = 0; i < n_my; ++i) {
            // the buffer of tile i + PD is the one tile i - 1 was read from: every compute wave left it before the last barrier
            if (i + PD < n_my) {
                issue(i + PD);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PD - 1) * NIW) : "memory");   // tile i + 1 has landed
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            wg_barrier();
        }
        return;
    }

    // ---- compute waves: wave w owns channel tile w % NM for rows 2 (w / NM), 2 (w / NM) + 1 of the tile (two 32 x 32 accumulator tiles)
    const int mt = wave % NM, row0 = 2 * (wave / NM);
    const unsigned char* wa = lds + (h * C + mt * 32 + j) * 16;                         // lane part of the weight fragments
    const int pbl = WBYTES + (h * NPIX + row0 * PWd + j) * 16;                          // lane part of the patch fragments
    float bv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) bv[e] = a.bias != nullptr ? a.bias[mt * 32 + 4 * h + (e & 3) + 8 * (e >> 2)] : 0.0f;
    float bs[EX ? 16 : 1];                                              // per-lane channel sums over all tiles of this workgroup (sum_of)
#pragma unroll
    for (int e = 0; e < (EX ? 16 : 1); ++e) bs[e] = 0.0f;
    wg_barrier();                                                       // weights + tile 0 are in LDS
    for (int i = 0; i < n_my; ++i) {
        const unsigned char* pb = lds + pbl + (i % NBUF) * PBYTES;
        const int tile = t_first + i * nslot;
        const int b = tile / a.tiles_per_image, rem = tile - b * a.tiles_per_image;
        const int th_i = rem / a.tiles_w, tw_i = rem - th_i * a.tiles_w;
        const unsigned op16 = (unsigned)HW * 16;
        const size_t opix0 = (size_t)(th_i * TH + row0) * a.W + tw_i * TW + j;
        const size_t ro0 = (((size_t)b * (a.res_ctot >> 4) + 2 * mt) * HW + opix0) * 16 + 4 * h;      // row n: + n * W * 16
        // residual / mask operands of the epilogue are requested BEFORE the MFMAs (their HBM latency runs under the tile's work):
        // lane (j, h) needs 4 consecutive bf16 at element 8(q & 1) + 4h of record q >> 1, q = 0..3 (add_f16k_residual)
        uint2 rv1[2][4], rv2[2][4], mv[2][4];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t o = ro0 + (size_t)n * a.W * 16 + (size_t)(q >> 1) * op16 + 8 * (q & 1);
                if (a.res1 != nullptr) rv1[n][q] = *reinterpret_cast<const uint2*>(a.res1 + o);
                if (a.res2 != nullptr) rv2[n][q] = *reinterpret_cast<const uint2*>(a.res2 + o);
                if (!EX && a.mask16 != nullptr) mv[n][q] = *reinterpret_cast<const uint2*>(a.mask16 + o);      // (EX: read in the epilogue -- registers)
            }
        f32x16 acc[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[n][e] = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const int ty = t / 3, tx = t - 3 * ty;
                const bf16x8 av = *reinterpret_cast<const bf16x8*>(wa + (t * KB + kb) * SLAB);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const bf16x8 bw = *reinterpret_cast<const bf16x8*>(pb + (kb * 2 * NPIX + (ty + n) * PWd + tx) * 16);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bw, acc[n], 0, 0, 0);
                }
            }
        }
        // ---- epilogue (the F16K store path of conv_f16k for one 32-channel tile)
        auto add4 = [](f32x16& tt, int q, const uint2 r) {
            tt[4 * q + 0] += __builtin_bit_cast(float, r.x << 16);
            tt[4 * q + 1] += __builtin_bit_cast(float, r.x & 0xffff0000u);
            tt[4 * q + 2] += __builtin_bit_cast(float, r.y << 16);
            tt[4 * q + 3] += __builtin_bit_cast(float, r.y & 0xffff0000u);
        };
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const size_t opix = opix0 + (size_t)n * a.W;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[n][e] = apply_act(acc[n][e] + bv[e], a.act);
            if (a.mask16 != nullptr) {
                if constexpr (EX) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) mv[n][q] = *reinterpret_cast<const uint2*>(a.mask16 + ro0 + (size_t)n * a.W * 16 + (size_t)(q >> 1) * op16 + 8 * (q & 1));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[n][4 * q + 0] *= __builtin_bit_cast(float, mv[n][q].x << 16) > 0.0f ? 1.0f : a.mask_slope;
                    acc[n][4 * q + 1] *= __builtin_bit_cast(float, mv[n][q].x & 0xffff0000u) > 0.0f ? 1.0f : a.mask_slope;
                    acc[n][4 * q + 2] *= __builtin_bit_cast(float, mv[n][q].y << 16) > 0.0f ? 1.0f : a.mask_slope;
                    acc[n][4 * q + 3] *= __builtin_bit_cast(float, mv[n][q].y & 0xffff0000u) > 0.0f ? 1.0f : a.mask_slope;
                }
            }
            if (a.y_pre != nullptr) store_f16k_tile(acc[n], a.y_pre + ro0 + (size_t)n * a.W * 16 + 4 * h, op16);
            if constexpr (EX) {
                if (a.sum_of == 1) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) bs[e] += (float)(__bf16)acc[n][e];
                }
            }
            if (a.res1 != nullptr) {
#pragma unroll
                for (int q = 0; q < 4; ++q) add4(acc[n], q, rv1[n][q]);
            }
            if (a.res2 != nullptr) {
#pragma unroll
                for (int q = 0; q < 4; ++q) add4(acc[n], q, rv2[n][q]);
            }
            store_f16k_tile(acc[n], a.y16 + (((size_t)b * (a.out_ctot >> 4) + (a.out_coff >> 4) + 2 * mt) * HW + opix) * 16 + 8 * h, op16);
            if constexpr (EX) {
                if (a.y2 != nullptr) {       // y2 = bf16(y) * act'(mask2): what the elementwise pass computed from the stored y (mask2 is read here,
                                             // not ahead of the MFMAs: the kernel has no registers left for a third prefetched operand)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint2 m2 = *reinterpret_cast<const uint2*>(a.mask2 + ro0 + (size_t)n * a.W * 16 + (size_t)(q >> 1) * op16 + 8 * (q & 1));
                        acc[n][4 * q + 0] = (float)(__bf16)acc[n][4 * q + 0] * (__builtin_bit_cast(float, m2.x << 16) > 0.0f ? 1.0f : a.mask2_slope);
                        acc[n][4 * q + 1] = (float)(__bf16)acc[n][4 * q + 1] * (__builtin_bit_cast(float, m2.x & 0xffff0000u) > 0.0f ? 1.0f : a.mask2_slope);
                        acc[n][4 * q + 2] = (float)(__bf16)acc[n][4 * q + 2] * (__builtin_bit_cast(float, m2.y << 16) > 0.0f ? 1.0f : a.mask2_slope);
                        acc[n][4 * q + 3] = (float)(__bf16)acc[n][4 * q + 3] * (__builtin_bit_cast(float, m2.y & 0xffff0000u) > 0.0f ? 1.0f : a.mask2_slope);
                    }
                    store_f16k_tile(acc[n], a.y2 + ro0 + (size_t)n * a.W * 16 + 4 * h, op16);
                    if (a.sum_of == 2) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) bs[e] += (float)(__bf16)acc[n][e];
                    }
                }
            }
        }
        wg_barrier();          // tile i + 1 has landed (loader); this tile's buffer may be refilled
    }
    if (EX && a.sum_part != nullptr) {       // lanes of one half-wave hold the same 16 channels for 32 different pixels
#pragma unroll
        for (int e = 0; e < (EX ? 16 : 1); ++e) {
            float v = bs[e];
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
            if (j == 0) a.sum_part[((size_t)blockIdx.x * 8 + wave) * 32 + 4 * h + (e & 3) + 8 * (e >> 2)] = v;
        }
    }
}

// out[c] = sum of the per-wave partials of conv3x3_resident_f16k (wave w of a workgroup holds channel tile w % NM): one block per channel,
// a lane takes every 64th partial, then a tree -- float64, fixed order
__global__ __launch_bounds__(64) void c3_sum_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int C, int nblocks) {
    const int c = blockIdx.x, NM = C / 32, mt = c / 32, cl = c - mt * 32, per = 8 / NM, K = nblocks * per;
    double s = 0.0;
    for (int k = threadIdx.x; k < K; k += 64) {
        const int b = k / per, w = mt + (k - b * per) * NM;
        s += (double)part[((size_t)b * 8 + w) * 32 + cl];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) out[c] = (float)s;
}

// weights of Conv2d(cin -> C, 3x3) [C][cin][3][3] float32 -> bf16 fragment slabs [tap][kb][k-half][co][8 k] with the input channels
// zero-padded to CI;  transposed: the slabs of the INPUT gradient of a Conv2d(C -> cin) layer (the stride-1 transposed convolution
// on the same tensor [cin][C][3][3]: taps mirrored, channel roles swapped)
__global__ __launch_bounds__(256) void pack_c3_weights_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int cin, int CI, int C, int transposed) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                 // one 16-byte record: (tap, kb, hh, co)
    const int KB = CI / 16;
    if (idx >= 9 * KB * 2 * C) return;
    const int co = idx % C, hh = (idx / C) & 1, kb = (idx / (2 * C)) % KB, t = idx / (2 * C * KB);
    unsigned v[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float f[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ci = kb * 16 + hh * 8 + 2 * p + q;
            f[q] = ci >= cin ? 0.0f : (transposed ? w[((size_t)ci * C + co) * 9 + (8 - t)] : w[((size_t)co * cin + ci) * 9 + t]);
        }
        v[p] = pack2bf(f[0], f[1]);
    }
    reinterpret_cast<uint4*>(out)[idx] = make_uint4(v[0], v[1], v[2], v[3]);
}

}  // namespace

// One row per compiled (CI, C) pair, the plain kernel in column 0 and the EX form in column 1; plan_c3 picks the row, the grid and the LDS
// bytes for the launcher and for masic_conv3x3_resident_plan_name.
typedef void (*C3LaunchFn)(int grid, int lds_bytes, hipStream_t st, const C3Args& a);
template <int CI, int C, bool EX>
static void c3_launch(int grid, int lds_bytes, hipStream_t st, const C3Args& a) {
    launch_lds<conv3x3_resident_f16k<CI, C, EX>>(dim3(grid), 768, lds_bytes, st, a);
}
struct C3Row { int ci, c; C3LaunchFn launch[2]; };
#define C3_ROW(CI, C) {CI, C, {c3_launch<CI, C, false>, c3_launch<CI, C, true>}}
static const C3Row C3_ROWS[] = {C3_ROW(16, 32), C3_ROW(32, 32), C3_ROW(16, 64), C3_ROW(32, 64), C3_ROW(64, 64)};
constexpr int C3_MAX_WGS = 256;            // one persistent workgroup per CU
static bool c3_pair_ok(int CI, int C) { return (C == 32 || C == 64) && (CI == 16 || CI == 32 || CI == 64) && (CI <= C || CI == C); }

extern "C" size_t masic_conv3x3_resident_packed_bytes(int Cin, int Cout) {
    const int CI = round_up(Cin, 16);
    return c3_pair_ok(CI, Cout) ? (size_t)9 * (CI / 16) * 2 * Cout * 16 : 0;
}

// Cin: real input channels (any value <= 64; the F16K input buffer holds round_up(Cin, 16) of them, the padding zero or anything
// finite: its weights are zero); Cout: 32 (needs H % 16 == 0) or 64 (H % 8 == 0); W % 32 == 0
extern "C" int masic_conv3x3_resident_supported(int B, int Cin, int Cout, int H, int W) {
    const int CI = round_up(Cin, 16);
    return B > 0 && Cin > 0 && c3_pair_ok(CI, Cout) && H % (512 / Cout) == 0 && W % 32 == 0 && (long)H * W * 32 * (CI / 16) < (1l << 31);
}

extern "C" int masic_conv3x3_resident_pack_weight(const float* w, void* w_packed, int Cin, int Cout, int transposed, void* stream) {
    const int CI = round_up(Cin, 16);
    MASIC_REQUIRE(w && w_packed && c3_pair_ok(CI, Cout), MASIC_ERR_UNSUPPORTED, "conv3x3_resident_pack_weight: Cin <= 64, Cout = 32 or 64");
    hipLaunchKernelGGL(pack_c3_weights_kernel, dim3(ceil_div(9 * (CI / 16) * 2 * Cout, 256)), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)w_packed, Cin, CI,
                       Cout, transposed);
    return masic_launch_status("conv3x3_resident_pack_weight");
}

static const char* const C3_UNSUPPORTED = "conv3x3_resident_fwd: needs Cin <= 64, Cout = 32 (H % 16 == 0) or 64 (H % 8 == 0), W % 32 == 0";
struct C3Plan { const C3Row* row; int grid, lds_bytes, tiles_w, tiles_per_image, ntiles, nbuf; };
// ex: the second output / the channel sums are asked for (the EX kernel); sum_of as in masic_conv3x3_resident_ex_fwd
static int plan_c3(int B, int Cin, int Cout, int H, int W, bool ex, int sum_of, C3Plan* p) {
    MASIC_REQUIRE(sum_of >= 0 && sum_of <= 2 && (ex || sum_of == 0), MASIC_ERR_ARG, "conv3x3_resident_fwd: sum_of / sum_out / sum_workspace");
    MASIC_REQUIRE(masic_conv3x3_resident_supported(B, Cin, Cout, H, W), MASIC_ERR_UNSUPPORTED, "%s", C3_UNSUPPORTED);
    const int CI = round_up(Cin, 16), C = Cout;
    p->row = nullptr;
    for (const C3Row& r : C3_ROWS)
        if (r.ci == CI && r.c == C) p->row = &r;
    MASIC_REQUIRE(p->row != nullptr, MASIC_ERR_UNSUPPORTED, "%s", C3_UNSUPPORTED);
    const int TH = 512 / C;
    p->tiles_w = W / 32, p->tiles_per_image = p->tiles_w * (H / TH), p->ntiles = B * p->tiles_per_image;
    // LDS: weights + patch ring + sink (the kernel's constants)
    const int wbytes = 9 * (CI / 16) * 2 * C * 16, pbytes = ((CI / 16) * 2 * (TH + 2) * 34 + 63) / 64 * 1024;
    p->nbuf = wbytes + 3 * pbytes + 1024 <= 160 * 1024 ? 3 : 2;
    p->lds_bytes = wbytes + p->nbuf * pbytes + 1024;
    p->grid = p->ntiles < C3_MAX_WGS ? round_up(p->ntiles, 8) : C3_MAX_WGS;
    return MASIC_OK;
}

// y = act(conv3x3(x) + bias) * act'(mask) + res1 + res2 on F16K buffers, y_pre = the value before the adds (see
// masic_conv_f16k_res_ex_fwd: same meaning of every operand); x: channels [in_coff, in_coff + round_up(Cin, 16)) of an in_ctot-channel
// buffer, y: channels [out_coff, out_coff + Cout) of an out_ctot-channel buffer, residual / mask / pre tensors: res_ctot channels.
extern "C" int masic_conv3x3_resident_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                                          const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, int B, int Cin, int Cout, int H, int W,
                                          int in_ctot, int in_coff, int out_ctot, int out_coff, int act, void* stream) {
    return masic_conv3x3_resident_ex_fwd(x_f16k, w_packed, bias, res1, res2, res_ctot, mask, mask_slope, y_pre_f16k, y_f16k, nullptr, 0.0f, nullptr, 0, nullptr,
                                         nullptr, B, Cin, Cout, H, W, in_ctot, in_coff, out_ctot, out_coff, act, stream);
}
extern "C" size_t masic_conv3x3_resident_sum_workspace_bytes(void) { return (size_t)256 * 8 * 32 * sizeof(float); }
// ... + y2 = y * act'(mask2) (res_ctot-channel tensors) and sum_out[Cout] = per-channel sums of the value before the residual adds
// (sum_of = 1) or of y2 (sum_of = 2), bf16-rounded as stored; sum_workspace: masic_conv3x3_resident_sum_workspace_bytes()
extern "C" int masic_conv3x3_resident_ex_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                                             const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, const void* mask2, float mask2_slope,
                                             void* y2_f16k, int sum_of, float* sum_out, void* sum_workspace, int B, int Cin, int Cout, int H, int W,
                                             int in_ctot, int in_coff, int out_ctot, int out_coff, int act, void* stream) {
    const int CI = round_up(Cin, 16), C = Cout;
    MASIC_REQUIRE((mask2 == nullptr) == (y2_f16k == nullptr), MASIC_ERR_ARG, "conv3x3_resident_fwd: mask2 and y2 come together");
    MASIC_REQUIRE(sum_of >= 0 && sum_of <= 2 && (sum_of == 0) == (sum_out == nullptr) && (sum_of == 0 || sum_workspace != nullptr) && (sum_of != 2 || y2_f16k != nullptr),
                  MASIC_ERR_ARG, "conv3x3_resident_fwd: sum_of / sum_out / sum_workspace");
    MASIC_REQUIRE(y2_f16k == nullptr || (res_ctot % 16 == 0 && res_ctot >= C), MASIC_ERR_SHAPE, "conv3x3_resident_fwd: y2 / mask2 need res_ctot >= Cout channels");
    MASIC_REQUIRE(x_f16k && w_packed && y_f16k, MASIC_ERR_ARG, "conv3x3_resident_fwd: null pointer");
    MASIC_REQUIRE(masic_conv3x3_resident_supported(B, Cin, Cout, H, W), MASIC_ERR_UNSUPPORTED, "%s", C3_UNSUPPORTED);
    MASIC_REQUIRE(in_ctot % 16 == 0 && in_coff % 16 == 0 && in_coff >= 0 && in_coff + CI <= in_ctot && out_ctot % 16 == 0 && out_coff % 16 == 0 &&
                      out_coff >= 0 && out_coff + C <= out_ctot, MASIC_ERR_SHAPE, "conv3x3_resident_fwd: channel views");
    MASIC_REQUIRE(res1 != nullptr || res2 == nullptr, MASIC_ERR_ARG, "conv3x3_resident_fwd: res2 without res1");
    MASIC_REQUIRE((res1 == nullptr && mask == nullptr && y_pre_f16k == nullptr) || (res_ctot % 16 == 0 && res_ctot >= C), MASIC_ERR_SHAPE,
                  "conv3x3_resident_fwd: residual / mask / pre tensors need >= Cout channels, a multiple of 16");
    MASIC_REQUIRE(act == MASIC_ACT_NONE || act == MASIC_ACT_RELU || act == MASIC_ACT_LEAKY, MASIC_ERR_UNSUPPORTED, "conv3x3_resident_fwd: activation");
    const bool ex = y2_f16k != nullptr || sum_of;
    C3Plan p;
    const int rc = plan_c3(B, Cin, Cout, H, W, ex, sum_of, &p);
    if (rc != MASIC_OK) return rc;
    C3Args a{(const unsigned short*)x_f16k, (const unsigned short*)w_packed, bias, (const unsigned short*)res1, (const unsigned short*)res2,
             (const unsigned short*)mask, (unsigned short*)y_pre_f16k, (unsigned short*)y_f16k, B, H, W, in_ctot / 16, in_coff / 16, out_ctot, out_coff,
             res_ctot, act, mask_slope, p.tiles_w, p.tiles_per_image, p.ntiles,
             (const unsigned short*)mask2, (unsigned short*)y2_f16k, mask2_slope, (float*)sum_workspace, sum_of};
    hipStream_t st = (hipStream_t)stream;
    p.row->launch[ex](p.grid, p.lds_bytes, st, a);
    if (sum_of) hipLaunchKernelGGL(c3_sum_finish_kernel, dim3(C), dim3(64), 0, st, (const float*)sum_workspace, sum_out, C, p.grid);
    return masic_launch_status("conv3x3_resident_fwd");
}

// the launches of masic_conv3x3_resident_[ex_]fwd (include/masic_hip.h); the integers of the kernel's line: ntiles tiles_w tiles_per_image NBUF
extern "C" int masic_conv3x3_resident_plan_name(int B, int Cin, int Cout, int H, int W, int ex, int sum_of, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0, MASIC_ERR_ARG, "conv3x3_resident_plan_name: no buffer");
    buf[0] = 0;
    C3Plan p;
    const int rc = plan_c3(B, Cin, Cout, H, W, ex != 0, sum_of, &p);
    if (rc != MASIC_OK) return rc;
    char name[64];
    snprintf(name, sizeof name, "conv3x3_resident_f16k<%d, %d, %s>", p.row->ci, p.row->c, ex ? "true" : "false");
    const int v[4] = {p.ntiles, p.tiles_w, p.tiles_per_image, p.nbuf};
    const bool ok = masic_plan_line_ints(buf, n, name, dim3(p.grid), 768, (size_t)p.lds_bytes, v, 4) &&
                    (!sum_of || masic_plan_line(buf, n, "c3_sum_finish_kernel", dim3(Cout), 64, 0));
    if (!ok) buf[0] = 0;
    MASIC_REQUIRE(ok, MASIC_ERR_ARG, "conv3x3_resident_plan_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}
