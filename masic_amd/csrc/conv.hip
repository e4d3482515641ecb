// conv.hip -- convolutions of the MASIC hot path for gfx950 (MI355X).
//
// Replaces every nn.Conv2d / nn.ConvTranspose2d / MaskedConv2d the reference issues from
// HSIC.forward (coremasic/mywork/MASIC.py:744-851; factories compressai/models/utils.py:128-146,
// compressai/layers/layers.py:52-83).
//
// One formulation covers all of them: an output "phase plane" pixel (r,c) accumulates, over live
// taps (a,b) and input channels ci,
//     In[ci, r*is + dh0 + a*dsh, c*is + dw0 + b*dsw] * W[co, ci, kh0 + a*khs, kw0 + b*kws]
// and lands at output (r*os + oph, c*os + opw).  A strided Conv2d is one phase (is = stride);
// a ConvTranspose2d with stride s is s*s phases with is = 1, os = s (no multiplies by the zeros of
// the zero-insertion form); a type-'A' masked conv is one phase that keeps only its 12 live taps.
//
// Kernel 1 (implicit GEMM on the matrix cores): the GEMM is  Out[co, pixel] = W[co, k] * Im2col[k, pixel]
// with k = (tap, ci).  NCHW rows are read coalesced into an LDS patch [ci][row][col] (halo
// included, padding zero-filled) once per KC input channels and re-used by every tap; the weights
// arrive pre-packed as [tap][ci][co] so their LDS image is a straight copy.  Each of the 4 waves
// owns a 32(co) x WN*32(pixel) block of the 64 x BN tile and issues v_mfma_f32_32x32x2_f32
// (float32 operands, float32 accumulate: bitwise a k-ordered fmaf chain).  The bf16-operand
// variant of the same structure is selected with desc.prec.
//
// Kernel 2 (direct): Cout <= 8 layers (128->3 synthesis output, 6->3 pre/after convs, the
// mask2weights chain) are HBM/L2-bound, so they skip the matrix cores: one thread per output pixel,
// all output channels in registers, weights through scalar loads.
#include "common.h"
#include "conv_geom.h"
#include "f16k_device.h"      // bf16x8

namespace {
struct ConvCfg {
    int direct;         // 1: direct kernel (Cout <= 8); 2: LDS-tiled 5x5 stride-2 transposed conv to <= 4 channels
    int wvm;            // waves along the channel dimension (2, or 1 for narrow layers); 4/wvm along pixels
    int wm;             // 32-channel sub-tiles per wave: block covers BM = 32*wm*wvm output channels
    int wn;             // pixel sub-tiles (of 32) per wave: 4 -> BM x 256 block tile, 1 -> BM x 64
    int buf_sz;         // floats per LDS buffer: patch [KC][PSZ] + weights [round4(taps*KC)][64]
    int vec4;           // 1x1 layers: the patch is staged with 16-byte DMA pieces
    int bf16;           // bf16-operand kernel (desc.prec == MASIC_PREC_BF16 and Cout > 8)
    int pf;             // bf16: small patch -> next chunk's pixels prefetched in registers
    int KC, KClog;      // input channels per LDS chunk
    int TW, TWlog, SR, TH;
    int Cin_pad, Cout_pad;
    int PH, PW, PWp, PSZ;
    int max_taps;
    size_t lds_bytes;
};

int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
constexpr int patch_bound(int TH, int TW) { return ((TH - 1) * 2 + 5) * ((TW - 1) * 2 + 5); }      // largest patch of a TH x TW tile: stride 2, 5 taps

ConvCfg choose_cfg(const masic_conv_desc_t& d, const ConvGeom* g, int nphase) {
    ConvCfg c{};
    if (d.Cout <= 4 && d.transposed && d.stride == 2 && d.KH == 5 && d.KW == 5 && d.pad == 2 && d.Cin >= 16 &&
        d.in_op == MASIC_INOP_NONE) {
        c.direct = 2; c.Cin_pad = round_up(d.Cin, 8); c.Cout_pad = 4;      // packed [ci][5][5][4]
        return c;
    }
    if (d.Cout <= 8 && d.Cin <= 8 && d.stride == 1 && d.KH == 5 && d.KW == 5 && d.pad == 2 && !d.masked &&
        d.in_op == MASIC_INOP_NONE && d.act != MASIC_ACT_SOFTMAX_C) {
        c.direct = 3; c.Cin_pad = d.Cin; c.Cout_pad = d.Cout <= 4 ? 4 : 8;  // packed [ci][5][5][4 or 8]
        return c;
    }
    if (d.Cout <= 8) {
        c.direct = 1; c.Cin_pad = d.Cin; c.Cout_pad = 8;
        return c;
    }
    int Hp = g[0].Hp, Wp = g[0].Wp, is = g[0].is;
    int span_h = 0, span_w = 0, max_taps = 0;
    for (int p = 0; p < nphase; ++p) {
        span_h = span_h > g[p].nth ? span_h : g[p].nth;
        span_w = span_w > g[p].ntw ? span_w : g[p].ntw;
        max_taps = max_taps > g[p].ntaps ? max_taps : g[p].ntaps;
    }
    c.max_taps = max_taps;
    c.TW = Wp > 16 ? 32 : (Wp > 8 ? 16 : 8);
    c.TWlog = ilog2(c.TW);
    c.SR = 32 / c.TW;
    // 128-channel blocks (2x4 MFMA tiles per wave: 0.75 LDS reads per MFMA) when Cout is a multiple of 128 and the
    // layer is big enough to still fill the chip; 64-channel blocks otherwise
    auto nblocks = [&](int wm, int wn) {
        int TH = c.SR * 2 * wn;
        return (long)ceil_div(Hp, TH) * ceil_div(Wp, c.TW) * (round_up(d.Cout, 64 * wm) / (64 * wm)) * d.B * nphase;
    };
    const bool m128 = round_up(d.Cout, 128) * 10 <= d.Cout * 11;          // <= 10 % padding waste with 128-wide blocks
    c.wvm = 2;
    if (d.Cout <= 32) { c.wvm = 1; c.wm = 1; c.wn = 2; }                    // 32 x 256 tile (CQE 32-channel layers)
    else if (d.Cout > 64 && d.Cout <= 96) { c.wvm = 1; c.wm = 3; c.wn = 2; } // 96 x 256 tile (CQE 96-channel layers)
    else if (m128 && nblocks(2, 4) >= 512) { c.wm = 2; c.wn = 4; }
    // bf16 1x1 layers are bound by operand staging, not MFMA: the widest tile amortises the weight stream and the
    // barriers best, and its small LDS footprint keeps every workgroup of a ~1-wave grid resident at once
    else if (m128 && d.prec == MASIC_PREC_BF16 && d.KH == 1 && d.KW == 1 && nblocks(2, 4) >= 192) { c.wm = 2; c.wn = 4; }
    else if (m128 && nblocks(2, 2) >= 512) { c.wm = 2; c.wn = 2; }
    else { c.wm = 1; c.wn = nblocks(1, 4) >= 768 ? 4 : (nblocks(1, 2) >= 512 ? 2 : 1); }
    const int wvn = 4 / c.wvm;
    const int BM = 32 * c.wm * c.wvm;
    c.Cout_pad = round_up(d.Cout, BM);
    // The per-channel patch must fit 24 DMA wave-instructions (MAXE = 6 per wave: 1536 floats), the bf16 patch MAXP * 256 = 1536 pixels.
    // Every tile does: TH * TW = 32 * wvn * wn <= 256 with TW = 8, 16 or 32, and check_desc admits stride <= 2 and kernels <= 5, so
    // PH * PW <= (2 (TH - 1) + 5) * (2 (TW - 1) + 5), which is largest for the 8 x 32 and 32 x 8 tiles: 19 * 67 = 1273.
    static_assert(patch_bound(8, 32) == 1273 && patch_bound(32, 8) == 1273 && patch_bound(16, 16) <= 1273 && 1273 <= 24 * 64 && 1273 <= 6 * 256,
                  "a 256-pixel tile's patch fits the DMA and the bf16 staging limits without shrinking the tile");
    c.TH = c.SR * wvn * c.wn;
    c.PH = (c.TH - 1) * is + span_h;
    c.PW = (c.TW - 1) * is + span_w;
    c.PWp = c.PW;                                       // LDS-DMA writes 64 consecutive floats: no row padding
    if (d.prec == MASIC_PREC_BF16) {
        // [pixel][KC+8] bf16 patch in one LDS buffer (two workgroups per CU overlap staging and MFMA)
        c.bf16 = 1;
        int KC = 32;
        while (KC > 16 && ((size_t)c.PH * c.PW * (KC + 8) * 2 > 64 * 1024 || KC > round_up(d.Cin, 16))) KC >>= 1;
        c.KC = KC; c.KClog = ilog2(KC);
        c.Cin_pad = round_up(d.Cin, KC);
        c.PSZ = c.PH * c.PW;
        c.buf_sz = 0;
        c.lds_bytes = (size_t)c.PH * c.PW * (KC + 8) * 2;
        c.pf = (c.PH * c.PW * (KC / 8) <= 1024) ? 1 : 0;
        return c;
    }
    c.PSZ = round_up(c.PH * c.PW, 64);                  // whole wave-instructions per channel
    const int groups = c.PSZ / 64;                      // DMA wave-instructions per channel
    const int epw = ceil_div(groups, 4);                // ... per wave
    const int cin2 = round_up(d.Cin, 2);
    // 1x1 layers (the GMM heads): rows are contiguous and 16-byte aligned -> dwordx4 DMA, 4x fewer instructions
    c.vec4 = (max_taps == 1 && d.KH == 1 && d.KW == 1 && d.stride == 1 && d.Wi % 4 == 0 && d.Cin >= 4 &&
              d.in_op == MASIC_INOP_NONE) ? 1 : 0;
    // two LDS buffers (the next chunk lands by DMA while this one is contracted); keep 2 blocks per CU
    int KC = 32;
    if (c.vec4) {
        while (KC > 4 && (KC * c.PSZ > 8192 || (size_t)2 * KC * (c.PSZ + BM) * 4 > 48 * 1024 || KC > round_up(d.Cin, 4))) KC >>= 1;
    } else {
        while (KC > 2 && ((size_t)2 * KC * (c.PSZ + max_taps * BM) * 4 > 80 * 1024 || KC > cin2 || KC * epw > 48)) KC >>= 1;
    }
    c.KC = KC; c.KClog = ilog2(KC);
    c.Cin_pad = round_up(d.Cin, KC);
    c.buf_sz = KC * c.PSZ + round_up(max_taps * KC, 256 / BM) * BM;
    c.lds_bytes = (size_t)2 * c.buf_sz * 4;
    return c;
}

// ------------------------------------------------------------------------------------------ pack

__global__ void pack_weight_kernel(const PackArgs a) {
    const ConvGeom g = a.gs[blockIdx.y];
    const size_t per_tap = (size_t)a.Cin_pad * a.Cout_pad;
    const size_t total = (size_t)g.ntaps * per_tap;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / per_tap);
        const int rem = (int)(i - (size_t)t * per_tap);
        const int ci = rem / a.Cout_pad, co = rem - ci * a.Cout_pad;
        float v = 0.0f;
        if (ci < a.Cin && co < a.Cout) {
            const int ta = t / g.ntw, tb = t - ta * g.ntw;
            const int kh = g.kh0 + ta * g.khs, kw = g.kw0 + tb * g.kws;
            const size_t src = a.transposed ? (((size_t)ci * a.Cout + co) * a.KH + kh) * a.KW + kw
                                            : (((size_t)co * a.Cin + ci) * a.KH + kh) * a.KW + kw;
            v = a.w[src];
        }
        a.wp[(size_t)g.tap_base * per_tap + i] = v;
    }
}

// ------------------------------------------------------------------------------------------ igemm
struct IgemmArgs {
    const float* x; const float* wp; const float* bias; const float* gate; const float* res1; const float* res2; float* y;
    int Cin, Hi, Wi, in_ctot, in_coff;
    int Cout, Ho, Wo, out_ctot, out_coff;
    int Cin_pad, Cout_pad, KC, KClog;
    int TW, TWlog, SR, TH, tiles_w;
    int PH, PW, PWp, PSZ, buf_sz, vec4;
    int in_op, act, gate_ctot, gate_c;
    GeomParams q;
    int nphase;
    unsigned short* y16;      // conv_igemm_bf16 only (masic_conv2d_f16k_out_fwd): instead of y, F16K [B][out_ctot/16][Ho*Wo][16] bf16 of the result
};

__device__ __attribute__((aligned(16))) float g_zero_word[4] = {0.0f, 0.0f, 0.0f, 0.0f};

// global -> LDS DMA (no VGPR round trip): per-lane source address, LDS destination = wave-uniform base + lane*size
__device__ __forceinline__ void dma4(const float* g, float* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
__device__ __forceinline__ void dma16(const float* g, float* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ---- shared epilogue: bias, activation, gate, residual adds, NCHW store (32 consecutive pixels per half-wave).
// Every load (bias, gate, residuals) is issued BEFORE the arithmetic of its tile: a load inside the per-element loop
// would put an s_waitcnt vmcnt(0) in front of every store and serialise the epilogue on memory latency.
template <int WM, int WN>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& a, const ConvGeom& g, f32x16 (&acc)[WM][WN], int b, int m0w,
                                               int r0, int c0, int wn, int jr, int jc, int h) {
    const size_t oplane = (size_t)a.Ho * a.Wo;
    float bv[WM][16];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = m0w + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            bv[m][e] = (a.bias != nullptr) ? a.bias[co < a.Cout ? co : a.Cout - 1] : 0.0f;
        }
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int r = r0 + (wn * WN + n) * a.SR + jr, c = c0 + jc;
        const bool pok = r < g.Hp && c < g.Wp;
        const int oh = pok ? r * g.os + g.oph : 0, ow = pok ? c * g.os + g.opw : 0;
        const size_t opix = (size_t)oh * a.Wo + ow;
        const float gv = (a.gate != nullptr) ? a.gate[((size_t)b * a.gate_ctot + a.gate_c) * oplane + opix] : 1.0f;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            float rv[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) rv[e] = 0.0f;
            if (a.res1 != nullptr) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int co = m0w + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    rv[e] = a.res1[((size_t)b * a.Cout + (co < a.Cout ? co : a.Cout - 1)) * oplane + opix];
                }
                if (a.res2 != nullptr) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int co = m0w + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                        rv[e] += a.res2[((size_t)b * a.Cout + (co < a.Cout ? co : a.Cout - 1)) * oplane + opix];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = m0w + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = apply_act(acc[m][n][e] + bv[m][e], a.act) * gv + rv[e];
                if (pok && co < a.Cout) a.y[((size_t)b * a.out_ctot + a.out_coff + co) * oplane + opix] = v;
            }
        }
    }
}

// ---- F16K output (conv_igemm_bf16, a.y16): bf16(act(acc + bias)) as 32-byte channel records for an F16K consumer -- what
// nchw_to_f16k_kernel makes of the float32 result of igemm_epilogue, bit for bit (that epilogue computes act(..) * 1.0f + 0.0f when there
// is no gate and no residual: the + 0.0f turns -0 into +0 and is kept here).  Lane (j, h) holds channels 8q + 4h + i of pixel j, the
// accumulator layout of conv_f16k.hip (f16k_device.h: store_f16k_tile): the halves of the wave swap their middle quarters (v_permlane32_swap) and each lane writes the 8
// consecutive channels 8h .. 8h+7 of a record with one 16-byte store.  Cout % 32 == 0: a 32-channel tile is valid or not as a whole.
template <int WM, int WN>
__device__ __forceinline__ void igemm_epilogue_f16k(const IgemmArgs& a, const ConvGeom& g, f32x16 (&acc)[WM][WN], int b, int m0w,
                                                    int r0, int c0, int wn, int jr, int jc, int h) {
    const size_t oplane = (size_t)a.Ho * a.Wo;
    float bv[WM][16];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = m0w + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            bv[m][e] = (a.bias != nullptr) ? a.bias[co < a.Cout ? co : a.Cout - 1] : 0.0f;
        }
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int r = r0 + (wn * WN + n) * a.SR + jr, c = c0 + jc;
        const bool pok = r < g.Hp && c < g.Wp;               // (a function of the lane's pixel j: the same in both halves of the wave)
        const int oh = pok ? r * g.os + g.oph : 0, ow = pok ? c * g.os + g.opw : 0;
        const size_t opix = (size_t)oh * a.Wo + ow;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            if (!pok || m0w + m * 32 >= a.Cout) continue;
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                const float v0 = apply_act(acc[m][n][e] + bv[m][e], a.act) * 1.0f + 0.0f;
                const float v1 = apply_act(acc[m][n][e + 1] + bv[m][e + 1], a.act) * 1.0f + 0.0f;
                typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
                bf16x2 t;
                t[0] = (__bf16)v0;
                t[1] = (__bf16)v1;
                pk[e >> 1] = __builtin_bit_cast(unsigned, t);
            }
            unsigned short* rec = a.y16 + (((size_t)b * (a.out_ctot >> 4) + ((a.out_coff + m0w + m * 32) >> 4)) * oplane + opix) * 16 + 8 * h;
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {     // record rr of the tile: channels 16 rr .. 16 rr + 15
                const auto s0 = __builtin_amdgcn_permlane32_swap(pk[4 * rr + 0], pk[4 * rr + 2], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(pk[4 * rr + 1], pk[4 * rr + 3], false, false);
                uint4 st;
                st.x = s0[0]; st.y = s1[0]; st.z = s0[1]; st.w = s1[1];
                *reinterpret_cast<uint4*>(rec + (size_t)rr * oplane * 16) = st;
            }
        }
    }
}

constexpr int MAXE = 6;   // DMA wave-instructions per wave per channel plane (patch <= 1536 floats)
constexpr int MAXQ = 8;   // 16-byte-DMA wave-instructions per wave per chunk (1x1 layers: KC*PSZ <= 8192 floats)

template <int WVM, int WM, int WN, int INOP, bool VEC4>
__global__ __launch_bounds__(256, 2) void conv_igemm_f32(const IgemmArgs a) {
    constexpr int BM = 32 * WM * WVM;           // output channels per block: WVM waves x WM x 32
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // two buffers, each: patch [KC][PSZ] (rows of PW floats, flattened) | weights [ntaps][KC][BM]
    const int wts_off = a.KC * a.PSZ;
    const int buf_sz = a.buf_sz;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WVM, wn = wave / WVM;
    const int j = lane & 31, h = lane >> 5;

    const int phase = blockIdx.x % a.nphase, tile = blockIdx.x / a.nphase;
    const ConvGeom g = make_geom(a.q, phase);
    const int tw_i = tile % a.tiles_w, th_i = tile / a.tiles_w;
    const int m0 = blockIdx.y * BM;
    const int b = blockIdx.z;
    const int r0 = th_i * a.TH, c0 = tw_i * a.TW;
    const int ih0 = r0 * g.is + g.dh_min, iw0 = c0 * g.is + g.dw_min;

    // ---- per-lane DMA source offsets, fixed for the whole K loop (-1: zero fill).
    //  dword mode : this wave's groups of 64 consecutive patch floats within one input channel plane
    //  VEC4 (1x1) : 16-byte pieces over the whole [KC][PSZ] chunk; per lane (channel-in-chunk, offset)
    constexpr int NOFF = VEC4 ? MAXQ : MAXE;
    const int groups = a.PSZ >> 6;
    const int nq = (a.KC * a.PSZ) >> 8;
    int goff[NOFF], gci[VEC4 ? MAXQ : 1];
#pragma unroll
    for (int i = 0; i < NOFF; ++i) {
        if (VEC4) {
            const int off = (wave + 4 * i) * 256 + lane * 4;
            const int ci = off / a.PSZ, rem = off - ci * a.PSZ;
            const int pr = rem / a.PW, pc = rem - pr * a.PW;
            const int ih = ih0 + pr, iw = iw0 + pc;
            const bool ok = (pr < a.PH) && ih >= 0 && ih < a.Hi && iw >= 0 && iw + 3 < a.Wi;
            gci[i] = ci;
            goff[i] = ok ? ci * (a.Hi * a.Wi) + ih * a.Wi + iw : -1;
        } else {
            const int e = (wave + 4 * i) * 64 + lane;
            const int pr = e / a.PW, pc = e - pr * a.PW;
            const int ih = ih0 + pr, iw = iw0 + pc;
            const bool ok = (pr < a.PH) && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
            goff[i] = ok ? ih * a.Wi + iw : -1;
        }
    }
    const size_t plane = (size_t)a.Hi * a.Wi;
    const float* xb = a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane;
    // weights: 16-byte pieces, BM/4 lanes per (tap,ci) row of BM co -> 256/BM rows per wave-instruction
    constexpr int LPR = BM / 4, RPI = 64 / LPR;     // BM = 96: 24 lanes per row, 2 rows + 16 idle lanes per instruction
    const int wrows = g.ntaps * a.KC;
    const int wq = lane % LPR, wr = lane / LPR;

    auto issue = [&](int cc, float* buf) {
        if (VEC4) {
            const float* xc = xb + (size_t)cc * plane;
#pragma unroll
            for (int i = 0; i < NOFF; ++i) {
                const int q = wave + 4 * i;
                if (q < nq) {
                    const float* src = (goff[i] >= 0 && cc + gci[VEC4 ? i : 0] < a.Cin) ? xc + goff[i] : g_zero_word;
                    dma16(src, buf + q * 256);
                }
            }
        } else {
            for (int ci = 0; ci < a.KC; ++ci) {
                const bool cok = (cc + ci) < a.Cin;
                const float* xc = xb + (size_t)(cc + ci) * plane;
                float* dst = buf + ci * a.PSZ;
#pragma unroll
                for (int i = 0; i < NOFF; ++i) {
                    const int g = wave + 4 * i;
                    if (g < groups) {
                        const float* src = (cok && goff[i] >= 0) ? xc + goff[i] : g_zero_word;
                        dma4(src, dst + g * 64);
                    }
                }
            }
        }
        float* wdst = buf + wts_off;
        for (int r = wave * RPI; r < wrows; r += 4 * RPI) {   // this wave-instruction covers rows r..r+RPI-1
            int row = r + wr;
            row = row < wrows ? row : wrows - 1;                // tail lanes duplicate the last row into the pad rows
            const int t = row >> a.KClog, ci = row & (a.KC - 1);
            const float* src = a.wp + ((size_t)(g.tap_base + t) * a.Cin_pad + cc + ci) * a.Cout_pad + m0 + wq * 4;
            if (RPI * LPR == 64 || lane < RPI * LPR) dma16(src, wdst + r * BM);
        }
    };

    const int jr = j >> a.TWlog, jc = j & (a.TW - 1);
    // per-lane LDS offsets: A fragment (co = wm*32*WM + mi*32 + j of k-row h), B fragment (pixel j of sub-tile n, channel h)
    const int lane_w = h * BM + wm * (32 * WM) + j;
    int lane_p[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int r = (wn * WN + n) * a.SR + jr;
        lane_p[n] = h * a.PSZ + (r * g.is) * a.PW + jc * g.is;
    }
    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.0f;

    const int kh = a.KC >> 1, khlog = a.KClog - 1;
    const int nsteps = g.ntaps << khlog;
    const int tap0_off = (g.dh0 - g.dh_min) * a.PW + (g.dw0 - g.dw_min);
    const int chan_span = 2 * a.PSZ * (kh - 1);                       // back to channel pair 0 of the chunk
    const int row_step = g.dsh * a.PW - g.dsw * (g.ntw - 1);   // first tap of the next kernel row

    const int nchunks = a.Cin_pad >> a.KClog;
    issue(0, lds);
    for (int c = 0; c < nchunks; ++c) {
        float* cur = lds + (c & 1) * buf_sz;
        // own DMAs landed (vmcnt(0)) + everyone finished reading the other buffer -> barrier
        __syncthreads();
        if (c + 1 < nchunks) issue((c + 1) << a.KClog, lds + ((c + 1) & 1) * buf_sz);
        const float* patch = cur;
        const float* wts = cur + wts_off;
        // k-steps (tap, channel pair) of this chunk, software-pipelined with two fragment sets: the LDS reads of
        // step s+1 are issued before the MFMAs of step s.  Offsets advance incrementally: weights are contiguous
        // in step order; the patch offset moves by two channels inside a tap, else to the next (row-major) tap.
        int sw = 0, sp = tap0_off, kk2 = 0, tb = 0;
        auto advance = [&]() {
            sw += 2 * BM;
            if (++kk2 < kh) {
                sp += 2 * a.PSZ;
            } else {
                kk2 = 0;
                sp -= chan_span;
                if (++tb < g.ntw) sp += g.dsw;
                else { tb = 0; sp += row_step; }
            }
        };
        float a0[WM], b0[WN], a1[WM], b1[WN];
#pragma unroll
        for (int m = 0; m < WM; ++m) a0[m] = wts[lane_w + m * 32];
#pragma unroll
        for (int n = 0; n < WN; ++n) b0[n] = patch[sp + lane_p[n]];
        for (int st = 0; st < nsteps; st += 2) {
            const bool more1 = st + 1 < nsteps;
            if (more1) {
                advance();
#pragma unroll
                for (int m = 0; m < WM; ++m) a1[m] = wts[sw + lane_w + m * 32];
#pragma unroll
                for (int n = 0; n < WN; ++n) b1[n] = patch[sp + lane_p[n]];
            }
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], apply_inop(b0[n], INOP), acc[m][n], 0, 0, 0);
            if (!more1) break;
            if (st + 2 < nsteps) {
                advance();
#pragma unroll
                for (int m = 0; m < WM; ++m) a0[m] = wts[sw + lane_w + m * 32];
#pragma unroll
                for (int n = 0; n < WN; ++n) b0[n] = patch[sp + lane_p[n]];
            }
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], apply_inop(b1[n], INOP), acc[m][n], 0, 0, 0);
        }
    }

    igemm_epilogue<WM, WN>(a, g, acc, b, m0 + wm * (32 * WM), r0, c0, wn, jr, jc, h);
}

// ------------------------------------------------------------------------------------------ direct
struct DirectArgs {
    const float* x; const float* wp; const float* bias; const float* gate; const float* res1; const float* res2; float* y;
    int Cin, Hi, Wi, in_ctot, in_coff;
    int Cout, Ho, Wo, out_ctot, out_coff;
    int in_op, act, gate_ctot, gate_c;
    GeomParams q;
    int nphase;
};

template <int CO>
__global__ __launch_bounds__(256) void conv_direct_f32(const DirectArgs a) {
    const int phase = blockIdx.x % a.nphase;
    const ConvGeom g = make_geom(a.q, phase);
    const int pix = (blockIdx.x / a.nphase) * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int npix = g.Hp * g.Wp;
    const bool live = pix < npix;
    const int r = live ? pix / g.Wp : 0, c = live ? pix - r * g.Wp : 0;
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.0f;
    const size_t plane = (size_t)a.Hi * a.Wi;
    const float* xb = a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane;
    for (int t = 0; t < g.ntaps; ++t) {
        const int ta = t / g.ntw, tb = t - ta * g.ntw;
        const int ih = r * g.is + g.dh0 + ta * g.dsh;
        const int iw = c * g.is + g.dw0 + tb * g.dsw;
        const bool ok = live && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        const float* xp = xb + (size_t)ih * a.Wi + iw;
        const float* wt = a.wp + (size_t)(g.tap_base + t) * a.Cin * 8;
        for (int ci = 0; ci < a.Cin; ++ci) {
            const float v = ok ? apply_inop(xp[(size_t)ci * plane], a.in_op) : 0.0f;
#pragma unroll
            for (int o = 0; o < CO; ++o) acc[o] = fmaf(v, wt[ci * 8 + o], acc[o]);
        }
    }
    if (!live) return;
    const int oh = r * g.os + g.oph, ow = c * g.os + g.opw;
    const size_t oplane = (size_t)a.Ho * a.Wo, opix = (size_t)oh * a.Wo + ow;
    float gv = 1.0f;
    if (a.gate) gv = a.gate[((size_t)b * a.gate_ctot + a.gate_c) * oplane + opix];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = (o < a.Cout) ? acc[o] + (a.bias ? a.bias[o] : 0.0f) : 0.0f;
    if (a.act == MASIC_ACT_SOFTMAX_C) {   // mask2weights: softmax over the output channels (MASIC.py:497-502)
        float mx = acc[0], sum = 0.0f;
#pragma unroll
        for (int o = 1; o < CO; ++o) if (o < a.Cout) mx = fmaxf(mx, acc[o]);
#pragma unroll
        for (int o = 0; o < CO; ++o) if (o < a.Cout) { acc[o] = expf(acc[o] - mx); sum += acc[o]; }
#pragma unroll
        for (int o = 0; o < CO; ++o) acc[o] = acc[o] / sum;
    } else {
#pragma unroll
        for (int o = 0; o < CO; ++o) acc[o] = apply_act(acc[o], a.act);
    }
#pragma unroll
    for (int o = 0; o < CO; ++o)
        if (o < a.Cout) {
            float v = a.gate ? acc[o] * gv : acc[o];
            if (a.res1) v += a.res1[((size_t)b * a.Cout + o) * oplane + opix];
            if (a.res2) v += a.res2[((size_t)b * a.Cout + o) * oplane + opix];
            a.y[((size_t)b * a.out_ctot + a.out_coff + o) * oplane + opix] = v;
        }
}

// ------------------------------------------------------------------------------------------ deconv to <=4 channels
// ConvTranspose2d(Cin -> Cout<=4, k=5, s=2, p=2, op=1): the last layer of both synthesis transforms
// (decoder{1,2}.g_s_conv4, MASIC.py:542,596).  Cout = 3 cannot feed a 32x32 MFMA tile, and the layer is bound by
// reading its 128-channel input once, so it runs on the VALU: a 16x16 tile of INPUT pixels per workgroup, the
// input staged through LDS by DMA (8 channels per chunk, halo 1), each thread producing the 2x2 output pixels of
// its input pixel for all output channels (25 taps x Cout FMAs per input channel, weights as scalar operands).
struct Deconv4Args {
    const float* x; const float* wp; const float* bias; float* y;
    int Cin, Cin_pad, Hi, Wi, in_ctot, in_coff;
    int Cout, Ho, Wo, out_ctot, out_coff;
    int act, tiles_w;
};

__global__ __launch_bounds__(256) void deconv5s2_small_cout(const Deconv4Args a, const float* __restrict__ wpk) {
    constexpr int T = 16, LW = T + 2, PLANE = LW * LW, PSZ = 384, KC = 8;   // 324 floats per channel -> 6 DMA groups
    __shared__ __attribute__((aligned(16))) float lds[2 * KC * PSZ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = tid & 15, ty = tid >> 4;
    const int tile_x = blockIdx.x % a.tiles_w, tile_y = blockIdx.x / a.tiles_w;
    const int b = blockIdx.y;
    const int r = tile_y * T + ty, c = tile_x * T + tx;
    const int ih0 = tile_y * T - 1, iw0 = tile_x * T - 1;

    int goff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = (wave + 4 * i) * 64 + lane;
        const int pr = e / LW, pc = e - pr * LW;
        const int ih = ih0 + pr, iw = iw0 + pc;
        const bool ok = e < PLANE && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        goff[i] = ok ? ih * a.Wi + iw : -1;
    }
    const size_t plane = (size_t)a.Hi * a.Wi;
    const float* xb = a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane;
    auto issue = [&](int cc, float* buf) {
#pragma unroll
        for (int ci = 0; ci < KC; ++ci) {
            const bool cok = (cc + ci) < a.Cin;
            const float* xc = xb + (size_t)(cc + ci) * plane;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int g = wave + 4 * i;
                if (g < 6) dma4((cok && goff[i] >= 0) ? xc + goff[i] : g_zero_word, buf + ci * PSZ + g * 64);
            }
        }
    };

    float acc[2][2][4];
#pragma unroll
    for (int i = 0; i < 16; ++i) (&acc[0][0][0])[i] = 0.0f;
    const int lbase = (ty + 1) * LW + tx + 1;
    const int nchunks = a.Cin_pad / KC;
    issue(0, lds);
    for (int ch = 0; ch < nchunks; ++ch) {
        const float* cur = lds + (ch & 1) * (KC * PSZ);
        __syncthreads();
        if (ch + 1 < nchunks) issue((ch + 1) * KC, lds + ((ch + 1) & 1) * (KC * PSZ));
#pragma unroll 1
        for (int ci = 0; ci < KC; ++ci) {
            const float* pl = cur + ci * PSZ + lbase;
            float v[3][3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) v[dy][dx] = pl[(dy - 1) * LW + dx - 1];
            const float* w = wpk + (ch * KC + ci) * 100;       // [kh][kw][4]; const __restrict__ + uniform -> s_load
            // out(2r+ph, 2c+pw) += in(r+1-a, c+1-b) * W[ph+2a][pw+2b]
#pragma unroll
            for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                for (int pw = 0; pw < 2; ++pw)
#pragma unroll
                    for (int ta = 0; ta < 3 - ph; ++ta)
#pragma unroll
                        for (int tb = 0; tb < 3 - pw; ++tb) {
                            const float xv = v[2 - ta][2 - tb];
                            const float* wt = w + ((ph + 2 * ta) * 5 + (pw + 2 * tb)) * 4;
#pragma unroll
                            for (int o = 0; o < 4; ++o) acc[ph][pw][o] = fmaf(xv, wt[o], acc[ph][pw][o]);
                        }
        }
    }
    if (r >= a.Hi || c >= a.Wi) return;
    const size_t oplane = (size_t)a.Ho * a.Wo;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (o >= a.Cout) break;
        const float bv = a.bias ? a.bias[o] : 0.0f;
        float* yo = a.y + ((size_t)b * a.out_ctot + a.out_coff + o) * oplane;
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            float2 st;
            st.x = apply_act(acc[ph][0][o] + bv, a.act);
            st.y = apply_act(acc[ph][1][o] + bv, a.act);
            *reinterpret_cast<float2*>(yo + (size_t)(2 * r + ph) * a.Wo + 2 * c) = st;
        }
    }
}

// packed layout for deconv5s2_small_cout: [ci (padded to 8)][kh][kw][4]
__global__ void pack_deconv4_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cin_pad, int Cout) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cin_pad * 100) return;
    const int ci = i / 100, rem = i - ci * 100, tap = rem >> 2, o = rem & 3;
    wp[i] = (ci < Cin && o < Cout) ? w[((size_t)ci * Cout + o) * 25 + tap] : 0.0f;
}

// ------------------------------------------------------------------------------------------ bf16-operand igemm
// Same implicit GEMM with bf16 operands on v_mfma_f32_32x32x16_bf16 (16x the f32 matrix rate), float32 accumulate,
// float32 NCHW tensors in HBM on both sides.  At this rate the contraction is no longer the bound -- operand delivery
// is -- so the staging differs from the f32 kernel:
//   * B (im2col) operand: a lane's fragment is 8 consecutive k = 8 consecutive input channels of one pixel, so the LDS
//     patch is [pixel][channel] bf16 (pixel pitch KC+8 elements: 16-byte pad against bank conflicts) and one
//     ds_read_b128 fetches a fragment.  NCHW float32 rows are read coalesced along W (one pixel per lane, 8 channel
//     planes per task), converted (v_cvt_pk_bf16_f32; |.| / round() fused here) and written with ds_write_b128:
//     the transpose happens in registers.
//   * A (weight) operand: straight from L2 into registers -- the weights are pre-packed as
//     [tap][ci/16][co][16 ci] bf16, so a wave's fragment load is 1 KiB contiguous -- prefetched one k-step ahead.
//     Keeping the 25-tap weights out of LDS is what lets the whole 5x5 patch of a 128 x 256 tile fit.

constexpr int MAXP = 6;    // pixel tasks per thread per 8-channel group (patch <= 1536 pixels)

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

template <int WVM, int WM, int WN, int INOP, bool PF>
__global__ __launch_bounds__(256, 2) void conv_igemm_bf16(const IgemmArgs a, const unsigned short* __restrict__ wpk) {
    constexpr int BM = 32 * WM * WVM;
    // A-fragment prefetch distance (k-steps): an L2 round trip under load is ~1-2 us, a k-step of a 1-MFMA wave tile
    // 13 ns -- the fewer MFMAs per k-step, the deeper the ring (same 32-64 VGPRs either way)
    constexpr int DEPTH = WM * WN >= 8 ? 4 : (WM * WN >= 2 ? 8 : 16);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* patch = reinterpret_cast<unsigned short*>(lds);          // [NP][KCP] bf16
    const int KCP = a.KC + 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WVM, wn = wave / WVM;
    const int j = lane & 31, h = lane >> 5;

    const int phase = blockIdx.x % a.nphase, tile = blockIdx.x / a.nphase;
    const ConvGeom g = make_geom(a.q, phase);
    const int tw_i = tile % a.tiles_w, th_i = tile / a.tiles_w;
    const int m0 = blockIdx.y * BM;
    const int b = blockIdx.z;
    const int r0 = th_i * a.TH, c0 = tw_i * a.TW;
    const int ih0 = r0 * g.is + g.dh_min, iw0 = c0 * g.is + g.dw_min;

    const int NP = a.PH * a.PW;
    const size_t plane = (size_t)a.Hi * a.Wi;
    const float* xb = a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane;
    auto pixel_offset = [&](int p) {     // patch pixel -> offset in an input channel plane (-1: zero fill)
        const int pr = p / a.PW, pc = p - pr * a.PW;
        const int ih = ih0 + pr, iw = iw0 + pc;
        return (ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi) ? ih * a.Wi + iw : -1;
    };
    // ---- staging maps.
    //  !PF: pixel p = tid + 256 i for every 8-channel group in turn (big patches)
    //   PF: (pixel, group) tasks t = tid + 256 i, t < NP * KC/8 <= 1024 (small patches: next chunk prefetched in registers)
    constexpr int NT = PF ? 4 : MAXP;
    int goff[NT], gch_t[PF ? 4 : 1], loff[PF ? 4 : 1];
    const int ngroups = a.KC >> 3;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = tid + 256 * i;
        if (PF) {
            const int gq = t / NP, p = t - gq * NP;
            goff[i] = gq >= ngroups ? -2 : pixel_offset(p);
            gch_t[i] = gq * 8;
            loff[i] = p * KCP + gq * 8;
        } else {
            goff[i] = t >= NP ? -2 : pixel_offset(t);
        }
    }

    const int jr = j >> a.TWlog, jc = j & (a.TW - 1);
    int lane_p[WN];        // LDS element offset of this lane's pixel (tap 0) + its k half
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int r = (wn * WN + n) * a.SR + jr;
        lane_p[n] = ((r * g.is) * a.PW + jc * g.is) * KCP + 8 * h;
    }
    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.0f;

    const int ksteps = a.KC >> 4, kslog = ksteps >> 1;              // 16-channel MFMA steps per tap (1 or 2)
    const int nsteps = g.ntaps * ksteps;
    const int tap0_off = ((g.dh0 - g.dh_min) * a.PW + (g.dw0 - g.dw_min)) * KCP;
    const int row_step = (g.dsh * a.PW - g.dsw * (g.ntw - 1)) * KCP;
    const int col_step = g.dsw * KCP;
    const int cin16 = a.Cin_pad >> 4;
    // A fragment address: ((tap * cin16 + c16) * Cout_pad + co) * 16 + 8h   (bf16 elements)
    const size_t a_lane = ((size_t)m0 + wm * (32 * WM) + j) * 16 + 8 * h;
    const size_t a_tap_stride = (size_t)cin16 * a.Cout_pad * 16;
    const size_t a_c16_stride = (size_t)a.Cout_pad * 16;

    float pre[PF ? 4 : 1][8];
    // raw, unconditional loads from clamped (always valid) addresses; the zero-fill select happens at store time so that
    // nothing consumes a loaded value here (a consumer would put an s_waitcnt behind every single load)
    auto load_tasks = [&](int cc) {
#pragma unroll
        for (int i = 0; i < (PF ? 4 : 1); ++i) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int cg = cc + gch_t[i] + c;
                pre[i][c] = xb[(size_t)(cg < a.Cin ? cg : a.Cin - 1) * plane + (goff[i] >= 0 ? goff[i] : 0)];
            }
        }
    };
    auto store_tasks = [&](int cc) {
#pragma unroll
        for (int i = 0; i < (PF ? 4 : 1); ++i) {
            if (goff[i] == -2) continue;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c)
                v[c] = (goff[i] >= 0 && cc + gch_t[i] + c < a.Cin) ? apply_inop(pre[i][c], INOP) : 0.0f;
            uint4 q;
            q.x = pack_bf16x2(v[0], v[1]); q.y = pack_bf16x2(v[2], v[3]);
            q.z = pack_bf16x2(v[4], v[5]); q.w = pack_bf16x2(v[6], v[7]);
            *reinterpret_cast<uint4*>(patch + loff[i]) = q;
        }
    };
    if (PF) load_tasks(0);

    for (int cc = 0; cc < a.Cin_pad; cc += a.KC) {
        // ---- stage: NCHW float32 -> [pixel][channel] bf16
        if (PF) {
            store_tasks(cc);
        } else {
            for (int gch = 0; gch < a.KC; gch += 8) {
                // all loads of this 8-channel group first (up to 48 in flight per lane), then convert + write:
                // one memory latency per group instead of one per pixel task
                float v[NT][8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int cg = cc + gch + c;
                    if (cg < a.Cin) {                     // wave-uniform: channels beyond Cin (3-channel image layers) cost no loads
                        const float* xc = xb + (size_t)cg * plane;
#pragma unroll
                        for (int i = 0; i < NT; ++i) {
                            const float t = xc[goff[i] >= 0 ? goff[i] : 0];
                            v[i][c] = goff[i] >= 0 ? t : 0.0f;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NT; ++i) v[i][c] = 0.0f;
                    }
                }
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    if (goff[i] == -2) continue;
                    uint4 q;
                    q.x = pack_bf16x2(apply_inop(v[i][0], INOP), apply_inop(v[i][1], INOP));
                    q.y = pack_bf16x2(apply_inop(v[i][2], INOP), apply_inop(v[i][3], INOP));
                    q.z = pack_bf16x2(apply_inop(v[i][4], INOP), apply_inop(v[i][5], INOP));
                    q.w = pack_bf16x2(apply_inop(v[i][6], INOP), apply_inop(v[i][7], INOP));
                    *reinterpret_cast<uint4*>(patch + (size_t)(tid + 256 * i) * KCP + gch) = q;
                }
            }
        }
        __syncthreads();
        if (PF && cc + a.KC < a.Cin_pad) load_tasks(cc + a.KC);        // in flight during the contraction
        // ---- contraction: k-steps (tap, 16 channels); A fragments stream from L2 through a DEPTH-deep register ring
        const unsigned short* wa = wpk + (size_t)g.tap_base * a_tap_stride + (size_t)(cc >> 4) * a_c16_stride + a_lane;
        auto a_offset = [&](int st) { return (size_t)(st >> kslog) * a_tap_stride + (size_t)(st & (ksteps - 1)) * a_c16_stride; };
        uint4 ring[DEPTH][WM];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
            if (u < nsteps) {
                const unsigned short* pa = wa + a_offset(u);
#pragma unroll
                for (int m = 0; m < WM; ++m) ring[u][m] = *reinterpret_cast<const uint4*>(pa + m * 32 * 16);
            }
        int sp = tap0_off, kk = 0, tb = 0;
        for (int st0 = 0; st0 < nsteps; st0 += DEPTH) {
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const int st = st0 + u;
                if (st < nsteps) {
                    bf16x8 bfrag[WN], afr[WM];
#pragma unroll
                    for (int n = 0; n < WN; ++n)
                        bfrag[n] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(patch + sp + lane_p[n] + kk * 16));
#pragma unroll
                    for (int m = 0; m < WM; ++m) afr[m] = __builtin_bit_cast(bf16x8, ring[u][m]);
                    if (st + DEPTH < nsteps) {
                        const unsigned short* pa = wa + a_offset(st + DEPTH);
#pragma unroll
                        for (int m = 0; m < WM; ++m) ring[u][m] = *reinterpret_cast<const uint4*>(pa + m * 32 * 16);
                    }
#pragma unroll
                    for (int m = 0; m < WM; ++m)
#pragma unroll
                        for (int n = 0; n < WN; ++n)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[m], bfrag[n], acc[m][n], 0, 0, 0);
                    if (++kk == ksteps) {
                        kk = 0;
                        if (++tb < g.ntw) sp += col_step;
                        else { tb = 0; sp += row_step; }
                    }
                }
            }
        }
        __syncthreads();
    }

    if (a.y16 != nullptr) {       // (uniform: a kernel argument)
        igemm_epilogue_f16k<WM, WN>(a, g, acc, b, m0 + wm * (32 * WM), r0, c0, wn, jr, jc, h);
        return;
    }
    igemm_epilogue<WM, WN>(a, g, acc, b, m0 + wm * (32 * WM), r0, c0, wn, jr, jc, h);
}


// ------------------------------------------------------------------------------------------ 5x5 stride-1, few channels
// Conv2d / ConvTranspose2d(k=5, s=1, p=2) with Cin <= 8 and Cout <= CO (4 or 8): encoder2.pre_conv (6->3) and
// decoder2.after_conv (6->3, transposed; MASIC.py:559,600), and with CO = 8 the input gradient of after_conv (3->6).  Full-resolution, HBM-bound (reads Cin, writes Cout
// planes): a 16x16 output tile per workgroup, the (16+4)^2 input tile of every channel staged by DMA, weights packed
// [ci][kh][kw][4] (flipped for the transposed layer, so the kernel is always a correlation) as scalar operands.
struct Conv5s1Args {
    const float* x; const float* bias; const float* gate; const float* res1; float* y;
    int Cin, H, W, in_ctot, in_coff, Cout, out_ctot, out_coff, act, tiles_w, gate_ctot, gate_c;
    // fused form of encoder2.pre_conv + pre_gdn and decoder2.after_gdn + cat + after_conv (MASIC.py:574-576, :617-621):
    const float* xb;          // second source: channels split .. Cin-1 come from xb[B][Cin-split][H][W] (no torch.cat)
    int split;                // channels taken from x (0: everything from x)
    const float* gin_beta; const float* gin_gamma; int gin_inverse;      // 3-channel (I)GDN applied to x's channels on load
    const float* gout_beta; const float* gout_gamma; int gout_inverse;   // 3-channel (I)GDN applied to the output
    float beta_bound, gamma_bound, pedestal;
};

// y_i = x_i * (beta^_i + sum_j gamma^_ij x_j^2)^(-1/2 or +1/2) over 3 channels, same operation order as gdn_generic
__device__ __forceinline__ void gdn3(float (&v)[3], const float* beta, const float* gamma, int inverse, float bb, float gb, float ped) {
    float sq[3], o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) sq[k] = __fmul_rn(v[k], v[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float bv = fmaxf(beta[i], bb);
        float n = __fsub_rn(__fmul_rn(bv, bv), ped);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float g = fmaxf(gamma[i * 3 + k], gb);
            s = fmaf(__fsub_rn(__fmul_rn(g, g), ped), sq[k], s);
        }
        n += s;
        const float r = sqrtf(n);
        o[i] = inverse ? v[i] * r : v[i] * (1.0f / r);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = o[i];
}

template <int CO>
__global__ __launch_bounds__(256) void conv5s1_small(const Conv5s1Args a, const float* __restrict__ wpk) {
    constexpr int T = 16, LW = T + 4, PLANE = LW * LW, PSZ = 448;       // 400 floats per channel -> 7 DMA groups
    __shared__ __attribute__((aligned(16))) float lds[8 * PSZ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // a wave takes rows wave, wave+4, wave+8, wave+12 of the tile: with the 20-float row pitch their 16-lane runs start 80 floats
    // = 16 banks apart, so the 64 lanes of a tap read hit 64 different banks (adjacent rows overlap in 12 of them: measured
    // half of the LDS cycles were conflicts)
    const int tx = tid & 15, ty = ((tid >> 4) & 3) * 4 + (tid >> 6);
    const int tile_x = blockIdx.x % a.tiles_w, tile_y = blockIdx.x / a.tiles_w;
    const int b = blockIdx.y;
    const int oy = tile_y * T + ty, ox = tile_x * T + tx;
    const size_t plane = (size_t)a.H * a.W;
    const float* xb = a.x + ((size_t)b * a.in_ctot + a.in_coff) * plane;
    const int split = a.xb != nullptr ? a.split : a.Cin;
    const float* xb2 = a.xb != nullptr ? a.xb + (size_t)b * (a.Cin - split) * plane : nullptr;
    for (int cg = wave; cg < a.Cin * 7; cg += 4) {
        const int ci = cg / 7, g = cg - ci * 7;
        const int e = g * 64 + lane;
        const int pr = e / LW, pc = e - pr * LW;
        const int ih = tile_y * T - 2 + pr, iw = tile_x * T - 2 + pc;
        const bool ok = e < PLANE && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        const float* src = ci < split ? xb + (size_t)ci * plane : xb2 + (size_t)(ci - split) * plane;
        if (e < PLANE) dma4(ok ? src + (size_t)ih * a.W + iw : g_zero_word, lds + ci * PSZ + g * 64);
    }
    __syncthreads();
    if (a.gin_beta != nullptr) {            // (I)GDN of the first three channels, per staged pixel (zero padding stays zero)
        for (int e = tid; e < PLANE; e += 256) {
            float v[3] = {lds[e], lds[PSZ + e], lds[2 * PSZ + e]};
            gdn3(v, a.gin_beta, a.gin_gamma, a.gin_inverse, a.beta_bound, a.gamma_bound, a.pedestal);
            lds[e] = v[0]; lds[PSZ + e] = v[1]; lds[2 * PSZ + e] = v[2];
        }
        __syncthreads();
    }
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.0f;
    const float* base = lds + ty * LW + tx;
    for (int ci = 0; ci < a.Cin; ++ci) {
        const float* w = wpk + ci * 25 * CO;
        const float* pl = base + ci * PSZ;
#pragma unroll
        for (int kh = 0; kh < 5; ++kh)
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
                const float xv = pl[kh * LW + kw];
#pragma unroll
                for (int o = 0; o < CO; ++o) acc[o] = fmaf(xv, w[(kh * 5 + kw) * CO + o], acc[o]);
            }
    }
    if (oy >= a.H || ox >= a.W) return;
    const size_t opix = (size_t)oy * a.W + ox;
    const float gv = a.gate ? a.gate[((size_t)b * a.gate_ctot + a.gate_c) * plane + opix] : 1.0f;
    if (a.gout_beta != nullptr) {           // 3-channel (I)GDN of the result (no activation / gate / residual in this form)
        float v[3] = {acc[0] + (a.bias ? a.bias[0] : 0.0f), acc[1] + (a.bias ? a.bias[1] : 0.0f), acc[2] + (a.bias ? a.bias[2] : 0.0f)};
        gdn3(v, a.gout_beta, a.gout_gamma, a.gout_inverse, a.beta_bound, a.gamma_bound, a.pedestal);
#pragma unroll
        for (int o = 0; o < 3; ++o) a.y[((size_t)b * a.out_ctot + a.out_coff + o) * plane + opix] = v[o];
        return;
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        if (o >= a.Cout) break;
        float v = apply_act(acc[o] + (a.bias ? a.bias[o] : 0.0f), a.act) * gv;
        if (a.res1) v += a.res1[((size_t)b * a.Cout + o) * plane + opix];
        a.y[((size_t)b * a.out_ctot + a.out_coff + o) * plane + opix] = v;
    }
}

// The pair form (6 -> 3, two 3-channel sources) of conv5s1_small<4> for W % 4 == 0 and 16-byte aligned tensors, same bits:
// a 64x16 output tile per workgroup, lane (tx, ty) owns the four adjacent pixels 4tx .. 4tx+3 of row ty.  Per channel LDS holds
// 20 rows of 72 floats (image columns tile_x*64 - 4 .. + 67: origin and pitch are 16-byte multiples), staged in 16-byte DMA
// pieces that are wholly inside or wholly outside the image; an outside piece gets an out-of-range buffer offset and lands
// as +0.0f.  A channel is 360 pieces, padded to 6 wave-instructions (384), so that one instruction has one source tensor.
// Per (ci, kh) a lane reads its 8-float window once and keeps it for the five kw and its four pixels; outputs (o0, o1) are
// one packed FMA, o2 a scalar one (the pack's fourth weight is zero and is not multiplied).  Every output's chain is
// fmaf(x, w, acc) from 0.0f in the order ci, kh, kw, then + bias: what conv5s1_small<4> computes.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256, 4) void conv5s1_pair_rows(const Conv5s1Args a, const float* __restrict__ wpk) {
    constexpr int TW = 64, TH = 16, LP = TW + 8, LR = TH + 4, RP = LP / 4, PCS = LR * RP, PSZ = 6 * 256;   // 360 pieces in 6 x 64
    constexpr int OOR = 0x7ffffff0;     // past every descriptor's range (the launcher keeps 3 planes below it): reads as zero
    __shared__ __attribute__((aligned(16))) float lds[6 * PSZ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // a wave takes rows 2w, 2w+8, 2w+1, 2w+9: eight rows are 576 floats = 9 x 64 banks, so the 16-lane runs of rows r and r+8
    // that share a ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...) read disjoint banks
    const int tx = tid & 15, ty = wave * 2 + ((tid >> 5) & 1) + ((tid >> 4) & 1) * 8;
    const int tile_x = blockIdx.x % a.tiles_w, tile_y = blockIdx.x / a.tiles_w;
    const int b = blockIdx.y;
    const size_t plane = (size_t)a.H * a.W;
    const float* srca = a.x + (size_t)b * 3 * plane;
    const float* srcb = a.xb + (size_t)b * 3 * plane;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int cg = k * 4 + wave;                    // 36 wave-instructions: channel cg / 6, pieces (cg % 6) * 64 + lane
        const int ci = cg / 6, g = cg - ci * 6;
        const int e = g * 64 + lane;
        const int pr = e / RP, pc = e - pr * RP;
        const int ih = tile_y * TH - 2 + pr, iw = tile_x * TW - 4 + pc * 4;
        const bool ok = e < PCS && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)(ci < 3 ? srca : srcb), 0, (int)(3 * plane * 4), 0x00020000);
        const int c3 = ci < 3 ? ci : ci - 3;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(lds + cg * 256), 16,
                                                 ok ? ((c3 * a.H + ih) * a.W + iw) * 4 : OOR, 0, 0, 0);
    }
    __syncthreads();
    if (a.gin_beta != nullptr) {            // (I)GDN of the first three channels, per staged pixel (zero padding stays zero)
        for (int e = tid; e < PCS; e += 256) {
            f32x4 p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = *reinterpret_cast<const f32x4*>(lds + c * PSZ + e * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[3] = {p[0][j], p[1][j], p[2][j]};
                gdn3(v, a.gin_beta, a.gin_gamma, a.gin_inverse, a.beta_bound, a.gamma_bound, a.pedestal);
                p[0][j] = v[0]; p[1][j] = v[1]; p[2][j] = v[2];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(lds + c * PSZ + e * 4) = p[c];
        }
        __syncthreads();
    }
    f32x2 acc01[4];
    float acc2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc01[j] = f32x2{0.0f, 0.0f}; acc2[j] = 0.0f; }
    const float* base = lds + ty * LP + tx * 4;
    for (int ci = 0; ci < 6; ++ci) {
        const float* w = wpk + ci * 100;
        const float* pl = base + ci * PSZ;
#pragma unroll
        for (int kh = 0; kh < 5; ++kh) {
            // LDS columns 4tx+2 .. 4tx+9 of row ty+kh: pixel j's tap kw is element j + kw.  Three 16-byte reads (conflict-free
            // with the row assignment above, 4 LDS cycles each).  The empty asm keeps the compiler from narrowing the two end
            // reads to their used halves and merging those into a ds_read2_b64 (8 cycles, two-way conflicts tx / tx + 8)
            f32x4 lo = *reinterpret_cast<const f32x4*>(pl + kh * LP);
            const f32x4 mid = *reinterpret_cast<const f32x4*>(pl + kh * LP + 4);
            f32x4 hi = *reinterpret_cast<const f32x4*>(pl + kh * LP + 8);
            asm("" : "+v"(lo), "+v"(hi));
            const float win[8] = {lo[2], lo[3], mid[0], mid[1], mid[2], mid[3], hi[0], hi[1]};
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
                const f32x2 w01 = *reinterpret_cast<const f32x2*>(w + (kh * 5 + kw) * 4);
                const float w2 = w[(kh * 5 + kw) * 4 + 2];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xv = win[j + kw];
                    acc01[j] = __builtin_elementwise_fma(f32x2{xv, xv}, w01, acc01[j]);
                    acc2[j] = fmaf(xv, w2, acc2[j]);
                }
            }
        }
    }
    const int oy = tile_y * TH + ty, ox = tile_x * TW + tx * 4;
    if (oy >= a.H || ox >= a.W) return;     // W % 4 == 0: a strip of four pixels is never ragged
    f32x4 out[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v[3] = {acc01[j][0] + (a.bias ? a.bias[0] : 0.0f), acc01[j][1] + (a.bias ? a.bias[1] : 0.0f), acc2[j] + (a.bias ? a.bias[2] : 0.0f)};
        if (a.gout_beta != nullptr) gdn3(v, a.gout_beta, a.gout_gamma, a.gout_inverse, a.beta_bound, a.gamma_bound, a.pedestal);
        out[0][j] = v[0]; out[1][j] = v[1]; out[2][j] = v[2];
    }
    float* yb = a.y + (size_t)b * 3 * plane + (size_t)oy * a.W + ox;
#pragma unroll
    for (int o = 0; o < 3; ++o) *reinterpret_cast<f32x4*>(yb + (size_t)o * plane) = out[o];
}

// [ci][kh][kw][CO]; the transposed layer's taps are flipped so that the kernel correlates
__global__ void pack_conv5s1_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int transposed, int CO) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cin * 25 * CO) return;
    const int ci = i / (25 * CO), rem = i - ci * 25 * CO, tap = rem / CO, o = rem - tap * CO;
    float v = 0.0f;
    if (o < Cout) v = transposed ? w[((size_t)ci * Cout + o) * 25 + (24 - tap)] : w[((size_t)o * Cin + ci) * 25 + tap];
    wp[i] = v;
}

// ------------------------------------------------------------------------------------------ host side: table, plan, launcher
enum { CF_IGEMM_F32, CF_IGEMM_BF16, CF_DIRECT, CF_DECONV4, CF_CONV5S1 };      // family: one argument struct and one kernel signature each
typedef void (*ConvKernelFn)();                // a kernel of any family; conv_run casts it back to its signature
template <class... A> void conv_run(ConvKernelFn k, dim3 grid, size_t lds, void* stream, const A&... a) {
    const auto fn = reinterpret_cast<void (*)(A...)>(k);
    hipLaunchKernelGGL(fn, grid, dim3(256), lds, (hipStream_t)stream, a...);
}
// One row per compiled tile shape; the igemm rows hold their in_op x VEC4 (f32) / PF (bf16) instantiations as columns.  plan_conv below
// is the only place a row is chosen; a (row, column) that is not in the table is not compiled.
struct ConvRow {
    int family;
    int t[3];                    // igemm: WVM, WM, WN; conv_direct_f32 / conv5s1_small: CO
    ConvKernelFn k[3][2];        // igemm: [in_op][VEC4 or PF] (VEC4 stages untransformed input only); the others: k[0][0]
};
#define KFN(...) reinterpret_cast<ConvKernelFn>(&__VA_ARGS__)
#define K1(K, V, M, N, OP) {KFN(K<V, M, N, OP, false>), nullptr}
#define K2(K, V, M, N, OP) {KFN(K<V, M, N, OP, false>), KFN(K<V, M, N, OP, true>)}
#define ROW_F32(V, M, N) {CF_IGEMM_F32, {V, M, N}, {K2(conv_igemm_f32, V, M, N, 0), K1(conv_igemm_f32, V, M, N, 1), K1(conv_igemm_f32, V, M, N, 2)}}
#define ROW_BF16(V, M, N) {CF_IGEMM_BF16, {V, M, N}, {K2(conv_igemm_bf16, V, M, N, 0), K2(conv_igemm_bf16, V, M, N, 1), K2(conv_igemm_bf16, V, M, N, 2)}}
const ConvRow CONV_ROWS[] = {
    ROW_F32(1, 1, 2), ROW_F32(1, 3, 2),                                        // one wave along the channels: 32 x 256 and 96 x 256 tiles
    ROW_F32(2, 1, 1), ROW_F32(2, 1, 2), ROW_F32(2, 1, 4),                      // 64 x 64 / 128 / 256
    ROW_F32(2, 2, 2), ROW_F32(2, 2, 4),                                        // 128 x 128 / 256
    ROW_BF16(1, 1, 2), ROW_BF16(1, 3, 2), ROW_BF16(2, 1, 1), ROW_BF16(2, 1, 2), ROW_BF16(2, 1, 4), ROW_BF16(2, 2, 2), ROW_BF16(2, 2, 4),
    {CF_DIRECT, {3, 0, 0}, {{KFN(conv_direct_f32<3>), nullptr}}}, {CF_DIRECT, {8, 0, 0}, {{KFN(conv_direct_f32<8>), nullptr}}},
    {CF_DECONV4, {0, 0, 0}, {{KFN(deconv5s2_small_cout), nullptr}}},
    {CF_CONV5S1, {4, 0, 0}, {{KFN(conv5s1_small<4>), nullptr}}}, {CF_CONV5S1, {8, 0, 0}, {{KFN(conv5s1_small<8>), nullptr}}},
};
constexpr int CONV_NROWS = sizeof(CONV_ROWS) / sizeof(CONV_ROWS[0]);
const ConvRow* conv_row(int family, int t0, int t1, int t2) {
    for (const ConvRow& r : CONV_ROWS)
        if (r.family == family && r.t[0] == t0 && r.t[1] == t1 && r.t[2] == t2) return &r;
    return nullptr;
}
// symbol: as masic_conv_kernel_name has always printed it -- conv5s1_small without its template argument
void conv_row_name(const ConvRow& r, int op, int col, bool symbol, char* buf, size_t n) {
    const char* f = col ? "true" : "false";
    if (r.family == CF_IGEMM_F32) snprintf(buf, n, "conv_igemm_f32<%d, %d, %d, %d, %s>", r.t[0], r.t[1], r.t[2], op, f);
    else if (r.family == CF_IGEMM_BF16) snprintf(buf, n, "conv_igemm_bf16<%d, %d, %d, %d, %s>", r.t[0], r.t[1], r.t[2], op, f);
    else if (r.family == CF_DIRECT) snprintf(buf, n, "conv_direct_f32<%d>", r.t[0]);
    else if (r.family == CF_DECONV4) snprintf(buf, n, "deconv5s2_small_cout");
    else if (symbol) snprintf(buf, n, "conv5s1_small");
    else snprintf(buf, n, "conv5s1_small<%d>", r.t[0]);
}

// Everything the launcher decides for one (layer, form); form: which optional operands the call has (MASIC_CONV_*).
struct ConvPlan {
    int rc;                      // MASIC_OK, or the launcher's refusal of this descriptor and form
    bool desc_ok;                // check_desc passed: geometry, configuration and packed_bytes are set whatever rc says (the weight pack reads them)
    bool empty;                  // no output pixels: MASIC_OK and no launch
    ConvGeom g[4];
    ConvCfg c;
    const ConvRow* row;
    int nphase, op, col, tiles_w;      // op, col: the row's column
    dim3 grid;
    size_t packed_bytes;
};
#define PLAN_REQUIRE(cond, code, ...) \
    do { if (!(cond)) { masic_set_error(__VA_ARGS__); p.rc = (code); return p; } } while (0)

ConvPlan plan_conv(const masic_conv_desc_t* d, int form) {
    ConvPlan p{};
    const bool f16k = form & MASIC_CONV_F16K_OUT, gate = form & MASIC_CONV_GATE, res1 = form & MASIC_CONV_RES1, res2 = form & MASIC_CONV_RES2;
    const char* const no_f16k = "conv2d_f16k_out_fwd: needs bf16 operands on the implicit-GEMM kernel, Cout % 32 == 0 and a 16-aligned output view";
    p.rc = check_desc(d);
    if (p.rc != MASIC_OK) {      // (the F16K-output form answers every descriptor it cannot take, a malformed one included, with its one refusal)
        if (f16k && d) { masic_set_error("%s", no_f16k); p.rc = MASIC_ERR_UNSUPPORTED; }
        return p;
    }
    p.desc_ok = true;
    p.nphase = build_geoms(*d, p.g);
    const ConvCfg& c = p.c = choose_cfg(*d, p.g, p.nphase);
    p.op = d->in_op == MASIC_INOP_ABS ? 1 : (d->in_op == MASIC_INOP_ROUND ? 2 : 0);
    int taps = 0;
    for (int i = 0; i < p.nphase; ++i) taps += p.g[i].ntaps;
    p.packed_bytes = (size_t)taps * c.Cin_pad * c.Cout_pad * (c.bf16 ? sizeof(unsigned short) : sizeof(float));
    if (c.direct == 2) { p.row = conv_row(CF_DECONV4, 0, 0, 0); p.packed_bytes = (size_t)c.Cin_pad * 100 * sizeof(float); }
    else if (c.direct == 3) { p.row = conv_row(CF_CONV5S1, c.Cout_pad, 0, 0); p.packed_bytes = (size_t)c.Cin_pad * 25 * c.Cout_pad * sizeof(float); }
    else if (c.direct) p.row = conv_row(CF_DIRECT, d->Cout <= 3 ? 3 : 8, 0, 0);
    else { p.row = conv_row(c.bf16 ? CF_IGEMM_BF16 : CF_IGEMM_F32, c.wvm, c.wm, c.wn); p.col = c.bf16 ? c.pf : c.vec4; }
    if (c.direct) p.op = 0;      // (conv_direct_f32 takes in_op as an argument; the other two have none)
    PLAN_REQUIRE(!f16k || (c.bf16 && d->Cout % 32 == 0 && d->out_ctot % 16 == 0 && d->out_coff % 16 == 0), MASIC_ERR_UNSUPPORTED, "%s", no_f16k);
    PLAN_REQUIRE(d->prec != MASIC_PREC_FP8, MASIC_ERR_UNSUPPORTED, "conv2d_fwd: fp8 operands exist on the F8K entry points only (masic_conv_f8k_fwd)");
    PLAN_REQUIRE(p.row && p.row->k[p.op][p.col], MASIC_ERR_UNSUPPORTED, "conv2d_fwd: no kernel compiled for tile <%d, %d, %d>, in_op %d, column %d",
                 c.wvm, c.wm, c.wn, p.op, p.col);
    if (p.g[0].Hp <= 0 || p.g[0].Wp <= 0) { p.empty = true; return p; }
    PLAN_REQUIRE(c.direct != 2 || (!gate && !res1 && !res2), MASIC_ERR_UNSUPPORTED, "conv2d_fwd: gate/residual on the small-Cout deconv path");
    PLAN_REQUIRE(c.direct != 2 || d->Wo % 2 == 0, MASIC_ERR_SHAPE, "conv2d_fwd: odd output width");
    PLAN_REQUIRE(c.direct != 3 || !res2, MASIC_ERR_UNSUPPORTED, "conv2d_fwd: two residuals on the small 5x5 path");
    p.tiles_w = c.direct ? ceil_div(d->Wi, 16) : ceil_div(p.g[0].Wp, c.TW);      // (conv_direct_f32 has no tiles)
    if (c.direct == 1) p.grid = dim3(ceil_div(p.g[0].Hp * p.g[0].Wp, 256) * p.nphase, d->B);
    else if (c.direct) p.grid = dim3(p.tiles_w * ceil_div(d->Hi, 16), d->B);
    else p.grid = dim3(p.tiles_w * ceil_div(p.g[0].Hp, c.TH) * p.nphase, c.Cout_pad / (32 * c.wm * c.wvm), d->B);
    return p;
}

// plan, refuse or return, fill the argument struct of the row's family, launch the row
int conv2d_launch(const float* x, const void* w_packed, const float* bias, const float* gate, const float* res1, const float* res2, float* y,
                  void* y_f16k, const masic_conv_desc_t* d, void* stream) {
    const ConvPlan p = plan_conv(d, (gate ? MASIC_CONV_GATE : 0) | (res1 ? MASIC_CONV_RES1 : 0) | (res2 ? MASIC_CONV_RES2 : 0) | (y_f16k ? MASIC_CONV_F16K_OUT : 0));
    if (p.rc != MASIC_OK || p.empty) return p.rc;
    const ConvCfg& c = p.c;
    const ConvKernelFn k = p.row->k[p.op][p.col];
    if (p.row->family == CF_DECONV4) {
        const Deconv4Args a{x, (const float*)w_packed, bias, y, d->Cin, c.Cin_pad, d->Hi, d->Wi, d->in_ctot, d->in_coff,
                            d->Cout, d->Ho, d->Wo, d->out_ctot, d->out_coff, d->act, p.tiles_w};
        conv_run(k, p.grid, 0, stream, a, (const float*)w_packed);
    } else if (p.row->family == CF_CONV5S1) {
        const Conv5s1Args a{x, bias, gate, res1, y, d->Cin, d->Hi, d->Wi, d->in_ctot, d->in_coff, d->Cout, d->out_ctot, d->out_coff,
                            d->act, p.tiles_w, d->gate_ctot, d->gate_c, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 0.0f, 0.0f, 0.0f};
        conv_run(k, p.grid, 0, stream, a, (const float*)w_packed);
    } else if (p.row->family == CF_DIRECT) {
        const DirectArgs a{x, (const float*)w_packed, bias, gate, res1, res2, y, d->Cin, d->Hi, d->Wi, d->in_ctot, d->in_coff,
                           d->Cout, d->Ho, d->Wo, d->out_ctot, d->out_coff, d->in_op, d->act, d->gate_ctot, d->gate_c, geom_params(*d), p.nphase};
        conv_run(k, p.grid, 0, stream, a);
    } else {
        const IgemmArgs a{x, (const float*)w_packed, bias, gate, res1, res2, y,
                          d->Cin, d->Hi, d->Wi, d->in_ctot, d->in_coff, d->Cout, d->Ho, d->Wo, d->out_ctot, d->out_coff,
                          c.Cin_pad, c.Cout_pad, c.KC, c.KClog, c.TW, c.TWlog, c.SR, c.TH, p.tiles_w,
                          c.PH, c.PW, c.PWp, c.PSZ, c.buf_sz, c.vec4,
                          d->in_op, d->act, d->gate_ctot, d->gate_c, geom_params(*d), p.nphase, (unsigned short*)y_f16k};
        if (p.row->family == CF_IGEMM_BF16) conv_run(k, p.grid, c.lds_bytes, stream, a, (const unsigned short*)w_packed);
        else conv_run(k, p.grid, c.lds_bytes, stream, a);
    }
    return masic_launch_status("conv2d_fwd");
}
}  // namespace

extern "C" size_t masic_conv_packed_bytes(const masic_conv_desc_t* d) { return plan_conv(d, 0).packed_bytes; }

// the kernel of the plain form (no gate, no residual, float32 NCHW output); MASIC_ERR_* and an empty string where the launcher refuses it
extern "C" int masic_conv_kernel_name(const masic_conv_desc_t* d, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0, MASIC_ERR_ARG, "conv_kernel_name: null buffer");
    buf[0] = 0;
    const ConvPlan p = plan_conv(d, 0);
    if (p.rc == MASIC_OK) conv_row_name(*p.row, p.op, p.col, true, buf, n);
    return p.rc;
}

extern "C" int masic_conv_pack_weight(const float* w, void* w_packed, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(w && w_packed, MASIC_ERR_ARG, "conv_pack_weight: null pointer");
    const ConvPlan p = plan_conv(d, 0);
    if (!p.desc_ok) return p.rc;
    const ConvCfg& c = p.c;
    if (c.direct == 2 || c.direct == 3) {
        if (c.direct == 2) hipLaunchKernelGGL(pack_deconv4_kernel, dim3(ceil_div(c.Cin_pad * 100, 256)), dim3(256), 0, (hipStream_t)stream,
                                              w, (float*)w_packed, d->Cin, c.Cin_pad, d->Cout);
        else hipLaunchKernelGGL(pack_conv5s1_kernel, dim3(ceil_div(d->Cin * 25 * c.Cout_pad, 256)), dim3(256), 0, (hipStream_t)stream,
                                w, (float*)w_packed, d->Cin, d->Cout, d->transposed, c.Cout_pad);
        return masic_launch_status("conv_pack_weight");
    }
    PackArgs a{w, (float*)w_packed, d->Cin, d->Cout, d->KH, d->KW, c.Cin_pad, c.Cout_pad, d->transposed, {}};
    int max_taps = 0;
    for (int i = 0; i < p.nphase; ++i) {
        a.gs[i] = p.g[i];
        max_taps = max_taps > p.g[i].ntaps ? max_taps : p.g[i].ntaps;
    }
    const size_t total = (size_t)max_taps * c.Cin_pad * c.Cout_pad;           // the largest phase sizes the grid (grid-stride loops)
    const int blocks = total > 4096 * 256 ? 4096 : (int)((total + 255) / 256);
    if (c.bf16) hipLaunchKernelGGL(pack_weight_bf16_kernel, dim3(blocks, p.nphase), dim3(256), 0, (hipStream_t)stream, a, (unsigned short*)w_packed);
    else hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks, p.nphase), dim3(256), 0, (hipStream_t)stream, a);
    return masic_launch_status("conv_pack_weight");
}

extern "C" int masic_conv2d_fwd_ex(const float* x, const void* w_packed, const float* bias, const float* gate,
                                   const float* res1, const float* res2, float* y, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(x && w_packed && y, MASIC_ERR_ARG, "conv2d_fwd: null pointer");
    return conv2d_launch(x, w_packed, bias, gate, res1, res2, y, nullptr, d, stream);
}

extern "C" int masic_conv2d_fwd(const float* x, const void* w_packed, const float* bias, const float* gate,
                                float* y, const masic_conv_desc_t* d, void* stream) {
    return masic_conv2d_fwd_ex(x, w_packed, bias, gate, nullptr, nullptr, y, d, stream);
}

// 1 when masic_conv2d_f16k_out_fwd has a kernel for the layer: bf16 operands on the implicit-GEMM kernel, whole 32-channel tiles
extern "C" int masic_conv2d_f16k_out_supported(const masic_conv_desc_t* d) { return d && plan_conv(d, MASIC_CONV_F16K_OUT).rc == MASIC_OK; }

extern "C" int masic_conv2d_f16k_out_fwd(const float* x, const void* w_packed, const float* bias, void* y_f16k,
                                         const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(x && w_packed && y_f16k && d, MASIC_ERR_ARG, "conv2d_f16k_out_fwd: null pointer");
    return conv2d_launch(x, w_packed, bias, nullptr, nullptr, nullptr, nullptr, y_f16k, d, stream);
}

// the launch of the call `form` names (MASIC_CONV_*): "kernel | gx,gy,gz | block | lds | integers", the integers being what the kernel is
// handed beside the descriptor's own -- igemm: Cin_pad Cout_pad KC TW TH SR PH PW PSZ buf_sz vec4 nphase; conv_direct_f32: nphase;
// deconv5s2_small_cout: Cin_pad tiles_w; conv5s1_small: tiles_w.  Returns the launcher's code; an empty string when it refuses or launches nothing.
extern "C" int masic_conv_plan_name(const masic_conv_desc_t* d, int form, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0, MASIC_ERR_ARG, "conv_plan_name: no buffer");
    buf[0] = 0;
    MASIC_REQUIRE(d && !(form & ~15) && !((form & MASIC_CONV_F16K_OUT) && (form & ~MASIC_CONV_F16K_OUT)), MASIC_ERR_ARG,
                  "conv_plan_name: no such form (flags %d)", form);
    const ConvPlan p = plan_conv(d, form);
    if (p.rc != MASIC_OK || p.empty) return p.rc;
    const ConvCfg& c = p.c;
    char name[64], ints[128];
    conv_row_name(*p.row, p.op, p.col, false, name, sizeof name);
    if (p.row->family == CF_DECONV4) snprintf(ints, sizeof ints, "%d %d", c.Cin_pad, p.tiles_w);
    else if (p.row->family == CF_CONV5S1) snprintf(ints, sizeof ints, "%d", p.tiles_w);
    else if (p.row->family == CF_DIRECT) snprintf(ints, sizeof ints, "%d", p.nphase);
    else snprintf(ints, sizeof ints, "%d %d %d %d %d %d %d %d %d %d %d %d", c.Cin_pad, c.Cout_pad, c.KC, c.TW, c.TH, c.SR, c.PH, c.PW, c.PSZ, c.buf_sz, c.vec4, p.nphase);
    const bool ok = (size_t)snprintf(buf, n, "%s | %u,%u,%u | %d | %zu | %s\n", name, p.grid.x, p.grid.y, p.grid.z, 256, c.lds_bytes, ints) < n;
    if (!ok) buf[0] = 0;
    MASIC_REQUIRE(ok, MASIC_ERR_ARG, "conv_plan_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}
// every compiled kernel of the table: rows 0 .., columns in_op 0 .. 2 x flag 0 / 1; MASIC_ERR_ARG past the last row and for a column the row lacks
extern "C" int masic_conv_row_name(int row, int in_op, int flag, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0 && row >= 0 && row < CONV_NROWS && in_op >= 0 && in_op < 3 && (flag == 0 || flag == 1) && CONV_ROWS[row].k[in_op][flag],
                  MASIC_ERR_ARG, "conv_row_name: row %d, column %d, %d", row, in_op, flag);
    conv_row_name(CONV_ROWS[row], in_op, flag, false, buf, n);
    return MASIC_OK;
}

// encoder2.pre_conv + pre_gdn and decoder2.after_gdn + cat + after_conv (MASIC.py:559-560, :574-576, :599-600, :617-621) as one
// launch each: Conv2d / ConvTranspose2d(6 -> 3, k5, s1, p2) whose six input channels come from two 3-channel tensors (no
// concat buffer), with an optional 3-channel (I)GDN on the first source while it is staged and / or on the result.
extern "C" int masic_conv5s1_pair_fwd(const float* xa, const float* xb, const float* w_packed, const float* bias,
                                      const float* gin_beta, const float* gin_gamma, int gin_inverse,
                                      const float* gout_beta, const float* gout_gamma, int gout_inverse, double beta_min,
                                      float* y, int B, int H, int W, void* stream) {
    MASIC_REQUIRE(xa && xb && w_packed && y, MASIC_ERR_ARG, "conv5s1_pair_fwd: null pointer");
    MASIC_REQUIRE(B > 0 && H > 0 && W > 0, MASIC_ERR_SHAPE, "conv5s1_pair_fwd: non-positive dimension");
    MASIC_REQUIRE((gin_beta == nullptr) == (gin_gamma == nullptr) && (gout_beta == nullptr) == (gout_gamma == nullptr), MASIC_ERR_ARG,
                  "conv5s1_pair_fwd: a GDN needs both beta and gamma");
    const double ped = 0x1p-36;
    Conv5s1Args a{xa, bias, nullptr, nullptr, y, 6, H, W, 3, 0, 3, 3, 0, MASIC_ACT_NONE, ceil_div(W, 16), 0, 0,
                  xb, 3, gin_beta, gin_gamma, gin_inverse, gout_beta, gout_gamma, gout_inverse,
                  (float)__builtin_sqrt(beta_min + ped), (float)__builtin_sqrt(ped), (float)ped};
    // conv5s1_pair_rows stages and stores in 16-byte pieces (plane rows and tensors 16-byte aligned) and addresses a source's
    // three planes by 32-bit buffer offsets below its out-of-range offset; every other call keeps conv5s1_small<4>
    const bool rows = W % 4 == 0 && (((uintptr_t)xa | (uintptr_t)xb | (uintptr_t)w_packed | (uintptr_t)y) & 15) == 0 &&
                      (size_t)3 * H * W * 4 <= (size_t)0x7ffffff0;
    if (rows) {
        a.tiles_w = ceil_div(W, 64);
        hipLaunchKernelGGL(conv5s1_pair_rows, dim3(ceil_div(W, 64) * ceil_div(H, 16), B), dim3(256), 0, (hipStream_t)stream, a, (const float*)w_packed);
    } else {
        hipLaunchKernelGGL(conv5s1_small<4>, dim3(ceil_div(W, 16) * ceil_div(H, 16), B), dim3(256), 0, (hipStream_t)stream, a, (const float*)w_packed);
    }
    return masic_launch_status("conv5s1_pair_fwd");
}
