// deconv_igdn.hip -- the transposed 5x5 stride-2 128 -> 128 convolution with fused inverse GDN of the synthesis transforms (g_s_conv2 /
// g_s_conv3, coremasic/mywork/MASIC.py), bf16 F16K in and out: a kernel of its own beside conv_f16k<2, 2, 2, 5, 1, true, 4, 2, false> /
// <2, 2, 3, 4, 2, true, 4, 1, false>, which run the same layers.  conv_f16k's rows, plan and grid are pinned by
// tests, and what this kernel does differently needs the layer's geometry at compile time.
//
// Same operands, same arithmetic, same bits: the weight stream is what masic_conv_f16k_pack_weight writes for the layer (per-phase
// streams of 9 / 6 / 6 / 4 taps padded to two per step, KS = 2, T = 2 -- with one co-block the four streams are ONE contiguous sequence of
// 4 x (5 + 3 + 3 + 2) slab groups of 16 KiB), the gamma^ / beta^ image is gdn_pack_f16k_kernel's, the contraction per phase runs channel
// chunks of 32 outermost, taps row-major two per step, the two 16-channel blocks of a tap innermost, on v_mfma_f32_32x32x16_bf16 with
// the bias as the accumulators' initial value, and the epilogue is the one-product gdn_in_registers.
//
// A workgroup owns an input tile and 4 / split of its output phases (blockIdx.y; split = 4: one phase, the default; 2: phases {0, 3} and
// {1, 2}, 13 and 12 taps; 1: all four).  What it does not do that conv_f16k does:
//   * no geometry from kernel arguments and no tap table: every phase reads the same (TH + 2) x (TW + 2) input patch with origin
//     (-1, -1), tap (ti, tj) of any phase is the record (2 - ti, 2 - tj) of it -- a few scalar instructions per step; the patch planes lie
//     packed back to back in LDS and a lane's DMA source offset is recomputed where the instruction is issued instead of held in
//     registers: 255 VGPRs without a spill where conv_f16k<2, 2, 2, 5, 1, true, 4, 2, false> spills 25 in its epilogue;
//   * gamma^ (32 KiB: the hi plane only), beta^ and the bias have LDS of their own and are fetched with the first slabs and the first
//     patch chunk, not after the K loop behind a full memory wait and a barrier: the epilogue starts when the last MFMA has retired.
// With more than one phase per workgroup the K loop is one loop over all its chunks: the weight ring (3 slots, look-ahead 2 steps) and
// the patch buffers (2, look-ahead one chunk) run on across the phase boundary, so the next phase's first slabs and patch land under the
// epilogue, and the later phases re-read the patch from the L2 of the workgroup's own XCD.
// LDS: 32 KiB gamma^ | 512 B beta^ | 512 B bias | 48 KiB weight ring | 2 patch buffers (39 KiB each for the 16 x 32 tile: the four
// (channel block, k-half) planes of 18 x 34 records) = 159 KiB.
#include "f16k_device.h"
#include "f16k_layer.h"
#include "masic_deconv.h"

namespace {

struct DeconvArgs {
    const unsigned short* x;      // F16K [B][8][Hi*Wi][16]
    const unsigned char* w;       // slab stream of masic_conv_f16k_pack_weight
    const float* bias;            // [128] or null
    const unsigned char* gdn;     // gdn_pack_f16k_kernel's image: 64 KiB of gamma^ pieces (even pieces = hi plane), then beta^[128]
    unsigned short* y;            // F16K [B][8][4*Hi*Wi][16]
    int Hi, Wi, tiles_w, ntiles, xcd_images;
    int nsplit;                   // workgroups per tile: 1 (all four phases), 2 (phases {0, 3} and {1, 2}: 13 and 12 taps) or 4 (one phase each), blockIdx.y
};

constexpr int DI_D = 2, DI_NWS = DI_D + 1, DI_WST = 16384;      // weight look-ahead (steps), ring slots, bytes per step (2 taps x 2 blocks x 4 KiB)
constexpr int DI_STEPS = 4 * (5 + 3 + 3 + 2);                   // slab groups of the whole stream

// NW waves (half of them stream weights, half the patch), NP 32-pixel sub-tiles per wave, tile = (32 / TW) NW NP rows of TW = 2^TWLOG pixels
template <int NW, int NP, int TWLOG>
__global__ __launch_bounds__(NW * 64, 1) void deconv_igdn_f16k(const DeconvArgs a) {
    constexpr int TW = 1 << TWLOG, SR = 32 / TW, TH = SR * NW * NP, PH = TH + 2, PW = TW + 2, PR = PH * PW;
    constexpr int NINSTR = (4 * PR + 63) / 64;                   // DMA wave-instructions (1 KiB) per patch chunk: 2 blocks x 2 k-halves x PR records
    constexpr int NWW = NW / 2;                                  // weight waves = patch waves
    constexpr int PSP = (NINSTR + 2 * NWW - 1) / (2 * NWW), NPI = 2 * PSP;   // patch instructions per patch wave per slice / per chunk
    constexpr int WI = 16 / NWW;                                 // weight instructions per weight wave per step
    constexpr int PB = NINSTR * 1024;
    constexpr int BETA = 32768, BIAS = BETA + 512, RING = BIAS + 512, PATCH0 = RING + DI_NWS * DI_WST;
    static_assert(NPI * NWW - NINSTR <= NWW && NINSTR > NWW, "a surplus DMA slot repeats the wave's previous instruction");
    static_assert(PATCH0 + 2 * PB <= 160 * 1024, "LDS");
    static_assert(NP == 1 || NP == 2, "fragment-wait helpers");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const bool wrole = wave < NWW;
    const int wq = wave & (NWW - 1);

    int tile, b;
    layer_block_map(a.xcd_images, tile, b);
    if (tile >= a.ntiles) return;
    const int th_i = tile / a.tiles_w, tw_i = tile - th_i * a.tiles_w;
    const int r0 = th_i * TH, c0 = tw_i * TW;
    const int plane_bytes = a.Hi * a.Wi * 32;

    const __amdgpu_buffer_rsrc_t rx = layer_rsrc(a.x + (size_t)b * 8 * (size_t)(a.Hi * a.Wi * 16), 8 * plane_bytes);
    const __amdgpu_buffer_rsrc_t rw = layer_rsrc(a.w, DI_STEPS * DI_WST), rg = layer_rsrc(a.gdn, LAYER_GDN_BYTES);

    // Patch DMA instruction I of a chunk fills bytes [1024 I, 1024 I + 1024) of the patch buffer: records q = 64 I + lane of the image
    // [block ks][k-half hh][row][col], planes packed back to back.  The lane's source offset is recomputed where the instruction is issued
    // (a dozen VALU instructions in the shadow of the MFMAs) and not kept in registers: the epilogue needs every register it can get.
    auto patch_dma = [&](int k, int pbuf, int xs, bool dead) {
        const int I = k * NWW + wq, Ie = I < NINSTR ? I : I - NWW;
        int lq = lane;
        asm volatile("" : "+v"(lq));                              // (keeps the offsets from being hoisted out of the K loop)
        const int q = Ie * 64 + lq;
        const int plane = q / PR, pp = q - plane * PR;
        const int pr = pp / PW, pc = pp - pr * PW;
        const int ih = r0 - 1 + pr, iw = c0 - 1 + pc;
        const bool ok = !dead && plane < 4 && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        dma_buf16(rx, lds + pbuf + Ie * 1024, ok ? (plane >> 1) * plane_bytes + (ih * a.Wi + iw) * 32 + (plane & 1) * 16 : LAYER_OOB, xs);
    };

    // ---- prologue: gamma^ (hi plane: the even 1 KiB pieces), beta^, bias; the first D slab groups; the first patch chunk
#pragma unroll
    for (int k = 0; k < 32 / NW; ++k) {
        const int p = wave * (32 / NW) + k;
        dma_buf16(rg, lds + p * 1024, lane * 16, p * 2048);
    }
    // the phases of this workgroup: p_first + i p_stride, i < p_count
    const int part = blockIdx.y;
    const int p_first = a.nsplit == 1 ? 0 : part;
    const int p_stride = a.nsplit == 2 ? (part ? 1 : 3) : 1;
    const int p_count = 4 / a.nsplit;
    // slab groups of a phase and in front of it in the stream: 4 chunks x (5, 3, 3, 2) steps
    auto phase_steps = [](int p) { return p == 0 ? 20 : (p == 3 ? 8 : 12); };
    auto phase_first = [](int p) { return p == 0 ? 0 : (p == 1 ? 20 : (p == 2 ? 32 : 44)); };
    // weight producer: byte offset of the next slab group in the stream, groups left in its phase, index of that phase
    int wsoff = phase_first(p_first) * DI_WST, wleft = phase_steps(p_first) - DI_D, wpi = 0;
    if (wrole) {
#pragma unroll
        for (int d = 0; d < DI_D; ++d) {
#pragma unroll
            for (int k = 0; k < WI; ++k) dma_buf16(rw, lds + RING + d * DI_WST + (k * NWW + wq) * 1024, lane * 16, wsoff + (k * NWW + wq) * 1024);
            wsoff += DI_WST;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NPI; ++k) patch_dma(k, PATCH0, 0, false);
    }
    layer_beta_bias_to_lds(reinterpret_cast<float*>(lds + BETA), reinterpret_cast<float*>(lds + BIAS), a.gdn, a.bias, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // wave w owns all 128 output channels of its NP pixel sub-tiles (conv_f16k's layout: the GDN finds a pixel's channels in the wave's registers)
    f32x16 acc[NP][4];
    layer_acc_from_bias<NP>(acc, reinterpret_cast<const float*>(lds + BIAS), h);

    const int jr = j >> TWLOG, jc = j & (TW - 1);
    int bl[NP];                                               // lane part of the B-fragment addresses
#pragma unroll
    for (int n = 0; n < NP; ++n) bl[n] = (h * PR + ((wave * NP + n) * SR + jr) * PW + jc) * 16;
    const int al = (h * 128 + j) * 16;                        // lane part of the A-fragment address

    int cslot = 0, pslot = (DI_D % DI_NWS) * DI_WST;          // byte offsets of the consumer / producer ring slots
    int cb = PATCH0, pb = PATCH0 + PB;                        // patch buffer of the chunk consumed / of the chunk fetched

    // One step (conv_f16k's with T = 2, KS = 2): 2 taps x 2 channel blocks of 4 x NP MFMAs; the step's DMA pieces -- weight waves: the
    // slab group of step g + D, patch waves: slice S of the next chunk -- go out behind the MFMAs of each k-step; counted wait; barrier.
    auto step = [&](auto slice, int t, int ntw, int ntaps, bool last, int xs, bool dead) {
        constexpr int S = decltype(slice)::value;
        const int wvo = wsoff < DI_STEPS * DI_WST ? lane * 16 : LAYER_OOB;      // slab groups past the end of the stream: zeros
        auto dma_pieces = [&](int first, int end) {
            if (wrole) {
#pragma unroll
                for (int k = first; k < end; ++k)
                    if (k < WI) dma_buf16(rw, lds + RING + pslot + (k * NWW + wq) * 1024, wvo, wsoff + (k * NWW + wq) * 1024);
            } else if (S >= 0) {
#pragma unroll
                for (int u = first; u < end; ++u)
                    if (u < PSP) patch_dma((S >= 0 ? S : 0) * PSP + u, pb, xs, dead);
            }
        };
        constexpr int NPIECES = WI > PSP ? WI : PSP, per = (NPIECES + 3) / 4;
        // taps 2t, 2t + 1 of the phase (a tap past the last one aliases tap 0; its weights are zero): tap (ti, tj) reads input pixel
        // (r + 1 - ti, c + 1 - tj) = record (2 - ti, 2 - tj) + (r - r0, c - c0) of the patch
        unsigned tapo[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int tp = 2 * t + tt < ntaps ? 2 * t + tt : 0;
            const int ti = ntw == 2 ? tp >> 1 : (tp * 11) >> 5, tj = tp - ti * ntw;
            tapo[tt] = (unsigned)(((2 - ti) * PW + (2 - tj)) * 16);
        }
        const unsigned wst = ldsb + RING + al + cslot;
        v4u af[2][4], bfr[2][NP];
        auto request = [&](auto ic, auto bc) {
            constexpr int i = decltype(ic)::value, buf = decltype(bc)::value;
            constexpr int tt = i / 2, ks = i % 2;
            const unsigned toff = ldsb + cb + tapo[tt] + ks * (2 * PR * 16);
            static_for<0, NP>([&](auto nc) {
                constexpr int n = decltype(nc)::value;
                ds_read128<0>(bfr[buf][n], toff + bl[n]);
            });
            static_for<0, 4>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                ds_read128<i * 4096 + m * 512>(af[buf][m], wst);
            });
        };
        request(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        static_for<0, 4>([&](auto ic) {
            constexpr int i = decltype(ic)::value, buf = i & 1;
            if constexpr (i + 1 < 4) request(std::integral_constant<int, i + 1>{}, std::integral_constant<int, (i + 1) & 1>{});
            constexpr int pending = i + 1 < 4 ? 4 + NP : 0;       // LDS returns in order: what was requested for i + 1 may stay out
            if constexpr (NP == 2) lgkm_wait<pending>(bfr[buf][0], bfr[buf][1], af[buf][0], af[buf][1], af[buf][2], af[buf][3]);
            else lgkm_wait<pending>(bfr[buf][0], af[buf][0], af[buf][1], af[buf][2], af[buf][3]);
            static_for<0, 4>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                static_for<0, NP>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[buf][m]), __builtin_bit_cast(bf16x8, bfr[buf][n]), acc[n][m], 0, 0, 0);
                });
            });
            __builtin_amdgcn_sched_barrier(0);
            dma_pieces(i * per, (i + 1) * per);
            __builtin_amdgcn_sched_barrier(0);
        });
        if (wrole) {
            wsoff += DI_WST;
            if (--wleft == 0) {                                   // on to the stream of the workgroup's next phase (none: past the end)
                ++wpi;
                const int np = p_first + wpi * p_stride;
                wsoff = wpi < p_count ? phase_first(np) * DI_WST : DI_STEPS * DI_WST;
                wleft = wpi < p_count ? phase_steps(np) : 1 << 30;
            }
            pslot = layer_ring_next<DI_NWS, DI_WST>(pslot);
        }
        cslot = layer_ring_next<DI_NWS, DI_WST>(cslot);
        // weight waves: the slab group of the next step has landed, the D - 1 groups after it stay in flight (stores of an epilogue in
        // between only make the wait stricter).  patch waves: at the end of a chunk the next chunk's patch has landed.
        if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DI_D - 1) * WI) : "memory");
        else if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    const size_t oplane = (size_t)(2 * a.Hi) * (size_t)(2 * a.Wi);
    const unsigned op16 = (unsigned)oplane * 16;
    for (int pi = 0; pi < p_count; ++pi) {
        const int phase = p_first + pi * p_stride, ph = phase >> 1, pw = phase & 1;
        const bool lastp = pi + 1 == p_count;
        const int ntw = pw ? 2 : 3, ntaps = (ph ? 2 : 3) * ntw, spc = (ntaps + 1) >> 1;
        for (int c = 0; c < 4; ++c) {
            // the chunk fetched under chunk c: c + 1 of this phase, or chunk 0 for the next phase (none after the last)
            const int xs = ((c + 1) & 3) * (2 * plane_bytes);
            const bool dead = lastp && c == 3;
            step(std::integral_constant<int, 0>{}, 0, ntw, ntaps, false, xs, dead);
            step(std::integral_constant<int, 1>{}, 1, ntw, ntaps, spc == 2, xs, dead);
            for (int t = 2; t < spc; ++t) step(std::integral_constant<int, -1>{}, t, ntw, ntaps, t + 1 == spc, xs, dead);
            const int tmp = cb; cb = pb; pb = tmp;
        }
        // the wave must not end (and its LDS go to another workgroup) with DMA in flight
        if (lastp) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        // ---- epilogue of the phase: inverse GDN from the resident image, F16K stores; the accumulators return to the bias
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            if (NP > 1) __builtin_amdgcn_sched_barrier(0);      // one sub-tile at a time (register pressure)
            gdn_in_registers<false, 1024>(acc[n], lds + lane * 16, reinterpret_cast<const float*>(lds + BETA) + 4 * h, 1);
            const int r = r0 + (wave * NP + n) * SR + jr, c = c0 + jc;
            if (r < a.Hi && c < a.Wi) {
                const size_t opix = (size_t)(2 * r + ph) * (size_t)(2 * a.Wi) + (size_t)(2 * c + pw);
                unsigned short* yb = a.y + (((size_t)b * 8) * oplane + opix) * 16 + 8 * h;
#pragma unroll
                for (int m = 0; m < 4; ++m) store_f16k_tile(acc[n][m], yb + (size_t)(2 * m) * op16, op16);
            }
        }
        if (!lastp) layer_acc_from_bias<NP>(acc, reinterpret_cast<const float*>(lds + BIAS), h);
    }
}

// tile 1: 16 x 32 input pixels (8 waves of 2 sub-tiles), tile 2: 8 x 32 (8 waves of one); split: workgroups per tile
struct DeconvPlan {
    int tile, split, TH, tiles_w, ntiles;
    size_t lds;
    dim3 grid;
    int xcd_images;
};

constexpr size_t di_lds(int TH, int TW) { return 32768 + 1024 + DI_NWS * DI_WST + 2 * (size_t)((4 * (TH + 2) * (TW + 2) + 63) / 64) * 1024; }

bool deconv_shape_ok(int B, int Hi, int Wi) { return layer_shape_ok(B, Hi, Wi, 4 * 256); }      // the output: four pixels per input pixel
bool deconv_form_ok(int tile, int split) { return tile >= 0 && tile <= 2 && (split == 0 || split == 1 || split == 2 || split == 4); }

DeconvPlan deconv_plan(int B, int Hi, int Wi, int tile, int split) {
    DeconvPlan p{};
    // One phase per workgroup unless the caller asks otherwise.  A workgroup that owns all four phases is the faster launch on an idle
    // chip where its grid is one round (8 x 128 x 128 on 16 x 32 tiles: 256 workgroups), but in the three-stream eval forward its
    // workgroups hold every CU four times as long: kernels of the other streams wait for a CU, workgroups that find a CU taken at
    // launch make a second round, and the step came out slower than with conv_f16k (profiles/deconv_igdn_ab.txt).
    p.split = split == 0 ? 4 : split;
    // The 16 x 32 tile (32 MFMAs per wave between barriers, the slabs read once per 512 pixels) where its grid is at least one workgroup
    // per CU -- both layers of the benchmark: 1024 and 256 workgroups -- else 8 x 32.
    if (tile == 0) tile = (long)ceil_div(Hi, 16) * ceil_div(Wi, 32) * B * p.split >= 256 ? 1 : 2;
    p.tile = tile;
    p.TH = tile == 1 ? 16 : 8;
    p.tiles_w = ceil_div(Wi, 32);
    p.ntiles = p.tiles_w * ceil_div(Hi, p.TH);
    p.lds = di_lds(p.TH, 32);
    p.xcd_images = B % 8 == 0;
    p.grid = dim3(p.xcd_images ? round_up(p.ntiles, 8) : p.ntiles, p.split, B);
    return p;
}

}  // namespace

extern "C" int masic_deconv_igdn_f16k_supported(int B, int Hi, int Wi) { return deconv_shape_ok(B, Hi, Wi) ? 1 : 0; }

extern "C" int masic_deconv_igdn_f16k_kernel_name(int B, int Hi, int Wi, int tile, int split, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0 && deconv_form_ok(tile, split) && deconv_shape_ok(B, Hi, Wi), MASIC_ERR_ARG, "deconv_igdn_f16k_kernel_name: bad arguments");
    const DeconvPlan p = deconv_plan(B, Hi, Wi, tile, split);
    MASIC_REQUIRE((size_t)snprintf(buf, n, p.tile == 1 ? "deconv_igdn_f16k<8, 2, 5>" : "deconv_igdn_f16k<8, 1, 5>") < n, MASIC_ERR_ARG,
                  "deconv_igdn_f16k_kernel_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}

extern "C" int masic_deconv_igdn_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, void* y_f16k,
                                          int B, int Hi, int Wi, int tile, int split, void* stream) {
    MASIC_REQUIRE(x_f16k && w_packed && gdn_packed && y_f16k, MASIC_ERR_ARG, "deconv_igdn_f16k_fwd: null pointer");
    MASIC_REQUIRE(deconv_form_ok(tile, split), MASIC_ERR_ARG, "deconv_igdn_f16k_fwd: tile %d (0, 1 = 16 x 32, 2 = 8 x 32) or split %d (0, 1, 2, 4)", tile, split);
    MASIC_REQUIRE(deconv_shape_ok(B, Hi, Wi), MASIC_ERR_UNSUPPORTED, "deconv_igdn_f16k_fwd: %d x %d x %d is not supported", B, Hi, Wi);
    const DeconvPlan p = deconv_plan(B, Hi, Wi, tile, split);
    const DeconvArgs a{(const unsigned short*)x_f16k, (const unsigned char*)w_packed, bias, (const unsigned char*)gdn_packed, (unsigned short*)y_f16k,
                       Hi, Wi, p.tiles_w, p.ntiles, p.xcd_images, p.split};
    if (p.tile == 1) launch_lds<deconv_igdn_f16k<8, 2, 5>>(p.grid, 512, p.lds, (hipStream_t)stream, a);
    else launch_lds<deconv_igdn_f16k<8, 1, 5>>(p.grid, 512, p.lds, (hipStream_t)stream, a);
    return masic_launch_status("deconv_igdn_f16k_fwd");
}
