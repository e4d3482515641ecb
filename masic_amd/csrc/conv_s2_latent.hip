// conv_s2_latent.hip -- the 5x5 stride-2 128 -> 192 latent layer of the analysis transforms (g_a_conv4, coremasic/mywork/MASIC.py), bf16 F16K
// in, the multi-output epilogue of conv_f16k_multi out: a kernel of its own beside conv_f16k_multi<1 | 2 | 4>, which runs the same layer
// (DESIGN.md section 4.1).  conv_f16k's rows, plan and grid are pinned by tests, and what this kernel does differently needs the layer's
// geometry and both channel counts at compile time.
//
// Same operands, same arithmetic, same bits: the weight stream is what masic_conv_f16k_pack_weight writes for the layer (one phase, two
// co-blocks of 8 chunks x 5 steps of 5 taps x 4 KiB; channels 64 .. 127 of the second co-block are zeros and are never read), the
// contraction runs channel chunks of 16 outermost, taps row-major five per step, on v_mfma_f32_32x32x16_bf16 with the bias as the
// accumulators' initial value, and the epilogue stores what conv_f16k_multi stores.  Waves (0-3 stream weights, 4-7 the patch), ring
// (3 slots, look-ahead 2 steps), patch buffers (2, look-ahead one chunk), counted waits, one raw barrier per step, the DMA pieces behind
// the taps, the parity-de-interleaved patch with immediate tap offsets and the block -> (tile, image) map are conv_s2_gdn_f16k's.  What
// differs from conv_f16k_multi:
//   * a workgroup owns all 192 output channels of its tile (4 x 32 output pixels, for every shape: a pixel's sum order does not depend on
//     the tile): wave w = output row w & 3, channel half w >> 2 = accumulator tiles 0-2 / 3-5.  conv_f16k_multi splits the channels of a
//     tile over up to 8 workgroups of which 6 are live, each fetching the whole patch and walking the whole K loop for 1 / 2 / 4 tiles;
//   * a tap of the ring is 6 KiB: the 4 KiB slab of co-block 0, then bytes [0, 1024) and [2048, 3072) of co-block 1's slab (the two
//     k-halves of its channels 0 .. 63), so the A fragment of every accumulator tile keeps an immediate offset per tap;
//   * 3 MFMAs per wave and tap on 3 A fragments and 1 B fragment (conv_f16k_multi<1>: 1 on 1 + 1);
//   * the patch of a tile is 11 x 67 input pixels with origin (-2, -2), 34 columns per parity, 768 records per k-half plane: 24 KiB a chunk.
// LDS: 90 KiB weight ring | 2 patch buffers of 24 KiB | 768 B bias = 138.75 KiB.
#include "f16k_device.h"
#include "f16k_layer.h"
#include "masic_latent.h"

namespace {

struct LatentArgs {
    const unsigned short* x;      // F16K [B][8][Hi*Wi][16]
    const unsigned char* w;       // slab stream of masic_conv_f16k_pack_weight: two co-blocks
    const float* bias;            // [192] or null
    float* y32;                   // the four outputs of conv_f16k_multi (F16kMulti, conv_f16k.hip), each optional
    float* r32;
    unsigned short* r16;
    unsigned short* a16;
    const float* gate;
    int r16_ctot, r16_coff, gate_ctot, gate_c;
    int Hi, Wi, Ho, Wo, tiles_w, ntiles, xcd_images;
};

constexpr int CL_COUT = 192;
constexpr int CL_T = 5, CL_D = 2, CL_NWS = CL_D + 1;                         // taps per step, weight look-ahead (steps), ring slots
constexpr int CL_SRC = CL_T * 4096, CL_CHUNKS = 8, CL_STEPS = CL_CHUNKS * 5; // bytes per step of one co-block's stream, 16-channel chunks, steps
constexpr int CL_CB1 = CL_STEPS * CL_SRC;                                    // byte offset of co-block 1's stream: 819 200
constexpr int CL_TAP = 6 * 1024, CL_WST = CL_T * CL_TAP;                     // ring bytes per tap / per step
constexpr int CL_WINSTR = CL_T * 6, CL_WSL = (CL_WINSTR + 3) / 4;            // weight DMA wave-instructions (1 KiB) per step; slots per weight wave
constexpr int CL_TH = 4, CL_TW = 32;                                         // output tile
constexpr int CL_PH = (CL_TH - 1) * 2 + 5, CL_PW = (CL_TW - 1) * 2 + 5, CL_PWH = (CL_PW + 1) / 2;   // patch: 11 rows x 67 columns, 34 per parity
constexpr int CL_HALF = CL_PH * CL_PWH;                                      // records per column parity
constexpr int CL_NPIX = (2 * CL_HALF + 31) / 32 * 32;                        // records per k-half plane: 768
constexpr int CL_NINSTR = CL_NPIX / 32;                                      // DMA wave-instructions (1 KiB) per patch chunk: 24
constexpr int CL_PB = CL_NINSTR * 1024;                                      // bytes per patch buffer
constexpr int CL_PSP = 3, CL_NPI = 2 * CL_PSP;                               // patch instructions per patch wave per slice / per chunk
constexpr int CL_RING = 0, CL_PATCH0 = CL_RING + CL_NWS * CL_WST, CL_BIAS = CL_PATCH0 + 2 * CL_PB;
constexpr int CL_LDS = CL_BIAS + CL_COUT * 4;
static_assert(CL_LDS <= 160 * 1024, "LDS");
static_assert(CL_NPI * 4 == CL_NINSTR, "every patch wave moves NPI instructions of a chunk");
static_assert(CL_WSL * 4 >= CL_WINSTR && (CL_WSL - 1) * 4 <= CL_WINSTR, "a surplus weight slot repeats instruction 4 (WSL - 2) + wave of the step");

// byte offset of tap tj of a tap row inside the LDS patch image (row ti adds ti * CL_PWH records)
constexpr int cl_tap(int tj) { return ((tj & 1) * CL_HALF + (tj >> 1)) * 16; }

__global__ __launch_bounds__(512, 1) void conv_s2_latent_f16k(const LatentArgs a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const bool wrole = wave < 4;
    const int wq = wave & 3, ch = wave >> 2;                  // DMA slot of the wave in its role = its output row; its channel half

    int tile, b;
    layer_block_map(a.xcd_images, tile, b);
    if (tile >= a.ntiles) return;
    const int th_i = tile / a.tiles_w, tw_i = tile - th_i * a.tiles_w;
    const int r0 = th_i * CL_TH, c0 = tw_i * CL_TW;
    const int plane_bytes = a.Hi * a.Wi * 32;

    const __amdgpu_buffer_rsrc_t rx = layer_rsrc(a.x + (size_t)b * 8 * (size_t)(a.Hi * a.Wi * 16), 8 * plane_bytes);
    const __amdgpu_buffer_rsrc_t rw = layer_rsrc(a.w, 2 * CL_CB1);

    // Weight DMA instruction n of a step = piece n % 6 of tap n / 6: pieces 0-3 are the slab of co-block 0, pieces 4 and 5 the first KiB
    // of each k-half of co-block 1's slab.  Slot k of weight wave wq is instruction 4 k + wq; the 2 slots past the last instruction
    // repeat slot WSL - 2 of the wave.
    int wsrc[CL_WSL], wdst[CL_WSL];                           // weight waves: byte offsets inside a step of the stream / of the ring
#pragma unroll
    for (int k = 0; k < CL_WSL; ++k) {
        const int n = k * 4 + wq < CL_WINSTR ? k * 4 + wq : (CL_WSL - 2) * 4 + wq;
        const int tap = n / 6, p = n - tap * 6;
        wsrc[k] = tap * 4096 + (p < 4 ? p * 1024 : CL_CB1 + (p - 4) * 2048);
        wdst[k] = tap * CL_TAP + p * 1024;
    }

    // ---- prologue: the first D slab groups (issued before anything is computed for the patch), the first patch chunk and the bias
    int wsoff = 0;                                            // weight producer: byte offset of the next slab group in a co-block's stream
    if (wrole) {
#pragma unroll
        for (int d = 0; d < CL_D; ++d) {
#pragma unroll
            for (int k = 0; k < CL_WSL; ++k) dma_buf16(rw, lds + CL_RING + d * CL_WST + wdst[k], lane * 16, wsoff + wsrc[k]);
            wsoff += CL_SRC;
        }
    }

    // Patch DMA instruction I of a chunk fills bytes [1024 I, 1024 I + 1024) of the patch buffer: records q = 64 I + lane of the image
    // [k-half hh][column parity][row][column / 2] (conv_s2_gdn_f16k's).  Slot k of patch wave wq is instruction 4 k + wq.
    int goff[CL_NPI];                                         // patch waves: byte offset of this lane's record in a chunk of the input
#pragma unroll
    for (int k = 0; k < CL_NPI; ++k) {
        const int q = (k * 4 + wq) * 64 + lane;
        const int hh = q >= CL_NPIX ? 1 : 0, pp = q - hh * CL_NPIX;
        const int par = pp >= CL_HALF ? 1 : 0, rem = pp - par * CL_HALF;
        const int pr = rem / CL_PWH, pc = 2 * (rem - pr * CL_PWH) + par;
        const int ih = 2 * r0 - 2 + pr, iw = 2 * c0 - 2 + pc;
        const bool ok = pp < 2 * CL_HALF && pc < CL_PW && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        goff[k] = ok ? (ih * a.Wi + iw) * 32 + hh * 16 : LAYER_OOB;
    }

    if (!wrole) {
#pragma unroll
        for (int k = 0; k < CL_NPI; ++k) dma_buf16(rx, lds + CL_PATCH0 + (k * 4 + wq) * 1024, goff[k], 0);
    }
    if (tid < CL_COUT) reinterpret_cast<float*>(lds + CL_BIAS)[tid] = a.bias != nullptr ? a.bias[tid] : 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // wave w owns accumulator tiles 3 ch .. 3 ch + 2 (32 output channels each) of output row w & 3; the accumulators start at the bias
    f32x16 acc[3];
    {
        const float* bp = reinterpret_cast<const float*>(lds + CL_BIAS) + ch * 96 + 4 * h;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bv = *reinterpret_cast<const float4*>(bp + m * 32 + 8 * q);
                acc[m][4 * q + 0] = bv.x; acc[m][4 * q + 1] = bv.y; acc[m][4 * q + 2] = bv.z; acc[m][4 * q + 3] = bv.w;
            }
        // a use in front of the K loop: the compiler waits for these reads here and not between the first MFMAs of every chunk
#pragma unroll
        for (int m = 0; m < 3; ++m) asm volatile("" : "+v"(acc[m]));
    }

    const int bl = (h * CL_NPIX + 2 * wq * CL_PWH + j) * 16;  // lane part of the B-fragment address: output pixel (wq, j) reads patch row 2 wq
    // lane part of the A-fragment address of the wave's tiles inside a tap of the ring: tile m < 4 is rows 32 m .. of co-block 0's slab
    // [k-half 2][co 128][8 ci], tiles 4 and 5 rows 0 .. 63 of the 2 KiB [k-half 2][co 64][8 ci] behind it
    int al[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int mg = 3 * ch + m;
        al[m] = mg < 4 ? (h * 128 + mg * 32 + j) * 16 : 4096 + (h * 64 + (mg - 4) * 32 + j) * 16;
    }

    int cslot = 0, pslot = (CL_D % CL_NWS) * CL_WST;          // byte offsets of the consumer / producer ring slots
    int cb = CL_PATCH0, pb = CL_PATCH0 + CL_PB;               // patch buffer of the chunk consumed / of the chunk fetched

    // One step (conv_s2_gdn_f16k's with 3 accumulator tiles): tap row t, 5 taps of 3 MFMAs; the step's DMA pieces -- weight waves: the
    // slab group of step g + D, patch waves: slice S of the next chunk (none in the last chunk) -- go out behind the MFMAs of each tap;
    // counted wait; barrier.
    auto step = [&](auto slice, int t, bool last, int xs, bool fetch) {
        constexpr int S = decltype(slice)::value;
        const int wvo = wsoff < CL_STEPS * CL_SRC ? lane * 16 : LAYER_OOB;       // slab groups past the end of the stream: zeros
        auto dma_pieces = [&](int first, int end) {
            if (wrole) {
#pragma unroll
                for (int k = first; k < end; ++k)
                    if (k < CL_WSL) dma_buf16(rw, lds + CL_RING + pslot + wdst[k], wvo, wsoff + wsrc[k]);
            } else if (S >= 0) {
                if (fetch) {
#pragma unroll
                    for (int u = first; u < end; ++u) {
                        constexpr int k0 = (S >= 0 ? S : 0) * CL_PSP;
                        if (u < CL_PSP) dma_buf16(rx, lds + pb + ((k0 + u) * 4 + wq) * 1024, goff[k0 + u], xs);
                    }
                }
            }
        };
        constexpr int NPIECES = CL_WSL > CL_PSP ? CL_WSL : CL_PSP, per = (NPIECES + CL_T - 1) / CL_T;
        const unsigned wst0 = ldsb + CL_RING + cslot + al[0], wst1 = ldsb + CL_RING + cslot + al[1], wst2 = ldsb + CL_RING + cslot + al[2];
        const unsigned pst = ldsb + cb + t * (CL_PWH * 16) + bl;
        v4u af[2][3], bfr[2];
        auto request = [&](auto ic, auto bc) {
            constexpr int i = decltype(ic)::value, buf = decltype(bc)::value;
            ds_read128<cl_tap(i)>(bfr[buf], pst);
            ds_read128<i * CL_TAP>(af[buf][0], wst0);
            ds_read128<i * CL_TAP>(af[buf][1], wst1);
            ds_read128<i * CL_TAP>(af[buf][2], wst2);
        };
        request(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        static_for<0, CL_T>([&](auto ic) {
            constexpr int i = decltype(ic)::value, buf = i & 1;
            if constexpr (i + 1 < CL_T) request(std::integral_constant<int, i + 1>{}, std::integral_constant<int, (i + 1) & 1>{});
            constexpr int pending = i + 1 < CL_T ? 4 : 0;         // LDS returns in order: what was requested for i + 1 may stay out
            lgkm_wait<pending>(bfr[buf], af[buf][0], af[buf][1], af[buf][2]);
            static_for<0, 3>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[buf][m]), __builtin_bit_cast(bf16x8, bfr[buf]), acc[m], 0, 0, 0);
            });
            __builtin_amdgcn_sched_barrier(0);
            dma_pieces(i * per, (i + 1) * per);
            __builtin_amdgcn_sched_barrier(0);
        });
        if (wrole) {
            wsoff += CL_SRC;
            pslot = layer_ring_next<CL_NWS, CL_WST>(pslot);
        }
        cslot = layer_ring_next<CL_NWS, CL_WST>(cslot);
        // weight waves: the slab group of the next step has landed, the D - 1 groups after it stay in flight.
        // patch waves: at the end of a chunk the next chunk's patch has landed.
        if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((CL_D - 1) * CL_WSL) : "memory");
        else if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    for (int c = 0; c < CL_CHUNKS; ++c) {
        const int xs = (c + 1) * plane_bytes;
        const bool fetch = c + 1 < CL_CHUNKS;
        step(std::integral_constant<int, 0>{}, 0, false, xs, fetch);
        step(std::integral_constant<int, 1>{}, 1, false, xs, fetch);
        for (int t = 2; t < 5; ++t) step(std::integral_constant<int, -1>{}, t, t == 4, xs, fetch);
        const int tmp = cb; cb = pb; pb = tmp;
    }
    // the wave must not end (and its LDS go to another workgroup) with DMA in flight: the weight waves' last two slab groups (zeros past
    // the end of the stream, issued one and two steps ago); the patch waves have nothing out
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue: conv_f16k_multi's.  v = conv + bias is stored in up to four layouts, each in the operation order of the stand-alone
    // kernel it replaces -- rintf in float32, times the gate in float32, ONE rounding to bf16 -- so the bits are the same, -0 included.
    const int r = r0 + wq, c = c0 + j;
    if (r < a.Ho && c < a.Wo) {
        const int m0 = ch * 96;
        const size_t oplane = (size_t)a.Ho * a.Wo, opix = (size_t)r * a.Wo + c;
        const unsigned op = (unsigned)oplane, op16 = op * 16;
        const size_t o32 = ((size_t)b * CL_COUT + m0 + 4 * h) * oplane + opix;
        if (a.y32 != nullptr) {
            float* yb = a.y32 + o32;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * op] = acc[m][e];
        }
        if (a.r32 != nullptr) {
            float* yb = a.r32 + o32;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * op] = rintf(acc[m][e]);
        }
        if (a.r16 != nullptr) {
            // (x * 1.0f is x, sign of zero included: the ungated form needs no second loop)
            const float gv = a.gate != nullptr ? a.gate[((size_t)b * a.gate_ctot + a.gate_c) * oplane + opix] : 1.0f;
            unsigned short* yb = a.r16 + (((size_t)b * (a.r16_ctot >> 4) + ((a.r16_coff + m0) >> 4)) * oplane + opix) * 16 + 8 * h;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                f32x16 t;
#pragma unroll
                for (int e = 0; e < 16; ++e) t[e] = rintf(acc[m][e]) * gv;
                store_f16k_tile(t, yb + (size_t)(2 * m) * op16, op16);
            }
        }
        if (a.a16 != nullptr) {
            unsigned short* yb = a.a16 + (((size_t)b * (CL_COUT >> 4) + (m0 >> 4)) * oplane + opix) * 16 + 8 * h;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                f32x16 t;
#pragma unroll
                for (int e = 0; e < 16; ++e) t[e] = fabsf(acc[m][e]);
                store_f16k_tile(t, yb + (size_t)(2 * m) * op16, op16);
            }
        }
    }
}

struct LatentPlan {
    int Ho, Wo, tiles_w, ntiles, xcd_images;
    dim3 grid;
};

// The smallest number of workgroups (tiles x images) at which the eval forward takes this kernel instead of conv_f16k_multi
// (profiles/conv_s2_latent_ab.txt): at 64 (8 x 512^2 pictures) the launch alone is as long as conv_f16k_multi's (+2 %) on a third of the
// CUs, and the serial forward and the three-stream step are faster with it; at 32 and 8 workgroups the launch alone is 13 % and 22 %
// slower and the step does not change.
constexpr int CL_PREFERRED_MIN_WGS = 64;

// 32-bit offsets inside an image: the float32 output (768 bytes per output pixel, never more output than input pixels) is the larger buffer
bool latent_shape_ok(int B, int Hi, int Wi) { return layer_shape_ok(B, Hi, Wi, CL_COUT * 4); }

LatentPlan latent_plan(int B, int Hi, int Wi) {
    LatentPlan p{};
    p.Ho = (Hi - 1) / 2 + 1;
    p.Wo = (Wi - 1) / 2 + 1;
    p.tiles_w = ceil_div(p.Wo, CL_TW);
    p.ntiles = p.tiles_w * ceil_div(p.Ho, CL_TH);
    p.xcd_images = B % 8 == 0;
    p.grid = dim3(round_up(p.ntiles, 8), 1, B);
    return p;
}

}  // namespace

extern "C" int masic_latent_s2_f16k_supported(int B, int Hi, int Wi) { return latent_shape_ok(B, Hi, Wi) ? 1 : 0; }

extern "C" int masic_latent_s2_f16k_preferred(int B, int Hi, int Wi) {
    if (!latent_shape_ok(B, Hi, Wi)) return 0;
    return (long long)latent_plan(B, Hi, Wi).ntiles * B >= CL_PREFERRED_MIN_WGS ? 1 : 0;
}

extern "C" int masic_latent_s2_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0 && latent_shape_ok(B, Hi, Wi), MASIC_ERR_ARG, "latent_s2_f16k_kernel_name: bad arguments");
    MASIC_REQUIRE((size_t)snprintf(buf, n, "conv_s2_latent_f16k") < n, MASIC_ERR_ARG, "latent_s2_f16k_kernel_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}

extern "C" int masic_latent_s2_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y32, float* round32, void* round16,
                                        void* abs16, const float* gate, int B, int Hi, int Wi, int round16_ctot, int round16_coff,
                                        int gate_ctot, int gate_c, void* stream) {
    MASIC_REQUIRE(x_f16k && w_packed, MASIC_ERR_ARG, "latent_s2_f16k_fwd: null pointer");
    MASIC_REQUIRE(y32 || round32 || round16 || abs16, MASIC_ERR_ARG, "latent_s2_f16k_fwd: no output");
    MASIC_REQUIRE(latent_shape_ok(B, Hi, Wi), MASIC_ERR_UNSUPPORTED, "latent_s2_f16k_fwd: %d x %d x %d is not supported", B, Hi, Wi);
    MASIC_REQUIRE(round16 == nullptr || (round16_ctot % 16 == 0 && round16_coff % 16 == 0 && round16_coff >= 0 && round16_coff + CL_COUT <= round16_ctot),
                  MASIC_ERR_SHAPE, "latent_s2_f16k_fwd: round16 needs a 16-aligned channel view that holds 192 channels");
    MASIC_REQUIRE(gate == nullptr || (round16 != nullptr && gate_c >= 0 && gate_c < gate_ctot), MASIC_ERR_SHAPE,
                  "latent_s2_f16k_fwd: the gate multiplies round16 only; gate channel out of range");
    const LatentPlan p = latent_plan(B, Hi, Wi);
    const LatentArgs a{(const unsigned short*)x_f16k, (const unsigned char*)w_packed, bias, y32, round32, (unsigned short*)round16,
                       (unsigned short*)abs16, gate, round16_ctot, round16_coff, gate_ctot, gate_c,
                       Hi, Wi, p.Ho, p.Wo, p.tiles_w, p.ntiles, p.xcd_images};
    launch_lds<conv_s2_latent_f16k>(p.grid, 512, CL_LDS, (hipStream_t)stream, a);
    return masic_launch_status("latent_s2_f16k_fwd");
}
