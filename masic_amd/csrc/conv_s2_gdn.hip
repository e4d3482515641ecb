// conv_s2_gdn.hip -- the 5x5 stride-2 128 -> 128 convolution with fused forward GDN of the analysis transforms (g_a_conv2 / g_a_conv3,
// coremasic/mywork/MASIC.py), bf16 F16K in and out: a kernel of its own beside conv_f16k<1, 5, 2, 6, 1, true, 4, 1, false>, which runs the
// same layers.  conv_f16k's rows, plan and grid are pinned by tests, and what this kernel does differently needs
// the layer's geometry at compile time.
//
// Same operands, same arithmetic, same bits: the weight stream is what masic_conv_f16k_pack_weight writes for the layer (one phase, one
// co-block: 8 chunks x 5 steps of 5 taps x 4 KiB), the gamma^ / beta^ image is gdn_pack_f16k_kernel's, the contraction runs channel
// chunks of 16 outermost, taps row-major five per step, on v_mfma_f32_32x32x16_bf16 with the bias as the accumulators' initial value,
// and the epilogue is the one-product gdn_in_registers.  Tile (8 x 32 output pixels, for every shape: a pixel's sum order does not depend
// on the tile), waves (0-3 stream weights, 4-7 the patch), ring (3 slots, look-ahead 2 steps), patch buffers (2, look-ahead one chunk),
// counted waits, one raw barrier per step and the block -> (tile, image) map are conv_f16k's for this layer.  What it does not do that
// conv_f16k does:
//   * no geometry from kernel arguments, no tap table and no DMA sink: the patch of a tile is 19 x 67 input pixels with origin (-2, -2),
//     its columns de-interleaved by parity (34 per half), 1312 records per k-half plane, and tap (ti, tj) is the record
//     ((tj & 1) 19 + ti) 34 + (tj >> 1) of it: an immediate offset per tap of a step plus one scalar product per step.  A surplus DMA
//     slot repeats an earlier instruction of the wave;
//   * bias and beta^ have 1 KiB of LDS of their own, written in the prologue: the accumulators start from the LDS copy instead of 64
//     scalar loads per lane;
//   * gamma^ (32 KiB: the hi plane only) is fetched by the patch waves during the last channel chunk, in the DMA slots that would move
//     the chunk past the last one, into the patch buffer that chunk leaves free.  Those waves wait for all their DMA before the last
//     barrier of the K loop anyway, so the epilogue starts right behind that barrier: no DMA round trip and no barrier after the K loop.
// LDS: 60 KiB weight ring | 2 patch buffers of 41 KiB | 512 B beta^ | 512 B bias = 143 KiB.
#include "f16k_device.h"
#include "f16k_layer.h"
#include "masic_conv_s2.h"

namespace {

struct ConvS2Args {
    const unsigned short* x;      // F16K [B][8][Hi*Wi][16]
    const unsigned char* w;       // slab stream of masic_conv_f16k_pack_weight
    const float* bias;            // [128] or null
    const unsigned char* gdn;     // gdn_pack_f16k_kernel's image: 64 KiB of gamma^ pieces (even pieces = hi plane), then beta^[128]
    unsigned short* y;            // F16K [B][8][Ho*Wo][16]
    int Hi, Wi, Ho, Wo, tiles_w, ntiles, xcd_images;
};

constexpr int CS_T = 5, CS_D = 2, CS_NWS = CS_D + 1, CS_WST = CS_T * 4096;   // taps per step, weight look-ahead (steps), ring slots, bytes per step
constexpr int CS_CHUNKS = 8, CS_STEPS = CS_CHUNKS * 5;                       // 16-channel chunks, slab groups of the whole stream
constexpr int CS_TH = 8, CS_TW = 32;                                         // output tile
constexpr int CS_PH = (CS_TH - 1) * 2 + 5, CS_PW = (CS_TW - 1) * 2 + 5, CS_PWH = (CS_PW + 1) / 2;   // patch: 19 rows x 67 columns, 34 per parity
constexpr int CS_HALF = CS_PH * CS_PWH;                                      // records per column parity
constexpr int CS_NPIX = (2 * CS_HALF + 31) / 32 * 32;                        // records per k-half plane: 1312
constexpr int CS_NINSTR = CS_NPIX / 32;                                      // DMA wave-instructions (1 KiB) per patch chunk: 41
constexpr int CS_PB = CS_NINSTR * 1024;                                      // bytes per patch buffer
constexpr int CS_PSP = 6, CS_NPI = 2 * CS_PSP;                               // patch instructions per patch wave per slice / per chunk
constexpr int CS_RING = 0, CS_PATCH0 = CS_RING + CS_NWS * CS_WST, CS_BETA = CS_PATCH0 + 2 * CS_PB, CS_BIAS = CS_BETA + 512;
constexpr int CS_LDS = CS_BIAS + 512;
static_assert(CS_LDS <= 160 * 1024, "LDS");
static_assert(CS_NPI * 4 >= CS_NINSTR && (CS_NPI - 2) * 4 <= CS_NINSTR, "a surplus DMA slot repeats instruction 4 (NPI - 3) + wave of the chunk");
static_assert(32 * 1024 + 4 * 1024 <= CS_PB && CS_NPI * 4 >= 32, "gamma^ and its surplus slots fit a patch buffer and the DMA slots of a chunk");

// byte offset of tap tj of a tap row inside the LDS patch image (row ti adds ti * CS_PWH records)
constexpr int cs_tap(int tj) { return ((tj & 1) * CS_HALF + (tj >> 1)) * 16; }

__global__ __launch_bounds__(512, 1) void conv_s2_gdn_f16k(const ConvS2Args a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const bool wrole = wave < 4;
    const int wq = wave & 3;

    int tile, b;
    layer_block_map(a.xcd_images, tile, b);
    if (tile >= a.ntiles) return;
    const int th_i = tile / a.tiles_w, tw_i = tile - th_i * a.tiles_w;
    const int r0 = th_i * CS_TH, c0 = tw_i * CS_TW;
    const int plane_bytes = a.Hi * a.Wi * 32;

    const __amdgpu_buffer_rsrc_t rx = layer_rsrc(a.x + (size_t)b * 8 * (size_t)(a.Hi * a.Wi * 16), 8 * plane_bytes);
    const __amdgpu_buffer_rsrc_t rw = layer_rsrc(a.w, CS_STEPS * CS_WST), rg = layer_rsrc(a.gdn, LAYER_GDN_BYTES);

    // ---- prologue: the first D slab groups (issued before anything is computed for the patch), the first patch chunk, beta^ and the bias
    int wsoff = 0;                                            // weight producer: byte offset of the next slab group in the stream
    if (wrole) {
#pragma unroll
        for (int d = 0; d < CS_D; ++d) {
#pragma unroll
            for (int k = 0; k < CS_T; ++k) dma_buf16(rw, lds + CS_RING + d * CS_WST + k * 4096 + wq * 1024, wq * 1024 + lane * 16, wsoff + k * 4096);
            wsoff += CS_WST;
        }
    }

    // Patch DMA instruction I of a chunk fills bytes [1024 I, 1024 I + 1024) of the patch buffer: records q = 64 I + lane of the image
    // [k-half hh][column parity][row][column / 2] (conv_f16k's for a strided layer: the stride-2 walk of a tap reads consecutive records).
    // Slot k of patch wave wq is instruction 4 k + wq; the 7 slots past the last instruction repeat slot NPI - 3 of the wave.
    auto patch_instr = [&](int k) { return k * 4 + wq < CS_NINSTR ? k * 4 + wq : (CS_NPI - 3) * 4 + wq; };
    int goff[CS_NPI];                                         // patch waves: byte offset of this lane's record in a chunk of the input
#pragma unroll
    for (int k = 0; k < CS_NPI; ++k) {
        const int q = patch_instr(k) * 64 + lane;
        const int hh = q >= CS_NPIX ? 1 : 0, pp = q - hh * CS_NPIX;
        const int par = pp >= CS_HALF ? 1 : 0, rem = pp - par * CS_HALF;
        const int pr = rem / CS_PWH, pc = 2 * (rem - pr * CS_PWH) + par;
        const int ih = 2 * r0 - 2 + pr, iw = 2 * c0 - 2 + pc;
        const bool ok = pp < 2 * CS_HALF && pc < CS_PW && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        goff[k] = ok ? (ih * a.Wi + iw) * 32 + hh * 16 : LAYER_OOB;
    }

    if (!wrole) {
#pragma unroll
        for (int k = 0; k < CS_NPI; ++k) dma_buf16(rx, lds + CS_PATCH0 + patch_instr(k) * 1024, goff[k], 0);
    }
    layer_beta_bias_to_lds(reinterpret_cast<float*>(lds + CS_BETA), reinterpret_cast<float*>(lds + CS_BIAS), a.gdn, a.bias, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // wave w owns all 128 output channels of pixel sub-tile w = row w of the tile (conv_f16k's layout: the GDN finds a pixel's channels in
    // the wave's registers); the accumulators start at the bias
    f32x16 acc[4];
    {
        const float* bp = reinterpret_cast<const float*>(lds + CS_BIAS) + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bv = *reinterpret_cast<const float4*>(bp + m * 32 + 8 * q);
                acc[m][4 * q + 0] = bv.x; acc[m][4 * q + 1] = bv.y; acc[m][4 * q + 2] = bv.z; acc[m][4 * q + 3] = bv.w;
            }
        // a use in front of the K loop: the compiler waits for these reads here and not, with a stricter lgkmcnt than the counted ones,
        // between the first MFMAs of every chunk (the loop header, where it has to assume them still out)
#pragma unroll
        for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(acc[m]));
    }

    const int bl = (h * CS_NPIX + 2 * wave * CS_PWH + j) * 16;   // lane part of the B-fragment address: output pixel (wave, j) reads patch row 2 wave
    const int al = (h * 128 + j) * 16;                        // lane part of the A-fragment address

    int cslot = 0, pslot = (CS_D % CS_NWS) * CS_WST;          // byte offsets of the consumer / producer ring slots
    int cb = CS_PATCH0, pb = CS_PATCH0 + CS_PB;               // patch buffer of the chunk consumed / of the chunk fetched

    // One step (conv_f16k's with T = 5, KS = 1): tap row t, 5 taps of 4 MFMAs; the step's DMA pieces -- weight waves: the slab group of
    // step g + D, patch waves: slice S of the next chunk (in the last chunk: of gamma^) -- go out behind the MFMAs of each tap; counted
    // wait; barrier.
    auto step = [&](auto slice, int t, bool last, int xs, bool gam) {
        constexpr int S = decltype(slice)::value;
        const int wvo = wsoff < CS_STEPS * CS_WST ? wq * 1024 + lane * 16 : LAYER_OOB;      // slab groups past the end of the stream: zeros
        auto dma_pieces = [&](int first, int end) {
            if (wrole) {
#pragma unroll
                for (int k = first; k < end; ++k)
                    if (k < CS_T) dma_buf16(rw, lds + CS_RING + pslot + k * 4096 + wq * 1024, wvo, wsoff + k * 4096);
            } else if (S >= 0) {
#pragma unroll
                for (int u = first; u < end; ++u) {
                    constexpr int k0 = (S >= 0 ? S : 0) * CS_PSP;
                    if (u < CS_PSP) {
                        if (gam) {
                            // piece p of gamma^'s hi plane = piece 2 p of the image; the slots past piece 31 write zeros behind it
                            const int p = (k0 + u) * 4 + wq;
                            dma_buf16(rg, lds + pb + (p < 32 ? p : 32 + wq) * 1024, p < 32 ? lane * 16 : LAYER_OOB, p < 32 ? p * 2048 : 0);
                        } else {
                            dma_buf16(rx, lds + pb + patch_instr(k0 + u) * 1024, goff[k0 + u], xs);
                        }
                    }
                }
            }
        };
        constexpr int NPIECES = CS_T > CS_PSP ? CS_T : CS_PSP, per = (NPIECES + CS_T - 1) / CS_T;
        const unsigned wst = ldsb + CS_RING + al + cslot;
        const unsigned pst = ldsb + cb + t * (CS_PWH * 16) + bl;
        v4u af[2][4], bfr[2];
        auto request = [&](auto ic, auto bc) {
            constexpr int i = decltype(ic)::value, buf = decltype(bc)::value;
            ds_read128<cs_tap(i)>(bfr[buf], pst);
            static_for<0, 4>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                ds_read128<i * 4096 + m * 512>(af[buf][m], wst);
            });
        };
        request(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        static_for<0, CS_T>([&](auto ic) {
            constexpr int i = decltype(ic)::value, buf = i & 1;
            if constexpr (i + 1 < CS_T) request(std::integral_constant<int, i + 1>{}, std::integral_constant<int, (i + 1) & 1>{});
            constexpr int pending = i + 1 < CS_T ? 5 : 0;         // LDS returns in order: what was requested for i + 1 may stay out
            lgkm_wait<pending>(bfr[buf], af[buf][0], af[buf][1], af[buf][2], af[buf][3]);
            static_for<0, 4>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[buf][m]), __builtin_bit_cast(bf16x8, bfr[buf]), acc[m], 0, 0, 0);
            });
            __builtin_amdgcn_sched_barrier(0);
            dma_pieces(i * per, (i + 1) * per);
            __builtin_amdgcn_sched_barrier(0);
        });
        if (wrole) {
            wsoff += CS_WST;
            pslot = layer_ring_next<CS_NWS, CS_WST>(pslot);
        }
        cslot = layer_ring_next<CS_NWS, CS_WST>(cslot);
        // weight waves: the slab group of the next step has landed, the D - 1 groups after it stay in flight.
        // patch waves: at the end of a chunk the next chunk's patch (gamma^ at the end of the last one) has landed.
        if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((CS_D - 1) * CS_T) : "memory");
        else if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    for (int c = 0; c < CS_CHUNKS; ++c) {
        const int xs = (c + 1) * plane_bytes;
        const bool gam = c + 1 == CS_CHUNKS;                  // the last chunk leaves pb free: gamma^ goes there
        step(std::integral_constant<int, 0>{}, 0, false, xs, gam);
        step(std::integral_constant<int, 1>{}, 1, false, xs, gam);
        for (int t = 2; t < 5; ++t) step(std::integral_constant<int, -1>{}, t, t == 4, xs, gam);
        const int tmp = cb; cb = pb; pb = tmp;
    }
    // the wave must not end (and its LDS go to another workgroup) with DMA in flight: the weight waves' last two slab groups (zeros past
    // the end of the stream, issued one and two steps ago); the patch waves have nothing out
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue: GDN from the image the last chunk fetched (8 chunks: into the first patch buffer), F16K stores
    gdn_in_registers<false, 1024>(acc, lds + CS_PATCH0 + lane * 16, reinterpret_cast<const float*>(lds + CS_BETA) + 4 * h, 0);
    const int r = r0 + wave, c = c0 + j;
    if (r < a.Ho && c < a.Wo) {
        const size_t oplane = (size_t)a.Ho * a.Wo;
        const unsigned op16 = (unsigned)oplane * 16;
        unsigned short* yb = a.y + (((size_t)b * 8) * oplane + (size_t)r * a.Wo + c) * 16 + 8 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m) store_f16k_tile(acc[m], yb + (size_t)(2 * m) * op16, op16);
    }
}
static_assert(CS_CHUNKS % 2 == 0, "the epilogue reads gamma^ from the first patch buffer");

struct ConvS2Plan {
    int Ho, Wo, tiles_w, ntiles, xcd_images;
    dim3 grid;
};

bool conv_s2_shape_ok(int B, int Hi, int Wi) { return layer_shape_ok(B, Hi, Wi, 256); }      // the input (the output is a quarter of it)

ConvS2Plan conv_s2_plan(int B, int Hi, int Wi) {
    ConvS2Plan p{};
    p.Ho = (Hi - 1) / 2 + 1;
    p.Wo = (Wi - 1) / 2 + 1;
    p.tiles_w = ceil_div(p.Wo, CS_TW);
    p.ntiles = p.tiles_w * ceil_div(p.Ho, CS_TH);
    p.xcd_images = B % 8 == 0;
    p.grid = dim3(round_up(p.ntiles, 8), 1, B);
    return p;
}

}  // namespace

extern "C" int masic_conv_s2_gdn_f16k_supported(int B, int Hi, int Wi) { return conv_s2_shape_ok(B, Hi, Wi) ? 1 : 0; }

extern "C" int masic_conv_s2_gdn_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0 && conv_s2_shape_ok(B, Hi, Wi), MASIC_ERR_ARG, "conv_s2_gdn_f16k_kernel_name: bad arguments");
    MASIC_REQUIRE((size_t)snprintf(buf, n, "conv_s2_gdn_f16k") < n, MASIC_ERR_ARG, "conv_s2_gdn_f16k_kernel_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}

extern "C" int masic_conv_s2_gdn_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, void* y_f16k,
                                          int B, int Hi, int Wi, void* stream) {
    MASIC_REQUIRE(x_f16k && w_packed && gdn_packed && y_f16k, MASIC_ERR_ARG, "conv_s2_gdn_f16k_fwd: null pointer");
    MASIC_REQUIRE(conv_s2_shape_ok(B, Hi, Wi), MASIC_ERR_UNSUPPORTED, "conv_s2_gdn_f16k_fwd: %d x %d x %d is not supported", B, Hi, Wi);
    const ConvS2Plan p = conv_s2_plan(B, Hi, Wi);
    const ConvS2Args a{(const unsigned short*)x_f16k, (const unsigned char*)w_packed, bias, (const unsigned char*)gdn_packed, (unsigned short*)y_f16k,
                       Hi, Wi, p.Ho, p.Wo, p.tiles_w, p.ntiles, p.xcd_images};
    launch_lds<conv_s2_gdn_f16k>(p.grid, 512, CS_LDS, (hipStream_t)stream, a);
    return masic_launch_status("conv_s2_gdn_f16k_fwd");
}
