// d2s_layer.hip -- the last layer of the synthesis transforms (g_s_conv4, ConvTranspose2d(128 -> C <= 8, k5, s2), coremasic/mywork/MASIC.py)
// as its equivalent stride-1 3x3 convolution to 32 padded rows (row 4c + 2ph + pw) with a depth-to-space store, bf16 F16K in, float32
// NCHW out: a kernel of its own beside conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false>, which runs the same layer at the large shapes
// (DESIGN.md section 4.1).  conv_f16k's rows, plan and grid are pinned by tests, and what this kernel does differently needs the layer's
// geometry at compile time.
//
// Same operands, same arithmetic, same bits: the weight stream is what masic_conv_f16k_pack_weight writes for the layer in that row's
// order (8 chunks of 16 channels x 5 steps of 2 taps x 4 KiB, the tenth tap zeros), the contraction runs the chunks outermost and the
// ten taps of a chunk row-major on v_mfma_f32_32x32x16_bf16 with the bias as the accumulators' initial value, and the epilogue is
// conv_f16k's depth-to-space store.  What differs:
//   * the weights are resident: once per workgroup the live quarter of every slab -- rows 0 .. 31 of both k-halves, two 512-byte runs,
//     1 KiB per (chunk, tap) -- goes into LDS (72 KiB).  conv_f16k streams the whole 4 KiB slab of every tap through a ring for every
//     tile: 320 KiB per tile, more than the tile's patch.  The tenth tap is not stored: its MFMA is issued with a zero A fragment and
//     the B fragment of tap 0, the operands conv_f16k's zero slab and aliased tap-table entry give it;
//   * workgroups are persistent (one per CU) and walk 16 x 32-pixel tiles of their XCD's share of the images (layer_block_map's
//     image-per-XCD rule for B % 8 == 0, plain order otherwise);
//   * waves 8-11 are loaders: the patch of a tile is fetched in 16-channel chunks of 18 x 34 records (origin (-1, -1), tap (u, v) is
//     record u * 34 + v: no tap table) into a ring of four 20-KiB buffers, three chunks ahead and across the tile boundary; a counted
//     vmcnt says that the next chunk has landed;
//   * waves 0-7 own two image rows of the tile each (two accumulator tiles): per chunk the 12 patch fragments of their four patch rows
//     serve the nine taps of both rows (21 LDS reads for 20 MFMAs; conv_f16k: 50 for 40) and ONE barrier hands the drained buffer back
//     to the loaders (conv_f16k: one per 8 MFMAs).
// A pixel's sum order is the chunk / tap order above whatever the tile and the workgroup.
// LDS: 72 KiB weights | 4 patch buffers of 20 KiB = 152 KiB.
#include "f16k_device.h"
#include "f16k_layer.h"
#include "masic_d2s.h"

namespace {

struct D2sArgs {
    const unsigned short* x;      // F16K [B][8][Hi*Wi][16]
    const unsigned char* w;       // slab stream of masic_conv_f16k_pack_weight for the row <1, 2, 3, 5, 2, false, 1, 4, false>
    const float* bias;            // [32] (row 4c + phase) or null
    float* y;                     // float32 [B][y_ctot][2 Hi][2 Wi], channels y_coff .. y_coff + C - 1
    int C, y_ctot, y_coff;
    int Hi, Wi, tiles_w, tpi, ntiles, xcd_images;     // tiles per image row / per image / per walk (an XCD's share or all), block map
};

constexpr int DL_CIN = 128, DL_CHUNKS = DL_CIN / 16;
constexpr int DL_TAPS = 9, DL_STREAM_TAPS = 10;                              // live taps; taps per chunk of the stream (5 steps of 2)
constexpr int DL_STREAM = DL_CHUNKS * DL_STREAM_TAPS * 4096;                 // bytes of the slab stream
constexpr int DL_WBYTES = DL_CHUNKS * DL_TAPS * 1024;                        // resident image: [chunk][tap][k-half][32 co][8 ci]
constexpr int DL_TH = 16, DL_TW = 32;                                        // tile
constexpr int DL_PH = DL_TH + 2, DL_PW = DL_TW + 2, DL_NPIX = DL_PH * DL_PW; // patch: 18 x 34 records per k-half plane
constexpr int DL_NI = (2 * DL_NPIX + 63) / 64;                               // DMA wave-instructions (1 KiB) per patch chunk: 20
constexpr int DL_PB = DL_NI * 1024;                                          // bytes per patch buffer
constexpr int DL_NBUF = 4, DL_PD = DL_NBUF - 1;                              // patch ring; chunks of look-ahead
constexpr int DL_NLW = 4;                                                    // loader waves (8 .. 11)
constexpr int DL_NIW = DL_NI / DL_NLW, DL_NWW = DL_WBYTES / 1024 / DL_NLW;   // patch pieces per loader wave and chunk; weight pieces per loader wave
constexpr int DL_PATCH0 = DL_WBYTES, DL_LDS = DL_PATCH0 + DL_NBUF * DL_PB;
constexpr int DL_MAX_WGS = 256;                                              // one persistent workgroup per CU
static_assert(DL_NIW * DL_NLW == DL_NI && DL_NWW * DL_NLW * 1024 == DL_WBYTES, "every loader wave moves the same number of pieces");
static_assert(DL_NWW + DL_PD * DL_NIW <= 60 && DL_LDS <= 160 * 1024, "vmcnt is 6 bits; LDS");

// s_barrier that the compiler does not move LDS accesses across; what crosses it was waited for explicitly (the loaders' vmcnt) or
// consumed by MFMAs (the compute waves' fragment reads)
__device__ __forceinline__ void dl_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(768, 1) void d2s_layer_f16k(const D2sArgs a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];      // [weights][4 patch chunks]
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;

    // The walk: with the image-per-XCD map, XCD k (block ids go round-robin over the XCDs, gridDim.x is a multiple of 8) walks the tiles
    // of images k, k + 8, ..., its workgroups interleaved; else all workgroups walk all tiles interleaved.
    const int xcd = a.xcd_images ? (int)(blockIdx.x & 7) : 0;
    const int first = a.xcd_images ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int stride = a.xcd_images ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    const int n_my = first < a.ntiles ? (a.ntiles - first + stride - 1) / stride : 0;
    if (n_my == 0) return;
    const int plane_bytes = a.Hi * a.Wi * 32;
    auto tile_of = [&](int i, int& b, int& r0, int& c0) {
        const int idx = first + i * stride;
        const int img = idx / a.tpi, rem = idx - img * a.tpi;
        const int th_i = rem / a.tiles_w;
        b = a.xcd_images ? img * 8 + xcd : img;
        r0 = th_i * DL_TH;
        c0 = (rem - th_i * a.tiles_w) * DL_TW;
    };
    const int ngroups = n_my * DL_CHUNKS;                     // a group = one 16-channel chunk of one tile

    if (wave >= 8) {
        // ---- loaders: wave 8 + lw takes pieces lw, lw + 4, ... of the weights and of every patch chunk
        const int lw = wave - 8;
        int prc[DL_NIW];                                      // k-half << 16 | patch row << 8 | patch column of this lane's record, or -1
#pragma unroll
        for (int k = 0; k < DL_NIW; ++k) {
            const int q = (k * DL_NLW + lw) * 64 + lane;
            const int hh = q >= DL_NPIX ? 1 : 0, pp = q - hh * DL_NPIX;
            const int pr = pp / DL_PW, pc = pp - pr * DL_PW;
            prc[k] = q < 2 * DL_NPIX ? (hh << 16 | pr << 8 | pc) : -1;
        }
        // piece p = tap p % 9 of chunk p / 9: lanes 0-31 bytes [0, 512) of its slab (rows 0 .. 31 of k-half 0), lanes 32-63 bytes [2048, 2560)
        const __amdgpu_buffer_rsrc_t rw = layer_rsrc(a.w, DL_STREAM);
#pragma unroll
        for (int k = 0; k < DL_NWW; ++k) {
            const int piece = k * DL_NLW + lw;
            const int c = piece / DL_TAPS, t = piece - c * DL_TAPS;
            dma_buf16(rw, lds + piece * 1024, j * 16 + h * 2048, (c * DL_STREAM_TAPS + t) * 4096);
        }
        int goff[DL_NIW];                                     // byte offset of this lane's records in a chunk of the current tile's image
        const unsigned short* xb = a.x;
        auto issue = [&](int g) {
            const int i = g >> 3, c = g & 7;
            if (c == 0) {                                     // a new tile (groups past the last one: zeros into a buffer nobody reads)
                int b = 0, r0 = 0, c0 = 0;
                if (i < n_my) {
                    tile_of(i, b, r0, c0);
                    xb = a.x + (size_t)b * DL_CHUNKS * (size_t)(a.Hi * a.Wi * 16);
                }
#pragma unroll
                for (int k = 0; k < DL_NIW; ++k) {
                    const int ih = r0 - 1 + ((prc[k] >> 8) & 0xff), iw = c0 - 1 + (prc[k] & 0xff);
                    const bool ok = i < n_my && prc[k] >= 0 && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
                    goff[k] = ok ? (ih * a.Wi + iw) * 32 + (prc[k] >> 16) * 16 : LAYER_OOB;
                }
            }
            const __amdgpu_buffer_rsrc_t rx = layer_rsrc(xb, DL_CHUNKS * plane_bytes);
            unsigned char* dst = lds + DL_PATCH0 + (g & (DL_NBUF - 1)) * DL_PB;
#pragma unroll
            for (int k = 0; k < DL_NIW; ++k) dma_buf16(rx, dst + (k * DL_NLW + lw) * 1024, goff[k], c * plane_bytes);
        };
#pragma unroll
        for (int g = 0; g < DL_PD; ++g) issue(g);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DL_PD - 1) * DL_NIW) : "memory");      // the weights and group 0 have landed
        dl_barrier();
        for (int g = 0; g < ngroups; ++g) {
            // the buffer of group g + PD is the one group g - 1 was read from: every compute wave left it before the last barrier
            issue(g + DL_PD);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DL_PD - 1) * DL_NIW) : "memory");  // group g + 1 has landed
            dl_barrier();
        }
        // the wave must not end (and its LDS go to another workgroup) with DMA in flight
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ---- compute waves: wave w owns image rows 2 w, 2 w + 1 of the tile, all 32 padded output rows (one accumulator tile per image row)
    float bv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) bv[e] = a.bias != nullptr ? a.bias[4 * h + (e & 3) + 8 * (e >> 2)] : 0.0f;
    const unsigned wa = ldsb + lane * 16;                                               // lane part of the A-fragment address
    const unsigned pbl = ldsb + DL_PATCH0 + (h * DL_NPIX + 2 * wave * DL_PW + j) * 16;    // lane part of the B-fragment address: patch row 2 w
    const size_t oplane = (size_t)a.Hi * a.Wi;
    dl_barrier();                                                                       // the weights and group 0 are in LDS
    for (int i = 0; i < n_my; ++i) {
        f32x16 acc[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[n][e] = bv[e];
        for (int c = 0; c < DL_CHUNKS; ++c) {
            const unsigned pb = pbl + ((i * DL_CHUNKS + c) & (DL_NBUF - 1)) * DL_PB, wc = wa + c * (DL_TAPS * 1024);
            // Patch row rr of the wave's four feeds tap row u of image row n where rr = n + u.  LDS reads go through inline asm with
            // hand-counted lgkmcnt (at most 15 out); LDS returns in order.
            v4u bf[4][3], af[DL_TAPS];
            auto read_b = [&](auto rc) {
                constexpr int rr = decltype(rc)::value;
                ds_read128<(rr * DL_PW + 0) * 16>(bf[rr][0], pb);
                ds_read128<(rr * DL_PW + 1) * 16>(bf[rr][1], pb);
                ds_read128<(rr * DL_PW + 2) * 16>(bf[rr][2], pb);
            };
            auto read_a = [&](auto uc) {
                constexpr int u = decltype(uc)::value;
                ds_read128<(3 * u + 0) * 1024>(af[3 * u + 0], wc);
                ds_read128<(3 * u + 1) * 1024>(af[3 * u + 1], wc);
                ds_read128<(3 * u + 2) * 1024>(af[3 * u + 2], wc);
            };
            auto taps = [&](auto uc) {                        // tap row u: the three taps of image row 0, then of image row 1
                constexpr int u = decltype(uc)::value;
                static_for<0, 2>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    static_for<0, 3>([&](auto vc) {
                        constexpr int v = decltype(vc)::value;
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[3 * u + v]), __builtin_bit_cast(bf16x8, bf[n + u][v]), acc[n], 0, 0, 0);
                    });
                });
            };
            read_b(std::integral_constant<int, 0>{});
            read_b(std::integral_constant<int, 1>{});
            read_a(std::integral_constant<int, 0>{});
            read_b(std::integral_constant<int, 2>{});
            read_a(std::integral_constant<int, 1>{});
            lgkm_wait<6>(bf[0][0], bf[0][1], bf[0][2], bf[1][0], bf[1][1], bf[1][2]);
            lgkm_wait<6>(af[0], af[1], af[2]);
            taps(std::integral_constant<int, 0>{});
            __builtin_amdgcn_sched_barrier(0);
            read_b(std::integral_constant<int, 3>{});
            read_a(std::integral_constant<int, 2>{});
            lgkm_wait<6>(bf[2][0], bf[2][1], bf[2][2], af[3], af[4], af[5]);
            taps(std::integral_constant<int, 1>{});
            lgkm_wait<0>(bf[3][0], bf[3][1], bf[3][2], af[6], af[7], af[8]);
            taps(std::integral_constant<int, 2>{});
            // the stream's tenth tap: a zero slab on tap 0's record (conv_f16k's padding taps alias tap 0)
            const v4u zero = {0u, 0u, 0u, 0u};
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, zero), __builtin_bit_cast(bf16x8, bf[0][0]), acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, zero), __builtin_bit_cast(bf16x8, bf[1][0]), acc[1], 0, 0, 0);
            dl_barrier();                                     // the next group has landed (loaders); this group's buffer may be refilled
        }
        // ---- epilogue: conv_f16k's depth-to-space store.  Row 4c + phase -> pixel (2r + phase / 2, 2c + phase % 2) of channel c: a lane
        // holds whole 2x2 output blocks (channel c = h + 2q in registers 4q .. 4q + 3), two 8-byte stores per block.
        int b, r0, c0;
        tile_of(i, b, r0, c0);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int r = r0 + 2 * wave + n, cx = c0 + j;
            if (r < a.Hi && cx < a.Wi) {
                float* yb = a.y + ((size_t)b * a.y_ctot + a.y_coff) * (4 * oplane) + (size_t)(2 * r) * (2 * a.Wi) + 2 * cx;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cc = h + 2 * q;
                    if (cc < a.C) {
                        float* yc = yb + (size_t)cc * (4 * oplane);
                        *reinterpret_cast<float2*>(yc) = make_float2(acc[n][4 * q], acc[n][4 * q + 1]);
                        *reinterpret_cast<float2*>(yc + 2 * a.Wi) = make_float2(acc[n][4 * q + 2], acc[n][4 * q + 3]);
                    }
                }
            }
        }
    }
}

struct D2sPlan {
    int tiles_w, tpi, ntiles, xcd_images, grid;
};

// The shapes at which conv_f16k runs the layer on the row this kernel stands for (choose_f16k: stride-1 walk, rows of at least 32 pixels,
// at least 512 tiles of 32 x 32 pixels) -- below it conv_f16k sums in 32-channel chunks and packs another stream -- and the smallest
// such tile count at which the eval forward takes this kernel (profiles/d2s_layer_ab.txt).
constexpr long long DL_ROW_MIN_TILES = 512;
constexpr long long DL_PREFERRED_MIN_TILES = 512;

long long d2s_row_tiles(int B, int Hi, int Wi) { return Wi >= 32 ? (long long)ceil_div(Wi, 32) * ceil_div(Hi, 32) * B : 0; }

// 32-bit offsets inside an image (256 bytes per input pixel; the output is at most 128); the tile count of a walk fits an int
bool d2s_shape_ok(int B, int Hi, int Wi) {
    return layer_shape_ok(B, Hi, Wi, 256) && (long long)ceil_div(Wi, DL_TW) * ceil_div(Hi, DL_TH) * B < (1ll << 27);
}

D2sPlan d2s_plan(int B, int Hi, int Wi, int max_wgs) {
    D2sPlan p{};
    p.tiles_w = ceil_div(Wi, DL_TW);
    p.tpi = p.tiles_w * ceil_div(Hi, DL_TH);
    const int cap = max_wgs > 0 && max_wgs < DL_MAX_WGS ? max_wgs : DL_MAX_WGS;
    p.xcd_images = B % 8 == 0 && cap >= 8;
    if (p.xcd_images) {
        p.ntiles = B / 8 * p.tpi;
        p.grid = 8 * (cap / 8 < p.ntiles ? cap / 8 : p.ntiles);
    } else {
        p.ntiles = B * p.tpi;
        p.grid = cap < p.ntiles ? cap : p.ntiles;
    }
    return p;
}

}  // namespace

extern "C" int masic_d2s_layer_f16k_supported(int B, int Hi, int Wi) { return d2s_shape_ok(B, Hi, Wi) ? 1 : 0; }

extern "C" int masic_d2s_layer_f16k_preferred(int B, int Hi, int Wi) {
    if (!d2s_shape_ok(B, Hi, Wi)) return 0;
    const long long t = d2s_row_tiles(B, Hi, Wi);
    return t >= DL_ROW_MIN_TILES && t >= DL_PREFERRED_MIN_TILES ? 1 : 0;
}

extern "C" int masic_d2s_layer_f16k_kernel_name(int B, int Hi, int Wi, char* buf, size_t n) {
    MASIC_REQUIRE(buf && n > 0 && d2s_shape_ok(B, Hi, Wi), MASIC_ERR_ARG, "d2s_layer_f16k_kernel_name: bad arguments");
    MASIC_REQUIRE((size_t)snprintf(buf, n, "d2s_layer_f16k") < n, MASIC_ERR_ARG, "d2s_layer_f16k_kernel_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}

extern "C" int masic_d2s_layer_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y_nchw, int C, int y_ctot, int y_coff,
                                        int B, int Hi, int Wi, int max_wgs, void* stream) {
    MASIC_REQUIRE(x_f16k && w_packed && y_nchw, MASIC_ERR_ARG, "d2s_layer_f16k_fwd: null pointer");
    MASIC_REQUIRE(d2s_shape_ok(B, Hi, Wi), MASIC_ERR_UNSUPPORTED, "d2s_layer_f16k_fwd: %d x %d x %d is not supported", B, Hi, Wi);
    MASIC_REQUIRE(C > 0 && 4 * C <= 32 && max_wgs >= 0, MASIC_ERR_UNSUPPORTED, "d2s_layer_f16k_fwd: needs 0 < C <= 8 and max_wgs >= 0");
    MASIC_REQUIRE(y_coff >= 0 && y_coff + C <= y_ctot, MASIC_ERR_SHAPE, "d2s_layer_f16k_fwd: output channel view out of range");
    const D2sPlan p = d2s_plan(B, Hi, Wi, max_wgs);
    const D2sArgs a{(const unsigned short*)x_f16k, (const unsigned char*)w_packed, bias, y_nchw, C, y_ctot, y_coff,
                    Hi, Wi, p.tiles_w, p.tpi, p.ntiles, p.xcd_images};
    launch_lds<d2s_layer_f16k>(dim3(p.grid), 768, DL_LDS, (hipStream_t)stream, a);
    return masic_launch_status("d2s_layer_f16k_fwd");
}
