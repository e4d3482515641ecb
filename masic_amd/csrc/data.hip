// data.hip -- the per-item preparation of the reference's paired dataset on the device (SURVEY.md 8(f)-4;
// compressai/datasets/utils.py:207-285): the paired crop as float32 CHW / 255 (ToTensor), and the grey 128 x 128 patch the
// homography network reads -- cv2.resize of the crop to 256 x 256 (uint8, INTER_LINEAR), ToTensor, Normalize with the scalar
// MEAN / STD of utils.py:26-27, mean over the channels, patch at (x, y).  The reference does this per picture in DataLoader
// workers (cv2 on the host); here the decoded uint8 picture is uploaded once and both outputs come out of two launches.
// The resize follows OpenCV's uint8 algorithm bit for bit (resize.cpp: pixel-centre mapping, 11-bit fixed-point coefficients,
// int32 horizontal pass, (b*(t>>4))>>16 vertical pass, +2 >>2; an exact 2x decimation runs as the rounded 2x2 box mean), and
// only the patch window of the resized picture is ever computed.  cv2 itself is absent: parity is pinned by the numpy
// restatement oracle/data_oracle.py.
// Below that: the two ends of the stereo file pipeline over a stack of pictures per launch -- masic_pairs_prep (uint8 pictures ->
// float planes padded by edge replication + the patches of the unpadded pictures) and masic_planes_to_u8 (planes -> cropped uint8).
// Last: masic_views_prep, the training batch of a device-resident dataset (masic_amd/data.py) -- P views, each its own crop of its own
// picture of an arena of decoded pictures, one descriptor per view in device memory, two launches for the whole batch -- and
// masic_udh_views_prep, the batch the homography net itself trains on (udh/udh/dataset.py), out of the same arena: PIL's antialiased
// two-pass bilinear Resize + CenterCrop, bit for bit, from coefficient tables the host computes as Pillow does.  The two resizes differ
// (cv2: two taps at any scale, 11-bit; PIL: a support that grows with the scale, 22-bit, uint8 between the passes); the grey tail is one.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void crop_to_tensor_kernel(const unsigned char* __restrict__ img, int W, int h0, int w0, int ph, int pw,
                                                             float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ph * pw) return;
    const int r = i / pw, c = i - r * pw;
    const unsigned char* p = img + ((size_t)(h0 + r) * W + (w0 + c)) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[(size_t)ch * ph * pw + i] = (float)p[ch] / 255.0f;
}

__device__ __forceinline__ void lin_coeff(int d, double scale, int src, int& s, int& c0, int& c1) {
    float f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= src - 1) { s = src - 1; f = 0.0f; }
    c0 = (int)rintf((1.0f - f) * 2048.0f);
    c1 = (int)rintf(f * 2048.0f);
}

// mean_c(Normalize(ToTensor(.))) of one resized uint8 pixel with the scalar MEAN / STD: the tail of every grey output of this file (the codec's
// patches and the UDH batch), so they cannot drift apart.  Each operation is rounded once (no fused multiply-add, no reciprocal).
__device__ __forceinline__ float grey_value(const int (&v)[3], float mean, float stdv) {
    float n[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) n[ch] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v[ch], 255.0f), mean), stdv);
    return __fdiv_rn(__fadd_rn(__fadd_rn(n[0], n[1]), n[2]), 3.0f);
}

// Element i of the patch of one picture (img: its first byte); shared by the per-picture and the batched kernel, so the two agree bit for bit.
__device__ __forceinline__ void homo_patch_element(const unsigned char* __restrict__ img, int W, int h0, int w0, int ph, int pw, int S, int px0,
                                                   int py0, int patch, float mean, float stdv, float* __restrict__ out, int i) {
    const int dy = py0 + i / patch, dx = px0 + i % patch;              // pixel of the S x S resized crop
    int v[3];
    if (ph == 2 * S && pw == 2 * S) {
        const unsigned char* p = img + ((size_t)(h0 + 2 * dy) * W + (w0 + 2 * dx)) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (p[ch] + p[3 + ch] + p[(size_t)W * 3 + ch] + p[(size_t)W * 3 + 3 + ch] + 2) >> 2;
    } else {
        int sx, a0, a1, sy, b0, b1;
        lin_coeff(dx, (double)pw / S, pw, sx, a0, a1);
        lin_coeff(dy, (double)ph / S, ph, sy, b0, b1);
        const int sx1 = min(sx + 1, pw - 1), sy1 = min(sy + 1, ph - 1);
        const unsigned char* r0 = img + ((size_t)(h0 + sy) * W + w0) * 3;
        const unsigned char* r1 = img + ((size_t)(h0 + sy1) * W + w0) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int t0 = r0[sx * 3 + ch] * a0 + r0[sx1 * 3 + ch] * a1;
            const int t1 = r1[sx * 3 + ch] * a0 + r1[sx1 * 3 + ch] * a1;
            const int o = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
            v[ch] = min(max(o, 0), 255);
        }
    }
    out[i] = grey_value(v, mean, stdv);
}

__global__ __launch_bounds__(256) void homo_patch_kernel(const unsigned char* __restrict__ img, int W, int h0, int w0, int ph, int pw,
                                                         int S, int px0, int py0, int patch, float mean, float stdv,
                                                         float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < patch * patch) homo_patch_element(img, W, h0, w0, ph, pw, S, px0, py0, patch, mean, stdv, out, i);
}

// The same patch of each of the P pictures of a stack [P][H0][W0][3] (blockIdx.y = picture), the whole picture being the crop.
__global__ __launch_bounds__(256) void homo_patches_kernel(const unsigned char* __restrict__ pics, int H0, int W0, int S, int px0, int py0,
                                                           int patch, float mean, float stdv, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= patch * patch) return;
    const size_t p = blockIdx.y;
    homo_patch_element(pics + p * H0 * W0 * 3, W0, 0, 0, H0, W0, S, px0, py0, patch, mean, stdv, out + p * patch * patch, i);
}

// ---- the two ends of the stereo file pipeline (masic_amd/stereofile.py): P pictures uint8 [P][H0][W0][3] <-> float32 planes [P][3][H][W],
// H >= H0, W >= W0.  Both stream: 3 bytes a pixel on the interleaved side, 12 on the planar side.  A lane owns FOUR consecutive pixels of a
// row -- one 16-byte access per plane -- and a workgroup one segment of `segl` lanes of 256 / segl rows (segl a multiple of 64: 64 lanes x 4
// rows for narrow pictures up to 256 x 1 row).  The 12 interleaved bytes of a lane start at a multiple of 3, so they go through LDS: a row
// segment's bytes cross the global boundary as aligned 32-bit words, laid out in LDS at the global address's offset within its word, and
// the lanes pick or place single bytes there (12-byte lane stride: three banks, conflict-free over a wavefront).
constexpr int PIX_REGION_WORDS = 776;      // rows * (3 * segl + 2) words at most: 4 * 194

struct pix_block {
    int r, l, y, x, valid;      // row of the block, lane of the segment, picture row, first pixel; lane inside the picture
    uint32_t* region;
};
__device__ __forceinline__ pix_block pix_block_of(uint32_t* lds, int segl, int Hlim) {
    pix_block b;
    const int rows = 256 / segl;
    b.r = threadIdx.x / segl;
    b.l = threadIdx.x - b.r * segl;
    b.y = blockIdx.y * rows + b.r;
    b.x = (blockIdx.x * segl + b.l) * 4;
    b.valid = b.r < rows && b.y < Hlim;
    b.region = lds + b.r * (3 * segl + 2);
    return b;
}

// planes[p][c][y][x] = pics[p][min(y, H0-1)][min(x, W0-1)][c] / 255 (the division of crop_to_tensor_kernel); vec: W % 4 == 0 and a 16-byte
// aligned base.  nbytes = P * H0 * W0 * 3; pics is 4-byte aligned, and the one word that may reach past nbytes is read bytewise.
__global__ __launch_bounds__(256) void pairs_planes_kernel(const unsigned char* __restrict__ pics, size_t nbytes, int H0, int W0, int H, int W,
                                                           int segl, int vec, float* __restrict__ planes) {
    __shared__ uint32_t lds[PIX_REGION_WORDS];
    const int rows = 256 / segl, seg_pix = segl * 4;
    const size_t p = blockIdx.z;
    const int x0 = blockIdx.x * seg_pix;
    const int s0 = min(x0, W0 - 1), s1 = max(min(x0 + seg_pix, W0), s0 + 1);      // source pixels [s0, s1) of this segment, never empty
    const uint32_t* words = reinterpret_cast<const uint32_t*>(pics);
    for (int r = 0; r < rows; ++r) {
        const int y = blockIdx.y * rows + r;
        if (y >= H) break;
        const size_t g0 = ((p * H0 + min(y, H0 - 1)) * W0 + s0) * 3;              // first byte of the segment's source pixels
        const int sh = (int)(g0 & 3), nw = (sh + (s1 - s0) * 3 + 3) >> 2;
        uint32_t* region = lds + r * (3 * segl + 2);
        for (int i = threadIdx.x; i < nw; i += 256) {
            const size_t wi = (g0 >> 2) + i;
            uint32_t v;
            if (wi * 4 + 4 <= nbytes) {
                v = words[wi];
            } else {
                v = 0;
                for (size_t k = wi * 4; k < nbytes; ++k) v |= (uint32_t)pics[k] << (8 * (k - wi * 4));
            }
            region[i] = v;
        }
    }
    __syncthreads();
    const pix_block b = pix_block_of(lds, segl, H);
    if (!b.valid || b.x >= W) return;
    const size_t g0 = ((p * H0 + min(b.y, H0 - 1)) * W0 + s0) * 3;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(b.region) + (g0 & 3);
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = (min(b.x + k, W0 - 1) - s0) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch][k] = (float)bytes[s + ch] / 255.0f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float* o = planes + ((p * 3 + ch) * H + b.y) * W + b.x;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (b.x + k < W) o[k] = v[ch][k];
        }
    }
}

// out[p][y][x][c] = floor(clamp(planes[p][c][y][x], 0, 1) * 255 + 0.5), NaN -> 0 (two float32 roundings: torchvision's save_image), for
// y < H0, x < W0.  out is 4-byte aligned; a word that holds bytes of a neighbouring segment or row is written bytewise.
__device__ __forceinline__ unsigned char to_u8(float v) {
    const float c = !(v > 0.0f) ? 0.0f : (v < 1.0f ? v : 1.0f);
    return (unsigned char)(int)floorf(__fadd_rn(__fmul_rn(c, 255.0f), 0.5f));
}

__global__ __launch_bounds__(256) void planes_to_u8_kernel(const float* __restrict__ planes, int H, int W, int H0, int W0, int segl, int vec,
                                                           unsigned char* __restrict__ out) {
    __shared__ uint32_t lds[PIX_REGION_WORDS];
    const int rows = 256 / segl, seg_pix = segl * 4;
    const size_t p = blockIdx.z;
    const int x0 = blockIdx.x * seg_pix, x1 = min(x0 + seg_pix, W0);             // pixels [x0, x1) of this segment; x0 < W0 by the grid
    const pix_block b = pix_block_of(lds, segl, H0);
    if (b.valid && b.x < W0) {
        const size_t g0 = ((p * H0 + b.y) * W0 + x0) * 3;
        unsigned char* bytes = reinterpret_cast<unsigned char*>(b.region) + (g0 & 3) + b.l * 12;
        float v[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = planes + ((p * 3 + ch) * H + b.y) * W + b.x;
            if (vec) {
                const float4 t = *reinterpret_cast<const float4*>(s);
                v[ch][0] = t.x; v[ch][1] = t.y; v[ch][2] = t.z; v[ch][3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[ch][k] = b.x + k < W0 ? s[k] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (b.x + k < W0) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) bytes[k * 3 + ch] = to_u8(v[ch][k]);
            }
    }
    __syncthreads();
    uint32_t* words = reinterpret_cast<uint32_t*>(out);
    for (int r = 0; r < rows; ++r) {
        const int y = blockIdx.y * rows + r;
        if (y >= H0) break;
        const size_t g0 = ((p * H0 + y) * W0 + x0) * 3;
        const int sh = (int)(g0 & 3), end = sh + (x1 - x0) * 3, nw = (end + 3) >> 2;      // the segment's bytes are [sh, end) of the region
        const uint32_t* region = lds + r * (3 * segl + 2);
        for (int i = threadIdx.x; i < nw; i += 256) {
            const size_t wi = (g0 >> 2) + i;
            if (4 * i >= sh && 4 * i + 4 <= end) {
                words[wi] = region[i];
            } else {
                const unsigned char* src = reinterpret_cast<const unsigned char*>(region);
                for (int k = max(4 * i, sh); k < min(4 * i + 4, end); ++k) out[wi * 4 + (k - 4 * i)] = src[k];
            }
        }
    }
}

// ---- the batch of a device-resident dataset (masic_amd/data.py): the pictures lie back to back in one uint8 arena, [H_i][W_i][3] each from a
// 16-byte aligned offset, and view p of a batch is the crop [start_h : +ph, start_w : +pw] of the picture its descriptor names.
// A descriptor that does not fit its picture or the arena is skipped whole by both kernels (the caller refuses it before it launches; a
// fault here would be everybody's), so no read leaves the arena whatever the table holds.
__device__ __forceinline__ bool view_inside(const masic_view_desc_t& d, size_t arena_bytes, int ph, int pw) {
    return d.W > 0 && d.H > 0 && d.start_h >= 0 && d.start_w >= 0 && d.start_h <= d.H - ph && d.start_w <= d.W - pw && d.offset <= arena_bytes &&
           (uint64_t)d.H * (uint64_t)d.W * 3u <= arena_bytes - d.offset;
}

// planes[p][c][y][x] = u8 / 255 of the crop of view p (the division of crop_to_tensor_kernel).  The lane and workgroup shapes are those of
// pairs_planes_kernel: a lane owns four consecutive pixels of a row, a workgroup one segment of `segl` lanes of 256 / segl rows; blockIdx.x =
// (p * ysegs + row block) * xsegs + segment, so the number of views is not bound by a grid extent.  A segment's bytes start anywhere --
// offset + ((start_h + y) * W_i + start_w + x0) * 3, every residue mod 4, another one on the next row when W_i is odd -- and cross the
// global boundary as the aligned 32-bit words that hold them, each lane fetching the words l, l + segl, ... of its own row: word i of
// the LDS region is word i of that run.  A lane's 12 bytes then begin `sh` bytes into word 3 l: four LDS words (stride 3 words: no bank
// is hit twice by a half-wavefront), shifted together, hold them.  arena_bytes % 4 == 0 and the arena is 4-byte aligned, so the last
// word of a picture lies inside the arena as well.
__global__ __launch_bounds__(256) void views_planes_kernel(const unsigned char* __restrict__ arena, size_t arena_bytes,
                                                           const masic_view_desc_t* __restrict__ desc, int ph, int pw, int segl, int xsegs,
                                                           int ysegs, int vec, float* __restrict__ planes) {
    __shared__ uint32_t lds[PIX_REGION_WORDS];
    const int rows = 256 / segl, seg_pix = segl * 4;
    const int xb = blockIdx.x % xsegs, yb = (blockIdx.x / xsegs) % ysegs;
    const size_t p = blockIdx.x / xsegs / ysegs;
    const masic_view_desc_t d = desc[p];
    if (!view_inside(d, arena_bytes, ph, pw)) return;
    const int r = threadIdx.x / segl, l = threadIdx.x - r * segl;
    const int y = yb * rows + r, x0 = xb * seg_pix, x = x0 + 4 * l;
    const bool row = r < rows && y < ph;
    const int n = min(seg_pix, pw - x0);                                            // pixels of this segment, > 0 by the grid
    const size_t g0 = d.offset + ((size_t)(d.start_h + (row ? y : 0)) * d.W + d.start_w + x0) * 3;
    const int sh = (int)(g0 & 3), nw = (sh + n * 3 + 3) >> 2;
    uint32_t* region = lds + r * (3 * segl + 2);
    if (row) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(arena) + (g0 >> 2);
        for (int i = l; i < nw; i += segl) region[i] = words[i];
    }
    __syncthreads();
    if (!row || x >= pw) return;
    const uint32_t w0 = region[3 * l], w1 = region[3 * l + 1], w2 = region[3 * l + 2], w3 = region[3 * l + 3];
    const int s8 = 8 * sh;
    uint32_t w[3];
    w[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> s8);
    w[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> s8);
    w[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> s8);
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int b = k * 3 + ch;
            v[ch][k] = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu) / 255.0f;
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float* o = planes + ((p * 3 + ch) * ph + y) * pw + x;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < pw) o[k] = v[ch][k];
        }
    }
}

// patches[p] = the patch at (patch_x, patch_y) of view p's crop resized to S x S: homo_patch_element itself, so the three resize branches
// are pair_prep's.  blockIdx.x = p * blocks per patch + block.
__global__ __launch_bounds__(256) void views_patches_kernel(const unsigned char* __restrict__ arena, size_t arena_bytes,
                                                            const masic_view_desc_t* __restrict__ desc, int ph, int pw, int S, int patch,
                                                            int nb, float mean, float stdv, float* __restrict__ out) {
    const size_t p = blockIdx.x / nb;
    const int i = (blockIdx.x - (int)p * nb) * 256 + threadIdx.x;
    if (i >= patch * patch) return;
    const masic_view_desc_t d = desc[p];
    if (!view_inside(d, arena_bytes, ph, pw) || d.patch_x < 0 || d.patch_y < 0 || d.patch_x > S - patch || d.patch_y > S - patch) return;
    homo_patch_element(arena + d.offset, d.W, d.start_h, d.start_w, ph, pw, S, d.patch_x, d.patch_y, patch, mean, stdv, out + p * patch * patch, i);
}

// ---- the batch of the homography net's own training (udh/udh/dataset.py: SyntheticDataset) out of the same arena: PIL's antialiased
// bilinear Resize(S) + CenterCrop(S) + the grey tail, of which only the rectangle a view asks for is computed.  PIL resizes in two passes
// with a uint8 picture between them; both run here in one workgroup, the intermediate in LDS.  A workgroup owns one view and one tile of
// 16 x 16 output pixels:
//   1. the tile's table entries (xmin, n per output column / row; the coefficients) go to LDS and are range-checked;
//   2. the source rows the tile's vertical taps reach, [y_lo, y_hi), are walked in chunks of 32: the bytes of the source columns the
//      tile's horizontal taps reach, [x_lo, x_hi), cross the global boundary as the aligned 32-bit words that hold them (coalesced, flat
//      over the chunk), then the horizontal pass writes 16 x 3 uint8 per row into `mid`.  In that pass a lane owns a ROW of the chunk and
//      a wavefront half one output column at a time, so the coefficients are broadcasts and the byte reads and writes of the 32 lanes go
//      to 32 rows whose strides (221 and 13 words) are odd: no bank is hit twice;
//   3. the vertical pass reads `mid` into registers, one lane per output pixel, then grey_value and the store; four neighbours' values
//      meet in one lane by shuffles for the 16-byte store.
// An axis that keeps its size has ksize 0 and no table: its bytes are copied (xmin = crop origin + position, one "tap" that is not
// multiplied).  LDS: 32 x 221 words of source + 291 x 13 words of intermediate + 2 x 16 x 35 coefficients + bounds = 47.0 KiB, sized for
// the largest scale served: Resize(S) by 16 on the shorter side leaves the longer one, whose output size is rounded down, a scale of up
// to 17 (256 x 300 -> 16 x 18 is 16.7), so ceil(in / out) <= 17 per axis, ksize <= 35, and a tile's 16 outputs reach at most
// 15 * 17 + 2 * 17 + 1 = 290 source pixels per axis; three workgroups fit a CU.  All arithmetic is int32 (255 * 2^22 + 2^21 < 2^31) or
// float32.
constexpr int UDH_TILE = 16, UDH_KMAX = 35, UDH_CHUNK = 32, UDH_SPAN = 291;
constexpr int UDH_SRC_WORDS = 221;      // (3 + 291 * 3 + 3) / 4 = 219 and a pad, odd
constexpr int UDH_MID_WORDS = 13;       // 16 x 3 bytes + 4, odd

__device__ __forceinline__ int round_half_even_half(int d) {      // Python's round(d / 2.0), d >= 0
    const int m = d >> 1;
    return (d & 1) ? m + (m & 1) : m;
}

// ksize of one axis as PIL computes it: 0 stands for "same size, no pass"; -1 for a scale that is not served
__device__ __forceinline__ int udh_axis_ksize(int in, int out) {
    if (in == out) return 0;
    const int s = in > out ? (in + out - 1) / out : 1;
    return s <= 17 ? 2 * s + 1 : -1;
}

// The host's check (ops.check_udh_view_descriptors) again; top / left: the centre crop's origin in the resized picture
__device__ __forceinline__ bool udh_view_inside(const masic_udh_view_desc_t& d, size_t arena_bytes, size_t table_words, int S, int out_h,
                                                int out_w, int& top, int& left) {
    if (d.W <= 0 || d.H <= 0 || d.W >= (1 << 24) || d.H >= (1 << 24)) return false;
    if (d.offset > arena_bytes || (uint64_t)d.H * (uint64_t)d.W * 3u > arena_bytes - d.offset) return false;
    if (d.x0 < 0 || d.y0 < 0 || d.x0 > S - out_w || d.y0 > S - out_h) return false;
    long long ow = S, oh = S;                                     // torchvision's Resize(int): the shorter side becomes S
    if (d.W <= d.H) oh = (long long)S * d.H / d.W; else ow = (long long)S * d.W / d.H;
    if (ow >= (1 << 24) || oh >= (1 << 24)) return false;
    const int ksh = udh_axis_ksize(d.W, (int)ow), ksv = udh_axis_ksize(d.H, (int)oh);
    if (ksh < 0 || ksv < 0 || ksh != d.h_ksize || ksv != d.v_ksize) return false;
    if (ksh && (d.h_table > table_words || (uint64_t)S * (uint64_t)(2 + ksh) > table_words - d.h_table)) return false;
    if (ksv && (d.v_table > table_words || (uint64_t)S * (uint64_t)(2 + ksv) > table_words - d.v_table)) return false;
    top = round_half_even_half((int)oh - S);
    left = round_half_even_half((int)ow - S);
    return true;
}

__global__ __launch_bounds__(256) void udh_views_kernel(const unsigned char* __restrict__ arena, size_t arena_bytes, const int* __restrict__ tables,
                                                        size_t table_words, const masic_udh_view_desc_t* __restrict__ desc, int S, int out_h,
                                                        int out_w, int xt, int yt, int vec, float mean, float stdv, float* __restrict__ out) {
    __shared__ uint32_t src[UDH_CHUNK * UDH_SRC_WORDS];
    __shared__ uint32_t mid[UDH_SPAN * UDH_MID_WORDS];
    __shared__ int hk[UDH_TILE * UDH_KMAX], vk[UDH_TILE * UDH_KMAX];
    __shared__ int hx[UDH_TILE], hn[UDH_TILE], vx[UDH_TILE], vn[UDH_TILE];
    const int t = threadIdx.x;
    const int tx = blockIdx.x % xt, ty = (blockIdx.x / xt) % yt;
    const size_t p = blockIdx.x / xt / yt;
    const masic_udh_view_desc_t d = desc[p];
    int top, left;
    if (!udh_view_inside(d, arena_bytes, table_words, S, out_h, out_w, top, left)) return;
    const int tw = min(UDH_TILE, out_w - tx * UDH_TILE), th = min(UDH_TILE, out_h - ty * UDH_TILE);      // > 0 by the grid
    const int X0 = d.x0 + tx * UDH_TILE, Y0 = d.y0 + ty * UDH_TILE;                                       // the tile in the S x S picture
    const int ksh = d.h_ksize, ksv = d.v_ksize;
    const int* ht = tables + (ksh ? d.h_table : 0u);
    const int* vt = tables + (ksv ? d.v_table : 0u);

    // 1. bounds and coefficients of the tile's columns and rows
    if (t < UDH_TILE) {
        const int c = min(t, tw - 1);
        hx[t] = ksh ? ht[X0 + c] : left + X0 + c;
        hn[t] = ksh ? ht[S + X0 + c] : 1;
    } else if (t < 2 * UDH_TILE) {
        const int r = min(t - UDH_TILE, th - 1);
        vx[t - UDH_TILE] = ksv ? vt[Y0 + r] : top + Y0 + r;
        vn[t - UDH_TILE] = ksv ? vt[S + Y0 + r] : 1;
    }
    for (int i = t; i < tw * ksh; i += 256) hk[i] = ht[2 * S + X0 * ksh + i];
    for (int i = t; i < th * ksv; i += 256) vk[i] = vt[2 * S + Y0 * ksv + i];
    __syncthreads();
    int x_lo = 0x7fffffff, x_hi = 0, y_lo = 0x7fffffff, y_hi = 0;
    bool good = true;
#pragma unroll
    for (int i = 0; i < UDH_TILE; ++i) {
        const int a = hx[i], an = hn[i], b = vx[i], bn = vn[i];
        good = good && a >= 0 && an >= 1 && an <= max(ksh, 1) && a <= d.W - an && b >= 0 && bn >= 1 && bn <= max(ksv, 1) && b <= d.H - bn;
        x_lo = min(x_lo, a); x_hi = max(x_hi, a + an);
        y_lo = min(y_lo, b); y_hi = max(y_hi, b + bn);
    }
    if (!good || x_hi - x_lo > UDH_SPAN || y_hi - y_lo > UDH_SPAN) return;      // the same for every lane: no barrier is left behind

    // 2. source rows [y_lo, y_hi), columns [x_lo, x_hi) -> mid[row - y_lo][16][3] uint8
    const int row_bytes = (x_hi - x_lo) * 3, nw_max = (row_bytes + 6) >> 2;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(arena);
    unsigned char* mid8 = reinterpret_cast<unsigned char*>(mid);
    for (int base = y_lo; base < y_hi; base += UDH_CHUNK) {
        const int rows = min(UDH_CHUNK, y_hi - base);
        for (int i = t; i < rows * nw_max; i += 256) {
            const int r = i / nw_max, w = i - r * nw_max;
            const size_t g0 = d.offset + ((size_t)(base + r) * d.W + x_lo) * 3;
            if (w < (((int)(g0 & 3) + row_bytes + 3) >> 2)) src[r * UDH_SRC_WORDS + w] = words[(g0 >> 2) + w];
        }
        __syncthreads();
        const int r = t & (UDH_CHUNK - 1);
        if (r < rows) {
            const size_t g0 = d.offset + ((size_t)(base + r) * d.W + x_lo) * 3;
            const unsigned char* s8 = reinterpret_cast<const unsigned char*>(src + r * UDH_SRC_WORDS) + (g0 & 3);
            unsigned char* m8 = mid8 + (base - y_lo + r) * (UDH_MID_WORDS * 4);
            for (int c = t / UDH_CHUNK; c < tw; c += 256 / UDH_CHUNK) {
                const unsigned char* q = s8 + (hx[c] - x_lo) * 3;
                if (ksh) {
                    const int n = hn[c];
                    const int* k = hk + c * ksh;
                    uint32_t a0 = 1u << 21, a1 = a0, a2 = a0;
                    for (int j = 0; j < n; ++j) {
                        const uint32_t kj = (uint32_t)k[j];
                        a0 += q[3 * j] * kj; a1 += q[3 * j + 1] * kj; a2 += q[3 * j + 2] * kj;
                    }
                    m8[c * 3] = (unsigned char)min(max((int)a0 >> 22, 0), 255);
                    m8[c * 3 + 1] = (unsigned char)min(max((int)a1 >> 22, 0), 255);
                    m8[c * 3 + 2] = (unsigned char)min(max((int)a2 >> 22, 0), 255);
                } else {
                    m8[c * 3] = q[0]; m8[c * 3 + 1] = q[1]; m8[c * 3 + 2] = q[2];
                }
            }
        }
        __syncthreads();
    }

    // 3. vertical pass, grey value, store
    const int r = t / UDH_TILE, c = t % UDH_TILE;
    const bool valid = r < th && c < tw;
    const int rr = min(r, th - 1), cc = min(c, tw - 1);
    const unsigned char* q = mid8 + (vx[rr] - y_lo) * (UDH_MID_WORDS * 4) + cc * 3;
    int v[3];
    if (ksv) {
        const int n = vn[rr];
        const int* k = vk + rr * ksv;
        uint32_t a0 = 1u << 21, a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = (uint32_t)k[j];
            a0 += q[j * (UDH_MID_WORDS * 4)] * kj; a1 += q[j * (UDH_MID_WORDS * 4) + 1] * kj; a2 += q[j * (UDH_MID_WORDS * 4) + 2] * kj;
        }
        v[0] = min(max((int)a0 >> 22, 0), 255); v[1] = min(max((int)a1 >> 22, 0), 255); v[2] = min(max((int)a2 >> 22, 0), 255);
    } else {
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    }
    const float g = grey_value(v, mean, stdv);
    const float g1 = __shfl_down(g, 1), g2 = __shfl_down(g, 2), g3 = __shfl_down(g, 3);      // every lane takes part
    float* o = out + ((p * out_h + ty * UDH_TILE + r) * out_w + tx * UDH_TILE + c);
    if (vec && r < th && (c | 3) < tw) {
        if ((c & 3) == 0) *reinterpret_cast<float4*>(o) = make_float4(g, g1, g2, g3);
    } else if (valid) {
        *o = g;
    }
}

// lanes of a row segment: the row's ceil(W / 4) lanes split evenly over the fewest workgroups, rounded up to whole wavefronts
inline int pix_segment_lanes(int W) {
    const int lanes = ceil_div(W, 4);
    const int segl = round_up(ceil_div(lanes, ceil_div(lanes, 256)), 64);
    return segl < 256 ? segl : 256;
}

}  // namespace

extern "C" int masic_pair_prep(const uint8_t* img_hwc, int H, int W, int start_h, int start_w, int ph, int pw, float* pic_chw,
                               int homopic, int patch_x, int patch_y, int homopatch, float* homo_patch, void* stream) {
    MASIC_REQUIRE(img_hwc && (pic_chw || homo_patch), MASIC_ERR_ARG, "pair_prep: null pointer");
    MASIC_REQUIRE(ph > 0 && pw > 0 && start_h >= 0 && start_w >= 0 && start_h + ph <= H && start_w + pw <= W, MASIC_ERR_SHAPE,
                  "pair_prep: crop [%d:%d, %d:%d] of a %d x %d picture", start_h, start_h + ph, start_w, start_w + pw, H, W);
    hipStream_t st = (hipStream_t)stream;
    if (pic_chw) hipLaunchKernelGGL(crop_to_tensor_kernel, dim3(ceil_div(ph * pw, 256)), dim3(256), 0, st, img_hwc, W, start_h, start_w, ph, pw, pic_chw);
    if (homo_patch) {
        MASIC_REQUIRE(homopic > 0 && homopatch > 0 && patch_x >= 0 && patch_y >= 0 && patch_x + homopatch <= homopic && patch_y + homopatch <= homopic,
                      MASIC_ERR_SHAPE, "pair_prep: patch [%d:%d, %d:%d] of the %d x %d resized crop", patch_y, patch_y + homopatch, patch_x,
                      patch_x + homopatch, homopic, homopic);
        const float mean = (0.485f + 0.456f + 0.406f) / 3.0f, stdv = (0.229f + 0.224f + 0.225f) / 3.0f;    // utils.py:26-27
        hipLaunchKernelGGL(homo_patch_kernel, dim3(ceil_div(homopatch * homopatch, 256)), dim3(256), 0, st, img_hwc, W, start_h, start_w, ph, pw,
                           homopic, patch_x, patch_y, homopatch, mean, stdv, homo_patch);
    }
    return masic_launch_status("pair_prep");
}

extern "C" int masic_pairs_prep(const uint8_t* pics_hwc, int P, int H0, int W0, int H, int W, float* planes, int homopic, int patch_x,
                                int patch_y, int homopatch, float* patches, void* stream) {
    MASIC_REQUIRE(pics_hwc && (planes || patches), MASIC_ERR_ARG, "pairs_prep: null pointer");
    MASIC_REQUIRE(P > 0 && P <= 65535 && H0 > 0 && W0 > 0, MASIC_ERR_ARG, "pairs_prep: %d pictures of %d x %d (1 .. 65535 pictures, no empty extent)", P, H0, W0);
    MASIC_REQUIRE(((size_t)pics_hwc & 3) == 0, MASIC_ERR_ARG, "pairs_prep: the picture stack must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (planes) {
        MASIC_REQUIRE(H >= H0 && W >= W0 && H <= 65535 && W <= 65535, MASIC_ERR_ARG,
                      "pairs_prep: planes of %d x %d for pictures of %d x %d (at least the picture, at most 65535)", H, W, H0, W0);
        MASIC_REQUIRE(((size_t)planes & 3) == 0, MASIC_ERR_ARG, "pairs_prep: the planes must be 4-byte aligned");
        const int segl = pix_segment_lanes(W), vec = W % 4 == 0 && ((size_t)planes & 15) == 0;
        hipLaunchKernelGGL(pairs_planes_kernel, dim3(ceil_div(W, 4 * segl), ceil_div(H, 256 / segl), P), dim3(256), 0, st, pics_hwc,
                           (size_t)P * H0 * W0 * 3, H0, W0, H, W, segl, vec, planes);
    }
    if (patches) {
        MASIC_REQUIRE(homopic > 0 && homopatch > 0 && patch_x >= 0 && patch_y >= 0 && patch_x + homopatch <= homopic && patch_y + homopatch <= homopic,
                      MASIC_ERR_ARG, "pairs_prep: patch [%d:%d, %d:%d] of the %d x %d resized picture", patch_y, patch_y + homopatch, patch_x,
                      patch_x + homopatch, homopic, homopic);
        MASIC_REQUIRE(homopic <= 16384, MASIC_ERR_ARG, "pairs_prep: resized picture of %d x %d (at most 16384)", homopic, homopic);
        const float mean = (0.485f + 0.456f + 0.406f) / 3.0f, stdv = (0.229f + 0.224f + 0.225f) / 3.0f;    // utils.py:26-27
        hipLaunchKernelGGL(homo_patches_kernel, dim3(ceil_div(homopatch * homopatch, 256), P), dim3(256), 0, st, pics_hwc, H0, W0, homopic,
                           patch_x, patch_y, homopatch, mean, stdv, patches);
    }
    return masic_launch_status("pairs_prep");
}

extern "C" int masic_planes_to_u8(const float* planes, int P, int H, int W, int H0, int W0, uint8_t* pics_hwc, void* stream) {
    MASIC_REQUIRE(planes && pics_hwc, MASIC_ERR_ARG, "planes_to_u8: null pointer");
    MASIC_REQUIRE(P > 0 && P <= 65535 && H0 > 0 && W0 > 0 && H0 <= H && W0 <= W && H0 <= 65535 && W0 <= 65535, MASIC_ERR_ARG,
                  "planes_to_u8: %d pictures of %d x %d out of planes of %d x %d (1 .. 65535 pictures; no empty extent, at most the planes and 65535)",
                  P, H0, W0, H, W);
    MASIC_REQUIRE(((size_t)pics_hwc & 3) == 0 && ((size_t)planes & 3) == 0, MASIC_ERR_ARG, "planes_to_u8: both buffers must be 4-byte aligned");
    const int segl = pix_segment_lanes(W0), vec = W % 4 == 0 && ((size_t)planes & 15) == 0;
    hipLaunchKernelGGL(planes_to_u8_kernel, dim3(ceil_div(W0, 4 * segl), ceil_div(H0, 256 / segl), P), dim3(256), 0, (hipStream_t)stream, planes,
                       H, W, H0, W0, segl, vec, pics_hwc);
    return masic_launch_status("planes_to_u8");
}

extern "C" int masic_views_prep(const uint8_t* arena, size_t arena_bytes, const masic_view_desc_t* desc_dev, int P, int ph, int pw, float* planes,
                                int homopic, int homopatch, float* patches, void* stream) {
    MASIC_REQUIRE(arena && desc_dev && (planes || patches), MASIC_ERR_ARG, "views_prep: null pointer");
    MASIC_REQUIRE(P > 0 && ph > 0 && pw > 0 && ph <= 65535 && pw <= 65535, MASIC_ERR_ARG,
                  "views_prep: %d views cropped to %d x %d (at least one view, extents 1 .. 65535)", P, ph, pw);
    MASIC_REQUIRE(((size_t)arena & 3) == 0 && (arena_bytes & 3) == 0 && ((size_t)desc_dev & 7) == 0, MASIC_ERR_ARG,
                  "views_prep: the arena must be 4-byte aligned and a multiple of 4 bytes long, the descriptors 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (planes) {
        MASIC_REQUIRE(((size_t)planes & 3) == 0, MASIC_ERR_ARG, "views_prep: the planes must be 4-byte aligned");
        const int segl = pix_segment_lanes(pw), vec = pw % 4 == 0 && ((size_t)planes & 15) == 0;
        const int xsegs = ceil_div(pw, 4 * segl), ysegs = ceil_div(ph, 256 / segl);
        MASIC_REQUIRE((long long)P * xsegs * ysegs <= 0x7fffffffLL, MASIC_ERR_ARG, "views_prep: %d views of %d x %d are more than one grid", P, ph, pw);
        hipLaunchKernelGGL(views_planes_kernel, dim3((unsigned)(P * xsegs * ysegs)), dim3(256), 0, st, arena, arena_bytes, desc_dev, ph, pw, segl,
                           xsegs, ysegs, vec, planes);
    }
    if (patches) {
        MASIC_REQUIRE(homopic > 0 && homopatch > 0 && homopatch <= homopic && homopic <= 16384, MASIC_ERR_ARG,
                      "views_prep: patch of %d x %d of the %d x %d resized crop (patch at most the crop, the crop at most 16384)", homopatch,
                      homopatch, homopic, homopic);
        const int nb = ceil_div(homopatch * homopatch, 256);
        MASIC_REQUIRE((long long)P * nb <= 0x7fffffffLL, MASIC_ERR_ARG, "views_prep: %d patches of %d x %d are more than one grid", P, homopatch, homopatch);
        const float mean = (0.485f + 0.456f + 0.406f) / 3.0f, stdv = (0.229f + 0.224f + 0.225f) / 3.0f;    // utils.py:26-27
        hipLaunchKernelGGL(views_patches_kernel, dim3((unsigned)(P * nb)), dim3(256), 0, st, arena, arena_bytes, desc_dev, ph, pw, homopic,
                           homopatch, nb, mean, stdv, patches);
    }
    return masic_launch_status("views_prep");
}

extern "C" int masic_udh_views_prep(const uint8_t* arena, size_t arena_bytes, const int32_t* tables, size_t table_words,
                                    const masic_udh_view_desc_t* desc_dev, int P, int out_h, int out_w, int pic_size, float* out, void* stream) {
    MASIC_REQUIRE(arena && desc_dev && out, MASIC_ERR_ARG, "udh_views_prep: null pointer");
    MASIC_REQUIRE(tables || table_words == 0, MASIC_ERR_ARG, "udh_views_prep: %zu table words at a null pointer", table_words);
    MASIC_REQUIRE(P > 0 && P <= 65535 && out_h > 0 && out_w > 0 && pic_size <= 16384 && out_h <= pic_size && out_w <= pic_size, MASIC_ERR_ARG,
                  "udh_views_prep: %d views of %d x %d out of a %d x %d picture (1 .. 65535 views, no empty extent, at most the picture, the picture at most 16384)",
                  P, out_h, out_w, pic_size, pic_size);
    MASIC_REQUIRE(((size_t)arena & 3) == 0 && (arena_bytes & 3) == 0 && ((size_t)desc_dev & 7) == 0 && ((size_t)tables & 3) == 0 && ((size_t)out & 3) == 0,
                  MASIC_ERR_ARG, "udh_views_prep: the arena, the tables and the output must be 4-byte aligned, the arena a multiple of 4 bytes long, the descriptors 8-byte aligned");
    const int xt = ceil_div(out_w, UDH_TILE), yt = ceil_div(out_h, UDH_TILE), vec = out_w % 4 == 0 && ((size_t)out & 15) == 0;
    MASIC_REQUIRE((long long)P * xt * yt <= 0x7fffffffLL, MASIC_ERR_ARG, "udh_views_prep: %d views of %d x %d are more than one grid", P, out_h, out_w);
    const float mean = (0.485f + 0.456f + 0.406f) / 3.0f, stdv = (0.229f + 0.224f + 0.225f) / 3.0f;    // dataset.py:10-11, the scalars of utils.py:26-27
    hipLaunchKernelGGL(udh_views_kernel, dim3((unsigned)(P * xt * yt)), dim3(256), 0, (hipStream_t)stream, arena, arena_bytes, tables, table_words,
                       desc_dev, pic_size, out_h, out_w, xt, yt, vec, mean, stdv, out);
    return masic_launch_status("udh_views_prep");
}
