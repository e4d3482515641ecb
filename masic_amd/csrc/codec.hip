// codec.hip -- per-symbol coding tables of the y latents (reference MASIC.py:986-1044, :1262-1296).
//
// For every (latent pixel, non-zero channel) the reference evaluates the K-component Gaussian-mixture PMF over the symbol
// alphabet 0 .. 2*minmax (value - mean shifted by minmax, |.| applied before the two standardized cumulatives, sigma
// lower-bounded, softmax-ed mixture weights), clips it to [2^-16, 1], renormalises to 2^16 and rounds -- once per symbol,
// through .cpu().numpy().  Here one wavefront (64 lanes) builds one table on the device: lanes own contiguous runs of the
// alphabet, wave reductions give the normaliser, the count total and the mode, a wave scan the interval starts.
// Difference to the reference, container-level: the rounded counts are forced to total exactly 2^16 (the surplus goes to
// the mode) because the rANS coder needs a power-of-two total, where `range_coder` takes any total.
// The same kernel serves both directions: the decoder fetches whole tables (u16 starts) for the current wavefront of
// pixels, the encoder only the (start, freq) of the symbols it holds.  Encoder and decoder run the SAME instruction
// sequence on the same parameters, so their tables agree bit for bit.
#include "common.h"

namespace {

constexpr int CDF_MAX_L = 1024;

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wavefront per (pixel i, stream s) row, block r = i * nstreams + s; the pixel is entry img * npix + i of the list, q = img * HW + p.
// streams: the launch's masic_code_stream_t table, one entry per (pair, coded channel) -- pairs differ in their channel sets and
// alphabets, and every row uses its own pair's.
template <int K>
__global__ __launch_bounds__(64) void gmm_cdf_kernel(const float* __restrict__ sigma, const float* __restrict__ mu,
                                                     const float* __restrict__ logits, int M, int HW,
                                                     const int* __restrict__ pix, int list_stride,
                                                     const masic_code_stream_t* __restrict__ streams, int nstreams,
                                                     float scale_bound, const float* __restrict__ y_hat,
                                                     unsigned short* __restrict__ starts, int* __restrict__ start_freq,
                                                     int* __restrict__ err, const int* __restrict__ step, int npix) {
    __shared__ float pm[CDF_MAX_L];
    __shared__ unsigned fr[CDF_MAX_L];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int i = r / nstreams;
    const masic_code_stream_t sd = streams[r - i * nstreams];
    if (step != nullptr) pix += (size_t)(*step) * list_stride;   // the wavefront list of coding step *step (device-side loop of the decoder)
    const int q = pix[(size_t)sd.img * npix + i], m = sd.chan, minmax = sd.minmax, b = sd.img;
    if (q < 0) return;                                     // padding entry of a fixed-size wavefront list (graph replay)
    const int L = 2 * minmax + 1;
    if (minmax < 1 || L > CDF_MAX_L) {                     // a descriptor the tables cannot hold
        if (lane == 0) atomicOr(err + b, 1);
        return;
    }
    const int p = q - b * HW;
    const int row = sd.row0 + i * sd.rstride;
    const size_t base = ((size_t)b * K * M + m) * HW + p, ks = (size_t)M * HW;
    float wk[K], sk[K], mk[K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        wk[k] = logits[base + k * ks];
        mx = fmaxf(mx, wk[k]);
        sk[k] = fmaxf(sigma[base + k * ks], scale_bound);
        mk[k] = mu[base + k * ks] + (float)minmax;
    }
    float ws = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) { wk[k] = expf(wk[k] - mx); ws += wk[k]; }
#pragma unroll
    for (int k = 0; k < K; ++k) wk[k] = wk[k] / ws;

    const int chunk = (L + 63) / 64, s0 = lane * chunk, s1 = min(L, s0 + chunk);
    const float cst = -0.70710678118654752440f;
    float part = 0.0f;
    for (int s = s0; s < s1; ++s) {
        float l = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float v = fabsf((float)s - mk[k]);
            const float up = 0.5f * erfcf(cst * ((0.5f - v) / sk[k]));
            const float lo = 0.5f * erfcf(cst * ((-0.5f - v) / sk[k]));
            const float term = __fmul_rn(up - lo, wk[k]);
            l = (k == 0) ? term : __fadd_rn(l, term);
        }
        l = fminf(fmaxf(l, 1.0f / 65536.0f), 1.0f);
        pm[s] = l;
        part += l;
    }
    const float Ssum = wave_sum(part);
    unsigned tot = 0, best = 0;
    int besti = 0x7fffffff;
    for (int s = s0; s < s1; ++s) {
        const float qq = rintf(pm[s] / Ssum * 65536.0f);
        const unsigned f = qq < 1.0f ? 1u : (unsigned)qq;
        fr[s] = f;
        tot += f;
        if (f > best) { best = f; besti = s; }
    }
    const unsigned T = wave_sum(tot);
    // mode: largest count, first index
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    const int fixed = (int)best + (65536 - (int)T);
    if (fixed < 1) {
        if (lane == 0) atomicOr(err + b, 1);
        return;
    }
    __syncthreads();
    if (lane == 0) fr[besti] = (unsigned)fixed;
    __syncthreads();
    unsigned run = 0;
    for (int s = s0; s < s1; ++s) run += fr[s];
    unsigned incl = run;                                   // inclusive scan over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    unsigned st = incl - run;
    int sym = -1;
    if (y_hat != nullptr) {
        sym = (int)y_hat[((size_t)b * M + m) * HW + p] + minmax;
        if ((sym < 0 || sym >= L) && lane == 0) atomicOr(err + b, 2);
    }
    unsigned short* srow = starts != nullptr ? starts + sd.soff + (size_t)i * sd.rstride * L : nullptr;
    for (int s = s0; s < s1; ++s) {
        if (srow != nullptr) srow[s] = (unsigned short)st;
        if (s == sym) { start_freq[2 * (size_t)row] = (int)st; start_freq[2 * (size_t)row + 1] = (int)fr[s]; }
        st += fr[s];
    }
}

int cdf_launch(const float* sigma, const float* mu, const float* logits, int M, int K, int HW, const int32_t* pix, const int32_t* step, int list_stride,
               int npix, const masic_code_stream_t* streams, int nstreams, float scale_bound, const float* y_hat, uint16_t* starts, int32_t* start_freq,
               int32_t* err_flag, void* stream) {
    const dim3 grid((unsigned)((size_t)npix * nstreams)), blk(64);
    hipStream_t st = (hipStream_t)stream;
#define CDF_CASE(KK)                                                                                                        \
    case KK:                                                                                                                \
        hipLaunchKernelGGL(gmm_cdf_kernel<KK>, grid, blk, 0, st, sigma, mu, logits, M, HW, (const int*)pix, list_stride, streams, nstreams, \
                           scale_bound, y_hat, (unsigned short*)starts, (int*)start_freq, (int*)err_flag, (const int*)step, npix); \
        break;
    switch (K) { CDF_CASE(1) CDF_CASE(2) CDF_CASE(3) CDF_CASE(4) CDF_CASE(5) CDF_CASE(6) CDF_CASE(7) CDF_CASE(8) }
#undef CDF_CASE
    return masic_launch_status("gmm_cdf_rows");
}

// ---- the decoder's symbol search on the device: one wavefront (64 lanes) per channel stream.
// The rANS state of a stream is one serial chain, but the streams are independent: with one stream per latent channel
// (masic_rans_encode_channels) the <= h symbols a channel has on the current coding wavefront are decoded by one wave while the other
// channels' waves do theirs.  The table rows do not depend on the coder state, so a wave first loads ALL its rows (lane l keeps entry l
// of every row; alphabets up to 64 entries in one register per row, larger ones in strides of 64), and the serial part is registers
// only: cum = x & 0xffff, one ballot finds the interval, x = freq * (x >> 16) + cum - start, and a 32-bit word is pulled in when x
// drops below 2^31 (the next words of the stream are prefetched two ahead).  The decoded values go straight into the latent
// (y_hat[img][chan][pix] = s - minmax), so the next coding step's context convolution sees them: nothing crosses PCIe inside the loop.
// Streams of a batch may differ in alphabet: each wave takes the register or the general form for its own stream.
// *step is incremented by the last wave of the launch to finish (an arrival counter over all streams): every wave reads it at its
// start only, and the next reader is the next launch.
constexpr int DEC_MAX_ROWS = 64;      // rows (pixels) per coding step a wave keeps in registers: a wavefront of the 5x5 mask has <= h of them
__global__ __launch_bounds__(64) void rans_decode_step_kernel(const unsigned* __restrict__ words,
                                                              const masic_code_stream_t* __restrict__ streams, int nstreams,
                                                              unsigned long long* __restrict__ state, unsigned* __restrict__ pos,
                                                              const unsigned short* __restrict__ starts, const int* __restrict__ pix_all,
                                                              int list_stride, int* __restrict__ step, int npix, int M,
                                                              float* __restrict__ y_hat, int HW,
                                                              int* __restrict__ err, int* __restrict__ done, unsigned short* __restrict__ y16) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int st = *step;
    const masic_code_stream_t sd = streams[c];
    const int b = sd.img, m = sd.chan, minmax = sd.minmax, L = 2 * minmax + 1;
    const int* pix = pix_all + (size_t)st * list_stride + (size_t)b * npix;
    const size_t ybase = (size_t)b * M * HW, y16base = (size_t)b * ((M + 15) / 16 * 16) * HW;
    const unsigned short* srows = starts + sd.soff;
    const size_t rs = (size_t)sd.rstride * L;              // u16 entries between the stream's consecutive rows
    const int nL = (L + 63) >> 6;                          // table entries per lane
    if (minmax < 1 || L > CDF_MAX_L) {
        if (lane == 0) atomicOr(err + b, 1);
    } else if (nL == 1 && npix <= DEC_MAX_ROWS) {
        unsigned ent[DEC_MAX_ROWS];                        // entry `lane` of row i (0x10000 past the end: never <= cum)
        int pr[DEC_MAX_ROWS];
#pragma unroll
        for (int i = 0; i < DEC_MAX_ROWS; ++i) {
            pr[i] = i < npix ? pix[i] : -1;
            ent[i] = (pr[i] >= 0 && lane < L) ? (unsigned)srows[(size_t)i * rs + lane] : 0x10000u;
        }
        unsigned long long x = state[c];
        unsigned pp = pos[c];
        const unsigned* w = words + sd.word_off;
        const unsigned wn = sd.word_cnt;
        unsigned w0 = pp < wn ? w[pp] : 0u, w1 = pp + 1 < wn ? w[pp + 1] : 0u;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < DEC_MAX_ROWS; ++i) {
            if (pr[i] < 0) continue;
            const int p = pr[i] - b * HW;
            const unsigned cum = (unsigned)(x & 0xffffu);
            const unsigned long long le = __ballot(ent[i] <= cum);          // entries 0 .. s are <= cum (strictly increasing starts)
            const int s = 63 - __builtin_clzll(le | 1ull);
            const unsigned sst = __shfl(ent[i], s, 64);
            const unsigned nxt = s + 1 < L ? __shfl(ent[i], s + 1, 64) : 0x10000u;
            x = (unsigned long long)(nxt - sst) * (x >> 16) + cum - sst;
            if (x < (1ull << 31)) {
                bad = bad || pp >= wn;
                x = (x << 32) | w0;
                ++pp;
                w0 = w1;
                w1 = pp + 1 < wn ? w[pp + 1] : 0u;
            }
            if (lane == 0) {
                y_hat[ybase + (size_t)m * HW + p] = (float)(s - minmax);
                if (y16 != nullptr) { const __bf16 bv = (__bf16)(float)(s - minmax); y16[y16base + ((size_t)(m >> 4) * HW + p) * 16 + (m & 15)] = __builtin_bit_cast(unsigned short, bv); }
            }
        }
        if (lane == 0) {
            state[c] = x;
            pos[c] = pp;
            if (bad) atomicOr(err + b, 4);
        }
    } else {
        // general form (alphabets above 64 entries or very tall latents): rows re-read per symbol, entries in strides of 64
        unsigned long long x = state[c];
        unsigned pp = pos[c];
        const unsigned* w = words + sd.word_off;
        const unsigned wn = sd.word_cnt;
        bool bad = false;
        for (int i = 0; i < npix; ++i) {
            const int q = pix[i];
            if (q < 0) continue;
            const int p = q - b * HW;
            const unsigned short* row = srows + (size_t)i * rs;
            const unsigned cum = (unsigned)(x & 0xffffu);
            int s = -1;
            for (int k = 0; k < nL; ++k) {
                const int e = k * 64 + lane;
                const unsigned v = e < L ? (unsigned)row[e] : 0x10000u;
                const unsigned long long le = __ballot(v <= cum);
                if (le != 0) s = k * 64 + 63 - __builtin_clzll(le);
            }
            s = s < 0 ? 0 : s;
            const unsigned sst = row[s], nxt = s + 1 < L ? (unsigned)row[s + 1] : 0x10000u;
            x = (unsigned long long)(nxt - sst) * (x >> 16) + cum - sst;
            if (x < (1ull << 31)) {
                bad = bad || pp >= wn;
                x = (x << 32) | (pp < wn ? w[pp] : 0u);
                ++pp;
            }
            if (lane == 0) {
                y_hat[ybase + (size_t)m * HW + p] = (float)(s - minmax);
                if (y16 != nullptr) { const __bf16 bv = (__bf16)(float)(s - minmax); y16[y16base + ((size_t)(m >> 4) * HW + p) * 16 + (m & 15)] = __builtin_bit_cast(unsigned short, bv); }
            }
        }
        if (lane == 0) {
            state[c] = x;
            pos[c] = pp;
            if (bad) atomicOr(err + b, 4);
        }
    }
    // the last wave to finish moves the loop on: the next launch (the next step's table kernel) reads the new *step
    __threadfence();
    if (lane == 0) {
        const int prev = atomicAdd(done, 1);
        if (prev == nstreams - 1) {
            *done = 0;
            *step = st + 1;
        }
    }
}

// ---- after the last coding step: did every stream end where its encoder began?  Every encoder of rans.hip starts from x = 2^31 and the
// decoder retraces its states backwards, so a stream read with the encoder's tables leaves the coder at exactly 2^31 with exactly its
// word_cnt words consumed; anything else (a flipped bit, another file's header, other weights or operand mode: other tables) meets both
// only by a ~2^-31 coincidence per stream.  One thread per stream; err bit 3.
__global__ __launch_bounds__(64) void rans_decode_finish_kernel(const masic_code_stream_t* __restrict__ streams, int nstreams,
                                                                const unsigned long long* __restrict__ state,
                                                                const unsigned* __restrict__ pos, int* __restrict__ err) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nstreams) return;
    if (pos[c] != streams[c].word_cnt || state[c] != (1ull << 31)) atomicOr(err + streams[c].img, 8);
}

// ---- the encoder's coder on the device: one LANE per channel stream (masic_rans_encode_channels of rans.hip, all streams of a call at once).
// A stream is one serial chain over its npix symbols, walked last pixel first as every rANS encoder does; the 2 M B chains of a call
// are independent, so lane l of workgroup g (one wavefront) runs stream 64 g + l.  Consecutive streams of a pair are consecutive
// channels, and the pair's rows are pixel-major (row0 + i * rstride), so the wave's loads of one pixel are one contiguous segment of
// 8-byte rows (512 bytes for a full wave of one pair).  The rows do not depend on the coder state: a tile of ENC_TILE pixels is loaded
// into registers while the chain works on the tile before it, which it reads from LDS ([pixel][lane], every lane only its own column:
// no barrier), and is written there once the chain is through.  The symbol loop is a real loop (not unrolled), so the loads are issued in
// the block before it and waited for in the block after it -- a prefetch carried in registers over the loop's back edge is waited for at
// once (README, round 2 third pass).
// Per symbol, put() of rans.hip: a word leaves when x >= 2^47 * freq, then x = ((x / freq) << 16) + x % freq + start.  x < 2^63 and
// freq <= 2^16; after the renormalisation the quotient is below 2^47, so the product of x and 1 / freq in double precision (three
// roundings of 2^-53 relative each) is within 2^47 * 3 * 2^-53 < 0.05 of it, its integer part within one, and the remainder says which.
// Words go backwards into the stream's own region of npix + 2 words of the workspace (at most one per symbol, and the two of the final
// state), and the region's tail [npix + 2 - length / 4, npix + 2) is the stream.  A row no coder can take (start < 0, freq < 1,
// start + freq > 2^16: the argument error of the host coder) is skipped and sets err bit 4 of its pair.
constexpr int ENC_TILE = 32;          // pixels per staged tile: 16 KB of LDS, 64 registers in flight

__host__ __device__ __forceinline__ void rans_divmod(unsigned long long x, unsigned freq, double rcp, unsigned long long& q, unsigned& r) {
    unsigned long long qq = (unsigned long long)((double)x * rcp);
    long long rr = (long long)(x - qq * freq);                 // exact in 64 bits: |x - qq * freq| <= 2 * freq
    if (rr < 0) { --qq; rr += freq; }
    if (rr >= (long long)freq) { ++qq; rr -= freq; }
    q = qq;
    r = (unsigned)rr;
}

__global__ __launch_bounds__(64) void rans_encode_channels_kernel(const int2* __restrict__ start_freq,
                                                                  const masic_code_stream_t* __restrict__ streams, int nstreams, int npix,
                                                                  unsigned* __restrict__ workspace, unsigned* __restrict__ lengths,
                                                                  int* __restrict__ err) {
    __shared__ int2 tile[ENC_TILE][64];
    const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
    if (s >= nstreams) return;                             // lanes share nothing: no barrier follows
    const masic_code_stream_t sd = streams[s];
    const int2* rows = start_freq + sd.row0;
    const size_t rs = (size_t)sd.rstride;
    const int cap = npix + 2;
    unsigned* out = workspace + (size_t)s * cap;
    int p = cap;                                           // next word goes to out[p - 1]; p >= 2 after npix symbols
    unsigned long long x = 1ull << 31;
    bool bad = false;
    const int ntiles = (npix + ENC_TILE - 1) / ENC_TILE;
    int2 nxt[ENC_TILE];
    if (ntiles > 0) {                                      // the last tile may be short: its tail repeats the last pixel and is never coded
        const int i0 = (ntiles - 1) * ENC_TILE;
#pragma unroll
        for (int k = 0; k < ENC_TILE; ++k) nxt[k] = rows[(size_t)min(i0 + k, npix - 1) * rs];
#pragma unroll
        for (int k = 0; k < ENC_TILE; ++k) tile[k][lane] = nxt[k];
    }
    for (int t = ntiles - 1; t >= 0; --t) {
        const int i0 = t * ENC_TILE, cnt = min(ENC_TILE, npix - i0);
        if (t > 0) {                                       // tile t - 1 is whole
#pragma unroll
            for (int k = 0; k < ENC_TILE; ++k) nxt[k] = rows[(size_t)(i0 - ENC_TILE + k) * rs];
        }
#pragma nounroll
        for (int k = cnt - 1; k >= 0; --k) {
            const int2 sf = tile[k][lane];
            const int st = sf.x, fr = sf.y;
            if (st < 0 || fr < 1 || fr > 65536 || st > 65536 - fr) { bad = true; continue; }
            const unsigned freq = (unsigned)fr;
            const double rcp = 1.0 / (double)freq;
            if (x >= ((unsigned long long)freq << 47)) {
                out[--p] = (unsigned)x;
                x >>= 32;
            }
            unsigned long long q;
            unsigned r;
            rans_divmod(x, freq, rcp, q, r);
            x = (q << 16) + r + (unsigned)st;
        }
        if (t > 0) {
#pragma unroll
            for (int k = 0; k < ENC_TILE; ++k) tile[k][lane] = nxt[k];
        }
    }
    p -= 2;
    out[p] = (unsigned)x;
    out[p + 1] = (unsigned)(x >> 32);
    lengths[s] = (unsigned)(cap - p) * 4u;
    if (bad) atomicOr(err + sd.img, 16);
}

// ---- framing on the device: workspace + lengths -> per pair the bytes codec.encode_channels returns (u32 n, n x u32 lengths, the n
// streams back to back), the B blobs one after another in `blob`, pair b at byte offsets[b] (offsets[B] = all bytes).  first[b] is the
// index of pair b's first stream (first[B] = nstreams), so a pair without streams still gets its four bytes.  Everything is a whole
// number of 32-bit words.  With S(k) = the words of streams 0 .. k-1, pair b starts at word b + first[b] + S(first[b]) (b headers of
// one word, first[b] length fields) and stream s of pair b at word b + 1 + first[b + 1] + S(s).  Workgroups 0 .. nstreams-1 copy one
// stream each, workgroups nstreams .. nstreams + B write one pair's header and offset each (the last one only offsets[B]); each sums the
// lengths it needs itself (a few thousand integers from L2): no order between workgroups, the same bytes every run.
constexpr int PACK_THREADS = 256;
__global__ __launch_bounds__(PACK_THREADS) void rans_pack_pairs_kernel(const unsigned* __restrict__ workspace, const unsigned* __restrict__ lengths,
                                                                       const masic_code_stream_t* __restrict__ streams, int nstreams, int npix,
                                                                       const int* __restrict__ first, int npairs,
                                                                       unsigned* __restrict__ blob, unsigned* __restrict__ offsets) {
    __shared__ unsigned part[PACK_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const bool copy = g < nstreams;
    const int b = copy ? streams[g].img : g - nstreams;
    const int upto = copy ? g : first[b];                  // S(upto)
    unsigned sum = 0;
    for (int k = tid; k < upto; k += PACK_THREADS) sum += lengths[k] >> 2;
    sum = wave_sum(sum);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    unsigned S = 0;
#pragma unroll
    for (int k = 0; k < PACK_THREADS / 64; ++k) S += part[k];
    if (copy) {
        const unsigned n = lengths[g] >> 2;
        const unsigned* src = workspace + (size_t)g * (npix + 2) + (npix + 2 - n);
        unsigned* dst = blob + (size_t)b + 1 + first[b + 1] + S;
        for (unsigned k = tid; k < n; k += PACK_THREADS) dst[k] = src[k];
    } else {
        const size_t w0 = (size_t)b + first[b] + S;
        if (tid == 0) offsets[b] = (unsigned)(w0 * 4);
        if (b < npairs) {
            const int f0 = first[b], n = first[b + 1] - f0;
            if (tid == 0) blob[w0] = (unsigned)n;
            for (int k = tid; k < n; k += PACK_THREADS) blob[w0 + 1 + k] = lengths[f0 + k];
        }
    }
}

}  // namespace

// The encoder's coder and framing on the device (include/masic_hip.h).
extern "C" size_t masic_rans_encode_batch_workspace_bytes(int nstreams, int npix) {
    if (nstreams < 0 || npix < 0) return 0;
    return (size_t)nstreams * ((size_t)npix + 2) * sizeof(uint32_t);
}

extern "C" size_t masic_rans_pack_pairs_bound(int nstreams, int npix, int npairs) {
    if (nstreams < 0 || npix < 0 || npairs < 0) return 0;
    return ((size_t)npairs + (size_t)nstreams + (size_t)nstreams * ((size_t)npix + 2)) * sizeof(uint32_t);
}

extern "C" int masic_rans_encode_channels_batch(const int32_t* start_freq, const masic_code_stream_t* streams, int nstreams, int npix,
                                                void* workspace, uint32_t* lengths, int32_t* err_flags, void* stream) {
    MASIC_REQUIRE(nstreams >= 0 && npix >= 0, MASIC_ERR_SHAPE, "rans_encode_channels_batch: nstreams=%d npix=%d", nstreams, npix);
    if (nstreams == 0) return MASIC_OK;
    MASIC_REQUIRE(start_freq && streams && workspace && lengths && err_flags, MASIC_ERR_ARG, "rans_encode_channels_batch: null pointer");
    hipLaunchKernelGGL(rans_encode_channels_kernel, dim3((nstreams + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const int2*)start_freq, streams,
                       nstreams, npix, (unsigned*)workspace, (unsigned*)lengths, (int*)err_flags);
    return masic_launch_status("rans_encode_channels_batch");
}

extern "C" int masic_rans_pack_pairs_batch(const void* workspace, const uint32_t* lengths, const masic_code_stream_t* streams, int nstreams, int npix,
                                           const int32_t* first, int npairs, void* blob, uint32_t* offsets, void* stream) {
    MASIC_REQUIRE(nstreams >= 0 && npix >= 0 && npairs >= 1, MASIC_ERR_SHAPE, "rans_pack_pairs_batch: nstreams=%d npix=%d npairs=%d", nstreams, npix, npairs);
    MASIC_REQUIRE(first && blob && offsets && (nstreams == 0 || (workspace && lengths && streams)), MASIC_ERR_ARG, "rans_pack_pairs_batch: null pointer");
    MASIC_REQUIRE(masic_rans_pack_pairs_bound(nstreams, npix, npairs) < ((size_t)1 << 32), MASIC_ERR_UNSUPPORTED,
                  "rans_pack_pairs_batch: the blobs of %d streams of %d symbols may pass 4 GiB (32-bit offsets)", nstreams, npix);
    hipLaunchKernelGGL(rans_pack_pairs_kernel, dim3(nstreams + npairs + 1), dim3(PACK_THREADS), 0, (hipStream_t)stream, (const unsigned*)workspace,
                       lengths, streams, nstreams, npix, (const int*)first, npairs, (unsigned*)blob, (unsigned*)offsets);
    return masic_launch_status("rans_pack_pairs_batch");
}

// Device side of a coding step over B pairs (include/masic_hip.h): masic_gmm_cdf_rows_batch builds the tables of step *step (or, without
// a step, of the whole list: the encoder's one pass), masic_rans_decode_step_batch decodes the step's symbols into the latent and
// increments *step.  streams: the device table of masic_code_stream_t (one pair is a table of that pair's streams); words: all channel
// streams back to back as little-endian 32-bit words; state[s] / pos[s]: coder state (initialised from the stream's first two words) and
// next word index (2) -- caller-initialised, kept between steps; pix_all: [nsteps][list_stride] pixel lists (-1 = padding); done:
// caller-zeroed int; err_flags: one int per image, bit 2 = a stream ended early, bit 3 (masic_rans_decode_finish_batch, once after the last
// step) = a stream did not end with all its words consumed and the coder in the encoders' initial state.  y_f16k (nullable): the latent also as F16K bf16
// [B][ceil16(M) / 16][HW][16] (exact for |value| <= 256) -- the input layout of the context model's kernels.
extern "C" int masic_gmm_cdf_rows_batch(const float* sigma, const float* mu, const float* logits, int M, int K, int HW,
                                        const int32_t* pix, const int32_t* step, int list_stride, int npix,
                                        const masic_code_stream_t* streams, int nstreams, float scale_bound,
                                        const float* y_hat, uint16_t* starts, int32_t* start_freq, int32_t* err_flags, void* stream) {
    MASIC_REQUIRE(sigma && mu && logits && pix && streams && err_flags, MASIC_ERR_ARG, "gmm_cdf_rows_batch: null pointer");
    MASIC_REQUIRE((y_hat != nullptr) == (start_freq != nullptr), MASIC_ERR_ARG, "gmm_cdf_rows_batch: y_hat and start_freq go together");
    MASIC_REQUIRE(starts || start_freq, MASIC_ERR_ARG, "gmm_cdf_rows_batch: no output requested");
    MASIC_REQUIRE(K >= 1 && K <= 8, MASIC_ERR_UNSUPPORTED, "gmm_cdf_rows_batch: K=%d", K);
    MASIC_REQUIRE(npix >= 1 && nstreams >= 0 && list_stride >= npix, MASIC_ERR_SHAPE, "gmm_cdf_rows_batch: bad shape");
    if (nstreams == 0) return MASIC_OK;
    return cdf_launch(sigma, mu, logits, M, K, HW, pix, step, list_stride, npix, streams, nstreams, scale_bound, y_hat, starts, start_freq, err_flags, stream);
}

extern "C" int masic_rans_decode_step_batch(const uint32_t* words, const masic_code_stream_t* streams, int nstreams, uint64_t* state, uint32_t* pos,
                                            const uint16_t* starts, const int32_t* pix_all, int list_stride, int32_t* step, int npix, int M,
                                            float* y_hat, void* y_f16k, int HW, int32_t* err_flags, int32_t* done, void* stream) {
    MASIC_REQUIRE(words && streams && state && pos && starts && pix_all && step && y_hat && err_flags && done, MASIC_ERR_ARG,
                  "rans_decode_step_batch: null pointer");
    MASIC_REQUIRE(npix >= 1 && nstreams >= 1 && M >= 1 && list_stride >= npix, MASIC_ERR_SHAPE, "rans_decode_step_batch: bad shape");
    hipLaunchKernelGGL(rans_decode_step_kernel, dim3(nstreams), dim3(64), 0, (hipStream_t)stream, (const unsigned*)words, streams, nstreams,
                       (unsigned long long*)state, (unsigned*)pos, (const unsigned short*)starts, (const int*)pix_all, list_stride, (int*)step, npix, M,
                       y_hat, HW, (int*)err_flags, (int*)done, (unsigned short*)y_f16k);
    return masic_launch_status("rans_decode_step_batch");
}

extern "C" int masic_rans_decode_finish_batch(const masic_code_stream_t* streams, int nstreams, const uint64_t* state, const uint32_t* pos,
                                              int32_t* err_flags, void* stream) {
    MASIC_REQUIRE(streams && state && pos && err_flags, MASIC_ERR_ARG, "rans_decode_finish_batch: null pointer");
    MASIC_REQUIRE(nstreams >= 0, MASIC_ERR_SHAPE, "rans_decode_finish_batch: nstreams=%d", nstreams);
    if (nstreams == 0) return MASIC_OK;
    hipLaunchKernelGGL(rans_decode_finish_kernel, dim3((nstreams + 63) / 64), dim3(64), 0, (hipStream_t)stream, streams, nstreams,
                       (const unsigned long long*)state, (const unsigned*)pos, (int*)err_flags);
    return masic_launch_status("rans_decode_finish_batch");
}
