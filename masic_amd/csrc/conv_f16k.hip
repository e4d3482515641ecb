#ifdef CONV_F16K_BODY
// ---- The body of the two conv_f16k kernels.  This file includes ITSELF with CONV_F16K_BODY defined, once inside each kernel template
// (see conv_f16k / conv_f16k_multi below): conv_f16k<KS, T, D, PSP, L, GDN, NM, NP, F8> with MULTI = false (one output, as F16kArgs
// describes it) and conv_f16k_multi<NM> with MULTI = true (the latent layer, its result stored in up to four layouts, F16kMulti mo).
// A textual include and not a shared __device__ function or a further template parameter: the symbols of the conv_f16k instantiations
// (which profiles, the benchmark and masic_conv_f16k_kernel_name spell out) and their code stay exactly what they were -- as a
// force-inlined function taking the kernel arguments by reference the same body compiled to different register figures for most of
// them (the dominant <1, 5, 2, 6, 1, true, 4, 1, false>: 207 -> 209 VGPRs).  In one file, so that whatever hashes or greps the kernel
// sources sees the K loop and the epilogue where they always were.
// In scope: the template parameters as compile-time constants, `const F16kArgs a`, `const F16kMulti mo`.
    static_assert(!MULTI || (!GDN && !F8 && NP == 1), "the multi-output epilogue exists for the plain bf16 form with 256-pixel tiles");
    static_assert(!GDN || NM == 4, "the fused GDN needs all 128 channels");
    static_assert(!F8 || (NM == 4 && NP == 1 && (T * KS) % 2 == 0 && T <= 4), "fp8 operands: 128-channel blocks, 256-pixel tiles, slab pairs");
    static_assert(NM + NP == 2 || NM + NP == 3 || NM + NP == 4 || NM + NP == 5 || NM + NP == 6, "fragment-wait helpers exist for 2, 4, 5 and 6 fragments per k-step");
    constexpr int WI = T * KS;                   // weight DMA wave-instructions per weight wave per step (4 waves x 1 KiB x WI = slab group)
    constexpr int NWS = D + 1;                   // weight ring slots
    constexpr int WST = T * KS * 4096;           // bytes per step of weights
    constexpr int NPI = PSP * 2;                 // patch DMA wave-instructions per patch wave per chunk (incl. dummies)
    constexpr int NB = L + 1;                    // patch buffers
    constexpr int PATCH0 = NWS * WST;            // LDS byte offset of the patch buffers
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int dummy_off = PATCH0 + NB * a.PB;    // 1 KiB sink for unused DMA slots, then the tap table
    const int table_off = dummy_off + 1024;
    const unsigned ldsb = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;   // LDS byte address of lds[0]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    // DMA roles: waves 0-3 stream the weight slabs, waves 4-7 the activation patch.  vmcnt is per wave and retires in
    // order, so the roles are what keeps a long-latency patch load (HBM) from gating the wait for the next weight slab (L2).
    const bool wrole = wave < 4;
    const int wq = wave & 3;

    // block -> (tile, phase): the phases of a tile sit 8 block ids apart, i.e. on the same XCD and next to each other in
    // time, so their interleaved output pixels meet in one L2
    // With a multiple of 8 images, image b = 8 slot + k is walked tile by tile on XCD k (workgroup ids go round-robin over the 8
    // XCDs and gridDim.x is a multiple of 8): the 5x5 halos that neighbouring tiles share are then re-read from that XCD's L2
    // instead of HBM (measured on the 128 -> 128 stride-2 layers: 142 -> 129 MB per launch against 105 algorithmic).
    int phase, tile, b;
    if (a.xcd_images) {
        const int idx = (blockIdx.x >> 3) + (gridDim.x >> 3) * blockIdx.z;
        const int slot = idx / (int)gridDim.x, rest = idx - slot * (int)gridDim.x;
        b = slot * 8 + (blockIdx.x & 7);
        phase = rest % a.nphase;
        tile = rest / a.nphase;
    } else {
        const int xcd = blockIdx.x & 7, rest = blockIdx.x >> 3;
        phase = rest % a.nphase;
        tile = (rest / a.nphase) * 8 + xcd;
        b = blockIdx.z;
    }
    if (tile >= a.ntiles) return;
    if (F16K_ABLATE == 6) return;                 // launch cost only
    // diagnostics: core-clock and 100 MHz constant-clock stamps of wave 0 of the first and of the last workgroup
    unsigned long long* const stamp = (a.stamps != nullptr && tid == 0 && blockIdx.y == 0 && blockIdx.z == 0 && (blockIdx.x == 0 || blockIdx.x + 1 == gridDim.x))
                                          ? a.stamps + (blockIdx.x == 0 ? 0 : 8) : nullptr;
    if (stamp) { stamp[0] = __builtin_amdgcn_s_memtime(); stamp[1] = __builtin_amdgcn_s_memrealtime(); }
    const int tw_i = tile % a.tiles_w, th_i = tile / a.tiles_w;
    const int r0 = th_i * a.TH, c0 = tw_i * a.TW;
    const int nchunks = a.Cin16 / KS;
    const int gpk = a.NPIXp >> 5;                             // DMA wave-instructions per 16-channel plane of the patch (2*NPIXp/64)
    const int plane_bytes = a.Hi * a.Wi * 32;                 // bytes per 16-channel plane of the input
    int SPC;                                                  // steps per chunk
    int bl[NP];                                               // lane part of the B-fragment addresses
    int goff[NPI];                                            // patch waves: byte offset of this lane's record in a chunk

    // Buffer resources: out-of-range offsets read as zero, so padding pixels (voffset = huge), chunks past the last one and
    // slab groups past the end of the stream need no special case, and the per-chunk / per-step offset rides in an SGPR.
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + ((size_t)b * a.in_c16tot + a.in_c16off) * (size_t)(a.Hi * a.Wi * 16)), 0, a.Cin16 * plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const unsigned char*)a.w + a.phase_off[phase] + (size_t)(blockIdx.y / a.msplit) * a.stream_bytes[phase]), 0, (int)a.stream_bytes[phase], 0x00020000);
    const int msub = (int)(blockIdx.y % a.msplit) * NM;       // first 32-channel tile of this workgroup inside the 128-channel slab
    if ((int)(blockIdx.y / a.msplit) * 128 + msub * 32 >= a.Cout) return;      // a sub-block past the last output channel (Cout = 192: second co-block)

    {   // ---- geometry-dependent setup (kept in a scope: nothing of the phase geometry stays live in the K loop)
        const ConvGeom g = make_geom(a.q, phase);
        SPC = (g.ntaps + T - 1) / T;
        const int ih0 = r0 * g.is + g.dh_min, iw0 = c0 * g.is + g.dw_min;
        const int ninstr = KS * gpk;
        // LDS images (16-byte records, the two k-halves of a 32-byte record in separate planes so that the 16 lanes of a
        // ds_read_b128 group read 256 contiguous bytes):
        //   weight slab (tap, ks): [hh][co 128]   (the packed stream already has this order: a linear copy)
        //   patch plane (ks):      [hh][pixel'] with pixel' = row * PW + col for stride-1 walks and, for strided convs,
        //                          columns de-interleaved by parity, pixel' = ((col & 1) * PH + row) * PWh + (col >> 1),
        //                          so that the stride-2 walk of a tap reads consecutive records too.
#pragma unroll
        for (int k = 0; k < NPI; ++k) {
            const int I = k * 4 + wq;
            const int ks = (int)__umulhi((unsigned)I, a.mg_gpk), grp = I - ks * gpk;
            const int q = grp * 64 + lane;
            const int hh = q >= a.NPIXp ? 1 : 0, pp = q - hh * a.NPIXp;
            int pr, pc;
            bool ok = I < ninstr;
            if (g.is == 2) {
                const int half = a.PH * a.PWh;
                const int par = pp >= half ? 1 : 0, rem = pp - par * half;
                pr = (int)__umulhi((unsigned)rem, a.mg_PWh);
                pc = 2 * (rem - pr * a.PWh) + par;
                ok = ok && pp < 2 * half && pc < a.PW;
            } else {
                pr = (int)__umulhi((unsigned)pp, a.mg_PW);
                pc = pp - pr * a.PW;
                ok = ok && pp < a.PH * a.PW;
            }
            const int ih = ih0 + pr, iw = iw0 + pc;
            ok = ok && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
            goff[k] = ok ? ks * plane_bytes + (ih * a.Wi + iw) * 32 + hh * 16 : 0x7ffffff0;
        }
        const int PWe = g.is == 2 ? a.PWh : a.PW;             // row pitch (records) of the LDS patch image
        const int jr = j >> a.TWlog, jc = j & (a.TW - 1);
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            if constexpr (F8) bl[n] = ((((wave * NP + n) * a.SR + jr) * g.is) * PWe + jc) * 16 + (KS == 2 ? h * gpk * 1024 : 0);   // both k-half planes are read; lane half = channel block (KS = 2) or tap (KS = 1)
            else bl[n] = (h * a.NPIXp + (((wave * NP + n) * a.SR + jr) * g.is) * PWe + jc) * 16;
        }
        // tap table: byte offset of each tap's record inside the LDS patch image (padding taps alias tap 0; their weights are zero)
        if (tid < MAXTAPS) {                                   // [step][TP] entries, TP = T rounded up to a power of two
            constexpr int TP = T == 5 ? 8 : T;
            const int tidx = (tid / TP) * T + (tid % TP);
            const int tap = (tid % TP) < T && tidx < g.ntaps ? tidx : 0;
            const int ti = tap / g.ntw, tj = tap - ti * g.ntw;
            const int ta = (g.dh0 - g.dh_min) + ti * g.dsh, tb = (g.dw0 - g.dw_min) + tj * g.dsw;
            const int slot = g.is == 2 ? ((tb & 1) * a.PH + ta) * a.PWh + (tb >> 1) : ta * a.PW + tb;
            reinterpret_cast<int*>(lds + table_off)[tid] = slot * 16;
        }
    }
    const int ninstr = KS * gpk;
    const int wvoff = wq * 1024 + lane * 16;                  // weight waves: this lane's record inside a 4 KiB slab
    const int al = F8 ? j * 16 + h * 4096 : (h * 128 + j) * 16;   // lane part of the A-fragment address (fp8: lane half = odd / even slab of the pair)
    int pdst[NPI];                                            // patch waves: LDS offset inside a patch buffer (or the sink)
#pragma unroll
    for (int k = 0; k < NPI; ++k) pdst[k] = (k * 4 + wq) < ninstr ? (k * 4 + wq) * 1024 : -1;

    // wave w owns all 128 output channels of pixel sub-tile w (4 accumulator tiles): the GDN epilogue needs every channel
    // of a pixel, and this way it finds them in the wave's own registers
    f32x16 acc[NP][NM];
#pragma unroll
    for (int n = 0; n < NP; ++n)
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[n][m][e] = 0.0f;

    // ---- prologue: weight slab groups of the first D steps, the first L patch chunks
    int wsoff = 0;                                            // weight producer: byte offset of the next slab group in the stream
    if (wrole) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int k = 0; k < WI; ++k) dma_buf16(rw, lds + d * WST + k * 4096 + wq * 1024, wvoff, wsoff + k * 4096);
            wsoff += WST;
        }
    } else {
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int k = 0; k < NPI; ++k)
                dma_buf16(rx, lds + (pdst[k] >= 0 ? PATCH0 + l * a.PB + pdst[k] : dummy_off), goff[k], l * (KS * plane_bytes));
    }
    // the accumulators start at the bias (its 16 ... 64 scalar loads per lane fly with the prologue's DMA) instead of at zero with 64 adds
    // behind a round trip to global memory in the epilogue; fp8 operands keep the add there (the dequantisation scale comes first)
    if constexpr (!F8) {
        if (a.bias != nullptr) {
            const float* bp = a.bias + (blockIdx.y / a.msplit) * 128 + msub * 32 + 4 * h;
            const int m0i = (blockIdx.y / a.msplit) * 128 + msub * 32;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                if (m0i + m * 32 < a.Cout) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float bv = bp[m * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                        for (int n = 0; n < NP; ++n) acc[n][m][e] = bv;
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (F16K_ABLATE == 7) return;                 // launch + prologue (setup, first DMA, wait)
    if (stamp) { stamp[2] = __builtin_amdgcn_s_memtime(); stamp[3] = __builtin_amdgcn_s_memrealtime(); }
    int cslot = 0, pslot = (D % NWS) * WST;                   // byte offsets of the consumer / producer ring slots
    int cb = PATCH0, pb = PATCH0 + (L % NB) * a.PB;           // byte offsets of the patch buffer of chunk c / of chunk c+L
    int xsoff = L * (KS * plane_bytes);                       // patch producer: byte offset of chunk c+L in the input

    v4u tvq;                                                  // tap offsets (LDS bytes inside a patch buffer) of the next step
    unsigned tv4q = 0;
    auto table_request = [&](int t) {
        if constexpr (T == 5) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(tvq) : "v"(ldsb + table_off + t * 32) : "memory");
            asm volatile("ds_read_b32 %0, %1 offset:16" : "=v"(tv4q) : "v"(ldsb + table_off + t * 32) : "memory");
        } else if constexpr (T == 4) asm volatile("ds_read_b128 %0, %1" : "=v"(tvq) : "v"(ldsb + table_off + t * 16) : "memory");
        else asm volatile("ds_read_b64 %0, %1" : "=v"(*reinterpret_cast<v2u*>(&tvq)) : "v"(ldsb + table_off + t * 8) : "memory");
    };
    table_request(0);

    // One step: slice S of the patch DMA (or none), T taps x KS k-steps of 2x2 MFMAs, counted wait, barrier.
    auto step = [&](auto slice, int t, bool last) {
        constexpr int S = decltype(slice)::value;
        // The step's DMA pieces -- weight waves: the slab group of step g+D; patch waves: slice S of chunk c+L -- are issued one or
        // two at a time AFTER the MFMAs of each k-step, in the shadow of the matrix pipe, instead of en bloc at the top of the step
        // (60-185 cycles apiece there, MI355X_MICROARCH.md).  Worth ~2 % (in-kernel stamps, tools/f16k_stamps.py: 47.0 -> 46.1 core
        // clocks per MFMA per SIMD in the K loop of the 128 -> 128 stride-2 layers): the K loop is not DMA-issue-bound -- see
        // DESIGN.md section 10 for what bounds it.  F16K_DMA_SPREAD=0 keeps the en-bloc issue (A/B timing).
        auto dma_pieces = [&](int first, int last) {
            if (F16K_ABLATE == 1) return;
            if (wrole) {
#pragma unroll
                for (int k = first; k < last; ++k)
                    if (k < WI) dma_buf16(rw, lds + pslot + k * 4096 + wq * 1024, wvoff, wsoff + k * 4096);
            } else if (S >= 0) {
#pragma unroll
                for (int u = first; u < last; ++u) {
                    constexpr int k = (S >= 0 ? S : 0) * PSP;
                    if (u < PSP) dma_buf16(rx, lds + (pdst[k + u] >= 0 ? pb + pdst[k + u] : dummy_off), goff[k + u], xsoff);
                }
            }
        };
        constexpr int NPIECES = WI > PSP ? WI : PSP;
        // D == 1: the slab group of the NEXT step is awaited at the end of this one, so it goes out first (its latency budget is the
        // step; the CU's other workgroup covers what is left of it)
        constexpr bool SPREAD = F16K_DMA_SPREAD != 0 && D > 1;
        if (!SPREAD) dma_pieces(0, NPIECES);
        // LDS reads of the K loop go through inline asm with hand-counted lgkmcnt: for a compiler-visible ds_read hipcc puts
        // `s_waitcnt vmcnt(0)` in front (the DMA in flight might alias it), which would drain the prefetch queue every step.
        // The fragments of k-step i+1 are requested before the MFMAs of k-step i are issued.
        // tap offsets of this step: requested a step ago (table_request), so the wait is over before it starts; the next step's
        // request goes out now and returns under this step's MFMAs (LDS returns in order: it is older than every fragment read the
        // counted waits below leave outstanding).  Read at the top of the step they cost every wave an LDS round trip right after
        // the barrier, with nothing else to issue.
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tvq), "+v"(tv4q)::"memory");
        const v4u tvv = tvq;
        const unsigned tv4 = tv4q;
        table_request(last ? 0 : t + 1);
        const unsigned wst = ldsb + al + cslot + msub * 512;
        constexpr int NQ = F8 ? 2 : 1;                            // ds_read_b128 per fragment
        constexpr int NKS = F8 ? (T * KS) / 2 : T * KS;           // MFMA k-steps per step
        v4u af[2][NM][NQ], bfr[2][NP][NQ];
        auto request = [&](auto ic, auto bc) {
            constexpr int i = decltype(ic)::value, buf = decltype(bc)::value;
            if constexpr (F8) {
                // slabs 2i (lanes 0-31) and 2i+1 (lanes 32-63) of the step; a fragment = the 16-byte records of both k-half planes
                unsigned toff = ldsb + cb;
                if constexpr (KS == 2) toff += tvv[i];                                   // same tap, the two channel blocks (lane part of bl)
                else toff += h ? tvv[2 * i + 1] : tvv[2 * i];                            // taps 2i / 2i+1
                const unsigned plane = (unsigned)a.NPIXp * 16;
                static_for<0, NP>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    ds_read128<0>(bfr[buf][n][0], toff + bl[n]);
                    ds_read128<0>(bfr[buf][n][1], toff + bl[n] + plane);
                });
                static_for<0, NM>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    ds_read128<i * 8192 + m * 512>(af[buf][m][0], wst);
                    ds_read128<i * 8192 + m * 512 + 2048>(af[buf][m][1], wst);
                });
            } else {
                constexpr int tt = i / KS, ks = i % KS;
                const unsigned toff = ldsb + cb + (tt < 4 ? tvv[tt < 4 ? tt : 0] : tv4) + ks * gpk * 1024;
                static_for<0, NP>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    ds_read128<0>(bfr[buf][n][0], toff + bl[n]);
                });
                static_for<0, NM>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    ds_read128<i * 4096 + m * 512>(af[buf][m][0], wst);
                });
            }
        };
        if (F16K_ABLATE != 3) request(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        static_for<0, NKS>([&](auto ic) {
            constexpr int i = decltype(ic)::value, buf = i & 1;
            if constexpr (i + 1 < NKS && F16K_ABLATE != 3) request(std::integral_constant<int, i + 1>{}, std::integral_constant<int, (i + 1) & 1>{});
            constexpr int pending = i + 1 < NKS ? (NM + NP) * NQ : 0;     // LDS returns in order: what was requested for i+1 may stay out
            if constexpr (F8) {
                lgkm_wait<pending>(bfr[buf][0][0], bfr[buf][0][1], af[buf][0][0], af[buf][0][1], af[buf][1][0], af[buf][1][1],
                                   af[buf][2][0], af[buf][2][1], af[buf][3][0], af[buf][3][1]);
                const v8i b8 = cat8(bfr[buf][0][0], bfr[buf][0][1]);
                static_for<0, NM>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    acc[0][m] = mfma_f8(cat8(af[buf][m][0], af[buf][m][1]), b8, acc[0][m]);
                });
            } else {
            if constexpr (NM == 4 && NP == 1) lgkm_wait<pending>(bfr[buf][0][0], af[buf][0][0], af[buf][1][0], af[buf][2][0], af[buf][3][0]);
            else if constexpr (NM == 4 && NP == 2) lgkm_wait<pending>(bfr[buf][0][0], bfr[buf][1][0], af[buf][0][0], af[buf][1][0], af[buf][2][0], af[buf][3][0]);
            else if constexpr (NM == 1 && NP == 4) lgkm_wait<pending>(bfr[buf][0][0], bfr[buf][1][0], bfr[buf][2][0], bfr[buf][3][0], af[buf][0][0]);
            else if constexpr (NM == 3 && NP == 2) lgkm_wait<pending>(bfr[buf][0][0], bfr[buf][1][0], af[buf][0][0], af[buf][1][0], af[buf][2][0]);
            else if constexpr (NM == 2 && NP == 2) lgkm_wait<pending>(bfr[buf][0][0], bfr[buf][1][0], af[buf][0][0], af[buf][1][0]);
            else if constexpr (NM == 2 && NP == 1) lgkm_wait<pending>(bfr[buf][0][0], af[buf][0][0], af[buf][1][0]);
            else lgkm_wait<pending>(bfr[buf][0][0], af[buf][0][0]);
            static_for<0, NM>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                static_for<0, NP>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    if (F16K_ABLATE != 4 || m == 0)
                        acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[buf][m][0]), __builtin_bit_cast(bf16x8, bfr[buf][n][0]), acc[n][m], 0, 0, 0);
                });
            });
            }
            if constexpr (SPREAD) {
                constexpr int per = (NPIECES + NKS - 1) / NKS;
                __builtin_amdgcn_sched_barrier(0);
                dma_pieces(i * per, (i + 1) * per);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        if (wrole && F16K_ABLATE != 1) {
            wsoff += WST;
            pslot = pslot + WST == NWS * WST ? 0 : pslot + WST;
        }
        cslot = cslot + WST == NWS * WST ? 0 : cslot + WST;
        // weight waves: the slab group of the next step has landed, the D-1 groups after it stay in flight.
        // patch waves: at the end of a chunk the next chunk's patch has landed, the L-1 chunks after it stay in flight.
        if (wrole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * WI) : "memory");
        else if (last) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((L - 1) * NPI) : "memory");
        if (F16K_ABLATE != 2) __builtin_amdgcn_s_barrier();
    };

    for (int c = 0; c < (F16K_ABLATE == 5 || F16K_ABLATE == 8 ? 0 : nchunks); ++c) {
        step(std::integral_constant<int, 0>{}, 0, false);
        step(std::integral_constant<int, 1>{}, 1, SPC == 2);
        for (int t = 2; t < SPC; ++t) step(std::integral_constant<int, -1>{}, t, t + 1 == SPC);
        cb = cb + a.PB == PATCH0 + NB * a.PB ? PATCH0 : cb + a.PB;
        pb = pb + a.PB == PATCH0 + NB * a.PB ? PATCH0 : pb + a.PB;
        xsoff += KS * plane_bytes;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tvq), "+v"(tv4q)::"memory");      // the last step's table request must not land in reused registers
    if (stamp) { stamp[4] = __builtin_amdgcn_s_memtime(); stamp[5] = __builtin_amdgcn_s_memrealtime(); }

    // ---- epilogue
    const ConvGeom g = make_geom(a.q, phase);
    const int m0 = (blockIdx.y / a.msplit) * 128 + msub * 32;
    const int jr = j >> a.TWlog, jc = j & (a.TW - 1);
    const size_t oplane = (size_t)a.Ho * a.Wo;
    // bias, then (inverse) GDN or the activation.  Cout is a multiple of 32, so a 32-channel block is valid or not as a whole.
    if constexpr (F8) {                      // dequantise: per-output-channel weight scale x the input tensor's scale
        const float* sp = a.wscale + m0 + 4 * h;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            if (m0 + m * 32 < a.Cout) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float sv = sp[m * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                    for (int n = 0; n < NP; ++n) acc[n][m][e] *= sv;
                }
            }
        }
    }
    if constexpr (F8) {
        if (a.bias != nullptr) {
            const float* bp = a.bias + m0 + 4 * h;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                if (m0 + m * 32 < a.Cout) {
                    float bv[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) bv[e] = bp[m * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                    for (int n = 0; n < NP; ++n)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[n][m][e] += bv[e];
                }
            }
        }
    }
    if constexpr (GDN && F16K_ABLATE != 10) {
        // The fragment image (+ beta^) is shared by the 8 waves through LDS (ring and patch buffers are free now): one DMA, one barrier.
        // Piece p = (m * 8 + k-step) * 2 + plane: the odd pieces are the low halves of the three-product split -- the one-product form
        // (the default) leaves them where they are: 32 KiB per workgroup instead of 64
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)a.gdn_img, 0, 65536 + 512, 0x00020000);
        const bool x3 = (a.gdn_inverse & 2) != 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (x3 || (k & 1) == 0) dma_buf16(rg, lds + (wave * 8 + k) * 1024, lane * 16, (wave * 8 + k) * 1024);
        if (wave == 0) dma_buf16(rg, lds + 65536, lane * 16, 65536);          // 512 bytes of beta^; lanes >= 32 read past the end: zeros
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        if (NP > 1) __builtin_amdgcn_sched_barrier(0);      // one sub-tile's epilogue at a time (register pressure)
        const int r = r0 + (wave * NP + n) * a.SR + jr, c = c0 + jc;
        const bool pok = r < g.Hp && c < g.Wp;
        const int oh = pok ? r * g.os + g.oph : 0, ow = pok ? c * g.os + g.opw : 0;
        const size_t opix = (size_t)oh * a.Wo + ow;
        if constexpr (MULTI) {
            // v = conv + bias is stored in up to four layouts; each is what the stand-alone kernel it replaces computes from the float32
            // tensor (masic_quantize_fwd, nchw_to_f16k_kernel, nchw_to_f16k_view_kernel: common.h / gemm_bf16.hip / f16k_ops.hip), in the
            // same order -- rintf in float32, times the gate in float32, ONE rounding to bf16 -- so the bits are the same, -0 included.
            if (pok) {
                const unsigned op = (unsigned)oplane, op16 = op * 16;
                const size_t o32 = ((size_t)b * a.Cout + m0 + 4 * h) * oplane + opix;
                if (mo.y32 != nullptr) {
                    float* yb = mo.y32 + o32;
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (m0 + m * 32 < a.Cout) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * op] = acc[n][m][e];
                        }
                }
                if (mo.r32 != nullptr) {
                    float* yb = mo.r32 + o32;
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (m0 + m * 32 < a.Cout) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * op] = rintf(acc[n][m][e]);
                        }
                }
                if (mo.r16 != nullptr) {
                    // (x * 1.0f is x, sign of zero included: the ungated form needs no second loop)
                    const float gv = mo.gate != nullptr ? mo.gate[((size_t)b * mo.gate_ctot + mo.gate_c) * oplane + opix] : 1.0f;
                    unsigned short* yb = mo.r16 + (((size_t)b * (mo.r16_ctot >> 4) + ((mo.r16_coff + m0) >> 4)) * oplane + opix) * 16 + 8 * h;
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (m0 + m * 32 < a.Cout) {
                            f32x16 t;
#pragma unroll
                            for (int e = 0; e < 16; ++e) t[e] = rintf(acc[n][m][e]) * gv;
                            store_f16k_tile(t, yb + (size_t)(2 * m) * op16, op16);
                        }
                }
                if (mo.a16 != nullptr) {
                    unsigned short* yb = mo.a16 + (((size_t)b * (a.Cout >> 4) + (m0 >> 4)) * oplane + opix) * 16 + 8 * h;
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (m0 + m * 32 < a.Cout) {
                            f32x16 t;
#pragma unroll
                            for (int e = 0; e < 16; ++e) t[e] = fabsf(acc[n][m][e]);
                            store_f16k_tile(t, yb + (size_t)(2 * m) * op16, op16);
                        }
                }
            }
            continue;
        }
        if constexpr (GDN) {
            if (a.y16_pre != nullptr && pok) {
                const int c16 = (a.out_coff + m0) >> 4;
                unsigned short* yp = a.y16_pre + (((size_t)b * (a.out_ctot >> 4) + c16) * oplane + opix) * 16 + 8 * h;
                const unsigned op16 = (unsigned)oplane * 16;
#pragma unroll
                for (int m = 0; m < NM; ++m) store_f16k_tile(acc[n][m], yp + (size_t)(2 * m) * op16, op16);
            }
            if (F16K_ABLATE != 9 && F16K_ABLATE != 10) {
                if (a.gdn_inverse & 2) gdn_in_registers<true>(acc[n], lds + lane * 16, reinterpret_cast<const float*>(lds + 65536) + 4 * h, a.gdn_inverse & 1);
                else gdn_in_registers<false>(acc[n], lds + lane * 16, reinterpret_cast<const float*>(lds + 65536) + 4 * h, a.gdn_inverse & 1);
            }
        } else {
            float gv = 1.0f;
            if (a.gate != nullptr && pok) gv = a.gate[((size_t)b * a.gate_ctot + a.gate_c) * oplane + opix];      // (float32 NCHW or F16K output)
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[n][m][e] = apply_act(acc[n][m][e], a.act) * gv;
        }
        if (F16K_ABLATE == 8) continue;               // everything but the K loop and the stores
        // stores: one 64-bit base per lane, 32-bit channel offsets
        if (pok && a.d2s > 0) {
            // depth-to-space: channel 4c + phase of the equivalent stride-1 convolution -> pixel (2r + phase/2, 2c + phase%2) of
            // channel c.  With that channel order a lane holds whole 2x2 output blocks (channel c = h + 2q in registers 4q..4q+3):
            // two 8-byte stores per block, 256 contiguous bytes per row and half-wave.
            float* yb = a.y32 + ((size_t)b * a.out_ctot + a.out_coff) * (4 * oplane) + (size_t)(2 * oh) * (2 * a.Wo) + 2 * ow;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cc = h + 2 * q;
                if (cc < a.d2s) {
                    float* yc = yb + (size_t)cc * (4 * oplane);
                    *reinterpret_cast<float2*>(yc) = make_float2(acc[n][0][4 * q], acc[n][0][4 * q + 1]);
                    *reinterpret_cast<float2*>(yc + 2 * a.Wo) = make_float2(acc[n][0][4 * q + 2], acc[n][0][4 * q + 3]);
                }
            }
        } else if (pok) {
            if (a.y32 != nullptr && a.cout_store < a.Cout) {
                // zero-padded output channels (a 96 -> 3 layer run as 96 -> 32): store the real ones, with the float32 residual
                const int cbase = m0 + 4 * h;
                float* yb = a.y32 + ((size_t)b * a.out_ctot + a.out_coff + cbase) * oplane + opix;
                const float* rb = a.res32 != nullptr ? a.res32 + ((size_t)b * a.cout_store + cbase) * oplane + opix : nullptr;
                const unsigned op = (unsigned)oplane;
#pragma unroll
                for (int m = 0; m < NM; ++m)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int cc = m * 32 + (e & 3) + 8 * (e >> 2);
                        if (cbase + cc < a.cout_store) yb[(unsigned)cc * op] = acc[n][m][e] + (rb != nullptr ? rb[(unsigned)cc * op] : 0.0f);
                    }
            } else if (a.y32 != nullptr) {
                float* yb = a.y32 + ((size_t)b * a.out_ctot + a.out_coff + m0 + 4 * h) * oplane + opix;
                const unsigned op = (unsigned)oplane;
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    if (m0 + m * 32 < a.Cout) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) yb[(unsigned)(m * 32 + (e & 3) + 8 * (e >> 2)) * op] = acc[n][m][e];
                    }
            } else if (a.y8 != nullptr) {
                // fp8 output for an fp8-operand consumer: tile m = record m of this 128-channel block (out_coff, m0 multiples of 32)
                const int c32 = (a.out_coff + m0) >> 5;
                unsigned char* yb = a.y8 + (((size_t)b * (a.out_ctot >> 5) + c32) * oplane + opix) * 32 + 16 * h;
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    if (m0 + m * 32 < a.Cout) store_f8k_tile(acc[n][m], yb + (size_t)m * oplane * 32, a.out_inv_scale);
            } else {
                // tile m = records 2m, 2m+1 of this 128-channel block (out_coff and m0 are multiples of 16)
                const int c16 = (a.out_coff + m0) >> 4;
                unsigned short* yb = a.y16 + (((size_t)b * (a.out_ctot >> 4) + c16) * oplane + opix) * 16 + 8 * h;
                const unsigned op16 = (unsigned)oplane * 16;
                if (a.res1 != nullptr || a.mask16 != nullptr || (!GDN && a.y16_pre != nullptr)) {
                    const size_t ro = (((size_t)b * (a.res_ctot >> 4) + (m0 >> 4)) * oplane + opix) * 16 + 4 * h;
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (m0 + m * 32 < a.Cout) {
                            if (a.mask16 != nullptr) mul_f16k_actmask(acc[n][m], a.mask16 + ro + (size_t)(2 * m) * op16, op16, a.mask_slope);
                            if (!GDN && a.y16_pre != nullptr) store_f16k_tile(acc[n][m], a.y16_pre + ro + 4 * h + (size_t)(2 * m) * op16, op16);
                            if (a.res1 != nullptr) add_f16k_residual(acc[n][m], a.res1 + ro + (size_t)(2 * m) * op16, op16);
                            if (a.res2 != nullptr) add_f16k_residual(acc[n][m], a.res2 + ro + (size_t)(2 * m) * op16, op16);
                        }
                }
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    if (m0 + m * 32 < a.Cout) store_f16k_tile(acc[n][m], yb + (size_t)(2 * m) * op16, op16);
            }
        }
    }
    if (stamp) { stamp[6] = __builtin_amdgcn_s_memtime(); stamp[7] = __builtin_amdgcn_s_memrealtime(); }
#else   // !CONV_F16K_BODY: the translation unit proper
// conv_f16k.hip -- bf16 implicit-GEMM convolutions on channel-blocked activations (gfx950 / MI355X).
//
// Same layers and the same phase geometry as conv.hip (reference: coremasic/mywork/MASIC.py:510-622 analysis /
// synthesis transforms, :170-187 and :690-700 hyper transforms; factories compressai/models/utils.py:128-146), for the
// bf16-operand forward.  conv.hip's bf16 kernel reads float32 NCHW and converts while staging, which makes every
// workgroup re-convert its halo and leaves the matrix cores waiting on VGPR staging and on L2 latency of the weight
// fragments.  Here both operands reach LDS by DMA (global_load_lds, 16 bytes per lane, no VGPR round trip):
//
//   activations  F16K  [B][C/16][H*W][16] bf16 (gemm_bf16.hip): a pixel's 16 channels are one 32-byte record, so the
//                patch of a tile for one 16-channel block is rows of contiguous records and an MFMA B fragment
//                (8 consecutive k of one pixel) is one ds_read_b128;
//   weights      [phase-tap][ci/16][co][16] bf16 (pack_weight_bf16_kernel): one (tap, 16-channel) slab of a
//                128-channel block is 4 KiB contiguous, an A fragment is one ds_read_b128.
//
// Workgroup = 8 waves (2 along co x 4 along pixels), tile 128 co x 256 pixels, wave tile 64 x 64 (2 x 2 MFMA
// 32x32x16 accumulators).  K runs over chunks of KS 16-channel blocks; within a chunk over "steps" of T taps.
// Every step each wave issues the same number of DMA wave-instructions -- WI for the weight slab of step g+D
// (D+1-deep ring) and PS for a slice of the patch of chunk c+L (L+1 buffers) -- so that completion can be awaited
// with a counted `s_waitcnt vmcnt((D-1)*(WI+PS))` (never 0 inside the loop) followed by one raw s_barrier per step:
// DMA stays in flight across barriers.  Unused issue slots go to a dummy 1 KiB LDS region to keep the count fixed.
//
// LDS images are XOR-swizzled in 16-byte slots, slot' = slot ^ ((slot >> 4) & 3): the stride-2 pixel walk of a
// strided conv (64 B between lanes), the stride-1 walk (32 B) and the weight rows (32 B) all become conflict-free for
// ds_read_b128's four 16-lane groups.  The swizzle is applied on the DMA side by permuting which record a lane fetches.
//
// Epilogue: bias + activation, then either float32 NCHW (channel view of a concat buffer, optional gate) or F16K bf16
// for the next layer.
#include "f16k_device.h"
#include "conv_geom.h"

namespace {

struct F16kArgs {
    const unsigned short* x;      // F16K [B][in_c16tot][Hi*Wi][16]
    const unsigned short* w;      // slab stream, see pack_f16k_stream_kernel
    const float* bias;
    const float* gate;            // float32 [B][gate_ctot][Ho][Wo] or null (NCHW output only)
    float* y32;                   // float32 NCHW view, or null
    unsigned short* y16;          // F16K [B][out_c16tot][Ho*Wo][16], or null
    const uint4* gdn_img;         // GDN epilogue: gamma^ fragments (gdn.hip: gdn_pack_f16k_kernel), then beta^[128] floats
    const unsigned short* res1;   // F16K output only: up to two residual tensors [B][res_ctot/16][Ho*Wo][16] added after the activation
    const unsigned short* res2;   //   (ResidualBlock / Enhancement_Block identities, compressai/layers/layers.py:189, MASIC.py:163)
    int res_ctot;
    unsigned short* y16_pre;      // fused GDN + F16K output: also store the convolution's result BEFORE the GDN (same view), or null --
                                  //   what the GDN backward of a training step needs (masic_amd/autograd.py: AnalysisFn / SynthesisFn);
                                  //   residual form: the activation's output BEFORE the residual adds (view of res_ctot channels)
    unsigned long long* stamps;   // diagnostics (masic_conv_f16k_set_stamps): {s_memtime, s_memrealtime} at 4 points of the first and last workgroup
    const unsigned short* mask16; // F16K output only: multiply by act'(mask) before the residual adds (mask: F16K of res_ctot channels;
    float mask_slope;             //   slope for mask <= 0: 0.01 LeakyReLU, 0 ReLU) -- input gradients of the training step
    const float* res32;           // float32 NCHW output only: residual [B][cout_store][Ho][Wo] added after the activation, or null
    int cout_store;               // float32 NCHW output: channels actually stored (< Cout when the weight was zero-padded to a multiple of 32)
    const float* wscale;          // fp8 operands: per-output-channel dequantisation factor (weight scale x input scale), else null
    unsigned char* y8;            // F8K [B][out_c32tot][Ho*Wo][32] fp8 output (quantised with out_inv_scale), or null
    float out_inv_scale;
    int gdn_inverse;
    int d2s;                      // > 0: channel 4c + phase (2x2 phases, c < d2s); y32 is [B][out_ctot][2Ho][2Wo] (depth-to-space store)
    int in_c16tot, in_c16off, Cin16;
    int Hi, Wi, Cout, Ho, Wo;
    int out_ctot, out_coff;       // channel view of the output (NCHW: channels; F16K: channels, multiples of 16)
    int gate_ctot, gate_c, act;
    int TW, TWlog, SR, TH, tiles_w, ntiles;
    int PH, PW, PWh, NPIXp;       // patch rows / row length (pixels), ceil(PW/2), records per k-half plane of the LDS image (x32)
    int PB;                       // bytes per patch buffer
    unsigned mg_PW, mg_PWh, mg_gpk;   // ceil(2^32 / d): x / d == __umulhi(x, magic) for the small x, d of the patch maps
    unsigned phase_off[4];        // byte offset of each phase's slab streams
    unsigned stream_bytes[4];     // bytes of one (phase, co-block) slab stream
    GeomParams q;
    int nphase;
    int xcd_images;               // B % 8 == 0: image b runs on XCD b % 8 (the halos of its tiles meet in one L2)
    int msplit;                   // workgroups per 128-channel co-block (4 / NM for layers whose grid would not fill the chip, else 1):
                                  //   blockIdx.y = co-block * msplit + sub-block, a sub-block = NM accumulator tiles of the slab
};

// The outputs of conv_f16k_multi (masic_conv_f16k_multi_fwd), each of them optional (null): v = conv(x) + bias, all Cout channels
struct F16kMulti {
    float* y32;                   // float32 [B][Cout][Ho][Wo]: v
    float* r32;                   // float32 [B][Cout][Ho][Wo]: rintf(v)
    unsigned short* r16;          // F16K of r16_ctot channels, written at channels r16_coff ..: bf16(rintf(v) * gate)
    unsigned short* a16;          // F16K [B][Cout/16][Ho*Wo][16]: bf16(|v|)
    const float* gate;            // float32 [B][gate_ctot][Ho][Wo], channel gate_c (r16 only), or null
    int r16_ctot, r16_coff, gate_ctot, gate_c;
};

#ifndef F16K_DMA_SPREAD
#define F16K_DMA_SPREAD 1  // 0: the K loop's DMA pieces issued en bloc at the top of every step (A/B timing, tools/ablate_f16k.sh)
#endif
#ifndef F16K_ABLATE
#define F16K_ABLATE 0     // timing experiments only (tools/ablate_f16k.sh): 1 no DMA in the K loop, 2 no barriers, 3 no fragment reads, 4 a quarter of the MFMAs
#endif
constexpr int MAXTAPS = 64;   // tap table entries ([step][T rounded up to a power of two])

// Weights for this path, in the order the kernel consumes them ("slab stream"): for each phase, each 128-channel
// co-block, each chunk c of KS 16-channel blocks, each step t of T taps (taps padded with zeros to a multiple of T):
// T*KS slabs of 4 KiB, each the LDS image [k-half hh][co 128][8 ci] of W[co, (c*KS+ks)*16 + hh*8 + e, tap].
// A step's slab group is one contiguous WST = T*KS*4096 bytes, so the DMA of step g is base + g*WST.
struct PackStreamArgs {
    const float* w;
    int Cin, Cout, KH, KW, transposed;
    int KS, T, nchunks, ncb;
    ConvGeom gs[4];           // one launch packs every phase (blockIdx.y)
    unsigned phase_offs[4];   // bytes
};

__device__ __forceinline__ void pack_f16k_stream_body(const PackStreamArgs& a, unsigned short* __restrict__ wp, int phase, int bx, int nbx) {
    const ConvGeom g = a.gs[phase];
    const unsigned phase_off = a.phase_offs[phase];
    const int spc = (g.ntaps + a.T - 1) / a.T;
    const size_t total = (size_t)a.ncb * a.nchunks * spc * a.T * a.KS * 2048;        // bf16 elements
    for (size_t i = (size_t)bx * blockDim.x + threadIdx.x; i < total; i += (size_t)nbx * blockDim.x) {
        size_t r = i;
        const int e = (int)(r & 7); r >>= 3;
        const int co = (int)(r & 127); r >>= 7;
        const int hh = (int)(r & 1); r >>= 1;
        const int ks = (int)(r % a.KS); r /= a.KS;
        const int tt = (int)(r % a.T); r /= a.T;
        const int t = (int)(r % spc); r /= spc;
        const int c = (int)(r % a.nchunks); r /= a.nchunks;
        const int cb = (int)r;
        const int tap = t * a.T + tt;
        const int ci = (c * a.KS + ks) * 16 + hh * 8 + e, cog = cb * 128 + co;
        float v = 0.0f;
        if (tap < g.ntaps && ci < a.Cin && cog < a.Cout) {
            const int ta = tap / g.ntw, tb = tap - ta * g.ntw;
            const int kh = g.kh0 + ta * g.khs, kw = g.kw0 + tb * g.kws;
            const size_t src = a.transposed ? (((size_t)ci * a.Cout + cog) * a.KH + kh) * a.KW + kw
                                            : (((size_t)cog * a.Cin + ci) * a.KH + kh) * a.KW + kw;
            v = a.w[src];
        }
        const __bf16 bv = (__bf16)v;
        wp[(phase_off >> 1) + i] = __builtin_bit_cast(unsigned short, bv);
    }
}

__global__ void pack_f16k_stream_kernel(const PackStreamArgs a, unsigned short* __restrict__ wp) {
    pack_f16k_stream_body(a, wp, blockIdx.y, blockIdx.x, gridDim.x);
}

// Many layers' streams in one launch (a training step re-packs every weight it touches -- each for its forward and for its input
// gradient -- ~50 launches of ~5 us whose work is a few microseconds): blockIdx.y = job, blockIdx.z = phase; a job is what one
// masic_conv_f16k_pack_weight call would launch.  The job table lives in device memory (built once per set of layers).
struct PackStreamJob { PackStreamArgs a; unsigned short* wp; int nb, np; };

__global__ void pack_f16k_stream_multi_kernel(const PackStreamJob* __restrict__ jobs) {
    const PackStreamJob& j = jobs[blockIdx.y];
    if ((int)blockIdx.z >= j.np || (int)blockIdx.x >= j.nb) return;
    pack_f16k_stream_body(j.a, j.wp, blockIdx.z, blockIdx.x, j.nb);
}

// fp8 operands: the same stream with 32-channel blocks -- slab (tap, block) = LDS image [k-half hh][co 128][16 ci] of
// fp8(W[co, (c*KS+ks)*32 + hh*16 + e, tap] / wscale[co]); wscale[co] = max |W[co]| / 448 (per-output-channel scaling).
__global__ void wscale_f8k_kernel(const float* __restrict__ w, float* __restrict__ ws, int Cin, int Cout, int taps, int transposed) {
    const int co = blockIdx.x;
    float m = 0.0f;
    for (int i = threadIdx.x; i < Cin * taps; i += blockDim.x) {
        const int ci = i / taps, t = i - ci * taps;
        m = fmaxf(m, fabsf(transposed ? w[((size_t)ci * Cout + co) * taps + t] : w[((size_t)co * Cin + ci) * taps + t]));
    }
    __shared__ float red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ws[co] = red[0] > 0.0f ? red[0] / 448.0f : 1.0f;
}

__global__ void pack_f8k_stream_kernel(const PackStreamArgs a, const float* __restrict__ ws, unsigned char* __restrict__ wp) {
    const ConvGeom g = a.gs[blockIdx.y];
    const unsigned phase_off = a.phase_offs[blockIdx.y];
    const int spc = (g.ntaps + a.T - 1) / a.T;
    const size_t total = (size_t)a.ncb * a.nchunks * spc * a.T * a.KS * 4096;        // fp8 elements = bytes
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int e = (int)(r & 15); r >>= 4;
        const int co = (int)(r & 127); r >>= 7;
        const int hh = (int)(r & 1); r >>= 1;
        const int ks = (int)(r % a.KS); r /= a.KS;
        const int tt = (int)(r % a.T); r /= a.T;
        const int t = (int)(r % spc); r /= spc;
        const int c = (int)(r % a.nchunks); r /= a.nchunks;
        const int cb = (int)r;
        const int tap = t * a.T + tt;
        const int ci = (c * a.KS + ks) * 32 + hh * 16 + e, cog = cb * 128 + co;
        float v = 0.0f;
        if (tap < g.ntaps && ci < a.Cin && cog < a.Cout) {
            const int ta = tap / g.ntw, tb = tap - ta * g.ntw;
            const int kh = g.kh0 + ta * g.khs, kw = g.kw0 + tb * g.kws;
            const size_t src = a.transposed ? (((size_t)ci * a.Cout + cog) * a.KH + kh) * a.KW + kw
                                            : (((size_t)cog * a.Cin + ci) * a.KH + kh) * a.KW + kw;
            v = a.w[src] / ws[cog];
        }
        wp[phase_off + i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.0f, 0, false) & 0xff);
    }
}

// KS 16-channel blocks per chunk, T taps per step, D weight-slab look-ahead (steps), PSP patch DMA wave-instructions per
// patch wave per step during the first 2 steps of a chunk, L patch look-ahead (chunks); GDN: (inverse) GDN over the 128
// output channels fused into the epilogue.  Output: float32 NCHW if a.y32 else F16K.
// NM: 32-channel accumulator tiles per wave -- 4 (a 128-channel block) or 1 (layers with <= 32 output channels).
// NP: 32-pixel sub-tiles per wave (tile = 256 NP pixels): larger tiles for the large stride-1-walk layers, whose
// per-workgroup fixed cost (launch, first DMA, epilogue) would otherwise rival their K loop.
// F8: fp8 (e4m3) operands -- the input is F8K (32-channel records), a slab is (tap, 32-channel block) and one MFMA (K = 64)
// consumes two consecutive slabs of the step, one per lane half: with KS = 2 the two channel blocks of a tap, with KS = 1
// two consecutive taps.  DMA, LDS images, ring and geometry are the bf16 kernel's (a record is 32 bytes in both layouts).
template <int KS, int T, int D, int PSP, int L, bool GDN, int NM, int NP, bool F8 = false>
__global__ __launch_bounds__(512, D == 1 ? 2 : 1) void conv_f16k(const F16kArgs a) {     // D == 1: the two-workgroups-per-CU ("lite") configurations
    constexpr bool MULTI = false;
    constexpr F16kMulti mo{};                    // (never read: every use sits behind `if constexpr (MULTI)`)
#define CONV_F16K_BODY
#include "conv_f16k.hip"
#undef CONV_F16K_BODY
}

// The latent-producing last layer of an analysis transform (128 -> 192, 5x5, stride 2) with the multi-output epilogue: the strided-5x5
// configuration <1, 5, 2, 6, 1> of conv_f16k (NM = 1 / 2 / 4 by the co-block split) with MULTI = true -- instead of the one output of
// `a`, any subset of the four latent layouts of F16kMulti is stored from the accumulators.  The extra stores exist in this kernel only.
template <int NM>
__global__ __launch_bounds__(512, 1) void conv_f16k_multi(const F16kArgs a, const F16kMulti mo) {
    constexpr int KS = 1, T = 5, D = 2, PSP = 6, L = 1, NP = 1;
    constexpr bool GDN = false, F8 = false, MULTI = true;
#define CONV_F16K_BODY
#include "conv_f16k.hip"
#undef CONV_F16K_BODY
}

struct F16kCfg {
    int ok;
    int KS, T, L, NP, D;          // template selection: strided conv <1,4,D,6,1>, stride-1 walk <2,2,D,3,2>, large stride-1 walk <1,2,D,*,2> with NP > 1
    int TW, TWlog, SR, TH, PH, PW, PWh, NPIXp, PB;
    int Cin16, ncb;
    unsigned phase_off[4], stream_bytes[4];
    size_t packed_bytes, lds_bytes;
};

constexpr int F16K_D = 3;
constexpr int F16K_LITE_MIN_COUT = 33;      // smallest Cout that takes the lite configuration (choose_f16k)

F16kCfg choose_f16k(const masic_conv_desc_t& d, const ConvGeom* g, int nphase) {
    F16kCfg c{};
    const bool f8 = d.prec == MASIC_PREC_FP8;       // fp8 operands: 32-channel blocks, 128-channel co-blocks only, 256-pixel tiles
    const int cblk = f8 ? 32 : 16;
    if (d.Cout < 32 || d.Cout % 32 != 0 || d.Cin < cblk || d.Cin % cblk != 0 || d.in_op != MASIC_INOP_NONE || d.act == MASIC_ACT_SOFTMAX_C) return c;
    if (f8 && d.Cout < 64) return c;
    int span_h = 0, span_w = 0, min_taps = 1 << 30, max_taps = 0;
    for (int p = 0; p < nphase; ++p) {
        span_h = span_h > g[p].nth ? span_h : g[p].nth;
        span_w = span_w > g[p].ntw ? span_w : g[p].ntw;
        min_taps = min_taps < g[p].ntaps ? min_taps : g[p].ntaps;
        max_taps = max_taps > g[p].ntaps ? max_taps : g[p].ntaps;
    }
    const int is = g[0].is, Wp = g[0].Wp, Hp = g[0].Hp;
    int NPI;
    c.NP = 1;
    c.D = F16K_D;
    if (is == 2) { c.KS = 1; c.T = 4; NPI = 12; c.L = 1; }    // strided conv: big patch, 16-channel chunks, 4 taps per step
    else { c.KS = 2; c.T = 2; NPI = 8; c.L = 2; }             // stride-1 walk (transposed phases, 3x3, 5x5 s1, masked): 32-channel chunks
    // strided 5x5: 5 taps per step -- 25 taps need no zero-weight padding (4 per step pad to 28: 12 % more MFMAs) and a chunk
    // takes 5 barriers instead of 7; the 20-KiB slab groups leave room for a 3-slot ring only (look-ahead 2 steps = 40 MFMAs per
    // wave).
    if (!f8 && is == 2 && min_taps == 25 && max_taps == 25) { c.T = 5; c.D = 2; }
    // large stride-1-walk layers: 512- (128-channel blocks) or 1024-pixel tiles (<= 32 channels), 16-channel chunks
    if (!f8 && is == 1 && Wp >= 32) {
        const int np = d.Cout <= 32 ? 4 : 2;
        const long tiles = (long)ceil_div(Wp, 32) * ceil_div(Hp, 8 * np) * nphase * d.B * ceil_div(d.Cout, 128);
        if (tiles >= 512 && ceil_div(min_taps, 2) >= 2) { c.NP = np; c.KS = 1; c.T = 2; c.L = 2; NPI = np == 4 ? 10 : 6; }
        // 128-channel blocks: 32-channel chunks (2 taps x 2 channel blocks = 32 MFMAs per wave and barrier instead of 16), one chunk of
        // patch look-ahead and a 3-slot ring.
        if (c.NP == 2 && d.Cin % 32 == 0) { c.KS = 2; c.D = 2; c.L = 1; NPI = 10; }
        // 64 / 96 output channels (no GDN: that needs 128) (the 3x3 layers of Independent_EN and their input gradients): the K loop is short (K = 9 x
        // 32 ... 96) and the per-workgroup prologue + epilogue were 35 % of a workgroup's life (in-kernel stamps: 4.9 + 17.5 + 5.6 us
        // on the 96 -> 96 layer).  "Lite" configuration: 256-pixel tiles, 2-slot weight ring, 2 patch buffers = 77 KiB of LDS and
        // <= 128 VGPRs, so that TWO workgroups share a CU and one's prologue / epilogue / barrier waits run under the other's MFMAs.
        if (c.NP > 1 && d.Cout >= F16K_LITE_MIN_COUT && d.Cout <= 96 && d.Cin % 32 == 0 && ceil_div(min_taps, 2) >= 2) {
            c.NP = 1; c.KS = 2; c.T = 2; c.D = 1; c.L = 1; NPI = 6;
        }
    }
    if (ceil_div(max_taps, c.T) * (c.T == 5 ? 8 : c.T) > MAXTAPS || ceil_div(min_taps, c.T) < 2) return c;
    c.Cin16 = d.Cin / cblk;                                   // channel blocks (records) per pixel
    if (c.Cin16 % c.KS != 0) return c;                        // whole chunks only
    c.TW = Wp > 16 ? 32 : (Wp > 8 ? 16 : 8);
    c.TWlog = 0;
    while ((1 << c.TWlog) < c.TW) ++c.TWlog;
    c.SR = 32 / c.TW;
    c.TH = c.SR * 8 * c.NP;
    c.PH = (c.TH - 1) * is + span_h;
    c.PW = (c.TW - 1) * is + span_w;
    c.PWh = (c.PW + 1) / 2;
    c.NPIXp = round_up(is == 2 ? 2 * c.PH * c.PWh : c.PH * c.PW, 32);
    const int ninstr = c.KS * (c.NPIXp / 32);
    if (ceil_div(ninstr, 4) > NPI) return c;
    c.PB = ninstr * 1024;
    c.ncb = ceil_div(d.Cout, 128);
    const int nchunks = c.Cin16 / c.KS;
    size_t off = 0;
    for (int p = 0; p < nphase; ++p) {
        const size_t sb = (size_t)nchunks * ceil_div(g[p].ntaps, c.T) * c.T * c.KS * 4096;
        c.phase_off[p] = (unsigned)off;
        c.stream_bytes[p] = (unsigned)sb;
        off += sb * c.ncb;
    }
    if (off >= (1u << 31)) return c;
    c.packed_bytes = off;
    c.lds_bytes = (size_t)(c.D + 1) * c.T * c.KS * 4096 + (size_t)(c.L + 1) * c.PB + 1024 + MAXTAPS * 4;
    if (c.lds_bytes > 160 * 1024 || c.lds_bytes < 65536 + 2048) return c;       // (the fused GDN parks its 64 KiB image + beta^ at offset 0)
    c.ok = 1;
    return c;
}

// One row per compiled instantiation of conv_f16k / conv_f16k_multi: its template parameters (what the kernel's name is printed
// from) and its launcher.  plan_f16k below is the only place a row is chosen; a new instantiation is a new row.
typedef void (*F16kLaunchFn)(dim3 grid, int block, size_t lds_bytes, hipStream_t st, const F16kArgs& a, const F16kMulti* mo);
struct F16kRow {
    int KS, T, D, PSP, L;
    bool GDN;
    int NM, NP;
    bool F8, MULTI;
    F16kLaunchFn launch;
};
template <int KS, int T, int D, int PSP, int L, bool GDN, int NM, int NP, bool F8>
void f16k_row_launch(dim3 grid, int block, size_t lds_bytes, hipStream_t st, const F16kArgs& a, const F16kMulti*) {
    launch_lds<conv_f16k<KS, T, D, PSP, L, GDN, NM, NP, F8>>(grid, block, lds_bytes, st, a);
}
template <int NM>
void f16k_multi_row_launch(dim3 grid, int block, size_t lds_bytes, hipStream_t st, const F16kArgs& a, const F16kMulti* mo) {
    launch_lds<conv_f16k_multi<NM>>(grid, block, lds_bytes, st, a, *mo);
}
#define F16K_ROW(KS, T, D, PSP, L, GDN, NM, NP, F8) {KS, T, D, PSP, L, GDN, NM, NP, F8, false, f16k_row_launch<KS, T, D, PSP, L, GDN, NM, NP, F8>}
#define F16K_MULTI_ROW(NM) {1, 5, 2, 6, 1, false, NM, 1, false, true, f16k_multi_row_launch<NM>}
const F16kRow F16K_ROWS[] = {
    // strided 5x5, 5 taps per step (NM = 4 / msplit); its multi-output form
    F16K_ROW(1, 5, 2, 6, 1, true, 4, 1, false),  F16K_ROW(1, 5, 2, 6, 1, false, 1, 1, false),
    F16K_ROW(1, 5, 2, 6, 1, false, 2, 1, false), F16K_ROW(1, 5, 2, 6, 1, false, 4, 1, false),
    F16K_MULTI_ROW(1), F16K_MULTI_ROW(2), F16K_MULTI_ROW(4),
    // other strided convolutions, 4 taps per step
    F16K_ROW(1, 4, F16K_D, 6, 1, true, 4, 1, false),  F16K_ROW(1, 4, F16K_D, 6, 1, false, 1, 1, false),
    F16K_ROW(1, 4, F16K_D, 6, 1, false, 2, 1, false), F16K_ROW(1, 4, F16K_D, 6, 1, false, 4, 1, false),
    // stride-1 walk, 256-pixel tiles (NM = 1: <= 32 output channels)
    F16K_ROW(2, 2, F16K_D, 4, 2, true, 4, 1, false),  F16K_ROW(2, 2, F16K_D, 4, 2, false, 1, 1, false),
    F16K_ROW(2, 2, F16K_D, 4, 2, false, 2, 1, false), F16K_ROW(2, 2, F16K_D, 4, 2, false, 4, 1, false),
    // large stride-1-walk layers: 1024-pixel tiles (<= 32 channels), 512-pixel tiles with 16- / 32-channel chunks
    F16K_ROW(1, 2, F16K_D, 5, 2, false, 1, 4, false),
    F16K_ROW(1, 2, F16K_D, 3, 2, true, 4, 2, false), F16K_ROW(1, 2, F16K_D, 3, 2, false, 4, 2, false),
    F16K_ROW(2, 2, 2, 5, 1, true, 4, 2, false),      F16K_ROW(2, 2, 2, 5, 1, false, 4, 2, false),
    // lite: 64 / 96 output channels, two workgroups per CU
    F16K_ROW(2, 2, 1, 3, 1, false, 2, 1, false), F16K_ROW(2, 2, 1, 3, 1, false, 3, 1, false),
    // fp8 operands
    F16K_ROW(1, 4, F16K_D, 6, 1, true, 4, 1, true), F16K_ROW(1, 4, F16K_D, 6, 1, false, 4, 1, true),
    F16K_ROW(2, 2, F16K_D, 4, 2, true, 4, 1, true), F16K_ROW(2, 2, F16K_D, 4, 2, false, 4, 1, true),
};
#undef F16K_ROW
#undef F16K_MULTI_ROW

// Everything a caller needs to pack for, name or launch a layer.  flags: MASIC_F16K_* (include/masic_hip.h).
struct F16kPlan {
    const F16kRow* row;           // null: nothing compiled runs this (descriptor, flags)
    F16kCfg c;                    // geometry, packed and LDS bytes; c.ok: the shape has a configuration at all
    ConvGeom g[4];
    int np;                       // phases
    int msplit, tiles_w, ntiles;
    int xcd_images;               // B % 8 == 0: the block -> tile map that walks image b on XCD b % 8
    dim3 grid;
    int block;                    // threads per workgroup (8 waves)
};

F16kPlan plan_f16k(const masic_conv_desc_t& d, int flags) {
    F16kPlan p{};
    p.np = build_geoms(d, p.g);
    const F16kCfg& c = p.c = choose_f16k(d, p.g, p.np);
    const bool gdn = flags & MASIC_F16K_GDN, nosplit = flags & MASIC_F16K_NOSPLIT, multi = flags & MASIC_F16K_MULTI;
    const bool f8 = d.prec == MASIC_PREC_FP8;
    if (!c.ok) return p;
    // the fused GDN contracts one 128-channel block; the multi-output epilogue stands alone and has no activation
    if (gdn && (d.Cout != 128 || d.act != MASIC_ACT_NONE)) return p;
    if (multi && (gdn || nosplit || d.act != MASIC_ACT_NONE)) return p;
    p.tiles_w = ceil_div(p.g[0].Wp, c.TW);
    p.ntiles = p.tiles_w * ceil_div(p.g[0].Hp, c.TH);
    // Layers whose grid leaves most of the 256 CUs idle (the 128 -> 192 layer at 64^2 -> 32^2, hyper transforms, context models:
    // 8 ... 128 workgroups): the 128-channel co-block is split over 2 or 4 workgroups of 2 / 1 accumulator tiles each.  The patch and
    // the slab DMA are repeated per workgroup (they come from L2), the MFMA work is not.
    p.msplit = 1;
    if (!f8 && !gdn && !nosplit && c.NP == 1 && d.Cout >= 64) {
        const long wgs = (long)p.ntiles * p.np * c.ncb * d.B;
        p.msplit = wgs <= 64 ? 4 : (wgs <= 160 ? 2 : 1);
    }
    p.grid = dim3(round_up(p.ntiles, 8) * p.np, c.ncb * p.msplit, d.B);
    p.block = 512;
    p.xcd_images = d.B % 8 == 0;
    // accumulator tiles per wave: the lite rows hold exactly Cout / 32, a stride-1 walk to <= 32 channels one, the rest 4 / msplit
    const int nm = c.D == 1 ? d.Cout / 32 : ((c.T == 2 && d.Cout <= 32) ? 1 : 4 / p.msplit);
    for (const F16kRow& r : F16K_ROWS)
        if (r.KS == c.KS && r.T == c.T && r.D == c.D && r.L == c.L && r.NP == c.NP && r.NM == nm && r.GDN == gdn && r.F8 == f8 && r.MULTI == multi) {
            p.row = &r;
            break;
        }
    return p;
}

// the symbol of a row's kernel as rocprofv3 prints it
void f16k_row_name(const F16kRow& r, char* buf, size_t n) {
    if (r.MULTI) snprintf(buf, n, "conv_f16k_multi<%d>", r.NM);
    else snprintf(buf, n, "conv_f16k<%d, %d, %d, %d, %d, %s, %d, %d, %s>", r.KS, r.T, r.D, r.PSP, r.L, r.GDN ? "true" : "false", r.NM, r.NP, r.F8 ? "true" : "false");
}

}  // namespace

extern "C" int masic_conv_f16k_supported(const masic_conv_desc_t* d) { return check_desc(d) == MASIC_OK && plan_f16k(*d, 0).row != nullptr; }

extern "C" int masic_conv_f16k_multi_supported(const masic_conv_desc_t* d) {
    return check_desc(d) == MASIC_OK && plan_f16k(*d, MASIC_F16K_MULTI).row != nullptr;
}

extern "C" int masic_conv_f16k_kernel_name(const masic_conv_desc_t* d, int flags, char* buf, size_t n) {
    int rc = check_desc(d);
    if (rc != MASIC_OK) return rc;
    MASIC_REQUIRE(buf && n > 0 && (flags & ~(MASIC_F16K_GDN | MASIC_F16K_NOSPLIT | MASIC_F16K_MULTI)) == 0, MASIC_ERR_ARG,
                  "conv_f16k_kernel_name: null buffer or unknown flag");
    const F16kRow* r = plan_f16k(*d, flags).row;
    MASIC_REQUIRE(r != nullptr, MASIC_ERR_UNSUPPORTED, "conv_f16k: no kernel runs this layer shape in this form");
    f16k_row_name(*r, buf, n);
    return MASIC_OK;
}

// The launch of the layer in the form `flags` names, in the format of masic_conv_plan_name: "kernel | gx,gy,gz | block | lds | integers",
// the integers being what plan_f16k decided and the launcher hands to the kernel:
//   TW TH NP KS T D L  msplit ntiles tiles_w nphase ncb  nchunks  steps per chunk of each of the nphase phases  PW PWh NPIXp  xcd_images
// Refusals and return codes are those of masic_conv_f16k_kernel_name; the buffer is empty after a refusal (and for an empty output plane,
// where the launcher launches nothing).  Host code only: the tests read every property of a case from this line.
extern "C" int masic_conv_f16k_plan_name(const masic_conv_desc_t* d, int flags, char* buf, size_t n) {
    if (buf && n > 0) buf[0] = 0;
    int rc = check_desc(d);
    if (rc != MASIC_OK) return rc;
    MASIC_REQUIRE(buf && n > 0 && (flags & ~(MASIC_F16K_GDN | MASIC_F16K_NOSPLIT | MASIC_F16K_MULTI)) == 0, MASIC_ERR_ARG,
                  "conv_f16k_plan_name: null buffer or unknown flag");
    const F16kPlan p = plan_f16k(*d, flags);
    MASIC_REQUIRE(p.row != nullptr, MASIC_ERR_UNSUPPORTED, "conv_f16k: no kernel runs this layer shape in this form");
    if (p.g[0].Hp <= 0 || p.g[0].Wp <= 0) return MASIC_OK;
    const F16kCfg& c = p.c;
    char name[96], spc[64];
    f16k_row_name(*p.row, name, sizeof name);
    size_t used = 0;
    for (int i = 0; i < p.np; ++i) used += (size_t)snprintf(spc + used, sizeof spc - used, "%d ", ceil_div(p.g[i].ntaps, c.T));
    const bool ok = (size_t)snprintf(buf, n, "%s | %u,%u,%u | %d | %zu | %d %d %d %d %d %d %d %d %d %d %d %d %d %s%d %d %d %d\n", name, p.grid.x, p.grid.y,
                                     p.grid.z, p.block, c.lds_bytes, c.TW, c.TH, c.NP, c.KS, c.T, c.D, c.L, p.msplit, p.ntiles, p.tiles_w, p.np, c.ncb,
                                     c.Cin16 / c.KS, spc, c.PW, c.PWh, c.NPIXp, p.xcd_images) < n;
    if (!ok) buf[0] = 0;
    MASIC_REQUIRE(ok, MASIC_ERR_ARG, "conv_f16k_plan_name: buffer of %zu bytes too small", n);
    return MASIC_OK;
}

// the table itself, for tests and tools: the name of row `row`, MASIC_ERR_ARG past the last one
extern "C" int masic_conv_f16k_row_name(int row, char* buf, size_t n) {
    if (!buf || n == 0 || row < 0 || row >= (int)(sizeof(F16K_ROWS) / sizeof(F16K_ROWS[0]))) return MASIC_ERR_ARG;
    f16k_row_name(F16K_ROWS[row], buf, n);
    return MASIC_OK;
}

extern "C" size_t masic_conv_f16k_packed_bytes(const masic_conv_desc_t* d) {
    if (check_desc(d) != MASIC_OK) return 0;
    const F16kPlan p = plan_f16k(*d, 0);
    return p.row ? p.c.packed_bytes : 0;
}

namespace {
// The packing kernels' arguments for the layer; nb: blocks for the largest (phase, all co-blocks) stream of `unit`-byte elements.
int pack_stream_args(const masic_conv_desc_t* d, const float* w, int unit, PackStreamArgs& a, int& nb, int& np) {
    const F16kPlan p = plan_f16k(*d, 0);
    MASIC_REQUIRE(p.row != nullptr, MASIC_ERR_UNSUPPORTED, "conv_f16k: layer shape has no F16K configuration");
    const F16kCfg& c = p.c;
    a = PackStreamArgs{w, d->Cin, d->Cout, d->KH, d->KW, d->transposed, c.KS, c.T, c.Cin16 / c.KS, c.ncb, {}, {}};
    size_t tot = 0;
    for (int i = 0; i < p.np; ++i) {
        a.gs[i] = p.g[i];
        a.phase_offs[i] = c.phase_off[i];
        const size_t t = (size_t)c.stream_bytes[i] / unit * c.ncb;
        tot = tot > t ? tot : t;
    }
    nb = (int)((tot + 255) / 256);
    if (nb > 8192) nb = 8192;
    np = p.np;
    return MASIC_OK;
}

int pack_stream_job(const float* w, void* w_packed, const masic_conv_desc_t* d, PackStreamJob& j) {
    int rc = check_desc(d);
    if (rc != MASIC_OK) return rc;
    MASIC_REQUIRE(w && w_packed, MASIC_ERR_ARG, "conv_f16k_pack_weight: null pointer");
    j.wp = (unsigned short*)w_packed;
    return pack_stream_args(d, w, 2, j.a, j.nb, j.np);
}
}  // namespace

extern "C" int masic_conv_f16k_pack_weight(const float* w, void* w_packed, const masic_conv_desc_t* d, void* stream) {
    PackStreamJob j{};
    const int rc = pack_stream_job(w, w_packed, d, j);
    if (rc != MASIC_OK) return rc;
    hipLaunchKernelGGL(pack_f16k_stream_kernel, dim3(j.nb, j.np), dim3(256), 0, (hipStream_t)stream, j.a, j.wp);
    return masic_launch_status("conv_f16k_pack_weight");
}

// Batched form: masic_conv_f16k_pack_job writes the job one masic_conv_f16k_pack_weight(w, w_packed, d) call stands for into host
// memory (masic_conv_f16k_pack_job_bytes() bytes per job; returns the job's grid width >= 1, or a negative error code);
// masic_conv_f16k_pack_jobs_run launches a table of such jobs -- in DEVICE memory, njobs <= 65535 -- as one kernel (max_nb: the
// largest grid width among them).  The pointers inside the jobs must stay valid; weights are read at launch time.
extern "C" size_t masic_conv_f16k_pack_job_bytes(void) { return sizeof(PackStreamJob); }

extern "C" int masic_conv_f16k_pack_job(const float* w, void* w_packed, const masic_conv_desc_t* d, void* job_host) {
    MASIC_REQUIRE(job_host != nullptr, MASIC_ERR_ARG, "conv_f16k_pack_job: null pointer");
    PackStreamJob j{};
    const int rc = pack_stream_job(w, w_packed, d, j);
    if (rc != MASIC_OK) return rc < 0 ? rc : -rc;
    if (j.nb > 96) j.nb = 96;            // the batched grid is (widest job, jobs, 4 phases): the loops are grid-stride, empty blocks are not free
    *(PackStreamJob*)job_host = j;
    return j.nb;
}

extern "C" int masic_conv_f16k_pack_jobs_run(const void* jobs_dev, int njobs, int max_nb, void* stream) {
    MASIC_REQUIRE(jobs_dev && njobs >= 1 && njobs <= 65535 && max_nb >= 1, MASIC_ERR_ARG, "conv_f16k_pack_jobs_run: bad arguments");
    hipLaunchKernelGGL(pack_f16k_stream_multi_kernel, dim3(max_nb, njobs, 4), dim3(256), 0, (hipStream_t)stream, (const PackStreamJob*)jobs_dev);
    return masic_launch_status("conv_f16k_pack_jobs_run");
}

namespace {
// What an entry point asks of f16k_launch: zero-initialised, then filled by field name.
struct F16kLaunch {
    const void* x;                // F16K (F8K with fp8 operands) input, packed weights
    const void* w;
    const float* bias;
    const float* gate;
    float* y_nchw;                // exactly one of the three outputs -- none with `multi`
    void* y_f16k;
    void* y_f8k;
    float out_inv_scale;          // fp8 output: 1 / scale of the produced tensor
    const float* wscale;          // fp8 operands: dequantisation scales
    const void* gdn;              // fused (I)GDN: packed parameters, flags
    int gdn_inverse;
    const void* res1;             // F16K output: residuals, act'(mask) factor, the value before the adds (res_ctot channels each)
    const void* res2;
    const void* mask;
    float mask_slope;
    void* y_pre;
    int res_ctot;
    const float* res32;           // few-channel form: float32 residual, channels stored
    int cout_store;
    int d2s_c, d2s_ctot, d2s_coff;  // depth-to-space form: real channels (> 0 selects it), channel view of y_nchw
    const F16kMulti* multi;
};

int f16k_launch(const F16kLaunch& l, const masic_conv_desc_t* d, void* stream) {
    int rc = check_desc(d);
    if (rc != MASIC_OK) return rc;
    const bool f8 = d->prec == MASIC_PREC_FP8, d2s = l.d2s_c > 0;
    const int cblk = f8 ? 32 : 16;
    MASIC_REQUIRE(l.x && l.w && ((l.y_nchw != nullptr) + (l.y_f16k != nullptr) + (l.y_f8k != nullptr) == (l.multi ? 0 : 1)), MASIC_ERR_ARG,
                  "conv_f16k_fwd: need input, weights and exactly one output");
    MASIC_REQUIRE(l.y_f8k == nullptr || (d->out_ctot % 32 == 0 && d->out_coff % 32 == 0 && l.gate == nullptr && !d2s), MASIC_ERR_SHAPE,
                  "conv_f16k: an fp8 output needs a 32-aligned channel view and no gate");
    MASIC_REQUIRE(!f8 || (l.wscale != nullptr && !d2s), MASIC_ERR_ARG, "conv_f16k: fp8 operands need the dequantisation scales");
    // the depth-to-space, few-channel and fp8-output epilogues are not compiled for a split co-block
    const int flags = (l.gdn ? MASIC_F16K_GDN : 0) | ((d2s || l.cout_store != 0 || l.y_f8k) ? MASIC_F16K_NOSPLIT : 0) | (l.multi ? MASIC_F16K_MULTI : 0);
    const F16kPlan p = plan_f16k(*d, flags);
    const F16kCfg& c = p.c;
    MASIC_REQUIRE(c.ok, MASIC_ERR_UNSUPPORTED, "conv_f16k: layer shape has no F16K configuration");
    MASIC_REQUIRE(d->in_ctot % cblk == 0 && d->in_coff % cblk == 0, MASIC_ERR_SHAPE, "conv_f16k: input channel view must be 16-aligned (32 for fp8)");
    MASIC_REQUIRE(l.y_f16k == nullptr || (d->out_ctot % 16 == 0 && d->out_coff % 16 == 0 && d->Cout % 4 == 0 && (l.gate == nullptr || l.gdn == nullptr)),
                  MASIC_ERR_SHAPE, "conv_f16k: F16K output needs a 16-aligned channel view and Cout % 4 == 0 (a gate only without the fused GDN)");
    MASIC_REQUIRE(p.row != nullptr && (l.gdn == nullptr || l.gate == nullptr), MASIC_ERR_UNSUPPORTED,
                  "conv_f16k: the fused GDN needs Cout = 128, no activation and no gate; only the strided 5x5 bf16 configuration has the "
                  "multi-output epilogue");
    if (p.g[0].Hp <= 0 || p.g[0].Wp <= 0) return MASIC_OK;
    F16kArgs a{};
    a.x = (const unsigned short*)l.x, a.w = (const unsigned short*)l.w, a.bias = l.bias, a.gate = l.gate;
    a.y32 = l.y_nchw, a.y16 = (unsigned short*)l.y_f16k, a.y8 = (unsigned char*)l.y_f8k, a.out_inv_scale = l.out_inv_scale;
    a.gdn_img = (const uint4*)l.gdn, a.gdn_inverse = l.gdn_inverse, a.wscale = l.wscale, a.stamps = g_f16k_stamps;
    a.res1 = (const unsigned short*)l.res1, a.res2 = (const unsigned short*)l.res2, a.res_ctot = l.res_ctot;
    a.y16_pre = (unsigned short*)l.y_pre, a.mask16 = (const unsigned short*)l.mask, a.mask_slope = l.mask_slope;
    a.res32 = l.res32, a.cout_store = l.cout_store > 0 ? l.cout_store : d->Cout, a.d2s = l.d2s_c;
    a.in_c16tot = d->in_ctot / cblk, a.in_c16off = d->in_coff / cblk, a.Cin16 = c.Cin16;
    a.Hi = d->Hi, a.Wi = d->Wi, a.Cout = d->Cout, a.Ho = d->Ho, a.Wo = d->Wo;
    a.out_ctot = d2s ? l.d2s_ctot : (l.cout_store > 0 ? l.cout_store : d->out_ctot);
    a.out_coff = d2s ? l.d2s_coff : d->out_coff;
    a.gate_ctot = d->gate_ctot, a.gate_c = d->gate_c, a.act = d->act;
    a.TW = c.TW, a.TWlog = c.TWlog, a.SR = c.SR, a.TH = c.TH, a.tiles_w = p.tiles_w, a.ntiles = p.ntiles;
    a.PH = c.PH, a.PW = c.PW, a.PWh = c.PWh, a.NPIXp = c.NPIXp, a.PB = c.PB;
    a.mg_PW = (unsigned)((0x100000000ull + c.PW - 1) / c.PW);
    a.mg_PWh = (unsigned)((0x100000000ull + c.PWh - 1) / c.PWh);
    a.mg_gpk = (unsigned)((0x100000000ull + c.NPIXp / 32 - 1) / (c.NPIXp / 32));
    for (int i = 0; i < 4; ++i) a.phase_off[i] = c.phase_off[i], a.stream_bytes[i] = c.stream_bytes[i];
    a.q = geom_params(*d), a.nphase = p.np, a.xcd_images = p.xcd_images, a.msplit = p.msplit;
    p.row->launch(p.grid, p.block, c.lds_bytes, (hipStream_t)stream, a, l.multi);
    return masic_launch_status("conv_f16k_fwd");
}
}  // namespace

extern "C" int masic_conv_f16k_gdn_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* gate,
                                       const void* gdn_packed, int gdn_inverse, float* y_nchw, void* y_f16k,
                                       const masic_conv_desc_t* d, void* stream) {
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.gate = gate;
    l.gdn = gdn_packed, l.gdn_inverse = gdn_inverse;
    l.y_nchw = y_nchw, l.y_f16k = y_f16k;
    return f16k_launch(l, d, stream);
}

extern "C" int masic_conv_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* gate,
                                   float* y_nchw, void* y_f16k, const masic_conv_desc_t* d, void* stream) {
    return masic_conv_f16k_gdn_fwd(x_f16k, w_packed, bias, gate, nullptr, 0, y_nchw, y_f16k, d, stream);
}

// Extended residual form for the training step of Independent_EN (masic_amd/autograd.py: EnhancementBlockFn), everything F16K:
//   y = act(conv(x) + bias) * act'(mask) + res1 + res2,   y_pre (optional) = the value before the residual adds.
// Forward: mask NULL, y_pre = the LeakyReLU output the backward needs for its mask.  Backward (input gradient = the transposed
// convolution on the same weight): mask = the forward activation's output of the PRODUCER layer, mask_slope = 0.01 / 0 (LeakyReLU /
// ReLU), res1 / res2 = the gradients arriving over the identity paths.  mask, res1, res2, y_pre: res_ctot channels.
extern "C" int masic_conv_f16k_res_ex_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                                          const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d != nullptr && y_f16k != nullptr, MASIC_ERR_ARG, "conv_f16k_res_ex_fwd: null pointer");
    MASIC_REQUIRE(res1 != nullptr || res2 == nullptr, MASIC_ERR_ARG, "conv_f16k_res_ex_fwd: res2 without res1");
    MASIC_REQUIRE((res1 == nullptr && mask == nullptr && y_pre_f16k == nullptr) || (res_ctot % 16 == 0 && res_ctot >= d->Cout), MASIC_ERR_SHAPE,
                  "conv_f16k_res_ex_fwd: residual / mask / pre tensors need >= Cout channels, a multiple of 16");
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.y_f16k = y_f16k;
    l.res1 = res1, l.res2 = res2, l.res_ctot = res_ctot;
    l.mask = mask, l.mask_slope = mask_slope, l.y_pre = y_pre_f16k;
    return f16k_launch(l, d, stream);
}

// masic_conv_f16k_gdn_fwd with F16K output that ALSO stores the convolution's result before the GDN (y_pre_f16k, same layout as
// y_f16k): the training-mode forward keeps both for the backward pass (GDN backward needs its input, the next layer's weight
// gradient its output).
extern "C" int masic_conv_f16k_gdn_dual_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                                            void* y_pre_f16k, void* y_f16k, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(gdn_packed && y_pre_f16k && y_f16k, MASIC_ERR_ARG, "conv_f16k_gdn_dual_fwd: null pointer");
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.y_f16k = y_f16k;
    l.gdn = gdn_packed, l.gdn_inverse = gdn_inverse, l.y_pre = y_pre_f16k;
    return f16k_launch(l, d, stream);
}

// A layer with few output channels (conv2 of Independent_EN: 96 -> 3, MASIC.py:1492-1496) on the MFMA path: `d` describes the
// convolution with its weight zero-padded to Cout = 32 (packed by the caller), y_nchw is [B][cout_store][Ho][Wo] float32 and
// receives channels 0 .. cout_store-1 of act(conv(x) + bias) + res32 (res32: float32 [B][cout_store][Ho][Wo] or NULL).
extern "C" int masic_conv_f16k_few_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* res32, float* y_nchw,
                                       int cout_store, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d != nullptr && y_nchw != nullptr && cout_store > 0 && cout_store <= d->Cout && d->Cout == 32 && d->out_coff == 0, MASIC_ERR_ARG,
                  "conv_f16k_few_fwd: needs a 32-channel (zero-padded) descriptor and 0 < cout_store <= 32");
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.y_nchw = y_nchw;
    l.res32 = res32, l.cout_store = cout_store;
    return f16k_launch(l, d, stream);
}

// F16K in, F16K out (a channel view per d->out_ctot / out_coff) with up to two F16K residual tensors of res_ctot channels added
// after the activation: out = act(conv(x) + bias) + res1 [+ res2] -- the ResidualBlock / Enhancement_Block form of Independent_EN
// (compressai/layers/layers.py:160-190, MASIC.py:149-164) with bf16 operands.
extern "C" int masic_conv_f16k_res_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                                       void* y_f16k, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d != nullptr && y_f16k != nullptr, MASIC_ERR_ARG, "conv_f16k_res_fwd: null pointer");
    MASIC_REQUIRE(res1 != nullptr || res2 == nullptr, MASIC_ERR_ARG, "conv_f16k_res_fwd: res2 without res1");
    MASIC_REQUIRE(res1 == nullptr || (res_ctot % 16 == 0 && res_ctot >= d->Cout), MASIC_ERR_SHAPE, "conv_f16k_res_fwd: residual tensors need >= Cout channels, a multiple of 16");
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.y_f16k = y_f16k;
    l.res1 = res1, l.res2 = res2, l.res_ctot = res_ctot;
    return f16k_launch(l, d, stream);
}

// fp8 (e4m3) operand form (BASELINE configs[4]): d->prec = MASIC_PREC_FP8 -- the input is F8K, weights come from
// masic_conv_f8k_pack_weight, wscale[Cout] = that call's per-channel weight scales times the input tensor's scale.  With
// d->prec = MASIC_PREC_BF16 this is masic_conv_f16k_gdn_fwd plus the option of an fp8 output (y_f8k, quantised with
// out_inv_scale = 1 / scale of the produced tensor) for an fp8-operand consumer.  Exactly one of y_nchw / y_f16k / y_f8k.
extern "C" int masic_conv_f8k_fwd(const void* x, const void* w_packed, const float* wscale, const float* bias, const float* gate,
                                  const void* gdn_packed, int gdn_inverse, float* y_nchw, void* y_f16k, void* y_f8k, float out_inv_scale,
                                  const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d != nullptr, MASIC_ERR_ARG, "conv_f8k_fwd: null descriptor");
    MASIC_REQUIRE((d->prec == MASIC_PREC_FP8) == (wscale != nullptr), MASIC_ERR_ARG, "conv_f8k_fwd: wscale goes with fp8 operands (prec = MASIC_PREC_FP8)");
    MASIC_REQUIRE(y_f8k == nullptr || out_inv_scale > 0.0f, MASIC_ERR_ARG, "conv_f8k_fwd: an fp8 output needs out_inv_scale > 0");
    F16kLaunch l{};
    l.x = x, l.w = w_packed, l.wscale = wscale, l.bias = bias, l.gate = gate;
    l.gdn = gdn_packed, l.gdn_inverse = gdn_inverse;
    l.y_nchw = y_nchw, l.y_f16k = y_f16k, l.y_f8k = y_f8k, l.out_inv_scale = out_inv_scale;
    return f16k_launch(l, d, stream);
}

extern "C" size_t masic_f8k_bytes(int B, int C, int HW) { return (size_t)B * round_up(C, 32) * HW; }

extern "C" int masic_conv_f8k_pack_weight(const float* w, void* w_packed, float* wscale, const masic_conv_desc_t* d, void* stream) {
    int rc = check_desc(d);
    if (rc != MASIC_OK) return rc;
    MASIC_REQUIRE(w && w_packed && wscale && d->prec == MASIC_PREC_FP8, MASIC_ERR_ARG, "conv_f8k_pack_weight: null pointer or prec != MASIC_PREC_FP8");
    PackStreamArgs a;
    int nb, np;
    rc = pack_stream_args(d, w, 1, a, nb, np);
    if (rc != MASIC_OK) return rc;
    hipLaunchKernelGGL(wscale_f8k_kernel, dim3(d->Cout), dim3(256), 0, (hipStream_t)stream, w, wscale, d->Cin, d->Cout, d->KH * d->KW, d->transposed);
    hipLaunchKernelGGL(pack_f8k_stream_kernel, dim3(nb, np), dim3(256), 0, (hipStream_t)stream, a, (const float*)wscale, (unsigned char*)w_packed);
    return masic_launch_status("conv_f8k_pack_weight");
}

// The latent layer of an analysis transform with its result written once, in the layouts its consumers read (include/masic_hip.h).
extern "C" int masic_conv_f16k_multi_fwd(const void* x_f16k, const void* w_packed, const float* bias, const masic_f16k_multi_out_t* out,
                                         const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d != nullptr && out != nullptr, MASIC_ERR_ARG, "conv_f16k_multi_fwd: null pointer");
    MASIC_REQUIRE(out->y32 || out->round32 || out->round16 || out->abs16, MASIC_ERR_ARG, "conv_f16k_multi_fwd: no output");
    MASIC_REQUIRE(d->act == MASIC_ACT_NONE && d->out_coff == 0 && d->out_ctot == d->Cout && d->Cout % 32 == 0, MASIC_ERR_UNSUPPORTED,
                  "conv_f16k_multi_fwd: needs no activation, the whole output (no channel view) and Cout % 32 == 0");
    MASIC_REQUIRE(out->round16 == nullptr || (out->round16_ctot % 16 == 0 && out->round16_coff % 16 == 0 && out->round16_coff >= 0 &&
                                              out->round16_coff + d->Cout <= out->round16_ctot),
                  MASIC_ERR_SHAPE, "conv_f16k_multi_fwd: round16 needs a 16-aligned channel view that holds Cout channels");
    MASIC_REQUIRE(out->gate == nullptr || (out->round16 != nullptr && out->gate_c >= 0 && out->gate_c < out->gate_ctot), MASIC_ERR_SHAPE,
                  "conv_f16k_multi_fwd: the gate multiplies round16 only; gate channel out of range");
    const F16kMulti mo{out->y32, out->round32, (unsigned short*)out->round16, (unsigned short*)out->abs16, out->gate,
                       out->round16_ctot, out->round16_coff, out->gate_ctot, out->gate_c};
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.multi = &mo;
    return f16k_launch(l, d, stream);
}

// ConvTranspose2d(Cin -> C, k5, s2, p2, output_padding 1) weight [Cin][C][5][5] -> the weight [32][Cin][3][3] (+ bias [32]) of the
// equivalent stride-1 3x3 convolution to 4C (<= 32) channels whose 2x2 depth-to-space is the transposed convolution's output:
// row 4c + 2ph + pw, tap (u, v) = W[:, c, ph + 2(2-u), pw + 2(2-v)], zero where that kernel index exceeds 4 (masic_amd/ops.py:
// deconv_s2_as_conv_weight is the torch-op form the inference path caches; a training step changes the weight every iteration).
namespace {
__global__ void d2s_weight_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wo, float* __restrict__ bo, int Cin, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 32) bo[idx] = (bias != nullptr && idx < 4 * C) ? bias[idx >> 2] : 0.0f;
    if (idx >= 32 * Cin * 9) return;
    const int v = idx % 3, u = (idx / 3) % 3, ci = (idx / 9) % Cin, row = idx / (9 * Cin);
    const int c = row >> 2, ph = (row >> 1) & 1, pw = row & 1;
    const int kh = ph + 2 * (2 - u), kw = pw + 2 * (2 - v);
    wo[idx] = (c < C && kh <= 4 && kw <= 4) ? w[(((size_t)ci * C + c) * 5 + kh) * 5 + kw] : 0.0f;
}
}  // namespace
extern "C" int masic_deconv_s2_as_conv_weight(const float* w, const float* bias, float* w_out, float* bias_out, int Cin, int C, void* stream) {
    MASIC_REQUIRE(w && w_out && bias_out && Cin > 0 && C > 0 && 4 * C <= 32, MASIC_ERR_ARG, "deconv_s2_as_conv_weight: null pointer or more than 8 output channels");
    const int total = 32 * Cin * 9;
    hipLaunchKernelGGL(d2s_weight_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, bias, w_out, bias_out, Cin, C);
    return masic_launch_status("deconv_s2_as_conv_weight");
}

// A stride-2 transposed convolution to few channels (g_s_conv4: 128 -> 3, MASIC.py:550, :598) run as its equivalent
// stride-1 3x3 convolution to (4 phases x C) channels with a depth-to-space store: `d` describes that equivalent
// Conv2d (Cout = 32, weights re-laid out by the caller), y_nchw is [B][out_ctot][2 Ho][2 Wo], channels out_coff..out_coff+C-1.
extern "C" int masic_conv_f16k_d2s_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y_nchw, int C,
                                       int y_ctot, int y_coff, const masic_conv_desc_t* d, void* stream) {
    MASIC_REQUIRE(d && C > 0 && 4 * C <= 32 && d->Cout == 32 && d->stride == 1 && !d->transposed, MASIC_ERR_UNSUPPORTED,
                  "conv_f16k_d2s: needs a stride-1 convolution to 32 (padded) channels and C <= 8");
    MASIC_REQUIRE(y_coff >= 0 && y_coff + C <= y_ctot, MASIC_ERR_SHAPE, "conv_f16k_d2s: output channel view out of range");
    F16kLaunch l{};
    l.x = x_f16k, l.w = w_packed, l.bias = bias, l.y_nchw = y_nchw;
    l.d2s_c = C, l.d2s_ctot = y_ctot, l.d2s_coff = y_coff;
    return f16k_launch(l, d, stream);
}

unsigned long long* g_f16k_stamps = nullptr;
// Diagnostics: a device buffer of 16 uint64 that every following conv_f16k launch fills with {s_memtime (core clock), s_memrealtime
// (100 MHz)} pairs at kernel entry, K-loop entry, K-loop exit and kernel exit of its first [0..7] and last [8..15] workgroup;
// NULL switches it off.  tools/f16k_stamps.py reads the phases and the shader clock the chip held from them.
extern "C" void masic_conv_f16k_set_stamps(void* device_buffer) { g_f16k_stamps = (unsigned long long*)device_buffer; }
#endif  // CONV_F16K_BODY
