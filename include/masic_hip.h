/* masic_hip.h -- C ABI of libmasic_hip.so: the MI355X (gfx950) implementation of the MASIC
 * stereo-codec hot path (reference: ywz978020607/MASIC, coremasic/mywork/MASIC.py:744-851
 * `HSIC.forward`, and the compressai layers/entropy models it calls).
 *
 * The reference has no FFI on this path -- the path sits behind a Python nn.Module API and
 * every op below is an ATen call there.  This header is therefore the boundary a maintainer
 * of the reference binds with ctypes (INTEGRATION.md shows the stub); each entry point cites
 * the reference interface it replaces.
 *
 * Conventions
 *   - plain C: raw device pointers + sizes, no C++/torch types.  All tensors are NCHW,
 *     contiguous, float32 unless stated; int32 for symbol streams.
 *   - the library never allocates, frees or retains device memory: inputs, outputs and
 *     workspaces are caller-owned (torch tensors in the Python host layer).
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*); no implicit
 *     synchronisation, safe to capture into a hipGraph.
 *   - return value: 0 = MASIC_OK, negative = error; masic_last_error() returns a thread-local
 *     message.  Nothing throws, nothing calls exit().
 */
#ifndef MASIC_HIP_H
#define MASIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MASIC_ABI_VERSION 1

enum { MASIC_OK = 0, MASIC_ERR_ARG = -1, MASIC_ERR_SHAPE = -2, MASIC_ERR_LAUNCH = -3, MASIC_ERR_UNSUPPORTED = -4 };

/* activation fused into conv epilogues (nn.ReLU / nn.LeakyReLU(0.01), MASIC.py:176-182,338-376,679-689) */
enum { MASIC_ACT_NONE = 0, MASIC_ACT_RELU = 1, MASIC_ACT_LEAKY = 2,
       MASIC_ACT_SOFTMAX_C = 3 /* softmax over the output channels (mask2weights, MASIC.py:497-502); Cout <= 8 only */ };
/* transform applied to conv inputs while they are staged (torch.abs MASIC.py:185; torch.round
 * of `_quantize(...,'dequantize')` entropy_models.py:116 feeding context_prediction MASIC.py:755-757) */
enum { MASIC_INOP_NONE = 0, MASIC_INOP_ABS = 1, MASIC_INOP_ROUND = 2 };
/* operand precision of the MFMA contraction; accumulation is always float32 */
enum { MASIC_PREC_F32 = 0, MASIC_PREC_BF16 = 1,
       MASIC_PREC_FP8 = 2 /* OCP e4m3fn operands on v_mfma_scale_f32_32x32x64_f8f6f4 (conv_f8k / gemm_f8k entry points only) */ };

int masic_version(void);
const char* masic_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Convolutions.  Replaces torch.nn.Conv2d / ConvTranspose2d as built by
 * compressai/models/utils.py:128-146 (`conv`: padding=k//2; `deconv`: padding=k//2,
 * output_padding=stride-1), compressai/layers/layers.py:52-78 (MaskedConv2d type 'A') and
 * layers.py:81-83 (conv3x3).
 *
 * Input  view: channels [in_coff, in_coff+Cin)  of a buffer [B, in_ctot,  Hi, Wi]
 * Output view: channels [out_coff,out_coff+Cout) of a buffer [B, out_ctot, Ho, Wo]
 * (views let producers write straight into torch.cat targets, MASIC.py:765,827, and consumers
 * read slices of them).  Optional gate: out *= gate[b, gate_c, oh, ow] from a buffer
 * [B, gate_ctot, Ho, Wo] (the mask2weights products of MASIC.py:827).
 */
typedef struct {
    int32_t B, Cin, Hi, Wi, in_ctot, in_coff;
    int32_t Cout, Ho, Wo, out_ctot, out_coff;
    int32_t KH, KW, stride, pad;
    int32_t transposed;   /* 0: Conv2d weight [Cout,Cin,KH,KW]; 1: ConvTranspose2d weight [Cin,Cout,KH,KW] */
    int32_t masked;       /* 1: MaskedConv2d type 'A' -- only the taps before the centre are live */
    int32_t in_op;        /* MASIC_INOP_* */
    int32_t act;          /* MASIC_ACT_*  */
    int32_t gate_ctot, gate_c;   /* used when the gate pointer is non-NULL */
    int32_t prec;         /* MASIC_PREC_* */
} masic_conv_desc_t;

/* bytes of the packed-weight buffer for this layer (weights are re-laid out once per weight
 * version into the K-major, Cout-contiguous order the implicit-GEMM kernel stages into LDS) */
size_t masic_conv_packed_bytes(const masic_conv_desc_t* d);
int masic_conv_pack_weight(const float* w, void* w_packed, const masic_conv_desc_t* d, void* stream);
/* the kernel masic_conv2d_fwd launches for this layer (one launch, all phases of a transposed conv included), as rocprofv3 prints
 * it without namespace and arguments -- bench.py attributes HIP-event timings to these symbols.  MASIC_ERR_* and an empty string for
 * a layer masic_conv2d_fwd refuses. */
int masic_conv_kernel_name(const masic_conv_desc_t* d, char* buf, size_t n);
/* The launch of one call, for tests and tools: form = the optional operands of the call (MASIC_CONV_GATE, _RES1, _RES2 for
 * masic_conv2d_fwd_ex; MASIC_CONV_F16K_OUT alone for masic_conv2d_f16k_out_fwd).  Writes "kernel | gx,gy,gz | block | lds bytes |
 * integers\n" -- the kernel with every template argument, then what it is handed beside the descriptor's own fields (implicit GEMM:
 * Cin_pad Cout_pad KC TW TH SR PH PW PSZ buf_sz vec4 nphase; conv_direct_f32: nphase; deconv5s2_small_cout: Cin_pad tiles_w;
 * conv5s1_small: tiles_w) -- and returns what the call returns; the string is empty when the call is refused or launches nothing.
 * masic_conv_row_name enumerates the compiled kernels the launcher chooses from: rows 0 .., columns in_op 0 .. 2 x flag 0 / 1
 * (VEC4 of conv_igemm_f32, PF of conv_igemm_bf16); MASIC_ERR_ARG past the last row and for a column the row lacks. */
enum { MASIC_CONV_GATE = 1, MASIC_CONV_RES1 = 2, MASIC_CONV_RES2 = 4, MASIC_CONV_F16K_OUT = 8 };
int masic_conv_plan_name(const masic_conv_desc_t* d, int form, char* buf, size_t n);
int masic_conv_row_name(int row, int in_op, int flag, char* buf, size_t n);
/* y = act(conv(in_op(x), w) + bias) [* gate].  bias may be NULL. */
int masic_conv2d_fwd(const float* x, const void* w_packed, const float* bias, const float* gate,
                     float* y, const masic_conv_desc_t* d, void* stream);
/* same, plus up to two residual tensors [B,Cout,Ho,Wo] added after the activation: the `out + identity` of
 * ResidualBlock (compressai/layers/layers.py:189), Enhancement_Block (MASIC.py:163) and Independent_EN (:1495-1496) */
int masic_conv2d_fwd_ex(const float* x, const void* w_packed, const float* bias, const float* gate,
                        const float* res1, const float* res2, float* y, const masic_conv_desc_t* d, void* stream);
/* The layer with its result stored as F16K bf16 instead of float32 NCHW: y_f16k = [B][out_ctot/16][Ho*Wo][16], channels out_coff ..
 * (both multiples of 16) = bf16(act(conv(x) + bias)), bit for bit what masic_nchw_to_f16k makes of masic_conv2d_fwd's float32 result
 * -- for a layer whose only reader is an F16K convolution (the second hyper-synthesis layer in front of the 3x3 one).  bf16 operands
 * on the implicit-GEMM kernel and Cout % 32 == 0 only (masic_conv2d_f16k_out_supported), no gate, no residuals. */
int masic_conv2d_f16k_out_supported(const masic_conv_desc_t* d);
int masic_conv2d_f16k_out_fwd(const float* x, const void* w_packed, const float* bias, void* y_f16k,
                              const masic_conv_desc_t* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * The 1x1 stacks of the GMM parameter heads (MASIC.py:330-468) as bf16 GEMMs whose intermediate activations stay in
 * the matrix-core-friendly layout F16K = [B][C/16][H*W][16] bf16 (see masic_amd/csrc/gemm_bf16.hip):
 *   masic_nchw_to_f16k     float32 NCHW channel view -> F16K (zero padded to a multiple of 16 channels)
 *   masic_gemm1x1_*        y = act(W x + b) with x in F16K; output either F16K (next layer) or float32 NCHW view.
 * `transposed` = 1 packs a ConvTranspose2d(k=1) weight [Cin,Cout] (the first two layers of the y1 stacks, :339-342). */
size_t masic_f16k_bytes(int B, int C, int HW);
int masic_nchw_to_f16k(const float* x, void* y, int B, int C, int HW, int ctot, int coff, void* stream);
/* the same with |x| / round(x) applied on the way (MASIC_INOP_*): the inputs of the hyper-analysis transform (MASIC.py:184)
 * and of the context model in eval mode (:770, :812) */
int masic_nchw_to_f16k_op(const float* x, void* y, int B, int C, int HW, int ctot, int coff, int in_op, void* stream);
size_t masic_gemm1x1_packed_bytes(int Cin, int Cout);
int masic_gemm1x1_pack_weight(const float* w, void* wp, int Cin, int Cout, int transposed, void* stream);
int masic_gemm1x1_bf16_fwd(const void* x_f16k, const void* w_packed, const float* bias, void* y_f16k, float* y_nchw,
                           int B, int Cin, int Cout, int HW, int out_ctot, int out_coff, int act, void* stream);

/* The same 1x1 layers with both operands staged by DMA (masic_amd/csrc/gemm_f16k.hip: gemm_f16k), Cin % 16 == 0 and
 * Cout % 32 == 0; own weight pack (per 128-channel block, 64-channel chunks in LDS-image order). */
size_t masic_gemm_f16k_packed_bytes(int Cin, int Cout);
int masic_gemm_f16k_pack_weight(const float* w, void* wp, int Cin, int Cout, int transposed, void* stream);
/* n (<= 18) such packs in one launch: the nine layers of an entropy-parameter head, forward and transposed (training step) */
int masic_gemm_f16k_pack_weights(const float* const* w, void* const* wp, const int* Cin, const int* Cout, const int* transposed, int n, void* stream);
int masic_gemm_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, void* y_f16k, float* y_nchw,
                        int B, int Cin, int Cout, int HW, int out_ctot, int out_coff, int act, void* stream);
/* Up to three such layers over the same B x HW pixels in ONE launch: layer i of the sigma / means / weights stacks of a GMM head
 * (reference MASIC.py:330-468: nine 1x1 layers per head, three per stack) -- 640 ... 864 workgroups instead of three launches of
 * 192 ... 288.  All groups bf16 operands (wscale NULL: x is F16K) or all fp8 (wscale set: x is F8K, weights from
 * masic_gemm_f8k_pack_weight, wscale = weight scales x the input tensor's scale); per group exactly one of y_f16k / y_f8k (quantised
 * with out_inv_scale) / y_nchw.  Results equal the single-layer calls bit for bit. */
typedef struct masic_gemm_group {
    const void* x;
    const void* w_packed;
    const float* wscale;
    const float* bias;
    void* y_f16k;
    void* y_f8k;
    float* y_nchw;
    float out_inv_scale;
    int Cin, Cout, out_ctot, out_coff, act;
} masic_gemm_group_t;
int masic_gemm_f16k_group_fwd(const masic_gemm_group_t* groups, int ngroups, int B, int HW, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same convolutions (nn.Conv2d / nn.ConvTranspose2d / MaskedConv2d of MASIC.py:510-622, :170-187, :690-700) with
 * the input -- and optionally the output -- in F16K: the bf16-operand forward keeps the 128/192-channel activations of
 * the analysis / synthesis / hyper transforms in that layout between layers, so both MFMA operands reach LDS by
 * 16-byte DMA (masic_amd/csrc/conv_f16k.hip).  The descriptor is the one of masic_conv2d_fwd; in_ctot/in_coff (and
 * out_ctot/out_coff for an F16K output) count channels of the F16K buffers and must be multiples of 16; in_op must
 * be NONE.  Exactly one of y_nchw (float32 channel view, optional gate as in masic_conv2d_fwd) / y_f16k is non-null.
 *   masic_conv_f16k_supported    1 when the layer shape has a configuration (Cout >= 64, Cin >= 16, ...), else 0
 *   masic_conv_f16k_packed_bytes / _pack_weight   [phase-tap][ci/16][co][16] bf16 weights for this path */
int masic_conv_f16k_supported(const masic_conv_desc_t* d);
/* masic_conv_f16k_kernel_name: the symbol, as rocprofv3 prints it, of the kernel that runs the layer in the form `flags` names;
 * MASIC_ERR_UNSUPPORTED where the forward call of that form would refuse the layer (fused GDN with Cout != 128 or an activation,
 * the multi-output form on any other configuration than its own, ...). */
#define MASIC_F16K_GDN 1       /* fused (I)GDN epilogue (masic_conv_f16k_gdn_fwd with gdn_packed) */
#define MASIC_F16K_NOSPLIT 2   /* the forms whose co-block is never split: _d2s_fwd, _few_fwd, an fp8 output of masic_conv_f8k_fwd */
#define MASIC_F16K_MULTI 4     /* masic_conv_f16k_multi_fwd: conv_f16k_multi<NM> */
int masic_conv_f16k_kernel_name(const masic_conv_desc_t* d, int flags, char* buf, size_t n);
/* masic_conv_f16k_plan_name: that kernel's launch as one line "kernel | gx,gy,gz | block | lds | integers" (the format of
 * masic_conv_plan_name); the integers are  TW TH NP KS T D L  msplit ntiles tiles_w nphase ncb  nchunks  <steps per chunk of each phase>
 * PW PWh NPIXp  xcd_images.  Refusals and return codes as masic_conv_f16k_kernel_name; the buffer is empty after a refusal. */
int masic_conv_f16k_plan_name(const masic_conv_desc_t* d, int flags, char* buf, size_t n);
int masic_conv_f16k_row_name(int row, char* buf, size_t n);   /* every compiled conv_f16k / conv_f16k_multi symbol: rows 0 .., MASIC_ERR_ARG past the last */
size_t masic_conv_f16k_packed_bytes(const masic_conv_desc_t* d);
int masic_conv_f16k_pack_weight(const float* w, void* w_packed, const masic_conv_desc_t* d, void* stream);
/* Batched packing (a training step re-packs every weight it touches, each for its forward and for its input gradient):
 * masic_conv_f16k_pack_job writes, into host memory (masic_conv_f16k_pack_job_bytes() bytes), the job that one
 * masic_conv_f16k_pack_weight(w, w_packed, d) call stands for and returns its grid width (>= 1; negative: error code);
 * masic_conv_f16k_pack_jobs_run launches a table of such jobs, held in DEVICE memory, as ONE kernel (max_nb = the largest grid
 * width in the table).  Pointers inside the jobs must stay valid; the weights are read when the kernel runs. */
size_t masic_conv_f16k_pack_job_bytes(void);
int masic_conv_f16k_pack_job(const float* w, void* w_packed, const masic_conv_desc_t* d, void* job_host);
int masic_conv_f16k_pack_jobs_run(const void* jobs_dev, int njobs, int max_nb, void* stream);
int masic_conv_f16k_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* gate,
                        float* y_nchw, void* y_f16k, const masic_conv_desc_t* d, void* stream);
/* The same with the (inverse) GDN that follows the 128-channel convolutions of the analysis / synthesis transforms
 * (MASIC.py:521-531, :544-554; compressai/layers/gdn.py:77-92) fused into the epilogue: y = GDN(conv(x) + bias).
 * gdn_packed: masic_gdn_pack_f16k of that GDN's stored beta/gamma (masic_gdn_f16k_packed_bytes bytes).
 * gdn_inverse (here and in masic_conv_f8k_fwd / masic_conv_a_gdn_fwd*): bit 0 = inverse GDN; bit 1 = contract gamma^ x x^2 as the
 * three-product bf16 hi/lo split (~2^-16 of the result) instead of ONE bf16 product (~2^-10: the order of the bf16 rounding the
 * result gets when it is stored for the next bf16-operand layer; a third of the epilogue's MFMAs). */
size_t masic_gdn_f16k_packed_bytes(void);
int masic_gdn_pack_f16k(const float* beta, const float* gamma, void* packed, int C, double beta_min, void* stream);
int masic_conv_f16k_gdn_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* gate,
                            const void* gdn_packed, int gdn_inverse, float* y_nchw, void* y_f16k,
                            const masic_conv_desc_t* d, void* stream);

/* The latent-producing last layer of an analysis transform (g_a_conv4: Conv2d(128 -> 192, k5, s2), MASIC.py:522, :570) with its result
 * v = conv(x) + bias written ONCE, from the float32 accumulators, in every layout a consumer of the eval forward reads -- instead of
 * float32 NCHW followed by masic_quantize_fwd / masic_nchw_to_f16k_op / masic_nchw_to_f16k_view_op passes over that tensor.  Any
 * non-empty subset of the four outputs; each is bit-identical to what those calls make of the float32 result (rintf in float32, then
 * the gate in float32, then one round-to-nearest-even to bf16; the sign of zero included):
 *   y32      float32 [B][Cout][Ho][Wo]     v
 *   round32  float32 [B][Cout][Ho][Wo]     rintf(v)                 (masic_quantize_fwd mode 0: the y_hat the model returns)
 *   round16  F16K of round16_ctot channels, channels round16_coff .. round16_coff + Cout - 1 (both multiples of 16):
 *                                          bf16(rintf(v) * gate)    (masic_nchw_to_f16k_view_op, MASIC_INOP_ROUND; gate: float32
 *                                          [B][gate_ctot][Ho][Wo], channel gate_c, or NULL = no gate)
 *   abs16    F16K [B][Cout/16][Ho*Wo][16]  bf16(|v|)                (masic_nchw_to_f16k_op, MASIC_INOP_ABS)
 * `d`: the layer with act = MASIC_ACT_NONE and no output view (out_ctot = Cout, out_coff = 0), Cout % 32 == 0; its gate fields are not
 * read.  masic_conv_f16k_multi_supported: 1 for the shapes that have this epilogue (the strided 5x5 bf16 configuration), else 0 --
 * masic_conv_f16k_multi_fwd then returns MASIC_ERR_UNSUPPORTED and the caller keeps the separate launches. */
typedef struct masic_f16k_multi_out {
    float* y32;
    float* round32;
    void* round16;
    void* abs16;
    const float* gate;
    int round16_ctot, round16_coff, gate_ctot, gate_c;
} masic_f16k_multi_out_t;
int masic_conv_f16k_multi_supported(const masic_conv_desc_t* d);
int masic_conv_f16k_multi_fwd(const void* x_f16k, const void* w_packed, const float* bias, const masic_f16k_multi_out_t* out,
                              const masic_conv_desc_t* d, void* stream);

/* encoder2.pre_conv + pre_gdn (MASIC.py:559-560, :574-576) and decoder2.after_gdn + torch.cat + after_conv (:599-600,
 * :617-621) as one launch each: Conv2d / ConvTranspose2d(6 -> 3, k5, s1, p2) on channels [xa(3) | xb(3)] of two float32
 * tensors, optional 3-channel (I)GDN on xa while it is staged (gin_*: stored beta[3], gamma[3,3]) and / or on the result
 * (gout_*).  w_packed: masic_conv_pack_weight of that layer.  Same float32 operation order as the separate kernels. */
int masic_conv5s1_pair_fwd(const float* xa, const float* xb, const float* w_packed, const float* bias,
                           const float* gin_beta, const float* gin_gamma, int gin_inverse,
                           const float* gout_beta, const float* gout_gamma, int gout_inverse, double beta_min,
                           float* y, int B, int H, int W, void* stream);

/* The last synthesis layer g_s_conv4 = ConvTranspose2d(128 -> 3, k5, s2) (MASIC.py:550, :598) as its equivalent stride-1
 * 3x3 convolution to (2x2 phases) x C channels with a depth-to-space store.  `d`: that Conv2d(Cin -> 32 (zero padded), k3,
 * s1, p1) with weight row (4c + phase) = W_t[:, c, phase_h + 2(2-u), phase_w + 2(2-v)] (zero where the index exceeds 4;
 * phase = 2 phase_h + phase_w) and bias row (4c + phase) = bias[c]; y_nchw: [B][y_ctot][2 Hi][2 Wi], channels
 * y_coff .. y_coff+C-1 are written. */
int masic_conv_f16k_d2s_fwd(const void* x_f16k, const void* w_packed, const float* bias, float* y_nchw, int C,
                            int y_ctot, int y_coff, const masic_conv_desc_t* d, void* stream);

/* First analysis layer g_a_conv1 + g_a_gdn1 (MASIC.py:515-516, :563-564) in one kernel: Conv2d(3 -> 128, k5, s2, p2) on
 * channels in_coff..in_coff+2 of a float32 NCHW tensor, GDN, result in F16K [B][8][Ho*Wo][16]. */
/* ------------------------------------------------------------------------------------------
 * fp8 (OCP e4m3fn) operand path -- BASELINE.json configs[4] ("fp8 MFMA conv path + int32 symbol quantise").  No reference
 * counterpart (the reference computes in float32): a declared-budget approximation of the layers above, gated against the
 * oracle in tests/test_gpu_fp8.py.  Activations: F8K = [B][C/32][H*W][32] fp8, stored as fp8(x / scale) with one scale per
 * tensor; weights: one scale per output channel, written by the pack calls.  Contraction:
 * v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales, float32 accumulate; dequantisation (wscale[co] = weight scale x
 * input scale) in the epilogue (masic_amd/csrc/conv_f16k.hip, gemm_f16k.hip, fp8.hip).
 *   masic_nchw_to_f8k            float32 NCHW channel view -> F8K (in_op as masic_nchw_to_f16k_op), x * inv_scale, saturating
 *   masic_absmax                 *out = max(*out, max|x|) over n float32 (bf16 = 0) or bf16 (bf16 = 1) values: calibration
 *   masic_conv_f8k_pack_weight   d->prec = MASIC_PREC_FP8: fp8 slab stream + wscale[Cout] (max|W[co]| / 448)
 *   masic_conv_f8k_fwd           d->prec = MASIC_PREC_FP8: x is F8K, wscale required; d->prec = MASIC_PREC_BF16: x is F16K, wscale NULL
 *                                (= masic_conv_f16k_gdn_fwd).  Exactly one of y_nchw / y_f16k / y_f8k (fp8(y * out_inv_scale)).
 *   masic_gemm_f8k_*             the 1x1 layers (masic_gemm_f16k_*) with fp8 operands
 *   masic_conv_a_gdn_fwd_ex      masic_conv_a_gdn_fwd with the option of an F8K output */
size_t masic_f8k_bytes(int B, int C, int HW);
int masic_nchw_to_f8k(const float* x, void* y, int B, int C, int HW, int ctot, int coff, int in_op, float inv_scale, void* stream);
int masic_absmax(const void* x, size_t n, int bf16, float* out, void* stream);
int masic_conv_f8k_pack_weight(const float* w, void* w_packed, float* wscale, const masic_conv_desc_t* d, void* stream);
int masic_conv_f8k_fwd(const void* x, const void* w_packed, const float* wscale, const float* bias, const float* gate,
                       const void* gdn_packed, int gdn_inverse, float* y_nchw, void* y_f16k, void* y_f8k, float out_inv_scale,
                       const masic_conv_desc_t* d, void* stream);
size_t masic_gemm_f8k_packed_bytes(int Cin, int Cout);
int masic_gemm_f8k_pack_weight(const float* w, void* wp, float* wscale, int Cin, int Cout, int transposed, void* stream);
int masic_gemm_f8k_fwd(const void* x_f8k, const void* w_packed, const float* wscale, const float* bias, void* y_f16k, void* y_f8k,
                       float* y_nchw, float out_inv_scale, int B, int Cin, int Cout, int HW, int out_ctot, int out_coff, int act, void* stream);
int masic_conv_a_gdn_fwd_ex(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                            void* y_f16k, void* y_f8k, float out_inv_scale, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream);

/* training-mode forms of the two fused conv + GDN entry points: F16K output plus the convolution's result BEFORE the GDN
 * (y_pre_f16k, same layout) -- the GDN backward needs its input, the next layer's weight gradient its output
 * (masic_amd/autograd.py: AnalysisFn / SynthesisFn run the inference kernels in the training step and keep bf16 activations) */
int masic_conv_f16k_gdn_dual_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                                 void* y_pre_f16k, void* y_f16k, const masic_conv_desc_t* d, void* stream);
int masic_conv_a_gdn_dual_fwd(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                              void* y_pre_f16k, void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream);
/* Training step, input gradients of the picture-end layers (newtrain_codec_real.py:141 `loss.backward()` through MASIC.py:515, :550):
 * masic_conv_a_fwd -- Conv2d(3 -> 128, k5, s2, p2) alone (the first-layer kernel without its GDN) on a float32 NCHW channel view,
 *   F16K out: the input gradient of g_s_conv4 = ConvTranspose2d(128 -> 3) (its weight tensor [128][3][5][5] is that convolution's);
 * masic_deconv_s2_as_conv_weight -- ConvTranspose2d(Cin -> C <= 8, k5, s2, p2, op1) weight [Cin][C][5][5] (+ bias [C] or NULL) ->
 *   weight [32][Cin][3][3] and bias [32] of the stride-1 convolution masic_conv_f16k_d2s_fwd runs; with a Conv2d(C -> Cin) weight
 *   [Cin][C][5][5] passed as it is, that launch computes the convolution's input gradient (g_a_conv1). */
int masic_conv_a_fwd(const float* x, const void* w_packed, const float* bias, void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff,
                     void* stream);
int masic_deconv_s2_as_conv_weight(const float* w, const float* bias, float* w_out, float* bias_out, int Cin, int C, void* stream);
/* weight gradient of Conv2d(Cin -> Cout, k3, s1, p1) with both operands in F16K (Cin, Cout multiples of 32): the 3x3 layers of
 * Independent_EN in the CQE training step (newtrain_cqe_real.py:128-174).  Pixel-major records become MFMA operands through the
 * hardware transpose read ds_read_b64_tr_b16 (masic_amd/csrc/wgrad_f16k.hip).  dw: float32 [Cout][Cin][3][3]; workspace:
 * masic_conv3x3_wgrad_f16k_workspace_bytes bytes; workspace_clean as masic_conv2d_wgrad_ws (0: zeroed by the call). */
size_t masic_conv3x3_wgrad_f16k_workspace_bytes(int Cin, int Cout);
int masic_conv3x3_wgrad_f16k_ws(const void* x_f16k, const void* dy_f16k, float* dw, void* workspace,
                             int B, int Cin, int Cout, int H, int W, int workspace_clean, void* stream);
/* The same for Conv2d(Cin -> Cout, k5, s1, p2): encode_hyper's first layer and the context model at latent resolution
 * (reference MASIC.py:170-187, :627; a MaskedConv2d gets the dense gradient -- the reference masks weight.data, not the gradient).
 * dw: float32 [Cout][Cin][5][5]; workspace_clean as masic_conv2d_wgrad_ws. */
/* Weight gradient (float32, 128 x 3 x 5 x 5) of the two picture-end 5x5 stride-2 layers in the bf16 mode -- g_a_conv1 = Conv2d(3 -> 128)
 * (MASIC.py:515) and g_s_conv4 = ConvTranspose2d(128 -> 3) (:550): p_f16k = the 128-channel tensor at Hc x Wc in F16K (dy of the
 * former: dW = [Cout][Cin][5][5]; x of the latter: dW = [Cin][Cout][5][5]), q = the 3-channel tensor at 2 Hc x 2 Wc, float32 NCHW
 * (channels q_coff .. q_coff + 2 of q_ctot).  Per-workgroup partials + a finishing pass: deterministic.  workspace:
 * masic_pic_wgrad_f16k_workspace_bytes() bytes, contents irrelevant on entry and exit. */
size_t masic_pic_wgrad_f16k_workspace_bytes(void);
int masic_pic_wgrad_f16k(const void* p_f16k, const float* q, float* dw, void* workspace, int B, int Hc, int Wc,
                         int q_ctot, int q_coff, void* stream);
size_t masic_conv5x5_wgrad_f16k_workspace_bytes(int Cin, int Cout);
int masic_conv5x5_wgrad_f16k_ws(const void* x_f16k, const void* dy_f16k, float* dw, void* workspace,
                                int B, int Cin, int Cout, int H, int W, int workspace_clean, void* stream);
/* Weight gradient of the 1x1 layers (the entropy-parameter stacks, reference MASIC.py:330-468) from F16K operands:
 * dw[a][q] = sum over batch and pixels of rows[b][a][p] * cols[b][q][p]; rows / cols: F16K [B][C/16][HW][16] bf16 with CA / CQ
 * channels (multiples of 16); dw float32 [CA][CQ].  Conv2d weight [Cout][Cin]: rows = dy, cols = x; ConvTranspose2d(k1) weight
 * [Cin][Cout]: rows = x, cols = dy.
 * With the layer's bias gradient in the same launch: bias_of 1: dw[CA*CQ .. CA*CQ + CA) = sums of the rows operand over batch and
 * pixels (dy of a Conv2d), 2: dw[CA*CQ .. CA*CQ + CQ) = sums of the columns operand (dy of a ConvTranspose2d); dw then holds that
 * many more floats.  0: the weight gradient alone. */
int masic_gemm_wgrad_bias_f16k(const void* rows_f16k, const void* cols_f16k, float* dw, int bias_of, int B, int CA, int CQ, int HW, void* stream);
/* F16K in, F16K out with up to two F16K residual tensors added after the activation: out = act(conv(x) + bias) + res1 [+ res2]
 * (ResidualBlock: compressai/layers/layers.py:160-190; Enhancement_Block: MASIC.py:149-164) -- Independent_EN with bf16
 * operands keeps its 32 / 64 / 96-channel full-resolution activations in F16K.  y_f16k is a channel view (d->out_ctot / out_coff). */
int masic_conv_f16k_res_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                            void* y_f16k, const masic_conv_desc_t* d, void* stream);
/* the same with the pieces the CQE training step needs (masic_amd/autograd.py: EnhancementBlockFn), everything F16K:
 *   y = act(conv(x) + bias) * act'(mask) + res1 + res2;  y_pre (optional) = the value before the residual adds.
 * Forward: mask NULL, y_pre = the LeakyReLU output (its sign is the mask of the backward).  Input gradient (d->transposed on the same
 * weight): mask = the producer's activation output, mask_slope 0.01 (LeakyReLU) / 0 (ReLU), res1 / res2 = gradients of the identity paths. */
int masic_conv_f16k_res_ex_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                               const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, const masic_conv_desc_t* d, void* stream);
/* F16K elementwise / reduction helpers of that backward: out = g * act'(y); out[c] = sum over (b, pixel) of x (a bias gradient) */
int masic_f16k_act_bwd(const void* g, const void* y, void* out, size_t n, float slope, void* stream);
size_t masic_f16k_channel_sum_workspace_bytes(int B, int C);
int masic_f16k_channel_sum(const void* x, float* out, void* workspace, int B, int C, int HW, void* stream);
/* out = g * act'(y) (as masic_f16k_act_bwd) and sums[C] = its per-channel sums (as masic_f16k_channel_sum of out) in one pass over the
 * tensors; workspace: masic_f16k_channel_sum_workspace_bytes(B, C) */
int masic_f16k_act_bwd_sum(const void* g, const void* y, void* out, float* sums, void* workspace, int B, int C, int HW, float slope, void* stream);
/* mask2weights_EN (reference MASIC.py:1411-1434, Kw = 2) in one launch: gates [B,2,H,W] = softmax over channels of four 3x3
 * stride-1 convolutions 1 -> 2 -> 4 -> 4 -> 2 with ReLUs on mask [B,1,H,W]; w_i [Cout][Cin][3][3], b_i [Cout], float32 on the
 * device.  Bit-identical to the four-launch form (masic_conv2d_fwd per layer). */
int masic_mask2weights_en_fwd(const float* mask, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                              const float* b3, const float* w4, const float* b4, float* gates, int B, int H, int W, void* stream);
/* Conv2d(Cin -> Cout, k3, s1, p1) on F16K with the whole weight tensor resident in LDS and persistent workgroups: Cout = 32 | 64,
 * Cin <= Cout (the input buffer holds round_up(Cin, 16) channels; a 3- or 6-channel picture is one zero-padded record per pixel) --
 * the 32- / 64-channel stages of Independent_EN and its input layers (reference MASIC.py:149-164, 1456-1482 / layers.py:99-121;
 * conv_f16k spends three quarters of such a launch in per-workgroup prologue / epilogue).  Same operand meaning as
 * masic_conv_f16k_res_ex_fwd; `transposed` in the pack selects the slabs of the INPUT gradient of a Conv2d(Cout -> Cin) layer
 * (weight [Cin][Cout][3][3]).  Needs W % 32 == 0 and H % 16 == 0 (Cout = 32) / H % 8 == 0 (Cout = 64). */
size_t masic_conv3x3_resident_packed_bytes(int Cin, int Cout);
int masic_conv3x3_resident_supported(int B, int Cin, int Cout, int H, int W);
int masic_conv3x3_resident_pack_weight(const float* w, void* w_packed, int Cin, int Cout, int transposed, void* stream);
int masic_conv3x3_resident_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                               const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, int B, int Cin, int Cout, int H, int W,
                               int in_ctot, int in_coff, int out_ctot, int out_coff, int act, void* stream);
/* ... for the backward chain of a residual block (autograd of reference layers.py:160-190 / MASIC.py:149-164 through the node of
 * masic_amd/autograd.py: EnhancementBlockFn): additionally y2 = bf16(y) * act'(mask2) -- the next layer's dy, exactly what a separate
 * g * act'(u) pass over the stored y would give -- and sum_out[Cout] = per-channel sums (a bias gradient) of the value before the residual
 * adds (sum_of = 1) or of y2 (sum_of = 2), bf16-rounded as stored, from per-wave partials in sum_workspace
 * (masic_conv3x3_resident_sum_workspace_bytes()) by a fixed-order finishing launch.  mask2 / y2: res_ctot-channel tensors. */
size_t masic_conv3x3_resident_sum_workspace_bytes(void);
int masic_conv3x3_resident_ex_fwd(const void* x_f16k, const void* w_packed, const float* bias, const void* res1, const void* res2, int res_ctot,
                                  const void* mask, float mask_slope, void* y_pre_f16k, void* y_f16k, const void* mask2, float mask2_slope,
                                  void* y2_f16k, int sum_of, float* sum_out, void* sum_workspace, int B, int Cin, int Cout, int H, int W,
                                  int in_ctot, int in_coff, int out_ctot, int out_coff, int act, void* stream);
/* diagnostics: 16 uint64 on the device, filled by every following conv_f16k launch with {core-clock, 100 MHz} stamp pairs at kernel
 * entry, K-loop entry, K-loop exit and kernel exit of its first and of its last workgroup; NULL switches it off (tools/f16k_stamps.py) */
void masic_conv_f16k_set_stamps(void* device_buffer);
/* a layer with few output channels (Independent_EN.conv2: 96 -> 3 + the picture as residual, MASIC.py:1492-1496) on the same kernels:
 * `d` describes the convolution with its weight zero-padded to Cout = 32; y_nchw / res32 are float32 [B][cout_store][Ho][Wo]. */
int masic_conv_f16k_few_fwd(const void* x_f16k, const void* w_packed, const float* bias, const float* res32, float* y_nchw,
                            int cout_store, const masic_conv_desc_t* d, void* stream);
/* layout-side helpers of those chains (masic_amd/csrc/f16k_ops.hip):
 *   masic_f16k_gate           dst[:, dst_coff : dst_coff+C] = (minv ? warp_perspective(src, minv) : src) * (gate ? gate[:, gate_c] : 1)
 *                             -- the gated concats of MASIC.py:1470-1482 written straight into their slice of the F16K buffer
 *   masic_nchw_to_f16k_view   float32 NCHW channel view -> a channel slice of an F16K buffer
 *   masic_f16k_to_nchw        F16K channel slice -> float32 NCHW channel view */
int masic_f16k_gate(const void* src, const float* gate, const float* minv, void* dst, int B, int C, int H, int W,
                    int dst_ctot, int dst_coff, int gate_ctot, int gate_c, void* stream);
int masic_nchw_to_f16k_view(const float* x, void* y, int B, int C, int HW, int ctot, int coff, int dst_ctot, int dst_coff, void* stream);
/* ... with |x| / round(x) (in_op) applied and an optional gate[b][gate_c][pixel] (float32 [B][gate_ctot][HW]) multiplied in before the
 * rounding to bf16: round(y) * gate into its slice of an F16K concat buffer (the gated concat of MASIC.py:827). */
int masic_nchw_to_f16k_view_op(const float* x, void* y, int B, int C, int HW, int ctot, int coff, int dst_ctot, int dst_coff, int in_op,
                               const float* gate, int gate_ctot, int gate_c, void* stream);
int masic_f16k_to_nchw(const void* x, float* y, int B, int C, int HW, int src_ctot, int src_coff, int ctot, int coff, void* stream);
int masic_f16k_to_nchw_bf16(const void* x, void* y, int B, int C, int HW, int src_ctot, int src_coff, int ctot, int coff, void* stream);   /* y: bf16 NCHW */

size_t masic_conv_a_packed_bytes(void);
int masic_conv_a_pack_weight(const float* w, void* w_packed, void* stream);
int masic_conv_a_gdn_fwd(const float* x, const void* w_packed, const float* bias, const void* gdn_packed, int gdn_inverse,
                         void* y_f16k, int B, int Hi, int Wi, int in_ctot, int in_coff, void* stream);

/* ------------------------------------------------------------------------------------------
 * GDN / inverse GDN: compressai/layers/gdn.py:77-92 with the NonNegativeParametrizer of
 * compressai/ops/parametrizers.py:47-64 applied to the *stored* beta[C], gamma[C,C] inside the
 * kernel: y = x * rsqrt(beta^ + gamma^ . x^2)  (inverse: * sqrt).  beta_min as gdn.py:57.
 */
int masic_gdn_fwd(const float* x, const float* beta, const float* gamma, float* y,
                  int B, int C, int H, int W, int inverse, double beta_min, void* stream);
/* prec = MASIC_PREC_BF16: the C x C contraction runs as a bf16x3 split product (gamma^ and x^2 as bf16 hi+lo, float32
 * accumulate, ~2^-16 relative) at 16/3 of the f32 matrix rate -- HBM-bound; MASIC_PREC_F32: exact float32 MFMA */
int masic_gdn_fwd_ex(const float* x, const float* beta, const float* gamma, float* y,
                     int B, int C, int H, int W, int inverse, double beta_min, int prec, void* stream);
/* Simplified GDN ("GDN1", compressai/layers/gdn.py:95-121): y_i = x_i / (beta^_i + sum_j gamma^_ij |x_j|) (inverse: multiply); float32, any C */
int masic_gdn1_fwd(const float* x, const float* beta, const float* gamma, float* y,
                   int B, int C, int H, int W, int inverse, double beta_min, void* stream);
/* Same, C = 128 only, result written as F16K bf16 [B][8][H*W][16] for masic_conv_f16k_fwd (bf16x3 contraction). */
int masic_gdn_fwd_f16k(const float* x, const float* beta, const float* gamma, void* y_f16k,
                       int B, int C, int H, int W, int inverse, double beta_min, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quantisation: compressai/entropy_models/entropy_models.py:98-125 with means=None.
 *   mode 3 'copy'      : y = x             (used with the gate / output view: x*w into a torch.cat slice, MASIC.py:1470-1482)
 *   mode 0 'dequantize': y = round(x)      (torch.round: half to even)
 *   mode 1 'noise'     : y = x + noise     (noise drawn by the caller, same shape)
 *   mode 2 'symbols'   : sym = (int32) round(x - median[c])   (median may be NULL -> 0)
 * Optional gate as above (y *= gate[b,gate_c,h,w]); output view as for convs.
 */
int masic_quantize_fwd(const float* x, const float* noise, const float* gate, float* y,
                       int B, int C, int H, int W, int out_ctot, int out_coff,
                       int gate_ctot, int gate_c, int mode, void* stream);
int masic_symbols_fwd(const float* x, const float* median, int32_t* sym,
                      int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * EntropyBottleneck.forward: entropy_models.py:384-411 (+ _likelihood :372-382,
 * _logits_cumulative :350-369, LowerBound 1e-9).  z [B,C,H,W]; params are the module's raw
 * parameters, concatenated per channel by the host into one table [C, 58]:
 *   matrices (3 + 9 + 9 + 9 + 3), biases (3 + 3 + 3 + 3 + 1), factors (3 + 3 + 3 + 3)
 * (filters (3,3,3,3), entropy_models.py:258); medians = quantiles[:,0,1].
 * training=1: z_hat = z + noise, noise given in the reference's draw layout (C, 1, B*H*W)
 * (entropy_models.py:386-394); training=0: z_hat = round(z - med) + med.
 */
#define MASIC_EB_PARAMS_PER_CHANNEL 58
int masic_entropy_bottleneck_fwd(const float* z, const float* params, const float* medians,
                                 const float* noise, float* z_hat, float* lik,
                                 int B, int C, int H, int W, int training, float lik_bound, void* stream);
/* The same with the medians read at a stride of median_stride floats: (&quantiles[0][0][1], 3) reads them in place from the
 * quantiles parameter [C][1][3] instead of from a contiguous copy made in front of every call. */
int masic_entropy_bottleneck_strided_fwd(const float* z, const float* params, const float* medians, int median_stride,
                                         const float* noise, float* z_hat, float* lik,
                                         int B, int C, int H, int W, int training, float lik_bound, void* stream);
/* EntropyBottleneck.loss(): entropy_models.py:345-348. out[0] = sum |logits(quantiles) - target| */
int masic_entropy_bottleneck_auxloss(const float* params, const float* quantiles, float* out,
                                     int C, double tail_mass, void* stream);

/* ------------------------------------------------------------------------------------------
 * GaussianMixtureConditional_gf.forward: entropy_models.py:808-858.
 *   y_hat = quantize(y) (mode as masic_quantize_fwd 0/1), K-component mixture likelihood with
 *   sigma lower-bounded at scale_bound (0.11) and the result at lik_bound (1e-9).
 * sigma, mu, wts: [B, K*M, H, W], component k of channel m at k*M+m (MASIC.py:389-393).
 * weights_are_logits=1 fuses the softmax over K of MASIC.py:389-393/459-464 into the kernel
 * (wts then holds the raw gmm_weights head output, and wts_out, if non-NULL, receives the
 * normalised weights).
 * training: 0 round(y), 1 y + noise, 2 y is the quantised latent already -- likelihood only
 * (the training forward draws y + noise where the reference does and evaluates the likelihood beside the synthesis transform).
 * y_hat may be NULL in every mode: the quantised latent is then not stored (the eval forward only keeps the likelihood); lik is
 * the same bit for bit.
 */
int masic_gmm_likelihood_fwd(const float* y, const float* noise, const float* sigma, const float* mu,
                             const float* wts, float* y_hat, float* lik, float* wts_out,
                             int B, int M, int K, int H, int W, int training, int weights_are_logits,
                             float scale_bound, float lik_bound, void* stream);
/* softmax over K on the (B,K,M,H,W) view: MASIC.py:389-393 */
int masic_softmax_k_fwd(const float* x, float* y, int B, int M, int K, int HW, void* stream);

/* ------------------------------------------------------------------------------------------
 * Perspective warp: kornia==0.5.0 warp_perspective(src, M, dsize) as called at
 * MASIC.py:638,644,781,821,833 (bilinear, zeros padding, align_corners=True).
 * minv_norm [B,3,3] = inverse(N_dst . M . N_src^-1) (normalised coordinates), computed by
 * masic_warp_matrix from the pixel-space M [B,3,3] in float64 and rounded to float32.
 * src NULL => warp an all-ones image (the mask of MASIC.py:636-638) with C=1.
 */
int masic_warp_matrix(const float* M, float* minv_norm, int B, int Hs, int Ws, int Hd, int Wd,
                      int invert_first, void* stream);
/* grid_sample convention of every warp of the library (forward, backward, masic_f16k_gate): 1 = align_corners=True -- kornia 0.5.0's
 * warp_perspective default, what the reference's pinned dependency runs (readme.md:12) and this library's default; 0 =
 * align_corners=False (kornia <= 0.4.1).  kornia is not vendored in the reference and no reference test pins a result at this
 * boundary, so the convention stays selectable.  Process-wide; set once before the first forward. */
void masic_set_warp_align_corners(int align_corners);
int masic_get_warp_align_corners(void);
int masic_warp_perspective_fwd(const float* src, const float* minv_norm, float* dst,
                               int B, int C, int Hs, int Ws, int Hd, int Wd,
                               int out_ctot, int out_coff, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small elementwise / reduction helpers.
 *   mul_inplace : MaskedConv2d's `weight.data *= mask` (layers.py:77)
 *   copy_view   : write a [B,C,H,W] tensor into a channel slice of a wider buffer (torch.cat)
 *   sum_log / sse : the reductions of RateDistortionLoss (newtrain_codec_real.py:79-83):
 *                   out[0] = sum(log(x)), out[0] = sum((a-b)^2); deterministic two-stage, fp64 final.
 *   workspace: at least masic_reduce_workspace_bytes() bytes.
 */
int masic_mul_inplace(float* x, const float* m, size_t n, void* stream);
/* LowerBound / LowerBoundFunction: compressai/ops/bound_ops.py:36-56 (standalone form; the hot path
 * fuses the bound into the GDN / EB / GMM kernels) */
int masic_lower_bound_fwd(const float* x, float* y, float bound, size_t n, void* stream);
int masic_lower_bound_bwd(const float* x, const float* g, float* gx, float bound, size_t n, void* stream);
int masic_copy_view(const float* x, float* y, int B, int C, int HW, int out_ctot, int out_coff, void* stream);
size_t masic_reduce_workspace_bytes(void);
int masic_sum_log(const float* x, size_t n, double* out, void* workspace, void* stream);
int masic_sse(const float* a, const float* b, size_t n, double* out, void* workspace, void* stream);
/* The rate-distortion criterion of the training step (newtrain_codec_real.py:73-87) in two launches: loss (float32) =
 * cm (mse1 + mse2) + bpp, mse_i = sum (x_i_hat - x_i)^2 / n_pic, bpp = cb sum_k sum log lik_k, per[k] = cb sum log lik_k (float64 device
 * scalars); nliks <= 4 (0: the distortion-only criterion of the CQE stage, newtrain_cqe_real.py:66-96).  Sums in the order of masic_sse /
 * masic_sum_log.  workspace: masic_rd_loss_workspace_bytes().  masic_rd_loss_bwd: its gradients times the float32 device scalar g in one
 * launch: g_x_i = (s_pic (x_i_hat - x_i)) g, g_liks[k] = (s_lik / lik_k) g. */
size_t masic_rd_loss_workspace_bytes(void);
int masic_rd_loss(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                  const float* const* liks, const size_t* lik_n, int nliks, double cb, double cm,
                  float* loss, double* mse1, double* mse2, double* bpp, double* const* per, void* workspace, void* stream);
int masic_rd_loss_bwd(const float* x1_hat, const float* x1, const float* x2_hat, const float* x2, size_t n_pic,
                      const float* const* liks, const size_t* lik_n, int nliks, float s_pic, float s_lik, const float* g,
                      float* g_x1, float* g_x2, float* const* g_liks, void* stream);

/* ==========================================================================================
 * Backward entry points (what torch autograd derives for the reference graph).
 * ========================================================================================== */

/* Weight gradient of Conv2d / ConvTranspose2d (same descriptor as the forward layer):
 *   Conv2d:          dW[co,ci,kh,kw] = sum_{b,oh,ow} dy[b,co,oh,ow] * x[b,ci,oh*s+kh-p,ow*s+kw-p]
 *   ConvTranspose2d: dW[ci,co,kh,kw] = sum_{b,ih,iw} x[b,ci,ih,iw] * dy[b,co,ih*s+kh-p,iw*s+kw-p]
 * x is the forward input view (in_ctot/in_coff of desc), dy a contiguous [B,Cout,Ho,Wo] tensor.
 * Pixel tiles are reduced with float atomics into `workspace` (>= masic_conv2d_wgrad_workspace_bytes(d) bytes)
 * and then transposed into dw (weight layout).
 * Input gradients need no entry point of their own: dx of a Conv2d is masic_conv2d_fwd with transposed=1 and
 * Cin/Cout swapped on the same weight tensor (and vice versa), see masic_amd/autograd.py. */
size_t masic_conv2d_wgrad_workspace_bytes(const masic_conv_desc_t* d);
/* workspace_clean 0: the call zero-fills the workspace itself (a kernel launch) and leaves it dirty.  != 0: a caller-owned PERSISTENT
 * workspace -- zeros promised on entry, zeros back on exit (the last pass of the call re-zeroes what it reads), so a training step's
 * ~80 weight gradients need no fill launch each. */
int masic_conv2d_wgrad_ws(const float* x, const float* dy, float* dw, void* workspace, const masic_conv_desc_t* d, int workspace_clean,
                          void* stream);
/* The 5x5 stride-2 layers of the bf16 mode with bf16 NCHW operands (x: [B][in_ctot][Hi][Wi], dy: [B][Cout][Ho][Wo], both bf16): the
 * GDN backward writes dx that way (masic_gdn_bwd_fused_ex2) and the saved F16K activations are converted that way
 * (masic_f16k_to_nchw_bf16) -- half the bytes of the float32 tensors on every side of the kernel. */
int masic_conv2d_wgrad_bf16in_supported(const masic_conv_desc_t* d);
int masic_conv2d_wgrad_bf16in(const void* x_bf16, const void* dy_bf16, float* dw, void* workspace, const masic_conv_desc_t* d,
                              int workspace_clean, void* stream);

/* y = op(a, b) elementwise over n floats; ops (s0,s1 scalars):
 *   0 act_bwd (a=grad, b=activation output, s0=MASIC_ACT_*)   1 abs_bwd (a=grad, b=x)   2 square   3 abs
 *   4 axpy s0*a+s1*b (b may be NULL)   5 s0/a   6 s0*(a-b)   7 a*b
 *   8 reparam max(a,s0)^2-s1 (parametrizers.py:61-64)   9 reparam_bwd (a=grad, b=stored param, s0=bound; incl. LowerBound rule)
 *   10 a+b */
int masic_elementwise(const float* a, const float* b, float* y, size_t n, int op, float s0, float s1, void* stream);
/* out[c] = sum over batch and pixels of channel coff+c of x[B,ctot,HW]  (bias / beta gradients; deterministic two-stage
 * reduction through `workspace` >= masic_channel_sum_workspace_bytes(C) bytes) */
size_t masic_channel_sum_workspace_bytes(int C);
int masic_channel_sum(const float* x, float* out, void* workspace, int B, int C, int HW, int ctot, int coff, void* stream);
/* y[B,C,HW] = x[B,ctot,HW][:, coff:coff+C]  (backward of copy_view / torch.cat) */
int masic_slice_copy(const float* x, float* y, int B, int C, int HW, int ctot, int coff, void* stream);
/* backward of y = x * gate[:,gate_c]: gx = g*gate, ggate[:,gate_c] = sum_c g*x (other gate channels untouched) */
int masic_gate_bwd(const float* g, const float* x, const float* gate, float* gx, float* ggate,
                   int B, int C, int HW, int gate_ctot, int gate_c, void* stream);
int masic_softmax_k_bwd(const float* g, const float* y, float* gx, int B, int M, int K, int HW, void* stream);
/* GDN backward, elementwise pieces (gdn.py:77-92; the three CxC contractions run on the conv / wgrad kernels):
 *   pre : s = g*n^(-1/2), t = dL/dn = -1/2 g x n^(-3/2)   (inverse: s = g*n^(1/2), t = +1/2 g x n^(-1/2))
 *   post: dx = s + 2 x u,  u = gamma^T t */
int masic_gdn_bwd_pre(const float* x, const float* nrm, const float* g, float* s, float* t, size_t n, int inverse, void* stream);
int masic_gdn_bwd_post(const float* x, const float* s, const float* u, float* dx, size_t n, void* stream);
/* The same backward for C <= 4 (MASIC.py:560 pre_gdn, :575 after_gdn: GDN(3) on full-resolution pictures) in one pass: float32
 * per-pixel algebra in registers, parameter sums reduced in float64 in a fixed order.  beta [C], gamma [C][C]: the STORED tensors;
 * g_beta, g_gamma: gradients with respect to them (reparametrisation rules included, as masic_gdn_bwd_fused). */
size_t masic_gdn_bwd_small_workspace_bytes(void);
int masic_gdn_bwd_small(const float* x, const float* g, const float* beta, const float* gamma, float* gx, float* g_beta,
                        float* g_gamma, void* workspace, int B, int C, int H, int W, int inverse, double beta_min, void* stream);
/* The whole GDN / inverse-GDN backward (gdn.py:77-92 under autograd, C = 128) in one pass over x and g = dL/dy, bf16
 * operands on the matrix cores with float32 accumulation -- the training step of the bf16-operand mode; the pieces above
 * remain the float32 parity path.  beta, gamma: the STORED tensors; g_beta [128], g_gamma [128][128]: gradients with
 * respect to them (NonNegativeParametrizer + LowerBound rules, parametrizers.py:61-64, bound_ops.py:40-42, included).
 * workspace: masic_gdn_bwd_fused_workspace_bytes() bytes of device memory. */
size_t masic_gdn_bwd_fused_workspace_bytes(void);
int masic_gdn_bwd_fused(const float* x, const float* g, const float* beta, const float* gamma, float* gx,
                        float* g_beta, float* g_gamma, void* workspace, int B, int C, int H, int W, int inverse,
                        double beta_min, void* stream);
/* The same with F16K operands: exactly one of x / x_f16k and of g / g_f16k (float32 NCHW or F16K bf16 [B][8][HW][16]); dx goes to
 * gx (float32 NCHW) and / or gx_f16k; g_sum [128] (or NULL) receives the per-channel sums of dx over batch and pixels -- the bias
 * gradient of the convolution in front of the GDN (autograd of `conv -> GDN`, reference MASIC.py:515-529, :538-552). */
int masic_gdn_bwd_fused_ex(const float* x, const void* x_f16k, const float* g, const void* g_f16k, const float* beta, const float* gamma,
                           float* gx, void* gx_f16k, float* g_sum, float* g_beta, float* g_gamma, void* workspace,
                           int B, int C, int H, int W, int inverse, double beta_min, void* stream);
/* ... with one more output: gx_bf16 (or NULL) = dx as bf16 NCHW [B][128][H][W], the operand of masic_conv2d_wgrad_bf16in. */
int masic_gdn_bwd_fused_ex2(const float* x, const void* x_f16k, const float* g, const void* g_f16k, const float* beta, const float* gamma,
                            float* gx, void* gx_f16k, void* gx_bf16, float* g_sum, float* g_beta, float* g_gamma, void* workspace,
                            int B, int C, int H, int W, int inverse, double beta_min, void* stream);
/* GaussianMixtureConditional_gf backward (entropy_models.py:808-858 + both LowerBound rules, bound_ops.py:40-42).
 * y_hat as returned by the forward; g_yhat may be NULL; weights_are_logits as in the forward. */
int masic_gmm_likelihood_bwd(const float* y_hat, const float* sigma, const float* mu, const float* wts,
                             const float* g_lik, const float* g_yhat, float* g_y, float* g_sigma, float* g_mu,
                             float* g_w, int B, int M, int K, int H, int W, int weights_are_logits,
                             float scale_bound, float lik_bound, void* stream);
/* EntropyBottleneck backward: g_z [B,C,H,W] and g_params [C,58] (same table layout as the forward) */
int masic_entropy_bottleneck_bwd(const float* z_hat, const float* params, const float* g_lik, const float* g_zhat,
                                 float* g_z, float* g_params, int B, int C, int H, int W, float lik_bound, void* stream);
/* Gradient of the [C][58] parameter table (torch.cat of the 14 per-channel tensors of an EntropyBottleneck, reference
 * entropy_models.py:289-300) split into the parameters' gradients in one launch: part t (width widths[t]) becomes the contiguous
 * block [C][widths[t]] at flat + C * (widths[0] + ... + widths[t-1]). */
int masic_eb_table_split(const float* g_table, float* flat, int C, const int* widths, int nparts, void* stream);
int masic_entropy_bottleneck_auxloss_bwd(const float* params, const float* quantiles, float* g_quantiles,
                                         int C, double tail_mass, float gout, void* stream);
/* The auxiliary step's loss and gradient (newtrain_codec_real.py:143-145: sum of EntropyBottleneck.loss() over the model's bottlenecks,
 * backward) for n <= 4 bottlenecks in two launches.  params[e]: [C[e]][58] tables, quantiles[e] / g_quantiles[e]: [C[e]][3];
 * loss[0] = total, loss[1 + e] = bottleneck e; workspace: >= n * 3 * max C floats. */
int masic_entropy_bottleneck_aux_step(const float* const* params, const float* const* quantiles, float* const* g_quantiles,
                                      const int* C, const double* tail_mass, int n, float* loss, float* workspace, int workspace_floats,
                                      void* stream);
/* warp backward w.r.t. the source image; g_src [B,C,Hs,Ws] must be ZERO-FILLED by the caller (float atomics) */
int masic_warp_perspective_bwd(const float* g_dst, const float* minv_norm, float* g_src,
                               int B, int C, int Hs, int Ws, int Hd, int Wd, void* stream);
/* The same adjoint (autograd's backward of kornia.warp_perspective -> F.grid_sample, reference MASIC.py:781, :1461-1480) as a gather over
 * source pixels: no atomics, a fixed summation order, g_src written once and needing NO zero fill.  flag: one int32 on the device, zero
 * on entry; set to 1 when some source pixel's footprint was outside the gather form's bounds (horizon inside the picture, magnification
 * beyond ~2 x) -- the call has then redone the whole tensor with the scatter form above (device-side test of the flag, no host round trip). */
int masic_warp_perspective_bwd_gather(const float* g_dst, const float* minv_norm, float* g_src, int* flag,
                                      int B, int C, int Hs, int Ws, int Hd, int Wd, void* stream);
/* ---- the warp differentiated with respect to its matrix (warp_bwd_matrix.hip): kornia.warp_perspective is differentiable in the
 * homography, and so is HSIC.forward in h_matrix.  No float atomics anywhere: bit-reproducible, and an item's result does not
 * depend on the batch around it.
 *   masic_warp_perspective_bwd_matrix  part [B][slots][9] (float64, slots = masic_warp_matrix_slots(Hd, Wd)): per-workgroup partial
 *                                      sums of d loss / d minv_norm of dst = warp(src; minv_norm) for the incoming gradient g_dst
 *                                      [B][C][Hd][Wd]; src NULL => the all-ones source (C = 1).  The sampling coordinates are the
 *                                      forward's own (same float32 operations, masic_set_warp_align_corners included), so the
 *                                      bilinear derivative is that of the cell the forward sampled (one-sided on cell boundaries);
 *                                      a destination pixel with non-finite coordinates contributes 0.  g_minv [B][3][3] (or NULL):
 *                                      the slots added in a fixed order by a second launch (one wave per item), rounded once to float32.
 *   masic_warp_matrix_bwd              the adjoint of masic_warp_matrix: g_M [B][3][3] from g_fwd [B][slots_fwd][9], the gradient of
 *                                      inverse(N_dst M N_src^-1), and / or g_inv [B][slots_inv][9], that of the invert_first chain
 *                                      (either may be NULL); the slots are float64 (slots_f64 = 1) or float32 (0) and are added in
 *                                      a fixed order (one wave per item: lane l takes slots l, l + 64, ..., then a butterfly); float64 inside, the chain re-evaluated at M.  NaN rows for a singular chain.
 *   masic_homography_from_corners_bwd  the adjoint of masic_homography_from_corners with respect to delta: g_h [B][3][3] ->
 *                                      g_delta [B][4][2] (h_adjust's scalings, the cofactor inverse, the 8 x 8 solve by implicit
 *                                      differentiation); NaN rows where the forward gives NaN. */
int masic_warp_matrix_slots(int Hd, int Wd);
int masic_warp_perspective_bwd_matrix(const float* src, const float* minv_norm, const float* g_dst, double* part, float* g_minv,
                                      int B, int C, int Hs, int Ws, int Hd, int Wd, void* stream);
int masic_warp_matrix_bwd(const float* M, const void* g_fwd, int slots_fwd, const void* g_inv, int slots_inv, int slots_f64, float* g_M,
                          int B, int Hs, int Ws, int Hd, int Wd, void* stream);
int masic_homography_from_corners_bwd(const float* corners, const float* delta, const float* g_h, float* g_delta, int B, float scale_a,
                                      float scale_b, void* stream);

/* ------------------------------------------------------------------------------------------
 * Host-side entropy coding (no device work).  Bit-exact replacements of the reference's pybind11
 * extensions: compressai/cpp_exts/ops/ops.cpp:41-106 (pmf_to_quantized_cdf) and compressai/cpp_exts/rans/
 * rans_interface.cpp:108-283 (RansEncoder.encode_with_indexes / RansDecoder.decode_with_indexes: rANS with a 64-bit
 * state, 32-bit renormalisation, 16-bit probabilities, 4-bit bypass digits for symbols outside a table).
 *   cdfs: ncdfs rows of cdf_stride int32; row i holds cdf_sizes[i] entries 0 = c[0] < ... < c[size-1] = 65536; its last
 *   symbol (size-2) is the escape.  A coded value is symbols[k] - offsets[indexes[k]].
 *   masic_rans_encode_bound(n) bytes always suffice for n symbols; *out_len receives the stream length. */
int masic_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* cdf /* n + 1 */);
size_t masic_rans_encode_bound(int nsymbols);
int masic_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, int n, const int32_t* cdfs, int cdf_stride,
                                   const int32_t* cdf_sizes, const int32_t* offsets, int ncdfs, uint8_t* out, size_t out_cap,
                                   size_t* out_len);
int masic_rans_decode_with_indexes(const uint8_t* in, size_t in_len, const int32_t* indexes, int n, const int32_t* cdfs,
                                   int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdfs, int32_t* symbols);

/* ---- upstream of the path, SURVEY.md 8(f)-3: h_matrix of a stereo pair from the UDH network's corner offsets --
 * udh/udh/model.py:100-111 (kornia.get_perspective_transform(corners, corners + delta), torch.inverse) + h_adjust
 * (newtrain_codec_real.py:49-59, scale_a = H / patch, scale_b = W / patch).  corners, delta: [B][4][2]; h_out: [B][3][3],
 * NaN for a degenerate quadrilateral. */
int masic_homography_from_corners(const float* corners, const float* delta, float* h_out, int B, float scale_a, float scale_b,
                                  void* stream);

/* ---- the UDH homography net itself (coremasic/mywork/model.py: Net), float32 throughout, fixed accumulation order, no float
 * atomics; a result row does not depend on the other rows of the batch.  Layers 2-8 are masic_conv2d_fwd_ex with MASIC_ACT_RELU.
 * All pointers device memory; asynchronous on `stream`; capturable into a HIP graph.
 *   masic_udh_conv1_fwd      y[B][Cout][H][W] = relu(conv3x3_pad1(cat(a, b)) + bias): a, b [B][1][H][W], w [Cout][2][3][3]
 *                            (the Conv2d weight as it is), Cout a multiple of 16.
 *   masic_maxpool2_fwd       MaxPool2d(2, 2) of `planes` planes of H x W (both even) -> H/2 x W/2; NaN propagates.
 *   masic_udh_fc_fwd         hidden[B][N] = relu(x[B][K] . w1[N][K]^T + b1), out[B][M] = hidden . w2[M][N]^T + b2.  w1 is read once
 *                            per group of <= 8 rows of x.  K a multiple of 512, N a multiple of 128; x and w1 16-byte aligned;
 *                            workspace: masic_udh_fc_workspace_bytes(B, K, N) bytes (the split-K partial sums; 0 = bad shape);
 *                            hidden may be NULL.
 *   masic_udh_shift_corners  out[b][k] = corners[b][k] - corners[b][0] for [B][4][2] corners (newtrain_codec_real.py:123). */
int masic_udh_conv1_fwd(const float* a, const float* b, const float* w, const float* bias, float* y, int B, int H, int W, int Cout,
                        void* stream);
int masic_maxpool2_fwd(const float* x, float* y, int planes, int H, int W, void* stream);
size_t masic_udh_fc_workspace_bytes(int B, int K, int N);
int masic_udh_fc_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, void* workspace,
                     float* hidden, float* out, int B, int K, int N, int M, void* stream);
int masic_udh_shift_corners(const float* corners, float* out, int B, void* stream);

/* ---- training the UDH homography net (udh/udh/train.py: Net + photometric_loss; masic_amd/csrc/udh_train.hip).  Float32, no float
 * atomics, every sum in a fixed order.  Masks are uint8 keep-bits (Dropout(0.5): kept values are scaled by 2); a NULL mask = no dropout.
 *   masic_maxpool2_relu_bwd   gx[planes][H][W]: gy[planes][H/2][W/2] at the first maximum of relu(x) in each 2 x 2 window (scan
 *                             order, as max_pool2d's backward), times [x > 0]; zeros elsewhere.  x may be the layer's output before or
 *                             after its ReLU.
 *   masic_udh_conv1_wgrad     dw[Cout][2][3][3], db[Cout] of masic_udh_conv1_fwd from a, b [B][1][H][W] and dy [B][Cout][H][W] (the
 *                             gradient in front of the ReLU); Cout a multiple of 4; workspace: ..._workspace_bytes (0 = bad shape).
 *   masic_udh_dropout_fwd     y = mask ? 2 x : 0 for n floats (n a multiple of 4).
 *   masic_udh_fc_train_fwd    masic_udh_fc_fwd on the (already dropped) input x, then out = (2 m2 hidden) . w2^T + b2; hidden [B][N] is
 *                             the activation before its dropout.  Same shapes and workspace as masic_udh_fc_fwd.  The inference
 *                             entry point runs whole and unchanged, so the second layer is computed twice (B x N x M, negligible) and
 *                             `out` holds the unmasked value until the masked kernel, next on the stream, overwrites it.
 *   masic_udh_fc_bwd          from gout [B][M], the dropped input xd [B][K], hidden [B][N], the masks m1 [B][K] / m2 [B][N] (or NULL),
 *                             w1 [N][K], w2 [M][N]: gw2, gb2, gb1, and in one streaming pass over w1 (per 32 batch rows) gw1 [N][K] and
 *                             gx [B][K] = 2 m1 (g_h . w1).  K a multiple of 256, N of 16; workspace: masic_udh_fc_bwd_workspace_bytes.
 *   masic_udh_photo_matrix    S[B][3][3] = inverse(N_dst inverse(h) N_src^-1), h = get_perspective_transform(corners - corners[:, :1],
 *                             corners + delta) (udh/udh/model.py:18-30), the matrix masic_warp_perspective_fwd samples with; source
 *                             Hs x Ws, output Hd x Wd; NaN rows for an exactly singular system (a zero pivot or determinant in float64, as
 *                             masic_homography_from_corners); a quadrilateral degenerate only up to rounding gives huge finite rows.
 *   masic_udh_photo_matrix_bwd  its adjoint: gS [B][slots][9] (slots added in index order) -> gdelta [B][4][2].
 *   masic_udh_photo_loss_fwd  loss[0] = mean |warp(img [B][1][Hs][Ws]; S) - patch_b [B][1][Hd][Wd]|, the sampling arithmetic of
 *                             masic_warp_perspective_fwd (zeros padding, masic_set_warp_align_corners); workspace: B * slots floats,
 *                             slots = masic_udh_photo_slots(Hd, Wd).
 *   masic_udh_photo_loss_bwd  gS_part [B][slots][9] from gloss[0] (device memory): sign(diff) gloss / count times grid_sample's
 *                             coordinate derivative, chained through the homogeneous divide (eps = 1e-8 rule included). */
int masic_maxpool2_relu_bwd(const float* x, const float* gy, float* gx, int planes, int H, int W, void* stream);
size_t masic_udh_conv1_wgrad_workspace_bytes(int B, int H, int W, int Cout);
int masic_udh_conv1_wgrad(const float* a, const float* b, const float* dy, void* workspace, float* dw, float* db, int B, int H, int W,
                          int Cout, void* stream);
int masic_udh_dropout_fwd(const float* x, const unsigned char* mask, float* y, size_t n, void* stream);
int masic_udh_fc_train_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const unsigned char* m2,
                           void* workspace, float* hidden, float* out, int B, int K, int N, int M, void* stream);
size_t masic_udh_fc_bwd_workspace_bytes(int B, int N);
int masic_udh_fc_bwd(const float* gout, const float* xd, const float* hidden, const unsigned char* m1, const unsigned char* m2,
                     const float* w1, const float* w2, void* workspace, float* gw1, float* gb1, float* gw2, float* gb2, float* gx,
                     int B, int K, int N, int M, void* stream);
int masic_udh_photo_matrix(const float* corners, const float* delta, float* S, int B, int Hs, int Ws, int Hd, int Wd, void* stream);
int masic_udh_photo_matrix_bwd(const float* corners, const float* delta, const float* gS, float* gdelta, int B, int slots, int Hs, int Ws,
                               int Hd, int Wd, void* stream);
int masic_udh_photo_slots(int Hd, int Wd);
int masic_udh_photo_loss_fwd(const float* img, const float* S, const float* patch_b, void* workspace, float* loss, int B, int Hs, int Ws,
                             int Hd, int Wd, void* stream);
int masic_udh_photo_loss_bwd(const float* img, const float* S, const float* patch_b, const float* gloss, float* gS_part, int B, int Hs, int Ws,
                             int Hd, int Wd, void* stream);

/* ---- host data path, SURVEY.md 8(f)-4: one view of a dataset item (compressai/datasets/utils.py:207-285) from the decoded
 * uint8 RGB picture [H][W][3] on the device: pic_chw (nullable) = the crop [start_h : +ph, start_w : +pw] as float32
 * [3][ph][pw] / 255 (ToTensor); homo_patch (nullable) = the [homopatch][homopatch] window at (patch_x, patch_y) of
 * mean_c(Normalize(ToTensor(cv2.resize(crop, (homopic, homopic))))) -- uint8 INTER_LINEAR resize with OpenCV's fixed-point
 * arithmetic (2x decimation = rounded 2x2 box mean), scalar MEAN / STD of utils.py:26-27. */
int masic_pair_prep(const uint8_t* img_hwc, int H, int W, int start_h, int start_w, int ph, int pw, float* pic_chw,
                    int homopic, int patch_x, int patch_y, int homopatch, float* homo_patch, void* stream);

/* ---- the two ends of the stereo file pipeline (masic_amd/stereofile.py), over a stack of P pictures per launch.
 *   masic_pairs_prep    uint8 [P][H0][W0][3] -> planes (nullable) float32 [P][3][H][W], H >= H0, W >= W0: u8 / 255 inside the picture
 *                       (the division of masic_pair_prep's crop), the last row and column replicated outside it; patches (nullable)
 *                       float32 [P][homopatch][homopatch]: masic_pair_prep's homo_patch of each WHOLE, unpadded picture.  One launch each.
 *   masic_planes_to_u8  float32 [P][3][H][W] -> uint8 [P][H0][W0][3], H0 <= H, W0 <= W: floor(min(max(x, 0), 1) * 255 + 0.5) in float32
 *                       (two roundings, no fused multiply-add: torchvision's save_image); NaN -> 0.  Inverts masic_pairs_prep exactly.
 * Buffers 4-byte aligned (planes 16-byte aligned and W % 4 == 0 for the 16-byte accesses); at most 65535 pictures, rows and columns.
 * MASIC_ERR_ARG for a null pointer, an empty extent, H0 > H or W0 > W, or a patch that leaves the resized picture. */
int masic_pairs_prep(const uint8_t* pics_hwc, int P, int H0, int W0, int H, int W, float* planes, int homopic, int patch_x, int patch_y,
                     int homopatch, float* patches, void* stream);
int masic_planes_to_u8(const float* planes, int P, int H, int W, int H0, int W0, uint8_t* pics_hwc, void* stream);

/* ---- the training batch of a device-resident dataset (masic_amd/data.py): masic_pair_prep for P views at once, each view its own crop
 * of its own picture, in one launch for the crops and one for the patches whatever P is.
 *   arena      uint8, 4-byte aligned, arena_bytes % 4 == 0: the decoded pictures back to back, picture i as [H_i][W_i][3] from a 16-byte
 *              aligned offset (so the aligned 32-bit word that holds a picture's last byte lies inside the arena)
 *   desc_dev   P descriptors in DEVICE memory, 8-byte aligned (filled by an asynchronous copy on `stream` before the call)
 *   planes     (nullable) float32 [P][3][ph][pw]: masic_pair_prep's pic_chw of view p, bit for bit; 16-byte stores when pw % 4 == 0 and the
 *              base is 16-byte aligned, scalar stores otherwise
 *   patches    (nullable) float32 [P][homopatch][homopatch]: masic_pair_prep's homo_patch of view p at (patch_x, patch_y), bit for bit
 * The library cannot read the descriptors: the caller checks each one on the host (crop inside the picture, picture inside the arena,
 * patch inside the homopic x homopic resized crop) before the call.  The kernels skip a view whose descriptor fails that check, so a bad
 * table leaves its outputs unwritten and reads nothing outside the arena.  No view's result depends on the other views of the call. */
typedef struct masic_view_desc_t {
    uint64_t offset;               /* first byte of the picture in the arena */
    int32_t W, H;                  /* the picture's row width and its rows */
    int32_t start_h, start_w;      /* top-left of the crop */
    int32_t patch_x, patch_y;      /* top-left of the patch in the resized crop */
} masic_view_desc_t;
int masic_views_prep(const uint8_t* arena, size_t arena_bytes, const masic_view_desc_t* desc_dev, int P, int ph, int pw, float* planes,
                     int homopic, int homopatch, float* patches, void* stream);

/* ---- the training batch of the homography net (UDH) out of the same arena: the item of the reference's udh/udh/dataset.py
 * (SyntheticDataset.__getitem__) for P views in one launch.  Element (r, c) of out[p] is pixel (y0 + r, x0 + c) of the
 * pic_size x pic_size grey picture
 *     mean_c(Normalize(ToTensor(CenterCrop(pic_size)(Resize(pic_size)(picture)))))
 * with Resize as PIL does it (Image.resize, BILINEAR, antialiased): a horizontal pass into uint8, then a vertical pass into uint8, each
 * `(2^21 + sum px * k) >> 22` clipped to 0 .. 255 in int32, the support growing with the scale; an axis that keeps its size gets NO pass
 * (its bytes are copied; no one-tap table is multiplied).  The grey value has the bits of masic_pair_prep's homo_patch.
 *   tables     int32 in device memory, 4-byte aligned: the coefficients, computed on the host in float64 as Pillow computes them
 *              (masic_amd/udh_data.py: pil_bilinear_tables).  One table per axis that is resized, for the pic_size output positions
 *              that survive the centre crop: xmin[pic_size], n[pic_size], k[pic_size][ksize], ksize = 2 * ceil(in / out) + 1
 *              (3 when up-scaling), 0 <= xmin, 1 <= n <= ksize, xmin + n <= the axis' input size.  The kernel computes no coefficient.
 *   desc_dev   P descriptors in DEVICE memory, 8-byte aligned
 *   out        float32 [P][out_h][out_w], 4-byte aligned; 16-byte stores when out_w % 4 == 0 and the base is 16-byte aligned
 * ceil(in / out) up to 17 per axis (ksize <= 35): Resize by up to 16 on the shorter side, the longer side's output size being rounded
 * down.  The library cannot read the descriptors: the caller checks each one on the host
 * (picture inside the arena, tables inside table_words, rectangle inside pic_size, ksize what the sizes give) before the call.  The kernel
 * checks the same again and skips a view that fails, and a tile whose table entries leave their ranges: outputs unwritten, nothing read
 * outside the arena or the tables.  No view's result depends on the other views of the call.
 * MASIC_ERR_ARG for a null pointer, an empty extent, P > 65535, a rectangle larger than pic_size or a misaligned buffer. */
typedef struct masic_udh_view_desc_t {
    uint64_t offset;               /* first byte of the picture in the arena */
    int32_t W, H;                  /* the picture's row width and its rows */
    uint32_t h_table, v_table;     /* first word of the horizontal / vertical table in `tables` (ignored when the ksize is 0) */
    int32_t h_ksize, v_ksize;      /* taps per output position; 0: the axis keeps its size, no pass and no table */
    int32_t x0, y0;                /* top-left of the out_h x out_w rectangle in the pic_size x pic_size picture */
} masic_udh_view_desc_t;
int masic_udh_views_prep(const uint8_t* arena, size_t arena_bytes, const int32_t* tables, size_t table_words,
                         const masic_udh_view_desc_t* desc_dev, int P, int out_h, int out_w, int pic_size, float* out, void* stream);

/* ---- HSIC.compress / decompress (MASIC.py:855-1408), SURVEY.md 8(f)-1: the y1 / y2 streams.
 * rANS with one table per symbol (host).  The reference drives the third-party `range_coder` package here
 * (MASIC.py:958, :1044, :1221, :1296), which is not part of its tree: the byte stream of this container is this
 * library's own (64-bit state, 32-bit renormalisation, 16-bit tables: the coder of the z streams above).
 * start_freq: [n][2] intervals in coding order.  The decoder is incremental -- the tables of a wavefront of latent pixels
 * exist only once the previous wavefront is decoded: open, decode_rows per wavefront (symbols[r] = index of the interval
 * of row r that holds the coder's value), close. */
int masic_rans_encode_freqs(const int32_t* start_freq, size_t n, uint8_t* out, size_t out_cap, size_t* out_len);
/* One rANS stream per channel -- the form the device decoder below reads (container "MSR2", masic_amd/codec.py).  start_freq:
 * [npix * nch][2], row i * nch + c = pixel i (coding order), channel c.  out: the nch streams back to back; lengths[c] bytes each
 * (multiples of 4, >= 8).  Replaces the reference's one `range_coder` stream per view (MASIC.py:1046-1140), whose bytes are parity-unpinned. */
int masic_rans_encode_channels(const int32_t* start_freq, int npix, int nch, uint8_t* out, size_t out_cap, uint32_t* lengths, size_t* out_len);
/* The entropy-parameter layers on a short pixel list (masic_amd/csrc/skinny.hip): up to three 1x1 layers (groups as in
 * masic_gemm_f16k_group_fwd, bf16 operands, w_packed from masic_gemm_f16k_pack_weight) or, with ctx != 0, ONE 5x5 type-A masked
 * convolution (w_packed from masic_skinny_ctx_pack_weight; latent h x w) evaluated at the pixels pix[(*step) * list_stride + i], i < npix
 * (step: device int or NULL), of a batch of nimg images: list entries q = b * HW + p name image b, pixel p (-1 = padding).
 * x [nimg][Cin / 16][HW][16] (exactly Cin channels per image) and the outputs [nimg][out_ctot]... are FULL-SIZE buffers: only the
 * listed pixels are written.  gate (nullable): float32 [nimg][gate_ctot][HW], plane gate_c multiplies the result after the activation.
 * A masked tap never reads another image (outside image b reads zeros, as at the picture edge).  A pixel's result depends on its own
 * operands only, whatever the list order and split: the encoder (all pixels, one launch) and the decoder (one coding wavefront per
 * launch) get bit-identical parameters, for one image or many.  Replaces the per-symbol crop + Conv2d calls of MASIC.py:986-1003 /
 * :1262-1280. */
size_t masic_skinny_ctx_packed_bytes(int Cin, int Cout);
int masic_skinny_ctx_pack_weight(const float* w, void* w_packed, int Cin, int Cout, void* stream);
int masic_skinny_group_fwd_batch(const masic_gemm_group_t* groups, int ngroups, int ctx, const int32_t* pix, const int32_t* step,
                                 int list_stride, int npix, int nimg, int h, int w, const float* gate, int gate_ctot, int gate_c, void* stream);
/* Per-symbol coding tables (MASIC.py:986-1044 in compress, :1262-1296 in decompress) and the device side of the decoder's loop over
 * coding steps (MASIC.py:1262-1408 runs it per symbol on the host), for the views of B >= 1 stereo pairs in one launch each
 * (HSIC.compress / decompress with B = 1, compress_batch / decompress_batch; masic_amd/codec.py encode_views / decode_views).
 * A table is the K-component Gaussian-mixture PMF of one latent element (image, pixel, channel) over the alphabet 0 .. 2*minmax,
 * clipped to [2^-16, 1], renormalised to 2^16 and rounded (:1040-1043), the count total then forced to exactly 2^16 at the mode.
 * Images are stacked: sigma / mu / logits [B][K*M][HW] head outputs (logits before the softmax over K), y_hat [B][M][HW],
 * y_f16k [B][ceil16(M) / 16][HW][16].  Pixel lists hold entries q = b * HW + p (-1 = padding: its rows are skipped); the list of
 * image b is pix[(*step) * list_stride + b * npix + i], i < npix (step: device int, nullable for the tables: no offset).
 * streams: a DEVICE array of nstreams descriptors, one per coded (image, channel):
 *   img, chan      the image b and latent channel m of the stream;
 *   minmax         its alphabet 0 .. 2 * minmax (L entries) -- images differ in minmax and in which channels are coded;
 *   row0, rstride  table row of the stream's pixel i: row0 + i * rstride -- the start_freq row ([rows][2]);
 *   soff           u16 offset of the starts row of pixel i: soff + i * rstride * L;
 *   word_off, word_cnt   the stream's 32-bit little-endian words inside `words` (reads never go past word_cnt: a short stream sets
 *                  err bit 2).
 * One pair with channels chan[0 .. nch): stream c = {0, chan[c], minmax, nch, c, c * L, ...}, the pixel-major rows i * nch + c that
 * masic_rans_encode_channels reads.
 * masic_gmm_cdf_rows_batch: npix * nstreams wavefronts (row r = i * nstreams + s).  starts (nullable): u16 interval starts -- the
 * decoder's view; y_hat + start_freq (nullable, together): the integer-valued latent and the (start, freq) of its symbols -- the
 * encoder's view.
 * masic_rans_decode_step_batch: one wavefront per stream decodes the step's symbols, each taking the register form (L <= 64) or the
 * general form for its own stream, and writes them into the latent (y_hat[b][chan][pix] = symbol - minmax; y_f16k, nullable, the same
 * as bf16); the last wave of the launch to finish (over ALL streams) increments *step.  state[s] / pos[s]: per-stream coder state
 * and next word index, caller-initialised (state = word0 | word1 << 32, pos = 2) and kept across steps; done: caller-zeroed device int.
 * err_flags: one caller-zeroed device int per image: bit 0 = a table could not be normalised, or a descriptor whose alphabet is
 * empty or exceeds 1024 entries; bit 1 = a symbol outside the alphabet; bit 2 = a stream ended early (bit 3: masic_rans_decode_finish_batch; bit 4: the device encoder below).
 * masic_rans_decode_finish_batch: one thread per stream, to be called ONCE, AFTER the last coding step (outside a graph that is replayed
 * per step) on the state / pos / err_flags of the steps: ORs bit 3 (value 8) into err_flags[img] of every stream with
 * pos != word_cnt or state != 2^31.  Every encoder (masic_rans_encode_freqs / _channels / _with_indexes) starts from state 2^31 and a
 * decoder retraces the encoder's states backwards, so a stream read with the encoder's own tables ends exactly there with exactly its
 * words consumed; a damaged stream, or one read with other tables (another file's header, other weights, another operand mode), does
 * so only by a ~2^-31 coincidence.  Before the last step it flags every stream that is not yet at its end.  nstreams = 0: no launch.
 * All pointers device memory; asynchronous on `stream`; capturable into a HIP graph. */
typedef struct {
    int32_t img, chan, minmax, rstride, row0;
    uint32_t soff, word_off, word_cnt;
} masic_code_stream_t;
int masic_gmm_cdf_rows_batch(const float* sigma, const float* mu, const float* logits, int M, int K, int HW,
                             const int32_t* pix, const int32_t* step, int list_stride, int npix,
                             const masic_code_stream_t* streams, int nstreams, float scale_bound,
                             const float* y_hat, uint16_t* starts, int32_t* start_freq, int32_t* err_flags, void* stream);
int masic_rans_decode_step_batch(const uint32_t* words, const masic_code_stream_t* streams, int nstreams, uint64_t* state, uint32_t* pos,
                                 const uint16_t* starts, const int32_t* pix_all, int list_stride, int32_t* step, int npix, int M,
                                 float* y_hat, void* y_f16k, int HW, int32_t* err_flags, int32_t* done, void* stream);
int masic_rans_decode_finish_batch(const masic_code_stream_t* streams, int nstreams, const uint64_t* state, const uint32_t* pos,
                                   int32_t* err_flags, void* stream);
/* The encoder's coder on the device: masic_rans_encode_channels for every channel stream of B >= 1 pairs in one launch, one lane per
 * stream, bit for bit the host coder's words.  start_freq: the DEVICE table masic_gmm_cdf_rows_batch wrote ([rows][2]); streams: the
 * same descriptors (img, rstride, row0 are read: the symbol of pixel i, coding order, is row row0 + i * rstride); npix: symbols per
 * stream.  Stream s writes backwards into its own region of npix + 2 words of `workspace` (masic_rans_encode_batch_workspace_bytes)
 * and nowhere else; its words are the last lengths[s] / 4 of that region, lengths[s] in bytes (a multiple of 4, >= 8).  A row with
 * start < 0, freq < 1 or start + freq > 65536 (the host coder's MASIC_ERR_ARG) is skipped and ORs bit 4 (value 16) into
 * err_flags[img]: the streams of the other images are unaffected.  nstreams = 0: no launch.
 * masic_rans_pack_pairs_batch frames them: per pair the bytes masic_amd.codec.encode_channels returns (u32 n, n x u32 lengths, the n
 * streams back to back), the npairs blobs one after another in `blob` (masic_rans_pack_pairs_bound bytes always suffice), pair b at byte
 * offsets[b], offsets[npairs] = the bytes used.  first: DEVICE int32 [npairs + 1], the index of every pair's first stream (streams are
 * ordered by pair; first[npairs] = nstreams), so a pair without coded channels still gets its u32 0.  The order is fixed: the same
 * bytes every run.  All pointers device memory; asynchronous on `stream`. */
size_t masic_rans_encode_batch_workspace_bytes(int nstreams, int npix);
int masic_rans_encode_channels_batch(const int32_t* start_freq, const masic_code_stream_t* streams, int nstreams, int npix,
                                     void* workspace, uint32_t* lengths, int32_t* err_flags, void* stream);
size_t masic_rans_pack_pairs_bound(int nstreams, int npix, int npairs);
int masic_rans_pack_pairs_batch(const void* workspace, const uint32_t* lengths, const masic_code_stream_t* streams, int nstreams, int npix,
                                const int32_t* first, int npairs, void* blob, uint32_t* offsets, void* stream);
int masic_rans_decoder_open(const uint8_t* in, size_t in_len, void** handle);
int masic_rans_decoder_decode_rows(void* handle, const uint16_t* starts, int nrows, int L, int32_t* symbols);
/* the next n symbols with tables picked by indexes (arguments as masic_rans_decode_with_indexes), keeping the coder state between
 * calls: reference RansDecoder::set_stream / decode_stream (rans_interface.cpp:286-353) */
int masic_rans_decoder_decode_indexes(void* handle, const int32_t* indexes, int n, const int32_t* cdfs, int cdf_stride,
                                      const int32_t* cdf_sizes, const int32_t* offsets, int ncdfs, int32_t* symbols);
/* *ok = 1 exactly when the decoder has consumed all words of its stream and its state is 2^31, the state every encoder starts from:
 * what holds after the last symbol of an intact stream (the host form of masic_rans_decode_finish_batch), else 0 */
int masic_rans_decoder_finished(void* handle, int* ok);
void masic_rans_decoder_close(void* handle);

/* ------------------------------------------------------------------------------------------
 * SSIM / MS-SSIM (masic_amd/csrc/ssim.hip): pytorch-msssim 0.2.1's `ssim` / `ms_ssim` as the reference drivers call them
 * (coremasic/mywork/test3_real.py:102-103, newtrain_cqe_real.py:93-94).  X, Y: float32 [N][C][H][W] device tensors.
 * taps: the 11 normalised Gaussian taps (host memory, computed by the caller); weights: the `levels` level weights (host; MS-SSIM only);
 * C1 = (K1 * data_range)^2, C2 = (K2 * data_range)^2.  SSIM is levels = 1 without MASIC_SSIM_MS.  Every level must be >= 11 x 11.
 * ws (masic_ssim_workspace_bytes(..., 0) bytes): written by masic_ssim_fwd (the pooled pyramid and per-tile partial sums) and
 * masic_ssim_finish (per-plane statistics), read by masic_ssim_bwd -- keep it from the forward to the backward.
 * bws (masic_ssim_workspace_bytes(..., 1) bytes): backward scratch.  out: [N] per-image values, or [1] with MASIC_SSIM_SIZE_AVERAGE.
 * gout: the gradient of out (same shape).  dX / dY (either nullable, not both): written, not accumulated.
 * No atomics: results are bit-reproducible.  No fills, no host synchronisation: capturable into a HIP graph.
 * Launches: masic_ssim_fwd `levels`, masic_ssim_finish 1, masic_ssim_bwd levels + 1.  0 bytes from the size query: bad shape. */
enum { MASIC_SSIM_MS = 1, MASIC_SSIM_SIZE_AVERAGE = 2, MASIC_SSIM_NONNEG = 4 /* relu on the SSIM value (ssim's nonnegative_ssim) */ };
size_t masic_ssim_workspace_bytes(int N, int C, int H, int W, int levels, int backward);
int masic_ssim_fwd(const float* X, const float* Y, int N, int C, int H, int W, int levels, const float* taps, float C1, float C2,
                   void* ws, void* stream);
int masic_ssim_finish(void* ws, int N, int C, int H, int W, int levels, const float* weights, int flags, float* out, void* stream);
int masic_ssim_bwd(const float* X, const float* Y, const float* gout, int N, int C, int H, int W, int levels, const float* taps,
                   const float* weights, float C1, float C2, int flags, const void* ws, void* bws, float* dX, float* dY, void* stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS, AlexNet trunk (masic_amd/csrc/lpips.hip; the schedule is masic_amd/lpips.py): what the implicit-GEMM convolution does not
 * cover of `lpips.LPIPS(net='alex')` as the reference's evaluators call it (coremasic/mywork/test2_real.py:105-112).  Float32, fixed
 * summation orders, no float atomics, no fills, no host synchronisation (capturable into a HIP graph); a picture's result does not
 * depend on which other pictures share the launch.  The two pictures of comparison n are images 2n and 2n + 1 of every batch.
 *   masic_lpips_conv1_pack_weight  w [64][3][11][11] -> the A-fragment image of masic_lpips_conv1_fwd (masic_lpips_conv1_packed_bytes).
 *   masic_lpips_conv1_fwd   y[2N][64][Ho][Wo] = relu(Conv2d(3 -> 64, k11, s4, p2)(s(x)) + bias), Ho = (H - 7) / 4 + 1; image 2n is
 *                           in0[n], image 2n + 1 is in1[n] (both [N][3][H][W], no concat copy); s(x) = ((normalize ? 2x - 1 : x) -
 *                           shift[c]) / scale[c] on in-image pixels, padding is zero after s.  shift, scale: 3 floats each, device
 *                           memory.  H, W >= 11.  Weights at the twelfth row / column of the 12 x 12 tap grid are zeros that multiply
 *                           in-image pixels, so a non-finite pixel reaches outputs one row / column further than in Conv2d.
 *   masic_maxpool3s2_fwd    MaxPool2d(3, 2) (floor mode) of `planes` planes of H x W (>= 3) -> ((H - 3) / 2 + 1) x ((W - 3) / 2 + 1);
 *                           NaN propagates, the first of equal values wins (torch's scan).
 *   masic_lpips_dist_fwd    f [2N][C][HW], lin [C]: per pixel the norms na = sqrt(sum_c a_c^2) + 1e-10 and nb first, then
 *                           sum_c lin_c (a_c / na - b_c / nb)^2; part[n][chunk] (double) = the sum over the chunk's pixels,
 *                           masic_lpips_dist_chunks(HW) chunks per picture.
 *   masic_lpips_finish      out[1 + t][n] = (float)(sum_chunk part_t[n][chunk] / hw[t]) for the five taps, out[0][n] their float32 sum in
 *                           tap order; part holds the taps' [N][nchunks[t]] blocks back to back; nchunks, hw: 5 ints each, host memory. */
size_t masic_lpips_conv1_packed_bytes(void);
int masic_lpips_conv1_pack_weight(const float* w, float* w_packed, void* stream);
int masic_lpips_conv1_fwd(const float* in0, const float* in1, const float* w_packed, const float* bias, const float* shift,
                          const float* scale, float* y, int N, int H, int W, int normalize, void* stream);
int masic_maxpool3s2_fwd(const float* x, float* y, int planes, int H, int W, void* stream);
int masic_lpips_dist_chunks(int HW);
int masic_lpips_dist_fwd(const float* f, const float* lin, double* part, int N, int C, int HW, void* stream);
int masic_lpips_finish(const double* part, const int* nchunks, const int* hw, int N, float* out, void* stream);

/* LPIPS input gradients (masic_amd/csrc/lpips_bwd.hip; the schedule is masic_amd/lpips.py): with the float32 implicit-GEMM convolution
 * run as the opposite layer kind for layers 2-5, the backward of the forward above with respect to the pictures -- in0, in1 or both;
 * no weight gradients.  The rules of the forward hold (float32, fixed summation orders, no float atomics, no fills, no host
 * synchronisation, an image's result independent of the rest of the launch).  `f` is always a tap of the forward, [2N][C][HW] with
 * images 2n and 2n + 1 compared.  A gradient tensor holds the images of ONE side, [N][..] (sides = 1: in0's, sides = 2: in1's), or
 * the interleaved [2N][..] of the forward (sides = 3).  Everything is written, not accumulated.
 *   masic_lpips_dist_bwd    g_pre = (g_dist + g_in) * [f > 0]: the gradient of the tap's PRE-activation.  g_dist is the gradient of
 *                           G[n] * mean_pixels sum_c lin_c (a_c / na - b_c / nb)^2 with G[n] = g_val[n] + g_res[n] read from device
 *                           memory (the upstream gradients of the value and of this tap's per-layer value): with u = a / na,
 *                           v = b / nb, d = u - v, d/da_c = (2 G / HW) (lin_c d_c / na - a_c (sum_k lin_k d_k a_k) / (na^2 sqrt(sum a^2))),
 *                           the mirror image with the opposite sign for b; d and the sum are formed from the normalised values.
 *                           DEVIATION from lpips's autograd, on purpose: at a pixel whose squares sum to 0 the second term is DEFINED
 *                           as 0 (d/da_c = 2 G lin_c d_c / (HW 1e-10) with u = 0), matching the forward's 0 / 1e-10 = 0; torch
 *                           computes 0 / 0 = NaN in sqrt's backward there.  (With the ReLU mask that pixel's own g_pre is 0 either
 *                           way; the other picture's gradient at the pixel is the regular formula with u = 0.)  g_in (nullable): what
 *                           arrives from the layer above, laid out as g_pre; g_pre may be g_in itself (in place).
 *   masic_maxpool3s2_bwd    gx [B][C][H][W] from gy [B][C][Ho][Wo] of MaxPool2d(3, 2): a gather over the <= 2 x 2 windows covering a
 *                           pixel in row-major window order, each window's winner recomputed with the forward's scan -- bit-equal to
 *                           torch's max_pool2d backward; rows / columns under no window get 0.  The forward input of image b is image
 *                           b * img_stride + img_off of x (x: a saved tap; stride 2, offset = side for a one-sided chain, else 1, 0).
 *   masic_lpips_conv1_bwd_pack_weight  w [64][3][11][11] -> the image [row phase][co][tap][c][column phase] read by masic_lpips_conv1_bwd
 *                           (masic_lpips_conv1_bwd_packed_bytes).
 *   masic_lpips_conv1_bwd   the input gradient of masic_lpips_conv1_fwd's convolution (g: the gradient of its pre-activation,
 *                           [B][64][Ho][Wo]) through the scaling layer and `normalize`: d[.][3][H][W] = convT(g) / scale[c] (* 2 under
 *                           normalize), every pixel written (exactly 0 where no window reaches).  d0 and d1 both given: B = 2N
 *                           interleaved images, image 2n goes to d0[n], image 2n + 1 to d1[n]; one of them null: B images to the other. */
int masic_lpips_dist_bwd(const float* f, const float* lin, const float* g_val, const float* g_res, const float* g_in, float* g_pre,
                         int N, int C, int HW, int sides, void* stream);
int masic_maxpool3s2_bwd(const float* x, const float* gy, float* gx, int B, int C, int H, int W, int img_stride, int img_off,
                         void* stream);
size_t masic_lpips_conv1_bwd_packed_bytes(void);
int masic_lpips_conv1_bwd_pack_weight(const float* w, float* w_packed, void* stream);
int masic_lpips_conv1_bwd(const float* g, const float* w_packed, const float* scale, float* d0, float* d1, int B, int H, int W,
                          int normalize, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic mode (masic_amd/determinism.py).  Siblings of the weight-gradient and warp-backward entry points
 * above with the same arguments and the same results up to summation order, but NO float atomics: each pixel split stores its partial
 * tile with plain stores into its own slab of `workspace` ([split][...], indexed by split number), and a finishing launch sums the slabs
 * in ascending split order in float32.  The split count depends only on the shape (and is capped so that one layer's slabs stay within
 * 64 MiB).  The result is therefore bitwise reproducible: the same inputs on the same device model and library build give the same
 * bits, whatever else runs concurrently.  `workspace` (at least the matching _det_workspace_bytes; for a weight gradient a whole
 * multiple of the weight's float32 size) has contents irrelevant on entry and on exit: no fill is needed and none is left behind.  A
 * weight gradient makes as many launches as the default call with a clean workspace.  The library keeps no mode of its own: the caller
 * picks the entry point.  0 from a size query: bad shape. */
size_t masic_conv2d_wgrad_det_workspace_bytes(const masic_conv_desc_t* d);
/* as masic_conv2d_wgrad_ws */
int masic_conv2d_wgrad_det(const float* x, const float* dy, float* dw, void* workspace, const masic_conv_desc_t* d, void* stream);
/* as masic_conv2d_wgrad_bf16in (only layers masic_conv2d_wgrad_bf16in_supported); workspace: masic_conv2d_wgrad_det_workspace_bytes(d) */
int masic_conv2d_wgrad_bf16in_det(const void* x_bf16, const void* dy_bf16, float* dw, void* workspace, const masic_conv_desc_t* d,
                                  void* stream);
/* as masic_conv3x3_wgrad_f16k_ws / masic_conv5x5_wgrad_f16k_ws */
size_t masic_conv3x3_wgrad_f16k_det_workspace_bytes(int B, int Cin, int Cout, int H, int W);
int masic_conv3x3_wgrad_f16k_det(const void* x_f16k, const void* dy_f16k, float* dw, void* workspace,
                                 int B, int Cin, int Cout, int H, int W, void* stream);
size_t masic_conv5x5_wgrad_f16k_det_workspace_bytes(int B, int Cin, int Cout, int H, int W);
int masic_conv5x5_wgrad_f16k_det(const void* x_f16k, const void* dy_f16k, float* dw, void* workspace,
                                 int B, int Cin, int Cout, int H, int W, void* stream);
/* as masic_gemm_wgrad_bias_f16k (dw: CA*CQ weights, then the nb bias sums); the bias sums come from per-split, per-workgroup slots of the
 * same workspace, summed in a fixed order by the same finishing launch */
size_t masic_gemm_wgrad_bias_f16k_det_workspace_bytes(int bias_of, int B, int CA, int CQ, int HW);
int masic_gemm_wgrad_bias_f16k_det(const void* rows_f16k, const void* cols_f16k, float* dw, void* workspace, int bias_of, int B, int CA,
                                   int CQ, int HW, void* stream);
/* What a weight-gradient call launches, as text: one line per launch in launch order, the zero fill and the finishing pass included,
 *     kernel<every template argument> | gx,gy,gz | block | dynamic LDS bytes
 * printed from the plan the launcher itself executes (kernel choice, pixel splits, grids are host-side decisions of the shape alone).
 * flags name the entry point: 0 the _ws form with workspace_clean = 0, MASIC_WGRAD_CLEAN with workspace_clean = 1, MASIC_WGRAD_DET the
 * _det form, MASIC_WGRAD_IN16 masic_conv2d_wgrad_bf16in[_det].  A form the launcher refuses: its error code and an empty buffer; a
 * form without an entry point (DET with CLEAN, ...) or a buffer too small: MASIC_ERR_ARG.
 * masic_wgrad_f16k_plan_name: kind 3 / 5: masic_conv{3x3,5x5}_wgrad_f16k_{ws,det} with s0 .. s4 = B, Cin, Cout, H, W; kind 1:
 * masic_gemm_wgrad_bias_f16k[_det] with s0 .. s4 = bias_of, B, CA, CQ, HW.  The _row_name queries list every compiled instantiation of
 * the tables the plans choose from (rows 0 .., det 0 / 1; MASIC_ERR_ARG past the last row). */
#define MASIC_WGRAD_DET 1
#define MASIC_WGRAD_IN16 2
#define MASIC_WGRAD_CLEAN 4
int masic_conv2d_wgrad_plan_name(const masic_conv_desc_t* d, int flags, char* buf, size_t n);
int masic_conv2d_wgrad_row_name(int row, int det, char* buf, size_t n);
int masic_wgrad_f16k_plan_name(int kind, int s0, int s1, int s2, int s3, int s4, int flags, char* buf, size_t n);
int masic_wgrad_f16k_row_name(int row, int det, char* buf, size_t n);
/* What the five persistent-workgroup launchers launch, in the same text form (one line per launch, finishing and packing passes
 * included), from the plan function the launcher itself executes.  Host code only: shapes and form arguments, no device pointers.  The
 * line of the persistent kernel carries, behind a fifth bar, the integers its tile loop runs on:
 *   masic_conv_a_plan_name            masic_conv_a_[gdn_[dual_]]fwd[_ex]: x_aligned16 = the input pointer is 16-byte aligned, gdn = a GDN
 *                                     follows, products = 1 or 3 (gdn_inverse & 2), out = 0 F16K, 1 fp8, 2 F16K + the pre-GDN result;
 *                                     integers: ntiles tiles_w tiles_per_image Ho Wo
 *   masic_gdn_fwd_plan_name           masic_gdn_fwd_ex (out_f16k = 0) / masic_gdn_fwd_f16k (out_f16k = 1, prec ignored); integers: work
 *                                     items (strips or tiles), items a workgroup takes per round of its loop, pixels per item, items per image
 *   masic_gdn_bwd_fused_plan_name     masic_gdn_bwd_fused_ex2 with x / g given as F16K (x_f16k, g_f16k) and g_sum asked for (want_sum);
 *                                     integers: ntiles (128 pixels each) pixels H*W
 *   masic_conv3x3_resident_plan_name  masic_conv3x3_resident_ex_fwd; ex = a second output or channel sums are asked for; integers:
 *                                     ntiles tiles_w tiles_per_image NBUF (the kernel's patch ring)
 *   masic_pic_wgrad_f16k_plan_name    masic_pic_wgrad_f16k; integers: chunks (64 coarse pixels each) chunks per image
 * A shape or form the launcher refuses: its error code and an empty buffer; a buffer too small: MASIC_ERR_ARG. */
int masic_conv_a_plan_name(int B, int Hi, int Wi, int x_aligned16, int gdn, int products, int out, char* buf, size_t n);
int masic_gdn_fwd_plan_name(int B, int C, int H, int W, int prec, int out_f16k, char* buf, size_t n);
int masic_gdn_bwd_fused_plan_name(int B, int C, int H, int W, int x_f16k, int g_f16k, int want_sum, char* buf, size_t n);
int masic_conv3x3_resident_plan_name(int B, int Cin, int Cout, int H, int W, int ex, int sum_of, char* buf, size_t n);
int masic_pic_wgrad_f16k_plan_name(int B, int Hc, int Wc, char* buf, size_t n);
/* as masic_warp_perspective_bwd_gather, but where the gather form raises *flag the fallback is a deterministic store-and-sum (entries
 * grouped by source pixel with integer counting atomics, each group summed in destination-pixel order) instead of the float-atomic
 * scatter; it covers every homography, a horizon inside the picture included.  The flag is still tested on the device.  workspace:
 * masic_warp_perspective_bwd_gather_det_workspace_bytes, int32 counters and entries. */
size_t masic_warp_perspective_bwd_gather_det_workspace_bytes(int B, int Hs, int Ws, int Hd, int Wd);
int masic_warp_perspective_bwd_gather_det(const float* g_dst, const float* minv_norm, float* g_src, int* flag, void* workspace,
                                          int B, int C, int Hs, int Ws, int Hd, int Wd, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MASIC_HIP_H */
