/*
 * gligen_hip.h -- C ABI of the MI355X (gfx950) kernels for the layout-conditioned denoising hot path
 * of LayoutLLM-T2I (modified GLIGEN UNet + PLMS sampler).
 *
 * The reference has no native layer: every op on the path is a torch call inside an
 * nn.Module.forward.  Each entry point below therefore names the reference *Python* code it replaces
 * (file:line relative to the reference root).  All pointers are raw DEVICE pointers (owned by the
 * caller, e.g. torch tensors); `stream` is a hipStream_t.  Every function returns 0 on success or a
 * hipError_t / negative gl error code; nothing throws across the ABI.
 *
 * Activation layout is token-major ("NHWC"): a feature map is [B, H*W, C] fp16 with C contiguous, so
 * 1x1 convs and Linear layers are plain GEMMs and the 3x3 conv is an implicit GEMM.  Weights are fp16
 * [N, K] row-major (torch Linear layout); 3x3 conv weights are repacked to [Cout, Cin/64, 3, 3, 64].
 * Accumulation and all normalisation/softmax statistics are fp32.
 */
#ifndef GLIGEN_HIP_H
#define GLIGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GL_ABI_VERSION 15

/* error codes (negative; positive values are hipError_t) */
#define GL_ERR_BAD_ARG (-1)
#define GL_ERR_UNSUPPORTED (-2)

/* ---- epilogues of gl_gemm / gl_conv3x3 ------------------------------------------------------- */
enum gl_epilogue {
    GL_EPI_BIAS = 0,      /* out = acc + bias                                                        */
    GL_EPI_SILU = 1,      /* out = silu(acc + bias)             PositionNet MLP, time_embed           */
    GL_EPI_GEGLU = 2,     /* out[:, j] = (acc_x + b) * gelu_erf(acc_gate + b); weights row-interleaved */
                          /*   in blocks of 32 (x rows, gate rows); N = 8C packed, out width N/2       */
    GL_EPI_RES = 3,       /* out = acc + bias + res                                                    */
    GL_EPI_GATE_RES = 4,  /* out = res + gate[0] * (acc + bias)   gated fuser residual                 */
    GL_EPI_ROWBIAS = 5    /* out = acc + bias + rowbias[m / rows_per_sample, n]   (+ time embedding)   */
};

enum gl_out_mode {
    GL_OUT_F16_ROWMAJOR = 0, /* out[m * ldc + n] fp16                                   */
    GL_OUT_F32_NCHW = 1,     /* out[(b * N + n) * HW + p] fp32, m = b * HW + p           */
    GL_OUT_F32_ROWMAJOR = 2  /* out[m * ldc + n] fp32: the RESIDUAL STREAM (ResBlock / transformer-block sums,
                                openaimodel.py:231, attention.py:395-402,446) is kept in fp32 so that ~100 chained
                                residual adds are not rounded to fp16 each; out2 (optional) gets an fp16 copy for
                                consumers that feed it to the matrix cores (down / up convs)                        */
    ,
    GL_OUT_F16_HILO = 3      /* split-fp16 operand for a following 1x1 product: out[m * ldc + n] = hi = fp16(v) and
                                out[m * ldc + N + n] = lo = fp16(v - hi)  (ldc >= 2N).  The consumer runs gl_gemm with
                                K = 2N against the weight stored twice, [W | W]: x.W = hi.W + lo.W restores ~22 mantissa
                                bits of the activation operand (proj_out of attention.py:444-446)            */
};

/*
 * gl_gemm: out[M, N] = A[M, K] . W[N, K]^T (+ epilogue).   K % 64 == 0.
 * Replaces nn.Linear / 1x1 nn.Conv2d calls: attention.py:43 (GEGLU proj), :61 (ff out), :124-126,
 * :160-162 (q/k/v), :143,:178 (to_out), :228 (fuser.linear), :440,:445 (proj_in/out);
 * openaimodel.py:190-194 (skip 1x1), :220 (emb_layers), :428-429 (time_embed);
 * text_grounding_net.py:41 (PositionNet MLP).
 * Two-source A (a2 != NULL): k < ksplit reads a[m*lda + k], else a2[m*lda2 + (k - ksplit)] -- this folds
 * th.cat([h, hs.pop()], 1) (openaimodel.py:456) into the skip-connection GEMM.  ksplit % 64 == 0.
 */
typedef struct gl_gemm_args {
    const void* a;      int32_t lda;
    const void* a2;     int32_t lda2;  int32_t ksplit;
    const void* w;                      /* fp16 [N, K] */
    const float* bias;                  /* fp32 [N] or NULL */
    int32_t M, N, K;
    int32_t epi;                        /* enum gl_epilogue */
    int32_t out_mode;                   /* enum gl_out_mode */
    void* out;          int32_t ldc;    /* fp16 row stride (elements); GEGLU: stride of the N/2-wide output */
    const void* res;    int32_t ldres;  /* fp16 residual [M, N] */
    const float* gate;                  /* device scalar for GL_EPI_GATE_RES */
    const void* rowbias; int32_t ld_rowbias; int32_t rows_per_sample;  /* fp16 [B, N] */
    int32_t hw;                         /* GL_OUT_F32_NCHW: pixels per sample */
    /* optional split-K scratch: when the (M, N) grid would leave most of the 256 CUs idle (8x8 / 16x16
     * levels: 40-160 tiles) and K is long, K is cut into slices that write fp32 partial tiles here and a
     * second kernel reduces them and applies the epilogue.  NULL disables splitting. */
    void* workspace;    int64_t workspace_bytes;
    int32_t res_f32;                    /* != 0: res is fp32 [M, ldres] (residual stream), else fp16 */
    void* out2;         int32_t ldc2;   /* optional fp16 copy [M, N] of a GL_OUT_F32_ROWMAJOR output; NULL = none */
    /* optional transposed tail (fused QKV projection, attention.py:160-162): columns [vt_col0, N) are NOT written to
     * out but as gl_attention's V^T operand, vt[((b * vt_H + h) * vt_d + c) * vt_ld + key] with b = m / vt_rows,
     * key = m % vt_rows, (h, c) = divmod(n - vt_col0, vt_d).  fp16 row-major out, epi BIAS only, vt_col0 % 64 == 0. */
    void* vt;           int32_t vt_col0, vt_rows, vt_d, vt_ld, vt_H;
    /* weight reuse along K (split-fp16 operands): with kwrap != 0 column k of the product reads w[n * ldw + k] for k < kwrap
     * and w[n * ldw + k - kwrap] beyond (ONE step back).  K = 2 * kwrap: A = [hi | lo] is multiplied against [W | W] without storing W
     * twice.  K = 3 * kwrap (ldw >= 2 * kwrap, weight rows [Whi | Wlo]): columns [0, kwrap) twice, then [kwrap, 2 * kwrap) -- with
     * A = [xhi | xlo] and the second source a2 = xhi at ksplit = 2 * kwrap that is the three-pass product xhi.Whi + xlo.Whi + xhi.Wlo.
     * kwrap % 64 == 0, kwrap < K <= 3 * kwrap.  ldw == 0: the row stride is K (kwrap == 0) or kwrap.  gl_gemm only (ignored by gl_conv3x3). */
    int32_t ldw, kwrap;
    int32_t rowbias_f32;                /* != 0: rowbias is fp32 [B, N] (ld_rowbias in floats) instead of fp16: the ResBlock's emb_layers output is
                                           added to the conv result unrounded (openaimodel.py:220-226) */
    /* ABI 15 (strict mode): with out_mode GL_OUT_F16_HILO the transposed tail takes BOTH halves -- vt receives fp16(v) and vt_lo (same layout)
     * fp16(v - fp16(v)) of the V columns [vt_col0, N): the two V^T operands of the split-fp16 attention (gl_attn_args.vt / vt_lo) straight
     * from the fused QKV projection's epilogue.  Required (non-NULL) exactly when vt != NULL and out_mode == GL_OUT_F16_HILO.  Implemented by the 8-wave
     * kernel's epilogue only: GL_ERR_UNSUPPORTED for launches it does not take (M < 256, K % 64, a tail that does not start on a wave's column range). */
    void* vt_lo;
} gl_gemm_args;

/*
 * gl_ff_fused: the whole FeedForward of a BasicTransformerBlock / GatedSelfAttentionDense in ONE launch (attention.py:38-62,
 * called at :231-232 and :401):   out = res (+|gate *) ( GEGLU(x . W1^T + b1) . W2^T + b2 )
 * for narrow channel widths (C in {64, 128, 192, 256, 320}; gl_ff_fused_supported(C)) -- the level whose [M, 4C]
 * GEGLU intermediate (84 MB at 64x64x320) would otherwise make a round trip through HBM between two gl_gemm launches.
 * w1 / b1 are gl_gemm's GL_EPI_GEGLU operands (rows interleaved in blocks of 32: x rows, gate rows), w2 is [C, 4C].
 * gate == NULL: out = y + res (GL_EPI_RES);  gate != NULL: out = res + gate[0] * y (GL_EPI_GATE_RES).
 * Agrees with the two-launch form to fp32 accumulation rounding (same fp16 intermediate, other summation order).
 */
typedef struct gl_ff_args {
    const void* x;      int32_t ldx;    /* fp16 [M, C] (already normalised rows) */
    const void* w1;     const float* b1;/* fp16 [8C, C] packed, fp32 [8C] packed   */
    const void* w2;     const float* b2;/* fp16 [C, 4C], fp32 [C]                  */
    const void* res;    int32_t ldres;  int32_t res_f32;   /* residual rows: fp32 stream (res_f32 != 0) or fp16 */
    const float* gate;                  /* device scalar or NULL */
    void* out;          int32_t ldc;    int32_t out_mode;  /* GL_OUT_F16_ROWMAJOR or GL_OUT_F32_ROWMAJOR */
    int32_t M, C;
} gl_ff_args;
int gl_ff_fused(const gl_ff_args* args, void* stream);
int gl_ff_fused_supported(int32_t C);
/* 1 when the fused form is the faster choice for [M, C] on the current device (enough 128-row blocks to fill whole rounds
 * of CUs); the engine uses it, and so must anything that wants to reproduce the engine's results bit for bit */
int gl_ff_fused_applicable(int32_t C, int32_t M);
int gl_sizeof_ff_args(void);

/*
 * gl_conv3x3: 3x3, pad 1 convolution as implicit GEMM over NHWC fp16 input [B, Hin, Win, Cin]
 * (Cin % 64 == 0; weights [Cout, Cin/64, 3, 3, 64], i.e. K = (channel block, tap, channel)).  M = B*Hout*Wout, N = Cout, K = 9*Cin.
 *   stride 1            : ResBlock convs openaimodel.py:158,184; conv_in :299; out conv :388
 *   stride 2            : Downsample.op openaimodel.py:105-107,:114
 *   upsample2x != 0     : F.interpolate(nearest, x2) + conv, openaimodel.py:82-84 (input is Hout/2 x Wout/2)
 *   upsample2x == 2     : the same layer with FOLDED weights: after nearest upsampling the nine taps of output pixel (2y + py, 2x + px) touch
 *                         only the 2 x 2 source pixels (y + py - 1 + a, x + px - 1 + b), so per output parity it is a 2x2 conv on the source
 *                         grid.  g.w is [4 Cout, 4 Cin]: rows (parity py * 2 + px, Cout), K = (64-channel block, tap a * 2 + b, channel), with
 *                         Wf[py,px][:, :, a, b] = sum of W[:, :, ky, kx] over ky in S(py, a), kx in S(px, b); S(0,0) = {0}, S(0,1) = {1,2},
 *                         S(1,0) = {0,1}, S(1,1) = {2}.  g.N stays Cout and must be the PACKED Cout (parity p's rows start at row p * g.N).  Needs stride 1, in_split 0, w_split 0 and a row-major output
 *                         (GL_OUT_F16_ROWMAJOR or GL_OUT_F32_ROWMAJOR, with or without out2); GL_ERR_BAD_ARG otherwise.  8-wave kernel only.
 * Epilogue fields are those of gl_gemm (the `g` member; g.a/g.K/g.M are ignored and derived here).
 */
typedef struct gl_conv_args {
    const void* in;
    int32_t B, Hin, Win, Cin;
    int32_t Hout, Wout;
    int32_t stride;        /* 1 or 2 */
    int32_t upsample2x;    /* 0, 1, or 2 = folded weights (stride must be 1) */
    gl_gemm_args g;        /* w, bias, N, epi, out_mode, out, ldc, res, ldres, rowbias..., hw */
    /* split-fp16 operands (ABI 14; strict mode).  in_split = 2: the input pixels are [hi | lo] rows of 2 Cin channels
     * (hi = fp16(x), lo = fp16(x - hi), e.g. gl_groupnorm_ex's out / out_lo with ldo = 2 Cin) and the K walk visits both halves against
     * the same weight: x.W = hi.W + lo.W (~22 mantissa bits of the activation); in_split = 3 (needs w_split): a third pass hi.Wlo.
     * w_split != 0: the weight rows are [Whi | Wlo], fp16 [Cout, 2, Cin/64, 3, 3, 64] (Wlo = fp16(W - Whi)); in_split 0 / 2 read Whi only. */
    int32_t in_split, w_split;
} gl_conv_args;

/*
 * gl_attention: out[b, q, h*d : (h+1)*d] = softmax_k(scale * Q.K^T) . V   (flash-style, no S x S tensor).
 * Replaces SelfAttention.forward attention.py:164-176 and CrossAttention.forward :128-141 (mask=None).
 * Q [B, Nq, *] fp16 rows of stride ldq, head h at column offset h*d; K likewise (ldk).
 * V is passed TRANSPOSED per head: vt[((b*H + h)*d + c) * ldvt + key], ldvt % 8 == 0 and >= Nk rounded up to 64 (the
 * pad keys are never used: the kernel masks them, so their contents are arbitrary).  d in {8..160}, d % 8 == 0.
 * Batch strides are in elements.
 */
typedef struct gl_attn_args {
    const void* q;  int64_t q_bstride;  int32_t ldq;
    const void* k;  int64_t k_bstride;  int32_t ldk;
    const void* vt; int32_t ldvt;
    void* out;      int64_t o_bstride;  int32_t ldo;
    int32_t B, H, d, Nq, Nk;
    float scale;
    int32_t q_prescaled;   /* != 0: scale * log2(e) is already folded into Q (the packer folds it into the q projection
                              weights); `scale` is then ignored and the running max is subtracted inside the MFMA */
    /* split-fp16 attention (ABI 14; strict mode): with q_lo != NULL every operand is hi + lo -- q_lo / k_lo / vt_lo hold the fp16 residuals
     * in the layouts (strides, batch strides) of q / k / vt, the logits are q.k = qhi.khi + qlo.khi + qhi.klo, the probabilities are split
     * P = Phi + Plo in registers, O = Phi.Vhi + Plo.Vhi + Phi.Vlo, and out / out_lo (same ldo, out_lo may be NULL) receive fp16(O) and
     * fp16(O - fp16(O)).  All three of q_lo, k_lo, vt_lo must be given. */
    const void* q_lo; const void* k_lo; const void* vt_lo; void* out_lo;
} gl_attn_args;

/* gl_transpose_v: V [B, Nk, *] (row stride ldv, head h at column h*d) -> vt [B, H, d, ldvt], zero-fills keys
 * [Nk, ldvt).  Layout glue for gl_attention's P.V MFMA operand.  d, ldv, ldvt, v_bstride multiples of 8 (16-byte
 * accesses), v and vt 16-byte aligned. */
int gl_transpose_v(const void* v, int64_t v_bstride, int32_t ldv, void* vt, int32_t ldvt,
                   int32_t B, int32_t H, int32_t d, int32_t Nk, void* stream);

/*
 * GroupNorm(32 groups) over NHWC fp16, fp32 statistics (GroupNorm32, util.py:226-228; Normalize,
 * attention.py:78-79), fused SiLU (openaimodel.py:155-157,180-181) and fused channel concat of two
 * sources (openaimodel.py:456): channels [0, C1) come from x1 [B, HW, C1], [C1, C1+C2) from x2.
 *   gl_groupnorm_stats : partial[b][chunk][32][2] = (mean, M2) per group and pixel chunk, fp32, gathered about a
 *                        per-channel shift and merged with the exact pairwise (Welford / Chan) formula
 *   gl_groupnorm_apply : y = (x - mean) * rstd * gamma + beta (, SiLU) -> fp16 [B, HW, C1+C2]
 */
int gl_groupnorm_stats(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t B, int32_t HW,
                       float* partial, int32_t nchunk, void* stream);
int gl_groupnorm_apply(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t B, int32_t HW,
                       const float* partial, int32_t nchunk, const float* gamma, const float* beta,
                       float eps, int32_t silu, void* out, void* stream);
/* gl_groupnorm: the whole operator.  Small maps with C % 256 == 0 (the 16x16 / 8x8 levels) run as ONE launch that keeps a
 * group's slab in registers (two-pass statistics); everything else as gl_groupnorm_stats + gl_groupnorm_apply (partial /
 * nchunk are only used then).  gl_groupnorm_launches tells which (1 or 2). */
int gl_groupnorm(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t B, int32_t HW, const float* gamma,
                 const float* beta, float eps, int32_t silu, void* out, float* partial, int32_t nchunk, void* stream);
int gl_groupnorm_launches(int32_t C, int32_t HW);

/* gl_groupnorm_ex: gl_groupnorm with the inputs optionally in fp32 (the residual stream: GroupNorm32 of openaimodel.py:155,
 * Normalize of attention.py:440 read the block input itself, not an fp16 copy of it) and two optional extra outputs that
 * feed split-fp16 1x1 products:
 *   out_lo : fp16 residual of the normalised rows, out_lo[m * ldo + c] = fp16(y - fp16(y))       (proj_in, attention.py:440)
 *   raw    : the INPUT concat itself as [hi | lo], raw[m * ldraw + c] = fp16(x), raw[m * ldraw + C + c] = fp16(x - fp16(x))
 *            (ResBlock skip_connection reads x, openaimodel.py:190-194,231), ldraw >= 2 (C1 + C2)
 * ldo = row stride of out / out_lo in elements (0: C1 + C2).  partial / nchunk as for gl_groupnorm. */
typedef struct gl_gn_args {
    const void* x1;     int32_t C1;
    const void* x2;     int32_t C2;       /* second source of the channel concat, or NULL */
    int32_t x_f32;                        /* != 0: x1 / x2 are fp32, else fp16 */
    int32_t B, HW;
    const float* gamma; const float* beta; float eps; int32_t silu;
    void* out;          int32_t ldo;
    void* out_lo;
    void* raw;          int32_t ldraw;
    float* partial;     int32_t nchunk;
} gl_gn_args;
int gl_groupnorm_ex(const gl_gn_args* args, void* stream);
int gl_groupnorm_launches_ex(int32_t C, int32_t HW, int32_t x_f32);

/*
 * gl_layernorm: row LayerNorm eps 1e-5 over C (attention.py:216-217,292-294,369-371), fp32 statistics (two-pass).
 * x_f32 is a bit set: bit 0 = the input rows are fp32 (the residual stream) instead of fp16; bit 1 = the OUTPUT rows are fp32
 * instead of fp16 (y, ldy then count floats: the conditioning text encoder's last_hidden_state, encoders/modules.py:167).
 * Input row r = (b, i) with i < rows_in; output row index
 * = b * rows_out + row_off + i -- this writes straight into the [x ; objs] concatenation of GatedSelfAttentionDense
 * (attention.py:230).  stats (optional): (mean, rstd) per input row, fp32 [B * rows_in, 2].  C % 8 == 0, C <= 2048.
 * x2 (optional, fp16, rows2 rows per sample, row stride ldx2): a second source whose rows follow the rows_in rows of x in
 * every sample's output block -- [x ; objs] normalised in one launch.
 */
int gl_layernorm(const void* x, int32_t ldx, int32_t x_f32, void* y, int32_t ldy, const float* gamma, const float* beta,
                 int32_t B, int32_t rows_in, int32_t rows_out, int32_t row_off, int32_t C, float eps, float* stats,
                 const void* x2, int32_t ldx2, int32_t rows2, void* stream);
/* x_f32 bit 2 (value 4): the second source x2 is fp32 (ldx2 in floats) -- the fuser's fuser.linear(objs) rows enter LayerNorm unrounded.
 * gl_layernorm_stats: only the per-row (mean, rstd) of fp32 rows [rows, C] (the same two-pass arithmetic as gl_layernorm), for consumers that
 * re-evaluate the normalisation themselves in fp32 (gl_rela_pool_ln3, gl_rela_merge): rela_fuse's LayerNorm3 output is then never stored. */
int gl_layernorm_stats(const float* x, int32_t ldx, int32_t rows, int32_t C, float eps, float* stats, void* stream);
/* x_f32 bit 3 (value 8; ABI 14): the fp16 output rows are written as [hi | lo] -- y[r * ldy + c] = fp16(v), y[r * ldy + C + c] = fp16(v - fp16(v)),
 * ldy >= 2 C -- the split-fp16 operand of the projection that follows (strict mode).  fp32 input rows only (bit 0; with a second source: bit 2). */
/* gl_split_f32: fp32 rows [rows, C] (row stride ldx floats) -> fp16 [rows, 2 C] rows [hi | lo] (row stride ldy): the split-fp16 form of a
 * residual-stream tensor for a matrix-core consumer that has no producer to write it (down / up convs, the conditioning tensors). C % 8 == 0. */
int gl_split_f32(const float* x, int32_t ldx, int64_t rows, int32_t C, void* y, int32_t ldy, void* stream);

/*
 * RelationCrossAttention (attention.py:315-359) in closed form:
 *   out = hid + (1/max_objs) * sum_i 1[p in rect_i] f_i ,  x_new = (out + x) / 2   (attention.py:398)
 * rects[b][i] = {top, bottom, left, right} int32 pixel bounds (already python-slice-normalised on the
 * host, attention.py:325-346), nvalid[b] = boxes before the first padded/degenerate one, poison[b] != 0
 * reproduces the reference's NaN for an empty (right < left) slice.
 *   gl_rela_pool  : feat[b, i, :] = mean_{p in rect_i} hid[b, p, :]   (0 rows for i >= nvalid[b]); with ln_out != NULL also
 *                   ln_out[b, i, :] = LayerNorm(feat[b, i, :]; ln_gamma, ln_beta, eps 1e-5)  (norm1, attention.py:348)
 *   gl_rela_merge : y = 0.5 * (x + hid + (1/max_objs) * sum_i 1[p in rect_i] f[b, i, :])
 *                   x / y fp32 when x_f32 != 0 (residual stream) else fp16.  hid = LayerNorm3(x) is either read (fp16,
 *                   ln_stats == NULL) or re-evaluated in fp32 from ln_stats = gl_layernorm's (mean, rstd) rows and
 *                   gamma / beta, so that it enters the stream unrounded.  With ln2_out != NULL (fp32 stream + ln_stats
 *                   form only, max_objs <= 32) the same launch also writes ln2_out = LayerNorm(y; ln2_gamma, ln2_beta,
 *                   eps 1e-5) in fp16 -- the norm2 in front of attn2 (attention.py:400) -- bit-identical to gl_layernorm(y).
 * slots (ABI 13): rows per sample of feat / ln_out / f, 0 < slots <= max_objs (0 = max_objs).  The reference runs the relation chain
 * (attention.py:348-351) over all max_objs = 30 rows of every sample although only the first nvalid[b] enter the result; a caller that knows
 * max_b nvalid[b] <= slots computes just `slots` rows per sample -- the rows are independent of one another, so the used ones are unchanged.
 * rects stays [B, max_objs, 4] and 1/max_objs stays the reference's divisor.
 */
int gl_rela_pool(const void* hid, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* rects,
                 const int32_t* nvalid, const int32_t* poison, int32_t max_objs, int32_t slots, void* feat, const float* ln_gamma,
                 const float* ln_beta, void* ln_out, void* stream);
/* gl_rela_pool_ln3 (round 4): gl_rela_pool on the fp32 stream: x fp32 [B, H*W, C] with the per-row (mean, rstd) of rela_fuse's LayerNorm3
 * (gl_layernorm_stats) and its gamma / beta; the pooled row is gamma * mean_rect((x - mean_r) * rstd_r) + beta in fp32 -- hid = LN3(x)
 * (attention.py:317) is neither rounded to fp16 nor stored. */
int gl_rela_pool_ln3(const float* x, const float* ln3_stats, const float* ln3_gamma, const float* ln3_beta, int32_t B, int32_t H,
                     int32_t W, int32_t C, const int32_t* rects, const int32_t* nvalid, const int32_t* poison, int32_t max_objs,
                     int32_t slots, void* feat, const float* ln_gamma, const float* ln_beta, void* ln_out, void* stream);
int gl_rela_merge(const void* x, int32_t x_f32, const void* hid, const float* ln_stats, const float* gamma,
                  const float* beta, const void* f, int32_t B, int32_t H, int32_t W, int32_t C,
                  const int32_t* rects, const int32_t* nvalid, const int32_t* poison, int32_t max_objs, int32_t slots,
                  void* y, const float* ln2_gamma, const float* ln2_beta, void* ln2_out, void* stream);

/*
 * gl_posnet_input: builds the PositionNet MLP input (text_grounding_net.py:30-41, util.py:12-26):
 *   out[b, i, :] = [ emb * m + (1 - m) * null_pos  |  fourier(box) * m + (1 - m) * null_xyxy ]   fp16
 * boxes [B, n, 4] fp32, masks [B, n] fp32, emb [B, n, in_dim] fp32, nulls fp32.
 */
int gl_posnet_input(const float* boxes, const float* masks, const float* emb, const float* null_pos,
                    const float* null_xyxy, int32_t rows, int32_t in_dim, int32_t num_freqs, void* out,
                    void* stream);

/* gl_timestep_embedding: [cos(t w_k) | sin(t w_k)], w_k = exp(-ln(1e4) k / half) (util.py:161-181) -> fp16 [B, dim] */
int gl_timestep_embedding(const float* t, int32_t B, int32_t dim, void* out, void* stream);
/* fp32-output forms (ABI 14; strict mode: the rows then go through gl_split_f32 and enter the first Linear as [hi | lo]) */
int gl_timestep_embedding_f32(const float* t, int32_t B, int32_t dim, float* out, void* stream);
int gl_posnet_input_f32(const float* boxes, const float* masks, const float* emb, const float* null_pos, const float* null_xyxy,
                        int32_t rows, int32_t in_dim, int32_t num_freqs, float* out, void* stream);

/*
 * text_image grounding (GLIGEN's *_box_text_image checkpoints; text_image_grounding_net.py:41-62, interface.py:114-130), additive to ABI 15.
 *   gl_posnet_input_ti(_f32) : both MLP inputs of the text_image PositionNet in one launch, one block per (b, i) row:
 *                              out_text [rows, in_dim + 8 F]  = [ text_emb * tm + (1 - tm) * null_text    | xyxy ]
 *                              out_image[rows, in_dim + 8 F]  = [ image_emb * im + (1 - im) * null_image  | xyxy ]
 *                              xyxy = fourier(box) * m + (1 - m) * null_xyxy, computed once.  masks / text_masks / image_masks [rows] fp32;
 *                              fp16 outputs, or fp32 with _f32 (strict mode, then gl_split_f32).
 *   gl_image_ground_feature  : out[i, :] = norm * (feat[i, :] . P) / || feat[i, :] . P ||_2 in fp32: the CLIP image embedding projected into the
 *                              text feature space and rescaled (interface.py:126-129: project(feature, P.T) = feature @ P, / norm() * 28.7).
 *                              feat, out [n, dim], proj [dim, dim] row-major, fp32; dim <= 1024; one block per image.
 */
int gl_posnet_input_ti(const float* boxes, const float* masks, const float* text_masks, const float* image_masks, const float* text_emb,
                       const float* image_emb, const float* null_text, const float* null_image, const float* null_xyxy, int32_t rows,
                       int32_t in_dim, int32_t num_freqs, void* out_text, void* out_image, void* stream);
int gl_posnet_input_ti_f32(const float* boxes, const float* masks, const float* text_masks, const float* image_masks, const float* text_emb,
                           const float* image_emb, const float* null_text, const float* null_image, const float* null_xyxy, int32_t rows,
                           int32_t in_dim, int32_t num_freqs, float* out_text, float* out_image, void* stream);
int gl_image_ground_feature(const float* feat, const float* proj, int32_t n, int32_t dim, float norm, float* out, void* stream);

/*
 * keypoint grounding (checkpoint_generation_keypoint.pth; keypoint_grounding_net.py:34-58), additive to ABI 15.
 *   gl_posnet_input_kp(_f32) : the MLP input of the keypoint PositionNet, one block per (b, t) token row, t in [0, tokens), tokens = 17 P:
 *                              out[b * tokens + t, :] = [ (person_emb[t / 17] + keypoint_emb[t % 17]) * m + (1 - m) * null_person   (D)
 *                                                       | fourier(points[b, t]) * m + (1 - m) * null_xy                           (4 F)
 *                                                       | 0                                                                      (pad) ]
 *                              with row stride ld = D + 4 F rounded up to a multiple of 64 (the padded K of linears.0; the kernel writes the
 *                              pad columns).  fp32 arithmetic, table sum before the blend; m = masks[b, t] is a blend factor.  Fourier order
 *                              per frequency 100^(j / F): sin(f x), sin(f y), cos(f x), cos(f y).  points [B, tokens, 2], masks [B, tokens],
 *                              person_emb [P, D], keypoint_emb [17, D], null_person [D], null_xy [4 F], fp32; tokens % 17 == 0.
 *                              fp16 output, or fp32 with _f32 (strict mode, then gl_split_f32 over ld columns).
 */
int gl_posnet_input_kp(const float* points, const float* masks, const float* person_emb, const float* keypoint_emb, const float* null_person,
                       const float* null_xy, int32_t B, int32_t tokens, int32_t D, int32_t num_freqs, void* out, void* stream);
int gl_posnet_input_kp_f32(const float* points, const float* masks, const float* person_emb, const float* keypoint_emb, const float* null_person,
                           const float* null_xy, int32_t B, int32_t tokens, int32_t D, int32_t num_freqs, float* out, void* stream);

/* gl_silu_f16: y = silu(x) elementwise fp16 (emb_layers SiLU, openaimodel.py:173). n % 8 == 0. */
int gl_silu_f16(const void* x, void* y, int64_t n, void* stream);

/*
 * PLMS step (plms.py:110-163) on fp32 NCHW latents, sigma = 0.
 *   gl_cfg_combine : e = e_u + s * (e_c - e_u)  from the UNet output of the 2B batch [cond ; uncond] (plms.py:123)
 *   gl_plms_update : e' = c0*e + c1*e1 + c2*e2 + c3*e3 (then / div), pred_x0 = (x - s1m*e') / sqrt_at,
 *                    x_prev = sqrt_aprev * pred_x0 + dir_coef * e'                       (plms.py:126-161)
 *                    evaluated in the reference's operation order with FP contraction off.
 *   gl_pack_latent : x fp32 NCHW [B, C, hw] -> fp16 NHWC [reps*B, hw, Cpad] (zero channel padding), the
 *                    first-conv input for both CFG halves.  split != 0 (Cpad >= 3C): channels [0, C) = hi = fp16(x), [C, 2C) = fp16(x - hi),
 *                    [2C, 3C) = hi again -- with first-conv weights packed [Whi | Whi | Wlo] over those channels the conv computes
 *                    xhi.Whi + xlo.Whi + xhi.Wlo in the padding it carries anyway (the engine's weight table always holds that packing;
 *                    gl_set_option 38 = 0 feeds hi alone).
 */
int gl_cfg_combine(const float* eps2b, float guidance, int64_t n, float* e_out, void* stream);
int gl_plms_update(const float* x, const float* e, const float* e1, const float* e2, const float* e3,
                   float c0, float c1, float c2, float c3, float div, float sqrt_at, float s1m,
                   float sqrt_aprev, float dir_coef, int64_t n, float* x_prev, void* stream);
/* gl_ddim_update: everything of one DDIM step behind the UNet (ddim.py:115-135) in ONE launch, additive to ABI 15.  eps = the UNet output
 * fp32 [reps * n]: reps == 2 = the [cond ; uncond] batch, e = e_u + guidance * (e_c - e_u) (ddim.py:118); reps == 1: e = eps, guidance is
 * not read.  Then pred_x0 = (x - s1m * e) / sqrt_at (:128) and x_out = (sqrt_aprev * pred_x0 + dir_coef * e) + sigma * noise (:131-133, left
 * to right), in the reference's operation order with FP contraction off: given the same eps, bit-identical to the torch fp32 expression.
 * noise fp32 [n], or NULL = the reference's 0 * randn: the term is skipped (for finite values the bits of adding the zero), sigma is not
 * read.  pred_x0 fp32 [n] receives the x0 prediction, or NULL.  x_out may be x (the normal use), pred_x0 may be any operand: every element
 * is read before the same element is written.  n % 4 == 0 and 16-byte pointers take the float4 path, everything else the scalar one. */
int gl_ddim_update(const float* eps, const float* x, const float* noise, int32_t reps, float guidance, float sqrt_at, float s1m,
                   float sqrt_aprev, float dir_coef, float sigma, int64_t n, float* x_out, float* pred_x0, void* stream);
/* gl_dpmpp_update: everything of one DPM-Solver++(2M) step (Lu et al., arXiv 2211.01095, Algorithm 2, data prediction) behind the UNet in
 * ONE launch, additive to ABI 15.  eps fp32 [reps * n] as for gl_ddim_update (reps == 2: e = e_u + guidance * (e_c - e_u)).  Then
 * x0 = (x - s1m * e) / sqrt_at; D = w1 * x0 + w0 * x0_old; x_out = c_x * x + c_d * D, left to right with FP contraction off: given the same
 * eps, bit-identical to the torch fp32 expression.  x0_old fp32 [n], or NULL = a first-order step: the w0 term is skipped, D = w1 * x0, and
 * w0 must be 0 (w1 is 1 there; host.dpm_step_coefs).  x0_out fp32 [n] is required: it is the history of the next step.  No no-alias
 * promise: x_out may be x and x0_out may be x0_old (one history buffer is enough) -- every thread loads all of its operands before it
 * stores.  n % 4 == 0 and 16-byte pointers take the float4 path, everything else the scalar one; the grid is gl_ddim_update's.
 * GL_ERR_BAD_ARG: reps other than 1 or 2, n <= 0, NULL eps / x / x_out / x0_out, x0_old == NULL with w0 != 0. */
int gl_dpmpp_update(const float* eps, const float* x, const float* x0_old, int32_t reps, float guidance, float sqrt_at, float s1m,
                    float c_x, float c_d, float w1, float w0, int64_t n, float* x_out, float* x0_out, void* stream);
/* gl_cfg3_combine: classifier-free guidance with separate text and layout scales (the two-condition form of InstructPix2Pix, Brooks et al.,
 * arXiv 2211.09800, eq. 3), additive to ABI 15.  eps3b = the UNet output fp32 [3n] of the conditioning batch [cond ; text-only ; uncond]:
 * e_c saw the prompt and the grounding, e_t the prompt and the null grounding, e_u neither.
 *     e_out = (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t)
 * left to right with FP contraction off: given the same eps, bit-identical to the torch fp32 expression.  s_layout == s_text is
 * gl_cfg_combine's e_u + s * (e_c - e_u) up to rounding (e_t cancels); s_layout == 0 weights e_c by zero.  e_out fp32 [n] aliases nothing.
 * n % 4 == 0 and 16-byte pointers take the float4 path, everything else the scalar one; the grid is gl_ddim_update's.
 * GL_ERR_BAD_ARG, before any device call: n <= 0, NULL eps3b / e_out. */
int gl_cfg3_combine(const float* eps3b, float s_text, float s_layout, int64_t n, float* e_out, void* stream);
int gl_pack_latent(const float* x, int32_t B, int32_t C, int32_t hw, int32_t Cpad, int32_t reps, int32_t split, void* out,
                   void* stream);
/* gl_pack_latent_extra: gl_pack_latent over the channel concatenation of TWO sources (the first-conv input of an inpaint_mode UNet,
 * openaimodel.py:439: cat([x, inpainting_extra_input], dim=1)): x fp32 [B, C, hw] and extra fp32 [Bs, Ce, hw], Bs = 1 (one extra for every
 * sample) or B -> fp16 NHWC [reps*B, hw, Cpad].  With Ct = C + Ce: channels [0, Ct) = fp16 of [x | extra], zero behind; split != 0
 * (Cpad >= 3 Ct): [0, Ct) = hi, [Ct, 2 Ct) = fp16(v - hi), [2 Ct, 3 Ct) = hi again, zero behind -- the [Whi | Whi | Wlo | 0] first-conv packing
 * over the 9 concatenated channels.  Additive to ABI 15. */
int gl_pack_latent_extra(const float* x, const float* extra, int32_t B, int32_t Bs, int32_t C, int32_t Ce, int32_t hw, int32_t Cpad,
                         int32_t reps, int32_t split, void* out, void* stream);

/*
 * VAE decode stage (AutoencoderKL.decode autoencoder.py:40-44, Decoder.forward model.py:535-568).
 * It reuses gl_conv3x3 / gl_gemm / gl_groupnorm_* ; only two extra kernels exist:
 *   gl_latent_affine_pack : z fp32 NCHW -> fp16 NHWC (channel-padded) of post_quant_conv(z / scale_factor)
 *   gl_softmax_rows       : in-place row softmax(scale * x) over fp16 [rows, n]: the d = 512 single-head
 *                           AttnBlock (model.py:150-202) is two GEMMs around it.
 */
int gl_latent_affine_pack(const float* z, const float* w, const float* bias, float pre, int32_t B, int32_t C,
                          int32_t hw, int32_t Cpad, void* out, void* stream);
int gl_softmax_rows(void* x, int32_t rows, int32_t n, int32_t ld, float scale, void* stream);

/*
 * VAE encode stage and masked PLMS sampling (GLIGEN inpainting: AutoencoderKL.encode autoencoder.py:34-38, plms.py:95-99).
 *   gl_vae_posterior : h fp32 NCHW [B, Cin, hw] (Encoder.conv_out) -> quant_conv 1x1 in fp32 (w fp32 [2E, Cin], bias [2E]) -> mean, logvar =
 *                      the two halves, logvar clamped to [-30, 20], z = (mean + exp(logvar / 2) * noise) * scale (distributions.py:24-36),
 *                      z fp32 NCHW [B, E, hw]; mean (optional, may be NULL) receives the posterior mean.
 *   gl_latent_blend  : in place on x fp32 [B, C, hw]: x = (a * x0 + s * noise) * m + (1 - m) * x (q_sample, ldm.py:19-22, then the blend),
 *                      in torch's operation order with FP contraction off (bit-identical to the torch expression).  x0 and noise have
 *                      x0_batch (1 or B) samples of [C, hw], the mask mask_batch (1 or B) samples of [1, hw].
 */
int gl_vae_posterior(const float* h, const float* w, const float* bias, const float* noise, float scale, int32_t B, int32_t Cin,
                     int32_t E, int32_t hw, float* z, float* mean, void* stream);
int gl_latent_blend(float* x, const float* x0, const float* noise, const float* mask, float a, float s, int32_t B, int32_t C,
                    int32_t hw, int32_t x0_batch, int32_t mask_batch, void* stream);
/* gl_q_sample: the forward process at one timestep (ldm.py:19-22; gl_latent_blend's q_sample without the mask), additive to ABI 15 -- the
 * start of image-to-image sampling (SDEdit, Meng et al., arXiv 2108.01073): the encoded image noised to the timestep the truncated schedule
 * starts at.  x0 fp32 [x0_batch, chw] with x0_batch = 1 (one image for every sample) or B, noise / out fp32 [B, chw]:
 *     out[b] = a * x0[b or 0] + s * noise[b]
 * two products and their sum, each rounded separately, FP contraction off: bit-identical to the torch fp32 expression.  out may be noise (in
 * place on the running latent: every thread loads its operands before it stores); out must not overlap x0.  chw % 4 == 0 and 16-byte
 * pointers take the float4 path (a float4 stays inside one sample), everything else the scalar one; the grid is gl_ddim_update's.
 * GL_ERR_BAD_ARG, before any device call: NULL x0 / noise / out, B <= 0, chw <= 0, x0_batch neither 1 nor B. */
int gl_q_sample(const float* x0, const float* noise, float a, float s, int32_t B, int32_t chw, int32_t x0_batch, float* out, void* stream);

/* =====================================================================================================
 * Forward-level API ("what a C-ABI replacement must export underneath"): one handle per device per
 * thread owns the block plan, the packed weights' layout, the activation pool, the hoisted conditioning and the
 * captured hipGraphs, so that a host in ANY language can run UNetModel.forward (openaimodel.py:413-459) and a PLMS
 * step (plms.py:110-163) through plain C calls.  All data pointers are DEVICE pointers owned by the caller.
 * ===================================================================================================== */
typedef struct gl_unet_config {          /* UNetModel.__init__ arguments (openaimodel.py:234-262; coco2014.yaml:9-30) */
    int32_t in_channels, model_channels, out_channels, num_res_blocks;
    int32_t n_levels;            int32_t channel_mult[8];
    int32_t n_attn_res;          int32_t attention_resolutions[8];     /* downsample factors that carry a transformer */
    int32_t num_heads, context_dim;
    int32_t pos_in_dim, pos_out_dim, fourier_freqs;                    /* PositionNet (text_grounding_net.py:7-24) */
    int32_t max_objs;                                                  /* 30 (interface.py:158,425) */
    int32_t split_weights;       /* ABI 14.  != 0: EVERY matrix of the weight table is stored [Whi | Wlo] (Whi = fp16(W), Wlo = fp16(W - Whi); Linear
                                    rows [N, 2K], 3x3 convs [Cout, 2, Cin/64, 3, 3, 64]): the layout the strict mode (gl_set_handle_option 50) needs for
                                    its third pass x.Wlo -- with it the engine reproduces the reference's fp32 weights to ~22 bits.  The default
                                    mode of such a handle reads the Whi halves and computes what a handle without the flag computes; the table is
                                    twice the size (5 GB for the GLIGEN UNet).  0 = the compact table (only the 1x1 convs keep [Whi | Wlo]). */
    int32_t grounding;           /* additive to ABI 15.  0 = the text PositionNet (text_grounding_net.py; a zeroed field keeps the earlier behaviour);
                                    1 = the text_image PositionNet (text_image_grounding_net.py): the weight table holds position_net.linears_text.* /
                                    linears_image.* / null_text / null_image / null_xyxy, every box yields TWO grounding tokens (text, image), and the
                                    handle is conditioned through gl_set_conditioning_ti.  n_ground = max_objs (0) or 2 * max_objs (1) is the token count
                                    of the gated self-attention (keys N + n_ground); gl_create rejects n_ground > 64.  The relation chain keeps
                                    max_objs boxes.
                                    2 = the keypoint PositionNet (keypoint_grounding_net.py): max_objs counts grounding TOKENS, 17 per person, and must be
                                    a multiple of 17, at most 136 (8 persons); pos_in_dim is the person-feature width (= pos_out_dim).  The table holds
                                    position_net.person_emb [max_objs / 17, D], keypoint_emb [17, D], null_person [D], null_xy [4 F] (fp32) and
                                    linears.{0,2,4}, linears.0 with K = pos_in_dim + 4 F zero-padded to the next multiple of 64 (800 -> 832; each of
                                    the [Whi | Wlo] halves of a split_weights table on its own).  The handle is conditioned through
                                    gl_set_conditioning_kp.  Requires no_relation = 1 (the relation chain pools over boxes) and inpaint_mode = 0, else
                                    GL_ERR_UNSUPPORTED.
                                    4 = the spatial families (canny / hed / depth / normal): the tokenizer, a ConvNeXt run by the caller once per image,
                                    is NOT part of the handle: the table has no position_net.* entries and the handle is conditioned through
                                    gl_set_conditioning_tokens with the finished grounding tokens; max_objs counts those tokens, <= 64.  Requires
                                    no_relation = 1, inpaint_mode = 0 and split_weights = 0, else GL_ERR_UNSUPPORTED.  The channels of the grounding
                                    downsampler are not in this struct: gl_set_extra_channels.  3 is not assigned (GL_ERR_UNSUPPORTED). */
    int32_t inpaint_mode;        /* additive to ABI 15.  0 = the first conv reads the latent alone (a zeroed field keeps the earlier behaviour).  1 = GLIGEN's
                                    inpainting checkpoints (openaimodel.py:293-299, :436-439): input_blocks.0.0 is [mc, 2 * in_channels + 1, 3, 3] and reads
                                    cat([x, z0 * mask, mask]); in_channels stays the latent's channel count.  The packed weight keeps its [mc, 9 * 64] slot
                                    ([Whi | Whi | Wlo | 0] over 3 * 9 = 27 of the 64 padded channels), the table has no sd_first_conv.* entries (the conv is
                                    not restorable, :296), and every forward needs gl_set_inpaint_extra first.  gl_create rejects
                                    2 * in_channels + 1 > 64. */
    int32_t no_relation;         /* additive to ABI 15.  0 = every transformer block carries the rela_fuse chain (attention.py:398; a zeroed field keeps the
                                    earlier behaviour).  1 = the upstream GLIGEN block (attention_original.py:312-316: attn1 -> fuser -> attn2 -> ff), what
                                    every public GLIGEN checkpoint was trained on: the weight table has no *.rela_fuse.* entries, the conditioning entries
                                    accept relations == NULL and ignore R (no relation K/V hoists, no box rectangles), and a forward launches nothing of
                                    the relation chain -- the fuser's output (attn1's at fuser scale 0) goes straight to LayerNorm(norm2) -> attn2.  Any
                                    other value: gl_create returns GL_ERR_UNSUPPORTED.  Combines with grounding, inpaint_mode and split_weights. */
} gl_unet_config;

typedef struct gl_engine gl_engine;      /* opaque */

typedef struct gl_weight_info {          /* one packed tensor of the flat weight buffer */
    char name[160];                      /* e.g. "input_blocks.1.1.transformer_blocks.0.attn1.qkv.w" (weights.py naming) */
    int64_t offset, nbytes;              /* 256-byte aligned slot inside the flat buffer */
    int32_t dtype;                       /* 0 = fp16, 1 = fp32 */
    int32_t ndim;   int64_t shape[4];
} gl_weight_info;

/* gl_create builds the plan and the weight table (no GPU needed); gl_destroy frees pool, graphs and the handle. */
int gl_create(const gl_unet_config* cfg, gl_engine** out);
int gl_destroy(gl_engine* e);
/* The packed-weight layout is defined HERE (the host packer fills it): count, i-th entry, total bytes. */
int gl_num_weights(const gl_engine* e);
int gl_weight_at(const gl_engine* e, int32_t i, gl_weight_info* info);
int64_t gl_weights_bytes(const gl_engine* e);
/* gl_load_weights: `packed` = device buffer laid out per the table (stays owned by the caller and must outlive the
 * handle); has_sd_conv != 0 when the "sd_first_conv.*" slots are filled (GLIGEN/SD_input_conv_weight_bias.pth). */
int gl_load_weights(gl_engine* e, const void* packed, int64_t bytes, int32_t has_sd_conv, void* stream);
/* gl_set_conditioning: everything that depends only on the image's conditioning, hoisted out of the 102 forwards
 * (PositionNet tokens text_grounding_net.py:26-43, fuser.linear attention.py:228, attn2 / rela_fuse K,V projections
 * attention.py:124-125,348-349, integer box rectangles attention.py:321-346).  fp32 inputs: context [Bn, Lc, ctx],
 * relations [Bn, R, ctx], boxes [Bn, max_objs, 4], masks [Bn, max_objs], pos_emb [Bn, max_objs, pos_in_dim]; null
 * grounding = zeros (text_layout_tokinzer_input.py:47-62).  hw = latent side.  On a handle created with no_relation = 1 this entry,
 * _hw and _ti accept relations == NULL and ignore relations and R; on every other handle relations == NULL or R <= 0 is
 * GL_ERR_BAD_ARG. */
int gl_set_conditioning(gl_engine* e, const float* context, const float* relations, const float* boxes,
                        const float* masks, const float* pos_emb, int32_t Bn, int32_t Lc, int32_t R, int32_t hw,
                        void* stream);
/* gl_set_conditioning_hw: the same for a RECTANGULAR latent of h rows and w columns (ABI 15, additive).  gl_set_conditioning(.., hw) is
 * gl_set_conditioning_hw(.., hw, hw) minus the shape check below: a square through either entry takes the same launches, tiles and graph.
 * Shape rules: h and w must each be a positive multiple of 2^(number of downsamples) (8 for the shipped model and for the tiny test
 * architecture) -- with fewer the upsampled tensor no longer matches the skip tensor it is concatenated with, where the reference fails
 * too -- else GL_ERR_BAD_ARG, before anything is launched and without touching the handle's conditioning.  Box x coordinates scale with
 * the level's w and box y coordinates with its h (attention.py:322-328); the per-level rectangle buffers and the graph cache are keyed by
 * (h, w), so 64 x 96, 96 x 64 and 64 x 64 conditionings can alternate on one handle.  gl_unet_forward and gl_plms_step take the shape
 * from the conditioning: every [.., hw, hw] below reads [.., h, w].  Tested range: up to 9216 tokens (64 x 96, 96 x 64 and 96 x 96 at
 * 2B = 8). */
int gl_set_conditioning_hw(gl_engine* e, const float* context, const float* relations, const float* boxes,
                           const float* masks, const float* pos_emb, int32_t Bn, int32_t Lc, int32_t R, int32_t h, int32_t w,
                           void* stream);
/* gl_set_conditioning_ti: the conditioning of a text_image handle (gl_unet_config.grounding = 1; additive to ABI 15).  The six grounding
 * tensors of text_image_grounding_net.py:41: boxes [Bn, max_objs, 4], masks / text_masks / image_masks [Bn, max_objs], text_emb / image_emb
 * [Bn, max_objs, pos_in_dim], fp32; null grounding = all six zero (tokens of MLP(null features)).  The grounding tokens of sample b are
 * objs[b] = [objs_text (max_objs rows) | objs_image (max_objs rows)] (cat(dim=1), :62).  (h, w): the shape rule of gl_set_conditioning_hw.
 * The text entries on a text_image handle, and this entry on a text handle, return GL_ERR_BAD_ARG. */
int gl_set_conditioning_ti(gl_engine* e, const float* context, const float* relations, const float* boxes, const float* masks,
                           const float* text_masks, const float* image_masks, const float* text_emb, const float* image_emb, int32_t Bn,
                           int32_t Lc, int32_t R, int32_t h, int32_t w, void* stream);
/* gl_set_conditioning_kp: the conditioning of a keypoint handle (gl_unet_config.grounding = 2; additive to ABI 15).  points [Bn, max_objs, 2]
 * (x, y in [0, 1]; token t of a sample is keypoint t % 17 of person t / 17) and masks [Bn, max_objs], fp32 on the device; null grounding = both
 * zero.  One MLP chain over Bn * max_objs rows; no relations, no rectangles.  (h, w): the shape rule of gl_set_conditioning_hw.  The text and
 * text_image entries on a keypoint handle, and this entry on a handle of another family, return GL_ERR_BAD_ARG with a gl_last_error message
 * that names the right entry, before any pointer is read. */
int gl_set_conditioning_kp(gl_engine* e, const float* context, const float* points, const float* masks, int32_t Bn, int32_t Lc, int32_t h,
                           int32_t w, void* stream);
/* gl_set_inpaint_extra: the inpainting_extra_input of an inpaint_mode handle (gligen_inference.py:406-407: cat([z0 * mask, mask], dim=1)),
 * extra fp32 [Bs, in_channels + 1, h, w] on the device, Bs = 1 (one extra for every sample) or the number of samples Bn / reps.  It is copied
 * (stream-ordered) into a buffer of the handle's pool whose address the captured graphs read at replay time, so a new extra needs no new
 * capture.  Valid only after a conditioning call has fixed (h, w); a conditioning call with another (h, w) invalidates it.  On an inpaint
 * handle gl_unet_forward / gl_plms_step return GL_ERR_BAD_ARG (with a gl_last_error message, before anything is launched) while no extra is
 * set, when Bs is neither 1 nor Bn / reps, and for sd_conv != 0; on any other handle this entry returns GL_ERR_BAD_ARG with a message.
 * Additive to ABI 15. */
int gl_set_inpaint_extra(gl_engine* e, const float* extra, int32_t Bs, void* stream);
/* gl_set_conditioning_tokens: the conditioning of a spatial handle (gl_unet_config.grounding = 4; additive to ABI 15).  objs fp32
 * [Bn, max_objs, pos_out_dim] on the device: the grounding tokens as the family's PositionNet returns them (the null tokens in the unconditional
 * half).  Hoists fuser.linear(objs) and the context K / V exactly as the other entries do after their PositionNet.  (h, w): the shape rule of
 * gl_set_conditioning_hw.  On a handle of another family, and the other entries on a spatial handle: GL_ERR_BAD_ARG with a gl_last_error
 * message naming the right entry, before any pointer is read. */
int gl_set_conditioning_tokens(gl_engine* e, const float* context, const float* objs, int32_t Bn, int32_t Lc, int32_t h, int32_t w, void* stream);
/* gl_set_extra_channels: the output channels Ce of the grounding downsampler of a spatial handle (grounding = 4; GLIGEN's canny / depth /
 * normal checkpoints have 8, hed has 1; openaimodel_original.py: h = cat([x, downsample_net(grounding_extra_input)], 1)), set once after
 * gl_create.  gl_unet_config keeps its layout: the weight table does not depend on Ce (input_blocks.0.0 is [mc, in_channels + Ce, 3, 3] in
 * the same 64-padded slot and the sd_first_conv.* entries stay -- this first conv IS restorable), only the pack launch of a GLIGEN-conv
 * forward and the size of the extra buffer do.  0 (what a new handle has) = the first conv reads the latent alone.  On a handle of another
 * family, channels < 0 or in_channels + channels > 64: GL_ERR_UNSUPPORTED with a gl_last_error message.  Additive to ABI 15. */
int gl_set_extra_channels(gl_engine* e, int32_t channels);
/* gl_set_grounding_extra: the downsampled grounding_extra_input of a spatial handle with Ce > 0 extra channels (gl_set_extra_channels), extra fp32
 * [Bs, Ce, h, w] on the device, Bs = 1 or the number of samples Bn / reps; both CFG halves read the same extra (plms.py:118-121).  Copied
 * (stream-ordered) into a pool buffer like gl_set_inpaint_extra's.  A forward with sd_conv = 0 packs cat([x, extra]) for the GLIGEN conv and is
 * refused (GL_ERR_BAD_ARG, gl_last_error) while no extra is set for the current latent shape; a forward with sd_conv = 1 reads x alone. */
int gl_set_grounding_extra(gl_engine* e, const float* extra, int32_t Bs, void* stream);
/* gl_last_error: the message of the handle's last GL_ERR_BAD_ARG that carries one (a conditioning entry of the wrong grounding family, a
 * latent shape that breaks the shape rule, strict mode without split weights, the inpaint_mode checks of gl_set_inpaint_extra), copied NUL-terminated into dst (at most bytes - 1
 * characters).  Returns the message's full length, 0 when there is none.  With e == NULL it returns the calling thread's last message of
 * the entries that take no handle (gl_layout_reward, gl_policy_select, gl_policy_grad, gl_policy_adam_step).  Additive to ABI 15. */
int gl_last_error(const gl_engine* e, char* dst, int32_t bytes);
/* gl_unet_forward: eps[Bn, out_ch, hw, hw] fp32 = UNet(x, t | conditioning).  x fp32 NCHW [Bn / reps, in_ch, hw, hw]:
 * with reps = 2 both CFG halves of a [cond ; uncond] conditioning batch share the latent.  t_dev: fp32 [Bn] device
 * timesteps, or NULL to use t_host for every sample.  fuser_scale = what set_alpha_scale wrote (interface.py:34-38;
 * 0 skips the gated self-attention exactly); sd_conv != 0 = restore_first_conv_from_SD is in effect
 * (openaimodel.py:393-405).  Replays a hipGraph captured on first use of each (shape, fuser on/off, conv) variant
 * unless use_graph == 0. */
int gl_unet_forward(gl_engine* e, const float* x, const float* t_dev, float t_host, int32_t reps, float fuser_scale,
                    int32_t sd_conv, float* eps, int32_t use_graph, void* stream);
/* gl_plms_step: one denoiser evaluation + classifier-free guidance + the PLMS / DDIM-sigma-0 update
 * (plms.py:110-163): eps = UNet(x_eval, t); e_out = eps_u + guidance (eps_c - eps_u) (reps == 2) or eps;
 * e' = (sum_j coef[j] * e_terms[j]) / div over n_terms <= 4 terms (Adams-Bashforth forms plms.py:144-159; terms
 * may alias e_out); x_out = sqrt_aprev * (x_base - s1m e') / sqrt_at + dir_coef * e', evaluated in the
 * reference's operation order (bit-identical to torch fp32 given the same eps). */
typedef struct gl_plms_step_args {
    const float* x_eval;  const float* x_base;  float* x_out;       /* fp32 [B, C, hw, hw] */
    float* e_out;                                                    /* guided eps of this evaluation */
    const float* e_terms[4];  float coef[4];  int32_t n_terms;  float div;
    float t;  int32_t reps;  float guidance;  float fuser_scale;  int32_t sd_conv;
    float sqrt_at, s1m, sqrt_aprev, dir_coef;
    int32_t use_graph;
} gl_plms_step_args;
int gl_plms_step(gl_engine* e, const gl_plms_step_args* a, void* stream);
/* gl_ddim_step: one denoiser evaluation + one gl_ddim_update launch (ddim.py:111-135), additive to ABI 15: eps = UNet(x, t) into the handle's
 * own output buffer (graph-cached like gl_unet_forward), then x_out / pred_x0 from (eps, x, noise) as gl_ddim_update describes -- the CFG
 * combine is part of that launch, there is no guided-eps buffer.  x fp32 [Bn / reps, C, h, w]; x_out may be x; noise and pred_x0 may be
 * NULL.  Refuses what gl_plms_step refuses: NULL x / x_out, reps other than 1 or 2 (GL_ERR_BAD_ARG), in_channels != out_channels
 * (GL_ERR_UNSUPPORTED), and everything gl_unet_forward refuses. */
typedef struct gl_ddim_step_args {
    const float* x;  float* x_out;                                   /* fp32 [B, C, h, w] */
    const float* noise;  float* pred_x0;                             /* fp32 [B, C, h, w] or NULL */
    float t;  int32_t reps;  float guidance;  float fuser_scale;  int32_t sd_conv;
    float sqrt_at, s1m, sqrt_aprev, dir_coef, sigma;
    int32_t use_graph;
} gl_ddim_step_args;
int gl_ddim_step(gl_engine* e, const gl_ddim_step_args* a, void* stream);
int gl_sizeof_ddim_step_args(void);
/* gl_dpmpp_step: one denoiser evaluation + one gl_dpmpp_update launch, additive to ABI 15: eps = UNet(x, t) into the handle's own output
 * buffer (graph-cached like gl_unet_forward), then x_out / x0_out from (eps, x, x0_old) as gl_dpmpp_update describes.  x fp32
 * [Bn / reps, C, h, w]; x_out may be x, x0_out may be x0_old; x0_old NULL = a first-order step.  Refuses what gl_ddim_step refuses, and a
 * NULL x0_out or a NULL x0_old with w0 != 0 (GL_ERR_BAD_ARG) before the forward runs. */
typedef struct gl_dpmpp_step_args {
    const float* x;  float* x_out;                                   /* fp32 [B, C, h, w] */
    const float* x0_old;  float* x0_out;                             /* fp32 [B, C, h, w]; x0_old or NULL */
    float t;  int32_t reps;  float guidance;  float fuser_scale;  int32_t sd_conv;
    float sqrt_at, s1m, c_x, c_d, w1, w0;
    int32_t use_graph;
} gl_dpmpp_step_args;
int gl_dpmpp_step(gl_engine* e, const gl_dpmpp_step_args* a, void* stream);
int gl_sizeof_dpmpp_step_args(void);
/* gl_cfg3_eval: one three-branch denoiser evaluation + one gl_cfg3_combine launch, additive to ABI 15: eps = UNet(x, t) with reps = 3 over
 * the conditioning batch [cond ; text-only ; uncond] into the handle's own output buffer (graph-cached like gl_unet_forward), then
 * e_out = (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t).  It updates no latent: the caller hands e_out fp32 [Bn / 3, C, h, w] to
 * gl_plms_update, or to gl_ddim_update / gl_dpmpp_update with reps = 1.  The evaluation's fields are those of the step structs; reps must
 * be 3 (gl_plms_step / gl_ddim_step / gl_dpmpp_step keep refusing every reps but 1 and 2) and guidance is not read -- the scales are s_text
 * and s_layout.  The shared cond / uncond prefix (option 44) is a reps == 2 form and does not apply.  Refuses what those entries refuse:
 * NULL x / e_out, a reps other than its own (GL_ERR_BAD_ARG), in_channels != out_channels (GL_ERR_UNSUPPORTED), everything
 * gl_unet_forward refuses; and a conditioning batch that is no multiple of 3 (GL_ERR_BAD_ARG with a gl_last_error message), before
 * anything is launched. */
typedef struct gl_cfg3_eval_args {
    const float* x;  float* e_out;                                   /* fp32 [Bn / 3, C, h, w] */
    float t;  int32_t reps;  float guidance;  float fuser_scale;  int32_t sd_conv;
    float s_text, s_layout;
    int32_t use_graph;
} gl_cfg3_eval_args;
int gl_cfg3_eval(gl_engine* e, const gl_cfg3_eval_args* a, void* stream);
int gl_sizeof_cfg3_eval_args(void);
/* introspection for tests / tools */
int64_t gl_pool_bytes(const gl_engine* e);
int gl_num_launches(const gl_engine* e);       /* kernel launches of the last eagerly executed / captured forward */
int gl_sizeof_unet_config(void);
int gl_sizeof_weight_info(void);
int gl_sizeof_plms_step_args(void);

/*
 * gl_reward_score: the GPU part of Reward_Model.forward for the train_rl.py rollout (models/policy.py:106-135,
 * tools/aesthetic.py:15-31,52-57), given CLIP features [B, D] fp32 (D = 768 for ViT-L/14) of the captions, the generated
 * images and the ground-truth images:
 *   sims_ti = <norm(txt), norm(pred)>, sims_ii = <norm(gt), norm(pred)>            (F.normalize, eps 1e-12)
 *   aesthetic = AestheticMLP(normalized(norm(pred)))   five Linear layers D -> 1024 -> 128 -> 64 -> 16 -> 1, fp32 weights
 *   partial_reward (optional) = sims_ti + sims_ii + 0.1 * aesthetic; the caller adds 10 * mIoU + 10 * DocSim (CPU python)
 */
typedef struct gl_reward_args {
    const float* txt; const float* img_pred; const float* img_gt;   /* [B, D] */
    int32_t B, D;
    const float* w1; const float* b1;   /* [1024, D], [1024] */
    const float* w2; const float* b2;   /* [128, 1024] */
    const float* w3; const float* b3;   /* [64, 128]   */
    const float* w4; const float* b4;   /* [16, 64]    */
    const float* w5; const float* b5;   /* [1, 16], [1] */
    float* sims_ti; float* sims_ii; float* aesthetic; float* partial_reward;   /* [B] each */
} gl_reward_args;
int gl_reward_score(const gl_reward_args* a, void* stream);
int gl_sizeof_reward_args(void);

/*
 * gl_layout_reward: the layout half of Reward.forward (models/policy.py:126-135), i.e. compute_maximum_iou (tools/metrics.py:58-91, with
 * compute_iou :29-42) and compute_docsim (tools/metrics.py:93-164) of B (ground truth, prediction) layout pairs, which the reference runs in
 * CPU python with scipy's linear_sum_assignment.  One 64-lane wave per (sample, term), all arithmetic in double.  A layout is padded to
 * GL_LAYOUT_MAX_BOXES rows; label ids are what Reward.label_to_id (policy.py:74-82) produces.  The reference's behaviour is kept, accidents
 * included: the four numbers of a box are (l, t, r, b) to the IoU and (cx, cy, w, h) to DocSim, and the matrices are filled in
 * np.meshgrid's 'xy' order (flat entry k = f(box1[k % n], box2[k / n]), reshaped to n x m).
 *   miou[b]   = sum over the distinct ground-truth labels of the best assignment's IoU sum, / n_gt[b]
 *   docsim[b] = mean of the best assignment's box similarities; 0 when the counts differ by 3 or more, or nothing is assigned
 * A term whose matrix holds a NaN (the IoU of two zero-area boxes) is NaN for that sample only; the reference raises from scipy there.
 * The counts are given twice: device arrays the kernel reads, and HOST arrays with the same values that this entry validates, so that
 * it returns GL_ERR_BAD_ARG, before anything is launched and with a message gl_last_error(NULL, ...) returns, for a null pointer, B < 1,
 * a count outside [0, GL_LAYOUT_MAX_BOXES] and n_gt == 0 (the reference: ZeroDivisionError).  Additive to ABI 15.
 */
#define GL_LAYOUT_MAX_BOXES 64
typedef struct gl_layout_reward_args {
    const double* boxes_gt; const double* boxes_pred;       /* device [B, 64, 4] */
    const int32_t* labels_gt; const int32_t* labels_pred;   /* device [B, 64] */
    const int32_t* n_gt; const int32_t* n_pred;             /* device [B]: boxes per layout */
    const int32_t* n_gt_host; const int32_t* n_pred_host;   /* HOST [B]: the same counts, read by the entry only */
    int32_t B;
    double* miou; double* docsim;                           /* device [B] */
} gl_layout_reward_args;
int gl_layout_reward(const gl_layout_reward_args* a, void* stream);
/* sizeof(gl_layout_reward_args), for the binding's layout check (tests/test_layout_host.py).  Replaces nothing of the reference (the
 * arguments of metrics.py:77-82,146-151 are Python lists).  Additive to ABI 15. */
int gl_sizeof_layout_reward_args(void);

/*
 * gl_policy_select: the scoring and ranking half of the policy's example selection (models/policy.py:11-33 with train_rl.py:167-172 and
 * txt2img.py:472-474, :429), which the reference runs as two nn.Linear calls and a torch.mm in fp32 and a Python sort on the host.
 *   scores[p, n] = (W prompt_p + bias) . (W cand_n + bias)                    fp32 [P, N]
 *   topk[p, 0 .. k)  = the k best candidate indices of prompt p, best first; equal scores: the lower index first (the stable
 *                      sorted(..., reverse=True)[:k] of txt2img.py:429); with k > N the first N slots are filled, the rest hold -1.
 *                      A NaN score ranks below every number, -inf included, lower index first (the reference's order with a NaN is
 *                      unspecified: Python's sort under an inconsistent comparison).  -0 and +0 rank as equal.
 *   probs[p, :]      = softmax(scores[p, :] / temperature) (train_rl.py:172), when probs != NULL: computed from the scores in DOUBLE (a second
 *                      pass over the pool with the unrounded fold) and rounded to fp32 once, so that the fp32 scores' rounding does not enter
 * The product is linear in the candidate, so the pool is not projected: q_p = W prompt_p + bias, v_p = W^T q_p and c_p = q_p . bias are
 * computed per call (summed in double, v and c stored as fp32) and scores[p, n] = v_p . cand_n + c_p streams the pool once per group of 8
 * prompts with 16-byte loads, fp32 fmaf and a 64-lane butterfly sum.  A row's score does not depend on its position, on N or on the grid: equal rows get bit-equal scores.  The top-k
 * runs in two stages (per 64-row block into scratch, then one merge block per prompt) without atomics; the result is deterministic.
 * W == NULL is the identity (add_linear=False): E must equal D, bias is not read.
 * Stream-ordered, no host synchronisation; the caller provides the scratch: gl_policy_scratch_bytes(P, N, D, E, k, W == NULL, probs != NULL) bytes of
 * device memory, 16-byte aligned like prompt, cand and W.  GL_ERR_BAD_ARG, before anything is launched and with a message
 * gl_last_error(NULL, ...) returns: a null pointer (args, prompt, cand, scores, bias with W, topk with k > 0, scratch), P outside
 * [1, GL_POLICY_MAX_PROMPTS], N < 1, D not a multiple of 4 or above GL_POLICY_MAX_DIM, E outside [1, GL_POLICY_MAX_DIM] (or != D with
 * W == NULL), k outside [0, GL_POLICY_MAX_SHOTS], temperature <= 0 (or NaN) with probs, a scratch that is too small, a misaligned pointer.
 * Additive to ABI 15.
 */
#define GL_POLICY_MAX_PROMPTS 64
#define GL_POLICY_MAX_DIM 1024
#define GL_POLICY_MAX_SHOTS 32
typedef struct gl_policy_args {
    const float* prompt;        /* device [P, D] */
    const float* cand;          /* device [N, D] */
    const float* W;             /* device [E, D], NULL = identity */
    const float* bias;          /* device [E] (not read when W == NULL) */
    int32_t P, N, D, E, k;
    double temperature;         /* read when probs != NULL */
    float* scores;              /* device [P, N] */
    int32_t* topk;              /* device [P, k] (may be NULL when k == 0) */
    float* probs;               /* device [P, N] or NULL */
    void* scratch; int64_t scratch_bytes;
} gl_policy_args;
int gl_policy_select(const gl_policy_args* a, void* stream);
/* sizeof(gl_policy_args), for the binding's layout check (tests/test_policy_host.py).  Additive to ABI 15. */
int gl_sizeof_policy_args(void);
/* bytes of scratch gl_policy_select needs for these sizes (identity != 0: W == NULL; probs != 0: probabilities asked for); GL_ERR_BAD_ARG for a
 * size below 1 (k below 0).
 * Replaces nothing of the reference.  Additive to ABI 15. */
int64_t gl_policy_scratch_bytes(int32_t P, int32_t N, int32_t D, int32_t E, int32_t k, int32_t identity, int32_t probs);

/*
 * gl_policy_grad: the REINFORCE loss of one rollout batch and its gradient to the policy layer (train_rl.py:167-172, :85-95 followed by
 * loss.backward(), :183), which the reference builds from two nn.Linear calls, a torch.mm, F.softmax and torch.log in fp32 and autograd.
 *   q_p = W prompt_p + bias,  c_n = W cand_n + bias,  z[p, n] = q_p . c_n / temperature
 *   logp[p]  = sum_j (z[p, sel[p, j]] - logsumexp_n z[p, :])                  double [P]
 *   loss     = -sum_p reward[p] logp[p]                                        double [1]
 *   grad_W   = d loss / d W  fp32 [E, D],   grad_b = d loss / d bias  fp32 [E]
 * with G[p, n] = -(reward[p] / temperature) (m[p, n] - k_p pi[p, n]), m[p, n] = how often n occurs in sel[p, :], k_p = the valid entries of
 * sel[p, :], pi = softmax(z): dQ = G C, dC = G^T Q, grad_W = dQ^T prompt + dC^T cand, grad_b = the column sums of dQ and dC.
 * An entry of sel outside [0, N) is skipped: it contributes nothing and is not counted in k_p (a row with fewer examples, a padded row);
 * no index read from device memory addresses outside the pool.  A repeated index counts as often as it occurs, as the reference's loop does.
 * reward is double, as the reference's is (its mIoU term comes from numpy).
 * All arithmetic is in double from the fp32 operands; the log-softmax is z - logsumexp(z), finite where the reference's fp32
 * log(softmax(z)) is -inf; grad_W and grad_b are rounded to fp32 once.  Four launches, no atomics, every sum in an order fixed by the sizes:
 * two calls on the same inputs give bit-equal outputs, and logp[p] does not depend on the row's index.
 * Stream-ordered, no host synchronisation; the caller provides gl_policy_grad_scratch_bytes(P, N, D, E, k) bytes of device memory, 16-byte
 * aligned like prompt, cand and W: three arrays of doubles, each rounded up to 256 bytes: [P + N, E] projections, [P, N] scores / G, [P + N, E] dQ and dC.
 * GL_ERR_BAD_ARG, before anything is launched and with a message gl_last_error(NULL, ...) returns: a null pointer (W included: the identity
 * policy has nothing to train), P outside [1, GL_POLICY_MAX_PROMPTS], N outside [1, GL_POLICY_TRAIN_MAX_CANDS], D not a multiple of 4 or above
 * GL_POLICY_MAX_DIM, E outside [1, GL_POLICY_MAX_DIM], k outside [1, GL_POLICY_MAX_SHOTS], temperature <= 0 (or NaN), a scratch that is too
 * small, a misaligned prompt / cand / W / scratch.  Additive to ABI 15.
 */
#define GL_POLICY_TRAIN_MAX_CANDS 4096
typedef struct gl_policy_grad_args {
    const float* prompt;        /* device [P, D] */
    const float* cand;          /* device [N, D] */
    const float* W;             /* device [E, D] */
    const float* bias;          /* device [E] */
    const int32_t* sel;         /* device [P, k]: the sampled candidate indices; outside [0, N) = skipped */
    const double* reward;       /* device [P] */
    int32_t P, N, D, E, k;
    double temperature;
    double* loss;               /* device [1] */
    double* logp;               /* device [P] */
    float* grad_W;              /* device [E, D] */
    float* grad_b;              /* device [E] */
    void* scratch; int64_t scratch_bytes;
} gl_policy_grad_args;
int gl_policy_grad(const gl_policy_grad_args* a, void* stream);
/* sizeof(gl_policy_grad_args), for the binding's layout check (tests/test_policy_train_host.py).  Additive to ABI 15. */
int gl_sizeof_policy_grad_args(void);
/* bytes of scratch gl_policy_grad needs for these sizes; GL_ERR_BAD_ARG for a size gl_policy_grad refuses.  Additive to ABI 15. */
int64_t gl_policy_grad_scratch_bytes(int32_t P, int32_t N, int32_t D, int32_t E, int32_t k);

/*
 * gl_policy_adam_step: one torch.optim.Adam step with the reference's settings (train_rl.py:119: weight_decay = 0, no amsgrad) on the policy
 * layer, in place, with the fp32 state exp_avg / exp_avg_sq of both tensors.  step is the step number AFTER the increment (>= 1).  Per
 * element, in double from the fp32 values, each stored value rounded to fp32 once:
 *   m = m + (g - m) (1 - beta1);   v = beta2 v + (1 - beta2) g^2
 *   p = p - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * One elementwise launch over the E D + E elements, stream-ordered.  GL_ERR_BAD_ARG, before anything is launched and with a message
 * gl_last_error(NULL, ...) returns: a null pointer, D or E out of gl_policy_grad's range, step < 1, lr or eps negative, infinite or NaN, a beta
 * outside [0, 1).  Additive to ABI 15.
 */
typedef struct gl_policy_adam_args {
    float* W; float* bias;                          /* device [E, D], [E]: updated in place */
    const float* grad_W; const float* grad_b;
    float* exp_avg_W; float* exp_avg_sq_W;          /* device [E, D] */
    float* exp_avg_b; float* exp_avg_sq_b;          /* device [E] */
    int32_t D, E;
    int64_t step;
    double lr, beta1, beta2, eps;
} gl_policy_adam_args;
int gl_policy_adam_step(const gl_policy_adam_args* a, void* stream);
/* sizeof(gl_policy_adam_args), for the binding's layout check.  Additive to ABI 15. */
int gl_sizeof_policy_adam_args(void);

int gl_gemm(const gl_gemm_args* a, void* stream);
int gl_conv3x3(const gl_conv_args* a, void* stream);
/* The VAE encoder's Downsample (model.py:60-79): F.pad(x, (0, 1, 0, 1)) then a 3x3 conv with stride 2 and pad 0, i.e. output (oy, ox)
 * reads input rows 2oy .. 2oy+2 and columns 2ox .. 2ox+2 with zeros at row Hin / column Win.  Needs stride == 2, upsample2x == 0,
 * in_split == 0 and Hout = Hin / 2, Wout = Win / 2 (GL_ERR_BAD_ARG otherwise); dispatched like gl_conv3x3. */
int gl_conv3x3_pad01(const gl_conv_args* a, void* stream);
int gl_attention(const gl_attn_args* a, void* stream);

/*
 * VAE decode stage behind a forward-level handle: AutoencoderKL.decode (GLIGEN/ldm/models/autoencoder.py:40-44)
 * = Decoder.forward (GLIGEN/ldm/modules/diffusionmodules/model.py:535-568) on z / scale_factor after post_quant_conv.
 * Same contract as the UNet handle: gl_vae_create builds the plan and the LIBRARY-DEFINED flat weight layout (no GPU needed;
 * gl_vae_num_weights / gl_vae_weight_at / gl_vae_weights_bytes; packed forms: 3x3 convs fp16 [Cout, Cin/64, 3, 3, 64] with the
 * latent's channels zero-padded to 64, 1x1 convs fp16 [N, K] with C^-0.5 folded into mid.attn_1.q, norm affine / biases /
 * post_quant_conv fp32), gl_vae_load_weights references a DEVICE buffer in that layout (the caller keeps it alive),
 * gl_vae_decode runs z fp32 [B, z_channels, side, side] -> out fp32 [B, out_ch, side * 2^(n_mult-1), ...] (device pointers),
 * as one hipGraph per (B, side) when use_graph != 0.  One handle per device per thread.
 */
typedef struct gl_vae_config {
    int32_t ch;                  /* ddconfig.ch (128) */
    int32_t ch_mult[8];          /* ddconfig.ch_mult (1, 2, 4, 4) */
    int32_t n_mult;              /* len(ch_mult) */
    int32_t num_res_blocks;      /* ddconfig.num_res_blocks (2) */
    int32_t z_channels;          /* 4 */
    int32_t out_ch;              /* 3 */
    int32_t embed_dim;           /* 4 (post_quant_conv input channels) */
    float scale_factor;          /* 0.18215 */
} gl_vae_config;
typedef struct gl_vae gl_vae;
int gl_vae_create(const gl_vae_config* cfg, gl_vae** out);
int gl_vae_destroy(gl_vae* v);
int gl_vae_num_weights(const gl_vae* v);
int gl_vae_weight_at(const gl_vae* v, int32_t i, gl_weight_info* info);
int64_t gl_vae_weights_bytes(const gl_vae* v);
int gl_vae_load_weights(gl_vae* v, const void* packed, int64_t bytes, void* stream);
int gl_vae_decode(gl_vae* v, const float* z, int32_t B, int32_t side, float* out, int32_t use_graph, void* stream);
/* gl_vae_decode_hw: z fp32 [B, z_channels, h, w] -> out fp32 [B, out_ch, f * h, f * w], f = 2^(n_mult-1); one hipGraph per (B, h, w), the
 * mid-block attention over h * w tokens.  gl_vae_decode(.., side) == gl_vae_decode_hw(.., side, side). */
int gl_vae_decode_hw(gl_vae* v, const float* z, int32_t B, int32_t h, int32_t w, float* out, int32_t use_graph, void* stream);
int gl_vae_num_launches(const gl_vae* v);
int64_t gl_vae_pool_bytes(const gl_vae* v);
int gl_sizeof_vae_config(void);
/*
 * VAE encode stage on the same handle type: AutoencoderKL.encode (autoencoder.py:34-38) = Encoder.forward (model.py:368-459, no
 * down-level attention), quant_conv and DiagonalGaussianDistribution.sample() * scale_factor.  gl_vae_encoder_create builds an
 * ENCODER handle (plan and flat weight table need no GPU; encoder.* / quant_conv.* in the decoder's packed forms, image channels =
 * out_ch, the 3x3 conv_in input zero-padded to 64 channels, quant_conv fp32).  gl_vae_encode maps x fp32 [B, out_ch, side, side]
 * -> z fp32 [B, embed_dim, side / f, side / f], f = 2^(n_mult-1), with the caller's posterior noise fp32 [B, embed_dim, side / f,
 * side / f]; side must be a multiple of f below 1024 (GL_ERR_BAD_ARG otherwise), one hipGraph per (B, side).  The
 * weight-table / load / option / launch-count / pool / destroy entries above apply unchanged; gl_vae_decode on an encoder handle and
 * gl_vae_encode on a decoder handle return GL_ERR_BAD_ARG.
 */
int gl_vae_encoder_create(const gl_vae_config* cfg, gl_vae** out);
int gl_vae_encode(gl_vae* v, const float* x, int32_t B, int32_t side, const float* noise, float* z, int32_t use_graph, void* stream);
/* gl_vae_encode_hw: x fp32 [B, out_ch, h, w] -> z fp32 [B, embed_dim, h / f, w / f] with noise of z's shape; h and w each a multiple of f
 * below 1024 (GL_ERR_BAD_ARG otherwise), one hipGraph per (B, h, w); the stride-2 Downsample pads one row below and one column right per
 * axis.  gl_vae_encode(.., side) == gl_vae_encode_hw(.., side, side). */
int gl_vae_encode_hw(gl_vae* v, const float* x, int32_t B, int32_t h, int32_t w, const float* noise, float* z, int32_t use_graph,
                     void* stream);

/*
 * CLIP towers of the reward stage: transformers.CLIPModel.get_image_features / get_text_features as the
 * reference's Reward_Model calls them (models/policy.py:106-113).  Projections / MLPs / LayerNorms / the vision tower's
 * attention run on gl_gemm / gl_layernorm / gl_attention; these are the tower-specific pieces.
 *   gl_clip_patchify      CLIPVisionEmbeddings.patch_embedding as a GEMM operand: pixel_values fp32 [B, 3, S, S] -> fp16
 *                         [B * (S/patch)^2, Kpad], K index (c * patch + i) * patch + j, zero-padded to Kpad (% 64 == 0)
 *   gl_clip_assemble      x[b, 0] = class_embedding, x[b, 1 + p] = patch_emb[b * (T-1) + p]; x += position_embedding; then, when
 *                         ln_gamma != NULL, x = LayerNorm(x) in fp32 (the vision tower's pre_layrnorm, whose OUTPUT is the start of
 *                         the fp32 residual stream); fp32 [B, T, C], C <= 4096
 *   gl_clip_embed_tokens  CLIPTextEmbeddings: x[b, t] = token_embedding[ids[b, t]] + position_embedding[t]; fp32 [B, T, C]
 *   gl_clip_gather_rows   out[b] = x[rows[b]]   (class-token rows / EOS rows = input_ids.argmax(-1)), fp32
 *   gl_attention_small    softmax(scale * q k^T [+ causal mask]) v for T <= 128, d <= 64; q / k / v fp16 rows of stride ld with head
 *                         h at column h * d (e.g. the three column blocks of a fused q|k|v projection), fp32 arithmetic;
 *                         the text tower's causal attention (create_causal_mask, CLIPTextModel.forward)
 */
int gl_clip_patchify(const float* pixel_values, int32_t B, int32_t S, int32_t patch, int32_t Kpad, void* out, void* stream);
int gl_clip_assemble(const void* patch_emb, int32_t ldpe, const float* class_emb, const float* pos_emb, int32_t B, int32_t T,
                     int32_t C, const float* ln_gamma, const float* ln_beta, float ln_eps, float* x, void* stream);
int gl_clip_embed_tokens(const int32_t* ids, const float* tok_emb, const float* pos_emb, int32_t B, int32_t T, int32_t C,
                         int32_t vocab, float* x, void* stream);
int gl_clip_gather_rows(const float* x, int32_t ldx, const int32_t* rows, int32_t B, int32_t C, float* out, void* stream);
int gl_attention_small(const void* q, const void* k, const void* v, int32_t ld, int32_t B, int32_t T, int32_t H, int32_t d,
                       float scale, int32_t causal, void* out, int32_t ldo, void* stream);

/*
 * Spatial grounding (GLIGEN's canny / hed / depth / normal checkpoints), additive to ABI 15: the stages of the ConvNeXt tokenizer
 * ({canny,hed,depth,normal}_grounding_net.py, convnext.py) around gl_gemm, and the grounding downsampler.  Run once per image.
 *   gl_sp_stem_patchify : map fp32 [B, 3, S, S] -> F.interpolate(map, R) (nearest: src = min(floor(dst * (float)S / R), S - 1)) -> fp16 rows
 *                         [B * (R/4)^2, 64] of the 4x4 stride-4 stem conv, K index (c * 4 + i) * 4 + j, columns 48..63 zero.  R % 4 == 0.
 *   gl_sp_layernorm     : y[r, :] = LayerNorm(x[r, :]) over C, eps 1e-6, fp32 in and out (y may be x).
 *   gl_sp_dwconv_ln     : x fp32 NHWC [B, H, W, C] -> depthwise 7x7 (pad 3, zero border; w fp32 [49, C] tap-major, bias [C]) -> LayerNorm over C
 *                         (eps 1e-6) -> fp16 rows [B * H * W, ldo], ldo % 64 == 0, ldo >= C, columns [C, ldo) written as zeros.  C <= 768.
 *   gl_sp_gelu          : y = 0.5 x erfc(-x / sqrt 2) (erf-GELU), fp16 in and out, fp32 arithmetic; n even.
 *   gl_sp_down_gather   : x fp32 NHWC -> per-pixel LayerNorm (eps 1e-6) -> fp16 rows [B * H/2 * W/2, 4 C], pixel (2 oy + ky, 2 ox + kx) at columns
 *                         [(ky * 2 + kx) * C, + C).  H, W even.
 *   gl_sp_assemble      : out[b * T + t, :] = feat[b * T + t, :] * mask[b] + null_feature * (1 - mask[b]) + pos[t, :], fp32 in, fp16 out.
 *   gl_sp_bicubic       : out[b, c, oy, ox] = sum_i wy[oy, i] sum_j wx[ox, j] in[b, c, iy[oy, i], ix[ox, j]] for the first C of the input's Ct
 *                         channels; iy / ix int32 [Hout | Wout, 4] clamped source indices, wy / wx fp32 [.., 4] (torch's bicubic: align_corners
 *                         False, A = -0.75, no antialias -- built by the host).  fp32.
 *   gl_sp_conv4x4s2     : Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW with an optional SiLU, Ci, Co <= 8, Hin, Win even.
 */
int gl_sp_stem_patchify(const float* map, int32_t B, int32_t S, int32_t R, void* out, void* stream);
int gl_sp_layernorm(const float* x, int64_t rows, int32_t C, const float* gamma, const float* beta, float* y, void* stream);
int gl_sp_dwconv_ln(const float* x, const float* w, const float* bias, const float* ln_gamma, const float* ln_beta, int32_t B, int32_t H,
                    int32_t W, int32_t C, int32_t ldo, void* out, void* stream);
int gl_sp_gelu(const void* x, void* y, int64_t n, void* stream);
int gl_sp_down_gather(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* ln_gamma, const float* ln_beta, void* out,
                      void* stream);
int gl_sp_assemble(const float* feat, const float* mask, const float* null_feature, const float* pos, int32_t B, int32_t T, int32_t C,
                   void* out, void* stream);
int gl_sp_bicubic(const float* in, int32_t B, int32_t Ct, int32_t C, int32_t Hin, int32_t Win, const int32_t* iy, const float* wy,
                  const int32_t* ix, const float* wx, int32_t Hout, int32_t Wout, float* out, void* stream);
int gl_sp_conv4x4s2(const float* in, const float* w, const float* bias, int32_t B, int32_t Ci, int32_t Co, int32_t Hin, int32_t Win,
                    int32_t silu, float* out, void* stream);

/*
 * Semantic-map grounding (GLIGEN's checkpoint_generation_sem.pth), additive to ABI 15.  On the engine a sem model is a spatial handle
 * (grounding = 4, gl_set_conditioning_tokens, gl_set_extra_channels(8), gl_set_grounding_extra); these three entries are its front end, run
 * once per image.  The reference convolves a fp32 one-hot tensor [B, classes, 512, 512]; a convolution over a one-hot input is a table
 * lookup, so the input here is the uint8 class map and the one-hot tensor is never built.
 *   gl_sem_gather_conv  : map uint8 [B, Hs, Ws] (class ids) -> nearest resize to R x R (the expression of gl_sp_stem_patchify, per axis) ->
 *                         Conv2d(classes, Co, K, stride, pad) of its one-hot (+ SiLU when silu != 0) -> out fp32 [B, Co, Ro, Ro],
 *                         Ro = (R + 2 pad - K) / stride + 1:  out[b, co, y, x] = bias[co] + sum over taps inside the R x R image of
 *                         table[class][ky * K + kx][co].  table fp32 [classes][K * K][CoP], CoP = Co rounded up to a multiple of 4, the pad
 *                         columns zero, 16-byte aligned (the conv weight [Co, classes, K, K] permuted by the host).  A class id >= classes is
 *                         clamped to classes - 1, so no read leaves the table (the host refuses such a map).  GL_ERR_BAD_ARG: a null pointer,
 *                         classes outside 2..256, K outside 1..4, stride not 1 or 2, pad >= K, Co outside 1..16, an odd R with stride 2, a
 *                         misaligned table, more than 2^31 blocks.
 *   gl_sem_conv4x4s2    : Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW, no activation (the downsampler's second conv, 16 -> 8), Ci, Co <= 64, Hin, Win
 *                         even; gl_sp_conv4x4s2 keeps its limit of 8 channels.
 *   gl_sem_onehot_index : x fp32 [B, C, H, W] -> out uint8 [B, H, W] = argmax over C (the first maximum), and bad int32 [B] = the number of
 *                         pixels of each sample that are not exactly one-hot (one channel == 1.0, every other == 0.0); bad is zeroed by the
 *                         entry, on the stream.  2 <= C <= 256, B <= 65535.
 */
int gl_sem_gather_conv(const uint8_t* map, int32_t B, int32_t Hs, int32_t Ws, int32_t R, const float* table, const float* bias,
                       int32_t classes, int32_t K, int32_t stride, int32_t pad, int32_t Co, int32_t silu, float* out, void* stream);
int gl_sem_conv4x4s2(const float* in, const float* w, const float* bias, int32_t B, int32_t Ci, int32_t Co, int32_t Hin, int32_t Win,
                     float* out, void* stream);
int gl_sem_onehot_index(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* out, int32_t* bad, void* stream);

/* ---- image preprocessing of the reward stage (models/policy.py:108-111: self.processor(images=...), the HuggingFace CLIP
 * feature extractor on PIL images; transformers 4.19.2 image_utils + Pillow) -- on the GPU, so rollout images stay in HBM
 * between the VAE decoder and the CLIP vision tower.
 *   gl_image_to_u8      decoded image fp32 [B, 3, H, W] in [-1, 1] -> uint8 [B, H, W, 3] with the arithmetic of
 *                       GLIGEN/interface.py:543-547 (clamp, * 0.5 + 0.5, * 255, truncation): the pixels of the PIL image there
 *   gl_resample_h_u8    Pillow's horizontal BICUBIC pass (src/libImaging/Resample.c ImagingResampleHorizontal_8bpc), bit-exact:
 *                       out[b, y, xx, c] = clip8((2^21 + sum_{k < bounds[xx][1]} in[b, y, bounds[xx][0] + k, c] * coeffs[xx][k]) >> 22);
 *                       bounds int32 [Wout, 2] and coeffs int32 [Wout, ksize] are DEVICE arrays built by the host
 *                       (layoutllm_t2i_amd/preprocess.py: Pillow's precompute_coeffs + normalize_coeffs_8bpc in float64)
 *   gl_resample_v_norm  Pillow's vertical pass on that 8-bit intermediate, restricted to the centre-crop window
 *                       [top, top + crop_h) x [left, left + crop_w) of the resized image, followed by the feature extractor's
 *                       float32(u8) / 255 -> (x - mean) / std -> channels first: fp32 [B, 3, crop_h, crop_w] (out_nchw) and / or the
 *                       cropped uint8 pixels [B, crop_h, crop_w, 3] (out_u8_hwc, for tests); mean3 / std3 are HOST pointers (3 floats). */
int gl_image_to_u8(const float* img_nchw, int32_t B, int32_t H, int32_t W, uint8_t* out_hwc, void* stream);
int gl_resample_h_u8(const uint8_t* in, int32_t B, int32_t H, int32_t W, const int32_t* bounds, const int32_t* coeffs, int32_t ksize,
                     int32_t Wout, uint8_t* out, void* stream);
int gl_resample_v_norm(const uint8_t* in, int32_t B, int32_t H, int32_t W, const int32_t* bounds, const int32_t* coeffs, int32_t ksize,
                       int32_t Hout, int32_t top, int32_t left, int32_t crop_h, int32_t crop_w, const float* mean3, const float* std3,
                       float* out_nchw, uint8_t* out_u8_hwc, void* stream);

/* introspection: ABI version and struct sizes (checked by the host loader) */
int gl_abi_version(void);
int gl_sizeof_gemm_args(void);
int gl_sizeof_conv_args(void);
int gl_sizeof_attn_args(void);
int gl_sizeof_gn_args(void);
/* tuning knobs for A/B measurements (results do not depend on them beyond fp32 summation order in split-K):
 * key 2 = GEMM tile shape policy (0 auto, 1 force 128x128, 2 prefer 128x160); key 3 = attention block shape (0 auto,
 * 3 always 8 waves, 4 always 4 waves); keys 4-7 = small-tile / split-K / 256-row-tile thresholds; key 8 = short-K GEGLU
 * GEMMs on the BK 32 / 4-blocks-per-CU variant (1 default, 0 off); key 10 = s_setprio around the attention MFMA
 * clusters (-1 auto, 0 off, 1 on); key 13 = intra-block K-split GEMM/conv variants (0 off, 1 auto = default, 2 always);
 * key 16 = GroupNorm apply pixels per block; key 17 = single-launch GroupNorm kernels (1 default: small maps + group bundles up to 80 KB per block, 2 = small maps only, 0 off); key 20 = (tests) execute the gated-SA fuser even at fuser_scale 0;
 * key 21 = V^T written by the QKV GEMM epilogue (1, default) or by gl_transpose_v (0); key 23 = output-tile order (0 N-tiles
 * fastest, 1 = default: M-tiles fastest when the weight matrix is the larger operand, so each XCD's L2 streams only its
 * slice of the weights, 2 always M-fastest); key 24 = skinny-GEMM kernel (M <= 1024 rows, register operands, four waves split
 * K) while its operand re-reads stay below this many MiB (64 default, 0 = LDS-staged kernels only); key 25 = gl_rela_merge
 * also writes the following LayerNorm (1, default) or a separate gl_layernorm launch does (0); key 27 = fused FeedForward where applicable (1, default) or never (0); key 29 =
 * attention keeps the running max in the padding column of Q / K where the head dim leaves one (d % 16 == 8; 1 default, 0 off);
 * key 30 = 8-wave deep-pipelined 256-row GEMM / conv kernel (0 off, 1 default: problems with at least key-31 (200) such tiles,
 * 2 wherever it applies, with split-K); key 32 = (measurement) its timestamping instantiation, see gl_debug_read; keys 33-35, 37 = its K order
 * / split-K slice length / minimum K / use on short-K multi-round grids that fill >= 80 % of their rounds (1 default).
 * Keys that DO change results (precision): key 41 = the engine's 1x1 convs (ResBlock skip_connection, proj_in, proj_out)
 * take split-fp16 activations ([hi | lo] against the same weight) and every GroupNorm that reads a residual-stream tensor reads it
 * in fp32 (1 default; 0 = round-3 behaviour: fp16 copies); key 42 = the ResBlock's first conv writes its output in fp32 for the
 * following GroupNorm (1 default, 0 = fp16).
 * key 44 = a [cond ; uncond] forward (reps == 2, one timestep for the batch) computes everything that precedes the first
 * conditioning-dependent op -- conv_in, the first ResBlock, proj_in .. attn1 of the first transformer block -- ONCE on the shared
 * latents and duplicates it for the uncond half (1 default; 0 = both halves computed; results equal up to the tile / split-K choice
 * of the half-sized launches).
 * key 38 = the first conv takes the latent as [hi | lo | hi] channels against [Whi | Whi | Wlo] weights (1 default; 0 = fp16(x) against Whi alone).
 * key 43 = the relation chain of rela_fuse (attention.py:348-351) runs on max_b nvalid[b] rows per sample (rounded up to 8) instead of all
 * max_objs = 30 (1 default; read when gl_set_conditioning runs, which then copies the nvalid counts back to the host once); the used rows
 * are unchanged up to the tile / split-K choice of GEMMs with fewer rows.
 * key 45 (with key 41) = the three kinds of 1x1 conv, whose weight rows are stored [Whi | Wlo] (Whi = fp16(W), Wlo = fp16(W - Whi)), add the
 * third pass xhi.Wlo to xhi.Whi + xlo.Whi for launches of more than this many rows (default 1024, the minimum; 0 = the fp16 weight alone): the rounding of those
 * weights is 57 % of the error of storing the UNet's weights in fp16.
 * key 46 = half-height (128-row) tiles of the 8-wave GEMM / conv kernel where the 256-row grid would cover at most half the chip (32x32
 * maps and below at 2B = 8): bit 0 = convs whose 256-row plan leaves <= 16 K-tiles per split-K slice, bit 1 = plain GEMMs, bit 2 = every
 * conv (A/B), bit 3 = multi-round plain GEMMs whose 256-row grid ends in a mostly empty round while the 128-row grid fills its rounds;
 * default 11, 0 = 256-row tiles only.  Results differ from the 256-row plan only through the number of split-K slices.
 * key 47 = plain GEMMs use the 8-wave kernel from this many blocks (tiles x K slices) on (default 100; the split-K decision keeps key 31).
 * key 50 = STRICT mode (0 default; handles created with gl_unet_config.split_weights only, GL_ERR_BAD_ARG otherwise): every matrix product of
 * the forward takes split-fp16 operands -- activations as [hi | lo] (LayerNorm / GroupNorm / GEGLU / attention / projection epilogues write
 * both halves, gl_split_f32 for stream tensors entering a down / up conv), 3x3 convs with gl_conv_args.in_split, attention with
 * gl_attn_args.q_lo / k_lo / vt_lo (three passes for Q.K^T and P.V, P split in registers) -- so that the output is within north_star's
 * rtol 1e-3 / atol 1e-4 of the fp32 reference for > 99 % of the elements (measured 0.1-0.2 % outside, rel-L2 < 1e-4, at 2-3x the
 * default mode's time).  The relation chain of rela_fuse (1/30 weight, 3e-6 of the result) and the fused first conv keep their forms.
 * key 51 = strict mode's third pass x.Wlo (1 default; 0 = activations split only: exact for fp16-representable weights except the
 * folded softmax scale of the q projections).  The strict mode's conditioning hoists are computed lazily: by gl_set_conditioning when key 50
 * is set at that time, else by the first strict forward after it (and again after key 51 changed) -- a split_weights handle that stays in
 * default mode never runs them.
 * key 52 = three-pass split-fp16 products xhi.Whi + xlo.Whi + xhi.Wlo (gl_gemm with K = 3 * kwrap whose second source is the first one again;
 * gl_conv3x3 with in_split = 3) run the DEDICATED three-pass main loop of the 8-wave kernel (1 default; csrc/gemm8.hip S3: a ring stage holds
 * one 32-wide k slice of {xhi, xlo, Whi, Wlo} and feeds three MFMA groups, so no operand is staged twice); 0 = the K-walk over
 * [xhi | xlo | xhi] x [Whi | Whi | Wlo].  Same products, other fp32 summation order.
 * key 54 = kx-reuse main loop of the 8-wave 3x3 conv (csrc/gemm8.hip KXR): the input rows of one (channel block, ky) are staged ONCE for the
 * three kx taps, which read their fragments at LDS rows shifted by kx (33 instead of 96 A staging units per three K-tiles).  Eligible launches:
 * 256-row tiles of the plain fp16 loop, stride 1, no upsample, no pad01 window, no split input, (channel block, tap) K order (key 33 = 0),
 * K slices of whole channel blocks (a multiple of 9 K-tiles); every other launch takes the plain loop whatever the value.  0 = never,
 * 1 = every eligible launch, 2 (default) = the eligible shapes on which it measured faster (profiles/kxreuse_shapes.txt).  Same bits as the
 * plain loop: same MFMA sequence on the same operand values.
 * key 55 = upsample convs (nearest-2x + 3x3) as four folded 2x2 convs, one per output parity, 4/9 of the matrix work (csrc/gemm8.hip UPF): 1
 * = the weight table of a handle holds [4 Cout, 4 Cin] folded kernels for every upsample conv (weights.pack_conv_upfold; a host that
 * fills the table by gl_weight_at has to fold) and the handle launches gl_conv3x3 with upsample2x = 2; 0 = [Cout, 9 Cin] rows and
 * upsample2x = 1; 2 (default) = for gl_create / gl_vae_create the same as 0 -- a host that creates a handle without knowing the fold gets the table
 * it always got -- while the Python packers (weights.pack_state_dict, vae.VAEDecoder) fold the configs whose up convs measured faster folded
 * (weights.fold_up_rule: profiles/upfold_shapes.txt) and create their handle under 1.  Read ONCE, when the handle is created (gl_create, gl_vae_create), and kept in it: a later change affects only handles created
 * afterwards, so one process can hold a folded and an unfolded engine.  A split_weights handle never folds.  Results differ from the 9-tap
 * form by the rounding of the summed weights (same distance to the exact conv). */
int gl_set_option(int key, int value);
/* the process default of `key` as gl_set_option left it (GL_ERR_BAD_ARG for a key out of range) */
int gl_get_option(int key);
/* gl_set_option writes the PROCESS defaults (op-level calls and every handle without an override see them).  A handle can
 * override individual keys for itself: while one of ITS entry points (gl_set_conditioning / gl_unet_forward / gl_plms_step,
 * gl_vae_decode) runs, lookups on that thread see the defaults with the handle's overrides applied, so two hosts in one
 * process tune independently.  A change drops only that handle's captured graphs.  Same keys and value normalisation as
 * gl_set_option; -1 for an unknown key. */
int gl_set_handle_option(gl_engine* e, int key, int value);
int gl_clear_handle_options(gl_engine* e);
int gl_vae_set_option(gl_vae* v, int key, int value);
/* measurement hook (tools/g8_probe.py): what = 8 copies the per-block cycle stamps [entry, prologue done, main loop done,
 * epilogue done] (4 x uint64 per block, up to 4096 blocks) that the timestamping instantiation of the 8-wave GEMM / conv
 * kernel writes while gl_set_option(32, 1) is in effect (synchronous device-to-host copy); what = 9 copies one uint64: the
 * number of gl_gemm / gl_conv3x3 calls this process has served with the 8-wave kernel (the tests of that kernel assert it moved);
 * what = 10 copies ten uint64: the gl_attention calls this process has served per kernel form -- [0] software-pipelined split-fp16
 * kernel, [1] 8-wave split-fp16 kernel, [2] 4-wave split-fp16 kernel, double-buffered, [3] 4-wave split-fp16 kernel, single buffer set,
 * [4..6] single-fp16 8-wave kernel with the running max on the FMA path / in the accumulator init / in the padding column (PRE 0 / 1 / 2),
 * [7..9] single-fp16 4-wave kernel, PRE 0 / 1 / 2 (tests/test_gpu_attention_layouts.py asserts which form took each launch);
 * what = 11 copies one uint64: the gl_conv3x3 calls this process has served with the kx-reuse loop of the 8-wave kernel (key 54);
 * what = 12 copies one uint64: the gl_conv3x3 calls served as folded upsample convs (upsample2x = 2); those always run on the 8-wave
 * kernel and are NOT part of what = 9, which counts the launches the dispatcher chose that kernel for. */
int gl_debug_read(int what, void* dst, int64_t bytes);
/* one-time per-process setup (raises dynamic-LDS limits of the tiled kernels); idempotent */
int gl_init(void);

#ifdef __cplusplus
}
#endif
#endif /* GLIGEN_HIP_H */
