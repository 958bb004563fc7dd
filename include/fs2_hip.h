/*
 * fs2_hip.h -- C ABI of the MI355X (gfx950) FastSpeech2-with-emotion-intensity train path.
 *
 * The reference (Orca0917/fine-grained-emotional-control-of-tts) has no native boundary:
 * its hot path is Python calling speechbrain/torch ops.  Each entry point below replaces
 * one op site of that path ("op-site inventory" K1..K17) and cites the
 * reference line(s) it stands in for.  Conventions (identical for every function):
 *
 *   - all tensor arguments are DEVICE pointers; sizes are explicit ints; row pitches are in
 *     ELEMENTS; nothing is allocated, freed or synchronised inside a call;
 *   - `dtype` selects the activation storage type: FS2_F32 (parity mode) or FS2_BF16;
 *     statistics, losses, gradients of parameters and optimiser state are always fp32;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered (graph-capturable);
 *   - return value: 0 on success, a hipError_t code (>0) on launch failure, or a negative
 *     FS2_E* code for an invalid argument (checked on the host before any launch).
 *
 * Row layout of every token tensor: row m = b*T + t (utterance-major, padded to T), channels
 * contiguous -- the (B, T_max, hidden) layout of the reference (model.py:335-431).
 */
#ifndef FS2_HIP_H
#define FS2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_F32 0
#define FS2_BF16 1

#define FS2_EINVAL (-1)  /* inconsistent sizes / pointers                                  */
#define FS2_EALIGN (-2)  /* pitch or pointer not 16-byte aligned where the kernel needs it */

/* ------------------------------------------------------------------------------------------
 * Generalised MFMA GEMM:  C[m][n] = epilogue( sum_k A(m,k) * B(k,n) )
 * Replaces: every nn.Linear / nn.Conv1d / bmm of the FFT blocks, variance predictors,
 * concat projection, mel linear and PostNet, forward and backward (K4, K6-K8, K12, K13, K16);
 * SB Conv1d "same"+reflect (App. A.1) is folded into the operand loader ("implicit conv").
 * ------------------------------------------------------------------------------------------ */
typedef struct fs2_gemm_desc {
  int M, N, K;          /* problem size; K is the iterated reduction length                  */
  int kvalid;           /* MN-major operands: k rows >= kvalid read as zero (<=0: = K)       */
  int mvalid, nvalid;   /* epilogue stores only m < mvalid, n < nvalid (<=0: M / N)          */
  int dtype;            /* FS2_F32 | FS2_BF16 : A, B and activation-typed outputs            */
  const void* A; int64_t lda; int a_kmajor;   /* 1: A(m,k)=A[m*lda+k]   0: A[k*lda+m]       */
  const void* B; int64_t ldb; int b_kmajor;   /* 1: B(k,n)=B[n*ldb+k]   0: B[k*ldb+n]       */
  /* implicit 1-D convolution over the token axis (SB Conv1d, reflect "same" padding):
   *   1: A fwd   A(m=(b,t), k=(j,c)) = X[b, reflect(t+j-P), c]                  (a_kmajor)
   *   2: A dgrad A(m=(b,s), k=(j,o)) = sum_{t: reflect(t+j-P)=s} dY[b, t, o]     (a_kmajor)
   *   3: B wgrad B(k=(b,t), n=(j,c)) = X[b, reflect(t+j-P), c]                  (!b_kmajor)
   *   4: A shift A(m=(b,p), k=(j,o)) = dY[b, p-j, o] (0 outside [0,T)), T+2P rows per
   *      utterance: the data gradient in the padded domain, finished by fs2_conv_fold
   *   5: A fwd   A(m=(b,t), k=(j,c)) = X[b, t+j-P, c], 0 outside [0,T): zero-padded "same"
   *      conv (torch nn.Conv1d(padding=k//2), IntensityExtractor FFN, rank_model/model.py:23-24)
   *   6: B wgrad, K-major over padded channel-major images (fs2_pad_transpose):
   *      B(k, n=(j,c)) = B[c*ldb + k + j - P] (b_kmajor; k runs over the padded token domain,
   *      T+2P columns per utterance; A = the zero-padded channel-major dY image, so products
   *      across utterances vanish).  B must have 64 readable elements before it and P after
   *      each row end; K % 64 == 0; fp32 output, split-K only as split_stride slices with
   *      K % (64 * split_k) == 0, no epilogue operations
   * P = (conv_kw-1)/2, conv_c = channels per tap, conv_t = tokens per utterance.          */
  int conv_mode, conv_t, conv_kw, conv_c;
  void* C; int64_t ldc; int c_fp32;           /* output; c_fp32: float output else dtype     */
  int c_conv_kw;        /* >0: output column n=(j,c) is stored at c*c_conv_kw + j            */
  const float* bias;    /* [N]       v += bias[n]                                             */
  int relu;             /* 1: v = max(v, 0); 2: v = GELU(v) = v/2 (1 + erf(v/sqrt 2));
                           3: leaky ReLU slope 0.1; 4: tanh                                    */
  const void* gate; int64_t ldg;              /* dtype [M][ldg]: v *= (gate > 0)             */
  const float* row_scale;                     /* [M]: v *= row_scale[m]                      */
  const void* residual; int64_t ldr;          /* dtype [M][ldr]: v += residual               */
  const float* row_scale_post;                /* [M]: v *= row_scale_post[m]                 */
  int accumulate;       /* fp32 output only: C += v (split_k > 1 implies atomic accumulate)   */
  int split_k;          /* >1: K split over blockIdx.z, fp32 atomics into C                  */
  int64_t split_stride; /* >0 (with split_k > 1, !accumulate): split z stores its fp32 partial
                         * to C + z*split_stride elements instead -- no atomics; slices a
                         * shortened split leaves unused are zeroed.  Consumers sum slices.    */
  /* batched: z in [0,batch): offset(z) = (z / batch_div)*s1 + (z % batch_div)*s2 (elements) */
  int batch, batch_div;
  int64_t sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2;
  int conv_dil;         /* dilation of conv modes 1 / 5 (tap j reads row t + (j-P)*dil); 0 = 1 */
  /* c_row_t > 0, c_row_pad > 0: output row m is stored at C row m + (m / c_row_t) * c_row_pad
   * -- a token-major result written into a padded token domain (c_row_pad zero rows between
   * utterances, which the caller keeps zero), e.g. the FFN conv2 data gradient straight into
   * the zero-padded dY image of the conv1 data gradient.  c_row_pad < 0: the inverse -- rows m
   * of a padded domain (L = c_row_t - c_row_pad rows per utterance) with m mod L < c_row_t are
   * stored at m - (m / L) * (-c_row_pad), the others dropped (a conv forward over the padded
   * domain, fs2_pad_rows).  bf16, both K-major, no split / batch / conv; runs on the 4-wave
   * or the persistent 256-row kernel (FS2_EINVAL where neither applies).                    */
  int c_row_t, c_row_pad;
  /* grid budget of the persistent GEMM kernels for this call (0 or >= 256: one block per CU):
   * a GEMM enqueued beside a latency-critical stream -- the weight gradients of the train step
   * (model.py:279-441 backward) beside the data-gradient chain -- leaves 256 - max_ctas CUs to
   * the other stream's kernels; 8..255, rounded down to 8.  Results do not depend on it.     */
  int max_ctas;
  /* a_kw > 0: tap-inner K order for a plain K-major A whose rows overlap (the conv1 data
   * gradient over the padded dY image, lda = the image's channel count Ci, K = a_kw * Ci,
   * Ci % 64 == 0): k = (chunk q, tap j, i) -> A(m, k) = A[(m + j)*lda + 64 q + i], i < 64 --
   * consecutive 64-deep K-stages read image rows one tap apart, so each row is fetched from HBM
   * about once instead of once per tap.  B must be in the same order (fs2_weight_prep w_okc
   * bit 2; the forward's Wf: bit 3).  bf16, no split / batch / conv; always the 4-wave
   * kernel.                                                                                 */
  int a_kw;
  /* conv_mode 6 only, optional: device int32 holding the effective K of token-compacted images
   * (the last offset handed to fs2_pad_transpose_bounded): columns >= *k_eff of A and B are
   * zeros up to where the transposes zero-filled, and every split walks max(2, ceil(ceil(k_eff / 64) / split_k))
   * K-tiles instead of K / 64 / split_k.  Read on the device (no host sync).  NULL: off.      */
  const int32_t* k_eff;
} fs2_gemm_desc;

int fs2_gemm(const fs2_gemm_desc* d, void* stream);

/* What fs2_gemm would do with a descriptor, decided on the host without any launch: the kernel
 * (the instantiation as a profiler prints it, e.g. "gemm_ps_kernel<0, 48, 1, 0>"; the 128 x 128
 * kernel reads "gemm_kernel<bf16|float, AK, BKM, GA, GB>"), its grid in blocks and block size,
 * and the tiling / split the kernel receives.  Returns what fs2_gemm would return before
 * launching (0 or an FS2_E* code); an empty problem (M or N = 0) returns 0 with kernel "".
 * The descriptor's pointers are only tested for NULL and 16-byte alignment, never followed.  */
typedef struct fs2_gemm_plan_info {
  char kernel[64];
  int grid[3];
  int block;
  int tiles_m, tiles_n;
  int split_k, k_per_split;
  int vec_ok, accumulate;
} fs2_gemm_plan_info;

int fs2_gemm_plan(const fs2_gemm_desc* d, fs2_gemm_plan_info* out);

/* reflect-padding adjoint + dgrad epilogue (K16): Xpad fp32 [B][T+2P][C] from conv_mode 4
 * (nsplit split-K slices split_stride floats apart, summed here; nsplit <= 1: one slice),
 *   out[b,s] = ((Xpad[s+P] + Xpad[P-s]{1<=s<=P} + Xpad[2(T-1)-s+P]{T-1-P<=s<=T-2}) * rs
 *              + residual) * rs2                                                           */
int fs2_conv_fold(const float* Xpad, int nsplit, int64_t split_stride, int B, int T, int P,
                  int C, void* out, int64_t ldo, const void* residual, int64_t ldr,
                  const float* row_scale, const float* row_scale_post, int dtype, void* stream);

/* channel-major padded image for conv_mode 6 (backward of the SB Conv1d weights, App. A.1;
 * model.py:241-267 FFN conv1): out[c][b*(T+2P) + i] = X[b*T + reflect(i-P)][c] (reflect = 1)
 * or X[b*T + i-P][c] inside [0,T) and 0 outside (reflect = 0), i in [0, T+2P); columns
 * [B*(T+2P), ncols) are written as 0.  X bf16 [B*T][ldx]; out bf16 [C][ldo]; C, ldx, ldo,
 * ncols multiples of 8, ldo >= ncols >= B*(T+2P), both pointers 16-byte aligned.
 * colsum (optional, reflect = 0 only): colsum[c] += sum_t X[t][c] -- the conv bias gradient
 * (K13 bias), replacing an fs2_colsum pass; workspace >= ceil(ncols/64) * C floats.        */
int fs2_pad_transpose(const void* X, int64_t ldx, int B, int T, int C, int P, int reflect,
                      void* out, int64_t ldo, int ncols, float* colsum, float* workspace,
                      int dtype, void* stream);
/* fs2_pad_transpose with the token axis compacted, for a weight gradient whose dY rows
 * t >= e_b of utterance b are exact zeros.  offs: device int32, B + 1 column offsets (offs[0] = 0,
 * offs[b + 1] = offs[b] + w_b, Pc the conv's pad, 0 <= e_b <= T) followed by INT32_MAX up to a
 * multiple of 16 and 16 more; read on the device.  w_b = T + 2 Pc - 64 r_b >= e_b + 2 Pc, r_b the
 * whole 64-column K-tiles of the uncompacted image inside utterance b's columns from e_b + 2 Pc
 * on: max(0, floor((b + 1)(T + 2 Pc) / 64) - ceil((b (T + 2 Pc) + e_b + 2 Pc) / 64)).  Only whole
 * tiles are dropped, so the remaining ones hold what they held uncompacted and the GEMM's sums
 * per split are unchanged bit for bit.  Utterance b keeps its rows t < w_b - 2 Pc and
 * occupies the columns [offs[b], offs[b + 1]); the reflect image still reflects about T.  (A
 * zero-padded token-major dY image, T + 2 Pc rows per utterance, is transposed with P = 0: its
 * first w_b rows per utterance.)  Columns from the compacted end offs[B] to where a
 * conv_mode-6 GEMM with split_k = ksplit and fs2_gemm_desc.k_eff = offs + B reads (64 past its
 * last K-tile) and the last 64 columns are written as 0, the ones between are left untouched.
 * ncols a multiple of 64 * ksplit, >= 128.  colsum as fs2_pad_transpose.                    */
int fs2_pad_transpose_bounded(const void* X, int64_t ldx, int B, int T, int C, int P, int reflect,
                              void* out, int64_t ldo, int ncols, float* colsum, float* workspace,
                              const int32_t* offs, int ksplit, int dtype, void* stream);

/* Row bounds of a padded batch's backward, from the utterance lengths on the device (no host
 * sync): end[b] = clamp(len[b] + halo, 0, T) (int32 [B]; the gradient rows t >= end[b] are
 * zeros, see fs2_attn_bwd_bounded) and the column offsets of the compacted conv_mode-6 images
 * for a conv pad P (fs2_pad_transpose_bounded): offs[0] = 0, offs[b + 1] = offs[b] + w_b as
 * defined there, offs[B + 1 .. noffs) = INT32_MAX, noffs >= round_up(B + 1, 16) + 16.  end or
 * offs may be NULL.                                                                         */
int fs2_grad_tail_bounds(const int64_t* len, int B, int T, int halo, int P, int32_t* end,
                         int32_t* offs, int noffs, void* stream);

/* out[i] (+)= sum_{s < nslices} ws[s*stride + i], i < n (fp32; n, stride multiples of 4,
 * 16-byte aligned): the sum of split-K weight-gradient slices written by fs2_gemm with
 * split_stride (no atomics; fixed summation order)                                         */
int fs2_sum_slices(const float* ws, int nslices, int64_t stride, int64_t n, float* out,
                   int accumulate, void* stream);

/* token-major padded image for a conv forward over the padded token domain (SB Conv1d
 * "same"+reflect, App. A.1; model.py:241-267 FFN conv1): out row b*(T+2P) + i = X row
 * b*T + reflect(i-P) (reflect = 1) or X row b*T + i-P inside [0,T) and zero outside
 * (reflect = 0), i in [0, T+2P); then `tail` zero rows (the guard the overlapping-row GEMM
 * reads past the last utterance).  With it the conv is a plain K-major GEMM over the padded
 * domain, A(m, k=(j,c)) = out[m*ldo + k] (lda = ldo = C), whose rows m with
 * m mod (T+2P) >= T are dropped by fs2_gemm's c_row (T, -2P).  bf16; C, ldx, ldo multiples
 * of 8, 16-byte aligned pointers. */
int fs2_pad_rows(const void* X, int64_t ldx, int B, int T, int C, int P, int reflect, int tail,
                 void* out, int64_t ldo, int dtype, void* stream);

/* column sums: out[n] (+)= sum_m X[m][n]   (bias gradients; SB Linear/Conv1d bias, K16) */
int fs2_colsum(const void* X, int64_t ldx, int M, int N, int dtype, float* out, int accumulate,
               float* workspace, void* stream);
int64_t fs2_colsum_workspace_floats(int M, int N);

/* ------------------------------------------------------------------------------------------
 * LayerNorm with fused residual / dropout / tanh / mask (K5, K8, K13)
 *   s = x + drop(r; p_r)          (r optional; SB TransformerEncoderLayer, App. A.2)
 *   y = LN(s)*gamma + beta         (eps per call: 1e-6 FFT, 1e-5 predictors/PostNet)
 *   y = tanh(y) (opt) ; y = drop(y; p_o) ; y *= row_mask (opt) ; y += post_add (opt)
 * ------------------------------------------------------------------------------------------ */
/* img (optional, bf16, M % img_t == 0, img_p < img_t): also y's reflect-padded token-major
 * image as fs2_pad_rows(y, ..., img_t, D, img_p, reflect 1, tail 0) writes it (row pitch D) --
 * the FFN conv1 forward's operand, written by the LayerNorm that produces its input
 * (SB Conv1d "same"+reflect, App. A.1) instead of a separate pass.                        */
int fs2_ln_fwd(const void* x, int64_t ldx, const void* r, int64_t ldr, float p_r, uint32_t salt_r,
               void* s_out, const float* gamma, const float* beta, float eps, int do_tanh,
               float p_o, uint32_t salt_o, const float* row_mask, const void* post_add,
               int64_t ldp, void* y, int64_t ldy, float* mean, float* rstd, int M, int D,
               int dtype, uint32_t seed, void* img, int img_t, int img_p, void* stream);

/* backward of fs2_ln_fwd; dgamma/dbeta (+)= column sums (fp32).  ds = dL/ds (optionally
 * gated by (s > 0) for a ReLU that produced s), dr = ds * dropmask_r / (1 - p_r).
 * dcol (optional) (+)= column sums of dr (or of ds when dr is NULL): the bias gradient of
 * the layer whose output fed r (resp. s), fused here instead of a separate fs2_colsum.    */
int fs2_ln_bwd(const void* dy, int64_t lddy, const void* s, int64_t lds, const float* mean,
               const float* rstd, const float* gamma, const float* beta, int do_tanh, float p_o,
               uint32_t salt_o, const float* row_mask, int relu_gate_in, void* ds, int64_t ldds,
               void* dr, float p_r, uint32_t salt_r, float* dgamma, float* dbeta, float* dcol,
               int M, int D,
               int dtype, uint32_t seed, float* workspace, void* stream);
int64_t fs2_ln_workspace_floats(int M, int D);

/* ------------------------------------------------------------------------------------------
 * Attention softmax over materialised scores, with the reference's key masking
 * (model.py:338-343 / 414-419 + key_padding_mask; head-major tiling quirk):
 *   mask_mode 1: batch z = b*H + h masks key k iff key_pad[b][k] || key_pad[(b*H+h) % B][k];
 *   mask_mode 0: plain key padding key_pad[b][k] (IntensityExtractor MHA,
 *                rank_model/model.py:35,101).
 * S: fp32 [z][Tq][ldt]; P, Pd: dtype [z][Tq][ldt] (softmax and dropped softmax, zero-padded
 * to ldt); scale applied to S before the softmax (torch MHA q-scaling).
 * ------------------------------------------------------------------------------------------ */
int fs2_softmax_fwd(const float* S, const uint8_t* key_pad, int mask_mode, int B, int H, int Tq,
                    int Tk, int ldt, float scale, float p_drop, uint32_t seed, uint32_t salt,
                    void* P, void* Pd, int dtype, void* stream);
/* dS = scale * P * (dP - rowsum(P*dP)) with dP = dPd * dropmask / (1-p). dPd fp32.        */
int fs2_softmax_bwd(const float* dPd, const void* P, int B, int H, int Tq, int Tk, int ldt,
                    float scale, float p_drop, uint32_t seed, uint32_t salt, void* dS, int dtype,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention (bf16; K4/K16): softmax(scale * Q K^T with the tiling mask) -> dropout -> PV
 * without materialising the (B*H, T, T) scores.  Q | K | V are column blocks of the packed
 * projection qkv [B*T][ldq] (head h at columns h*dh of each block); out [B*T][ldo] gets head h
 * at h*dh; lse [B*H][T] keeps the log2-domain log-sum-exp for the backward, which writes
 * dQ | dK | dV into dqkv with the same layout as qkv.  Same mask rule and dropout indices as
 * fs2_softmax_fwd/bwd.  Requires dtype bf16, dh in {64,128,192,256}, T <= 2048
 * (fs2_attn_supported); workspace: fs2_attn_workspace_floats.
 * ------------------------------------------------------------------------------------------ */
int fs2_attn_supported(int T, int dh, int dtype);
int fs2_attn_fwd(const void* qkv, int64_t ldq, const uint8_t* key_pad, int mask_mode, int B,
                 int H, int T, int dh, float scale, float p_drop, uint32_t seed, uint32_t salt,
                 void* out, int64_t ldo, float* lse, int dtype, void* stream);
int fs2_attn_bwd(const void* qkv, int64_t ldq, const uint8_t* key_pad, int mask_mode,
                 const void* out,
                 int64_t ldo, const void* dout, int64_t lddo, const float* lse, int B, int H,
                 int T, int dh, float scale, float p_drop, uint32_t seed, uint32_t salt,
                 void* dqkv, int64_t lddq, float* workspace, int dtype, void* stream);
/* fs2_attn_bwd for a dO whose rows t >= q_bound[b] of utterance b are exact zeros (q_bound:
 * device int32 [B], indexed by the utterance, read on the device): the query tiles past
 * min(T, q_bound[b]) are skipped; bit-identical to fs2_attn_bwd on such a dO.  Workspace rows
 * of skipped query blocks stay unwritten.                                                  */
int fs2_attn_bwd_bounded(const void* qkv, int64_t ldq, const uint8_t* key_pad, int mask_mode,
                         const void* out, int64_t ldo, const void* dout, int64_t lddo,
                         const float* lse, int B, int H, int T, int dh, float scale,
                         float p_drop, uint32_t seed, uint32_t salt, void* dqkv, int64_t lddq,
                         float* workspace, const int32_t* q_bound, int dtype, void* stream);
int64_t fs2_attn_workspace_floats(int B, int H, int T);

/* ------------------------------------------------------------------------------------------
 * Token embedding + positional encoding + pad mask (K1, K2; model.py:331-337)
 *   X[m] = (E[tok[m]] + pe[t]) * (tok[m] != pad);  keep[m] = (tok[m] != pad)
 * ------------------------------------------------------------------------------------------ */
int fs2_embed_fwd(const int64_t* tokens, const float* table, const float* pe, int pad_idx,
                  int B, int T, int D, void* X, float* keep, int dtype, void* stream);
/* dTable[v] (+)= sum_{m: tok[m]==v} dX[m] * keep[m]   (deterministic: token-chunk partials in
 * per-wave LDS accumulators, summed in a fixed order); V <= 128;
 * workspace >= fs2_embed_bwd_workspace_floats(D, V) floats                                 */
int fs2_embed_bwd(const int64_t* tokens, const void* dX, const float* keep, int M, int D,
                  int V, float* dtable, float* workspace, int dtype, void* stream);
int64_t fs2_embed_bwd_workspace_floats(int D, int V);

/* key padding masks: from tokens (tok==pad) or from lengths (t >= len)                    */
int fs2_keypad_from_tokens(const int64_t* tokens, int pad_idx, int M, uint8_t* key_pad,
                           void* stream);
int fs2_keypad_from_lengths(const int64_t* lens, int B, int T, uint8_t* key_pad, float* keep,
                            void* stream);

/* concat [feats, spk_emb[spk[b]], intensity, 0-pad] (model.py:352-358) -> cat [M][ldc]    */
int fs2_concat_fwd(const void* feats, const float* spk_table, const int64_t* spk,
                   const float* intensity, int B, int T, int D, int E, void* cat, int ldc,
                   int dtype, void* stream);
/* dSpk[spk[b]] (+)= sum_t dcat[b,t,D:2D]                                                  */
int fs2_concat_bwd_spk(const void* dcat, int ldc, const int64_t* spk, int B, int T, int D,
                       int n_spk, float* dspk, int dtype, float* workspace /* B*D */,
                       void* stream);

/* rows: X[m][:] *= keep[m]   (in place)                                                   */
int fs2_mask_rows(void* X, int64_t ldx, const float* keep, int M, int D, int dtype, void* stream);
/* X = (X + Y + Z) * keep[row] over M x D (row pitch ld for all three), summed in fp32 and
 * rounded once: the join of the predictor input gradients when the duration / pitch predictor
 * backward runs on its own stream (model.py:365-403 variance adaptor backward).  Z may be null
 * (X = (X + Y) * keep[row]). */
int fs2_add3_mask_rows(void* X, const void* Y, const void* Z, int64_t ld, const float* keep,
                       int M, int D, int dtype, void* stream);

/* predictor head: y[m] = (dot(u[m], w) + b) * scale (SB DurationPredictor.linear, App. A.7) */
int fs2_rowdot_fwd(const void* u, int64_t ldu, const float* w, const float* b, float scale, int M,
                   int D, void* y, int dtype, void* stream);
/* du = dy*scale*w ; dw (+)= sum_m dy*scale*u ; db (+)= sum_m dy*scale                     */
int fs2_rowdot_bwd(const void* dy, const void* u, int64_t ldu, const float* w, float scale, int M,
                   int D, void* du, float* dw, float* db, int dtype, float* workspace,
                   void* stream);

/* average_over_durations (SB, App. A.10; model.py:383,397): mean of NON-ZERO frame values
 * per phoneme via double-accumulated prefix sums (replicates torch CPU cumsum).            */
int fs2_avg_over_durations(const float* values, int Tm_in, const int64_t* durs, int B, int Tp,
                           float* avg, float* workspace, void* stream);
int64_t fs2_avg_workspace_floats(int B, int Tm_in);

/* pitch/energy embedding conv (SB Conv1d(1->D, k, reflect), model.py:226-240,384-403) fused
 * with the residual add:  out[b,t,:] = base[b,t,:] + bias + sum_j W[:, 0, j] a[b, refl(t+j-P)] */
int fs2_embed1d_fwd(const void* base, const float* a, const float* W, const float* bias, int B,
                    int T, int D, int KW, void* out, int dtype, void* stream);
/* dW[o][j] (+)= sum dOut[b,t,o] a[b,refl(t+j-P)]; dbias (+)= sum dOut                     */
int fs2_embed1d_bwd(const void* dout, const float* a, int B, int T, int D, int KW, float* dW,
                    float* dbias, int dtype, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * LengthRegulator (SB upsample, App. A.9; model.py:406-413), K11.
 *   n[b,p] = (int64)(pace * (float)d[b,p])  (float32 product, truncation == .long())
 *   mel_len[b] = sum_p n[b,p];  frame_src[b,t] = p with cum[p-1] <= t < cum[p], -1 past mel_len
 * The integer expansion is bit-exact to repeat_interleave.  d: int64 (teacher forcing) or
 * float (predicted, already clamp(expm1(.),0)) selected by d_is_float.
 * ------------------------------------------------------------------------------------------ */
int fs2_lr_index(const void* durs, int d_is_float, float pace, int B, int Tp, int Tm,
                 int64_t* mel_len, int32_t* cum, int32_t* frame_src, void* stream);
/* Y[b,t] = (X[b, frame_src[b,t]] + pe[t]) * keep[b,t]  (fused decoder PE add, model.py:422-423) */
int fs2_lr_gather(const void* X, const int32_t* frame_src, const float* pe, int B, int Tp,
                  int Tm, int D, void* Y, float* keep, int dtype, void* stream);
/* dX[b,p] = sum_{t in segment p} dY[b,t] * keep[b,t]                                      */
int fs2_lr_scatter(const void* dY, const int32_t* cum, const float* keep, int B, int Tp, int Tm,
                   int D, void* dX, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss (loss.py:62-186), K14/K15.  loss_out[8] fp32 = {total, ssim, mel, postnet, dur, pitch,
 * energy, ssim_gradient_scale}; gradients are written for a unit upstream gradient.
 * ------------------------------------------------------------------------------------------ */
typedef struct fs2_loss_desc {
  int B, Tm, Tp, NM;           /* Tm: padded frames of predictions AND target               */
  int dtype;                   /* predictions' dtype                                         */
  const void* mel_out; const void* postnet_out;       /* [B][Tm][NM]                       */
  const void* log_dur; const void* pitch_pred; const void* energy_pred;  /* [B][Tp]         */
  const float* mel_tgt;                               /* [B][Tm][NM]                        */
  const int64_t* dur_tgt;                             /* [B][Tp]                            */
  const float* pitch_avg; const float* energy_avg;    /* [B][Tp] (average_over_durations)   */
  const int64_t* mel_len; const int64_t* phon_len;    /* [B]                                */
  float w_ssim, w_mel, w_post, w_dur, w_pitch, w_energy;
  float* loss_out;                                     /* [8]                                */
  void* d_mel_out; void* d_postnet_out;               /* dtype, [B][Tm][NM]                 */
  void* d_log_dur; void* d_pitch; void* d_energy;     /* dtype, [B][Tp]                     */
  float* workspace;                                    /* fs2_loss_workspace_floats()        */
} fs2_loss_desc;
int fs2_loss_fwd_bwd(const fs2_loss_desc* d, void* stream);
int64_t fs2_loss_workspace_floats(int B, int Tm, int NM);
/* The seven values and loss_out[7] alone (validation): the five d_* pointers are ignored and
 * may be null, no gradient is computed or stored, and the workspace is the smaller
 * fs2_loss_fwd_workspace_floats().  No float atomic: the values are reproducible bit for bit. */
int fs2_loss_fwd(const fs2_loss_desc* d, void* stream);
int64_t fs2_loss_fwd_workspace_floats(int B, int Tm, int NM);

/* ------------------------------------------------------------------------------------------
 * Optimiser + weight preparation (K17; train.py:232 torch.optim.AdamW defaults).
 * ------------------------------------------------------------------------------------------ */
/* torch AdamW (single-tensor algorithm, fp32), grads scaled by grad_scale (1/world_size).
 * c_* constants are computed on the host exactly as torch does (see fastspeech2/optim.py). */
int fs2_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
              float decay_mul, float one_minus_beta1, float beta2, float one_minus_beta2,
              float step_size, float bc2_sqrt, float eps, float grad_scale, void* stream);

/* master weight W (fp32) -> fwd copy Wf[O][KW][C] and dgrad copy Wb[C][KW][O] in dtype, each
 * with row pitch padded to ldf / ldb elements (zeros in the pad).  W is stored torch-style
 * [O][C][KW] (w_okc bit 0 clear) or [O][KW][C] (bit 0 set, the flat-buffer layout of conv
 * weights).  w_okc bit 1: Wb's taps reversed, Wb[C][KW-1-j][O] -- the order in which the conv
 * data gradient over a zero-padded token-major dY image is a plain K-major GEMM whose A rows
 * overlap (A(m, k) = image[m*O + k], lda = O).  w_okc bit 2 (O % 64 == 0): Wb's columns in
 * tap-inner 64-channel chunks, column (o/64)*KW*64 + j*64 + o%64 (fs2_gemm_desc.a_kw); bit 3
 * (C % 64 == 0, ldf == KW*C): Wf's columns the same way, (c/64)*KW*64 + j*64 + c%64. */
int fs2_weight_prep(const float* W, int O, int C, int KW, int w_okc, void* Wf, int ldf, void* Wb,
                    int ldb, int dtype, void* stream);

/* All of a model's weight images in ONE launch: descs (DEVICE memory) lists n weights, each
 * cut into 64 x 64 tiles of its [O][ldf] forward image; tile0 = first tile index of weight i
 * (prefix sum, ascending), tiles_k = ceil(ldf / 64).  Each tile is read once (coalesced),
 * written to Wf, and transposed through LDS into Wb (coalesced along o); Wb may be NULL.
 * total_tiles = tile0 + tiles of the last weight; n <= 256.                               */
typedef struct fs2_wprep_desc {
  const float* W; void* Wf; void* Wb;
  int O, C, KW, w_okc, ldf, ldb;
  int tile0, tiles_k;
} fs2_wprep_desc;
int fs2_weight_prep_batched(const fs2_wprep_desc* descs, int n, int total_tiles, int dtype,
                            void* stream);
/* AdamW fused with the weight images (replaces fs2_adamw + fs2_weight_prep_batched after an
 * optimiser step, K17 of SURVEY §2): the descriptor table's weights are updated tile by tile
 * and their Wf / Wb images written from the updated values; every other parameter lies in
 * `ranges` (int64 triples: flat start, length, first block; 1024 elements per block).  All
 * pointers index the same flat layout: descs[i].W - param is a weight's flat offset.
 * Every master is read as [O][KW][C] (element (o, j, c) at W[(o*KW + j)*C + c]) whatever bit 0
 * of w_okc says: it must be set whenever KW > 1 (with KW == 1 the two layouts coincide), or the
 * images come out wrong without an error -- fs2_weight_prep_batched honours the bit, this call
 * does not.  Wb's columns from KW*O up to ldb are not written (fs2_weight_prep zeroes them).
 * param, grad, exp_avg and exp_avg_sq must be 16-byte aligned: the 16-byte form of a tile is
 * chosen from the weight's flat offset and pitches alone. */
int fs2_adamw_prep(const fs2_wprep_desc* descs, int n, int total_tiles, const int64_t* ranges,
                   int n_ranges, int range_blocks, float* param, const float* grad,
                   float* exp_avg, float* exp_avg_sq, float decay_mul, float one_minus_beta1,
                   float beta2, float one_minus_beta2, float step_size, float bc2_sqrt, float eps,
                   float grad_scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frozen IntensityExtractor forward pieces + phoneme averaging (SURVEY §8f-1;
 * rank_model/model.py:96-109, fastspeech2/train.py:16-51).  The extractor's GEMMs use
 * fs2_gemm (conv_mode 5 zero-padded k=9 convs, relu=2 GELU), fs2_attn_fwd / fs2_softmax_fwd
 * with mask_mode 0, and fs2_ln_fwd (eps 1e-5).
 * ------------------------------------------------------------------------------------------ */
/* rank_X fp32 (B,T,C) (layout_bct=0) or the collate's (B,C,T) (layout_bct=1, the explicit fix of
 * SURVEY App. B-2) -> GEMM rows X[B*T][ldx] in dtype, columns >= C zero.                    */
int fs2_intensity_input(const float* x, int layout_bct, int B, int T, int C, void* X, int ldx,
                        int dtype, void* stream);
/* I[b,t,e] = (t < lengths[b]) ? (H[b,t] + emo_table[emotions[b]]) . Wc[e] + bc[e] : bc[e]
 * (model.py:103-107: emotion embedding add, masked_fill, classifier); I fp32 (B,T,E), E <= 8 */
int fs2_intensity_head(const void* H, int64_t ldh, const float* emo_table,
                       const int64_t* emotions, const int64_t* lengths, const float* Wc,
                       const float* bc, int B, int T, int D, int E, float* I, int dtype,
                       void* stream);
/* out[b,p,:] = sum of I[b, t, :] over phoneme p's frames [sum d[:p], sum d[:p+1]) (clipped to
 * T) / max(d[b,p], 1) for p < phon_len[b]; 0 otherwise (train.py:33-49). Tp <= 1024.
 * The sum runs over t in ascending order in fp32 and is divided once.  When the durations of an
 * utterance add up to more than T, frames from T on are not read (a phoneme that starts at or
 * after T sums nothing and comes out as +0), and the divisor is still the full d[b,p].
 * phon_len[b] is clamped to [0, Tp]; positions p >= phon_len[b] are written as +0.0, and
 * durations there are not read.  Durations must be >= 0.  Tp > 1024 is FS2_EINVAL.         */
int fs2_phoneme_average(const float* I, int T, int E, const int64_t* durations,
                        const int64_t* phon_len, int B, int Tp, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rank-model evaluation path (rank_model/model.py:138-166 in eval mode, loss.py:36-55,
 * inference.py:98-114).  The extractor runs once over the 2B mixed sequences staged by
 * fs2_rank_mixup_input.  Every reduction below has a fixed order and uses no atomics.
 * ------------------------------------------------------------------------------------------ */
/* emo_X, neu_X fp32 (B,T,C), lambdas fp32 (2,B) -> GEMM rows X[2*B*T][ldx] in dtype: rows
 * [0, B*T) = lam_i*emo + (1-lam_i)*neu, rows [B*T, 2*B*T) the same with lam_j (two fp32
 * products and one add, not fused), columns >= C zero.                                       */
int fs2_rank_mixup_input(const float* emo_X, const float* neu_X, const float* lambdas, int B,
                         int T, int C, void* X, int ldx, int dtype, void* stream);
/* h[b,e] = (sum over ALL T frames of I[b,t,e]) / float(length[b]) (padded frames hold the
 * classifier bias and are summed, as model.py:160 does); r[b] = sum_e h[b,e] * Wp[e].
 * I fp32 (B,T,E), E <= 8, length[b] >= 1.                                                    */
int fs2_rank_pool(const float* I, const int64_t* length, const float* Wp, int B, int T, int E,
                  float* h, float* r, void* stream);
/* out[0..2] = (alpha*L_mixup + beta*L_rank, L_mixup, L_rank) of loss.py:36-55: the four
 * batch-mean cross entropies of hi / hj (B,E) against y_emo / y_neu, weighted by the
 * per-sample lambdas and averaged; L_rank with sigmoid(ri-rj), log(p + 1e-8) and
 * lam_diff = (lam_i-lam_j+1)/2.  A target outside [0,E) gives NaN.  One block, fp32.        */
int fs2_rank_loss_fwd(const float* lam_i, const float* lam_j, const float* hi, const float* hj,
                      const float* ri, const float* rj, const int64_t* y_emo,
                      const int64_t* y_neu, int B, int E, float alpha, float beta, float* out,
                      void* stream);
/* out[g,k,:] = mean of bucket k of group g's frames (inference.py:98-114).  order[grp_off[g] ..
 * grp_off[g+1]) are the group's utterances in ascending score order; cstart[j] (j = 0..U) is
 * the number of frames before sorted utterance j; utterance u's frames are rows
 * [utt_off[u], ...) of frames fp32 [.][E].  The group's N concatenated frames are split as
 * np.array_split(N, K) does.  fp64 sums in a fixed order, fp32 out.  Empty group: zeros;
 * empty bucket (N < K): NaN.  E <= 8.                                                        */
int fs2_bucket_means(const float* frames, const int64_t* order, const int64_t* cstart,
                     const int64_t* utt_off, const int64_t* grp_off, int G, int K, int E,
                     float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rank-model training (rank_model/train.py:19-43): the pieces of the train-mode forward and of
 * the backward that are not GEMMs, attention or LayerNorm.  fp32 parameter gradients, fixed
 * summation orders, no atomics.  E <= 8; p in [0, 1).
 * ------------------------------------------------------------------------------------------ */
/* rank_model/model.py:42-43 (activation, dropout): Hc[m][n] = keep(m*N + n) * GELU(Z[m][n]) /
 * (1 - p), GELU in fs2_gemm's erf form (relu = 2).  keep = the pair-hash mask of (seed, salt),
 * indexed by m*N + n whatever the row pitches (all >= N).  Z is the conv1 output with bias and no
 * activation: in dtype, or (z_fp32 != 0) the fp32 output of a c_fp32 GEMM, so that beside bf16
 * activations GELU sees the unrounded value as the evaluation path's fused epilogue does.  Zact
 * (optional): Z rounded to dtype, what fs2_gelu_dropout_bwd reads.  Hc, Zact in dtype.      */
int fs2_gelu_dropout_fwd(const void* Z, int64_t ldz, int z_fp32, void* Zact, int64_t ldza,
                         void* Hc, int64_t ldh, int M, int N, float p, uint32_t seed,
                         uint32_t salt, int dtype, void* stream);
/* its backward: dZ[m][n] = dHc[m][n] * keep(m*N + n) / (1 - p) * GELU'(Z[m][n]),
 * GELU'(z) = (1 + erf(z / sqrt 2)) / 2 + z exp(-z^2 / 2) / sqrt(2 pi).  dZ may be dHc.       */
int fs2_gelu_dropout_bwd(const void* dHc, int64_t lddh, const void* Z, int64_t ldz, void* dZ,
                         int64_t lddz, int M, int N, float p, uint32_t seed, uint32_t salt,
                         int dtype, void* stream);
/* rank_model/model.py:103-107 backwards, from gI fp32 (B,T,E):
 *   dH[b,t,:] = t < lengths[b] ? sum_e gI[b,t,e] Wc[e,:] : 0                       (dtype)
 *   dWc[e,:]  = sum_{b, t < lengths[b]} gI[b,t,e] (H[b,t,:] + emo_table[emotions[b],:])
 *   dbc[e]    = sum_{b, ALL t < T} gI[b,t,e]   (padded frames hold the bias)
 *   dEmb[k,:] = sum_{b: emotions[b] = k} sum_{t < lengths[b]} dH[b,t,:] (before rounding);
 *               (n_emotions, D), rows of emotions no sequence carries are exact zeros
 * Outputs are overwritten.  workspace >= fs2_intensity_head_bwd_workspace_floats floats.    */
int fs2_intensity_head_bwd(const float* gI, const void* H, int64_t ldh, const float* emo_table,
                           const int64_t* emotions, int n_emotions, const int64_t* lengths,
                           const float* Wc, int B, int T, int D, int E, void* dH, int64_t lddh,
                           float* dWc, float* dbc, float* dEmb, float* workspace, int dtype,
                           void* stream);
int64_t fs2_intensity_head_bwd_workspace_floats(int B, int T, int D, int E);
/* rank_model/model.py:160-164 backwards: dI[b,t,e] = gI[b,t,e] + (gh[b,e] + gr[b] Wp[e]) /
 * float(length[b]) for ALL t < T (gI may be NULL: zeros); dWp[e] = sum_b gr[b] h[b,e] in
 * ascending b.  fp32; dI and gI 16-byte aligned.                                            */
int fs2_rank_pool_bwd(const float* gI, const float* gh, const float* gr, const float* h,
                      const float* Wp, const int64_t* length, int B, int T, int E, float* dI,
                      float* dWp, void* stream);
/* rank_model/loss.py:36-55: out[0..2] as fs2_rank_loss_fwd, and the gradients of out[0]:
 * dhi, dhj (B,E), dri, drj (B,).  F.cross_entropy is the batch mean and the per-sample lambdas
 * multiply that scalar, so dhi[b] = alpha/B (mean(lam_i) (softmax(hi[b]) - onehot(y_emo[b])) +
 * (1 - mean(lam_i)) (softmax(hi[b]) - onehot(y_neu[b]))); dri = -beta/B (t / (p + 1e-8) -
 * (1 - t) / (1 - p + 1e-8)) p (1 - p), p = sigmoid(ri - rj), t = (lam_i - lam_j + 1) / 2,
 * drj = -dri; fp32 in the reference's order (a saturated p gives exactly 0).  One block.     */
int fs2_rank_loss_fwd_bwd(const float* lam_i, const float* lam_j, const float* hi,
                          const float* hj, const float* ri, const float* rj,
                          const int64_t* y_emo, const int64_t* y_neu, int B, int E, float alpha,
                          float beta, float* out, float* dhi, float* dhj, float* dri, float* drj,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * GPU collate: TextMelCollateWithAlignment (fastspeech2/dataset.py:62-133) over
 * one packed upload.  Item u's phonemes / durations are [offsets[u], offsets[u+1]) of the
 * packed int64 arrays; its mel is (n_mels, T_u) channel-major at frame_offsets[u] * n_mels,
 * pitch / energy at frame_offsets[u].  order[i] = item placed at batch row i (the collate's
 * descending torch.sort of phoneme lengths).  Outputs are zero padded: phoneme / duration
 * (B, Tp) int64, mel (B, Tm, n_mels) (the collate's permute(0,2,1), contiguous), pitch /
 * energy (B, Tm), rank_x (B, n_mels+2, Tm) = cat(mel, pitch, energy), lengths (B,) int64.
 * ------------------------------------------------------------------------------------------ */
int fs2_collate_phonemes(const int32_t* order, const int64_t* offsets, const int64_t* phonemes,
                         const int64_t* durations, int B, int Tp, int64_t* phoneme_padded,
                         int64_t* duration_padded, int64_t* input_lengths, void* stream);
int fs2_collate_frames(const int32_t* order, const int64_t* frame_offsets, const float* mel,
                       const float* pitch, const float* energy, int B, int Tm, int n_mels,
                       float* mel_padded, float* pitch_padded, float* energy_padded,
                       float* rank_x, int64_t* output_lengths, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rank-model pair collate (rank_model/dataset.py:71-115) from a device-resident store.  Row b's
 * emotional item is (C, emo_len[b]) channel-major fp32 at store + emo_off[b] (row pitch
 * emo_len[b], offsets in floats, 4-byte alignment only), its neutral item likewise; two rows may
 * name the same item.  length[b] = min(emo_len[b], neu_len[b], T) (a negative length counts as
 * 0; :93), emo_X[b,t,c] = emo_item[c,t] for t < length[b] and 0 for length[b] <= t < T, neu_X
 * the same (:96-107: truncate the pair to the shorter, zero-pad to T, permute(0,2,1), here
 * contiguous (B, T, C)).  T is the caller's: the collate's max over ALL untruncated lengths of
 * the batch (:76-77), which may exceed every length[b].  One launch writes both outputs and
 * length; no workspace, no atomics.  Returns 0 without a launch when B*T == 0; FS2_EINVAL for a
 * null pointer, B < 0, T < 0, B > 65535, C < 3 or C > 130 (n_mels 1..128).
 * ------------------------------------------------------------------------------------------ */
int fs2_rank_collate(const float* store, const int64_t* emo_off, const int64_t* emo_len,
                     const int64_t* neu_off, const int64_t* neu_len, int B, int T, int C,
                     float* emo_X, float* neu_X, int64_t* length, void* stream);

/* ------------------------------------------------------------------------------------------
 * The FastSpeech2 collate (fastspeech2/dataset.py:62-133) from a device-resident store
 * (fastspeech2/device_store.py), one launch.  fstore: per utterance its (n_mels + 2, T_u)
 * channel-major fp32 block cat(mel, pitch, energy), blocks back to back (bases 4-byte aligned
 * only); istore: per utterance n_phon int64 phoneme ids, then n_phon durations.  desc is the
 * batch's gathered descriptor table, (7, B) row-major int64, row b of the batch in column b:
 * float offset, frames, int offset, phonemes, speaker, emotion, cache offset (offsets in
 * elements; speaker and emotion are not read).  Outputs as fs2_collate_phonemes /
 * fs2_collate_frames write them: phoneme / duration (B, Tp) int64 zero padded, input_lengths =
 * phonemes, mel (B, Tm, n_mels) contiguous, pitch / energy (B, Tm), rank_x (B, n_mels + 2, Tm),
 * output_lengths = frames; frames >= Tm and phonemes >= Tp are not written past Tm / Tp.  With
 * cache != NULL also intensity (B, Tp, E) fp32: row b's cached (phonemes, E) block at cache +
 * cache offset, zeros past it (all zeros for a negative cache offset).  No workspace, no atomics.
 * Returns 0 without a launch when B*Tm == 0; FS2_EINVAL for a null pointer (cache and, without
 * a cache, intensity may be null), B, Tp or Tm < 0, B > 65535, n_mels outside [1, 128], or a
 * cache with E < 1.
 * ------------------------------------------------------------------------------------------ */
int fs2_store_collate(const float* fstore, const int64_t* istore, const int64_t* desc,
                      const float* cache, int B, int Tp, int Tm, int n_mels, int E,
                      int64_t* phoneme_padded, int64_t* duration_padded, int64_t* input_lengths,
                      float* mel_padded, float* pitch_padded, float* energy_padded, float* rank_x,
                      int64_t* output_lengths, float* intensity, void* stream);

/* ------------------------------------------------------------------------------------------
 * HiFi-GAN generator forward (speechbrain HIFIGAN.decode_batch,
 * fastspeech2/inference.py:60-63,85).  Convs on fs2_gemm (conv_mode 1 + conv_dil, transposed
 * convs as 3-tap polyphase conv_mode 5, act 3 / 4 epilogues, residual epilogue).
 * ------------------------------------------------------------------------------------------ */
/* mel (B, n_mels, T) fp32 -> X[B*(T+2 pad)][ldx] (dtype), pad replicated frames each side:
 * row t of an utterance holds frame min(max(t - pad, 0), T - 1), so pad may exceed T - 1 (every
 * pad row repeats the first or the last frame; never a reflection).  Columns n_mels..ldx-1 are
 * zeros.  FS2_EINVAL for ldx < n_mels, T < 1, pad < 0 or a null pointer.                     */
int fs2_vocoder_input(const float* mel, int B, int n_mels, int T, int pad, void* X, int ldx,
                      int dtype, void* stream);
/* y = leaky_relu(x, slope) = x >= 0 ? x : x * slope in fp32 (-0.0 stays -0.0, NaN stays NaN);
 * n % (16 / sizeof(dtype)) == 0, x and y 16-byte aligned, else FS2_EINVAL.  y may be x (in
 * place): every element is read and written by the same thread.                            */
int fs2_leaky_relu(const void* x, void* y, int64_t n, float slope, int dtype, void* stream);
/* y = leaky_relu(((a + b) + c) / 3, slope), each fp32 operation rounded once, in this order;
 * the same size and alignment rules for a, b, c and y; y may be any of the inputs            */
int fs2_mean3_leaky_relu(const void* a, const void* b, const void* c, void* y, int64_t n,
                         float slope, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Log-mel front end (rank_model/audio_util.py:23-40 get_mel: speechbrain mel_spectogram with
 * power 1, slaney filterbank, L2 energy, log compression, min-max energy normalisation;
 * fastspeech2/audio.py builds the tables and restates the reference).  fp32 in and out.
 *
 * fs2_melspec: wav is the batch's waveforms packed back to back, utterance b the samples
 * [offsets[b], offsets[b+1]) (offsets: B + 1 int64 on the device; 4-byte alignment only), L_b of
 * them.  Frame t of an utterance is the n_fft samples from t * hop - n_fft / 2, reflected once at
 * either end (torch.stft center=True, pad_mode="reflect"), times window; T_b = 1 + L_b / hop
 * frames.  The reflection needs L_b > n_fft / 2: the lengths are on the device, so the caller
 * checks that; the kernel clamps the reflected index into the utterance, so a shorter one gives
 * other values but never a read outside its own samples (L_b == 0 reads nothing: zeros).
 * Tables, all fp32 on the device except bands: window (n_fft, the hann window already
 * zero-padded centred from win_length), twiddle (n_fft / 2 pairs cos, sin of 2 pi j / n_fft),
 * band_w (the filters' weights back to back: filter m's bins bands[2m] .. bands[2m] +
 * bands[2m+1] - 1).  bands is HOST memory, n_mels pairs (first bin, bins) of int32, read and
 * validated before the call returns; a filter with no bins is (0, 0).  The device evaluates no
 * transcendental but the final log.
 *   mel[m] = sum over the filter's bins of band_w * |X|; with compression log of max(mel, 1e-5)
 *   energy = sqrt of the sum of mel^2 over the filters, before compression
 * Outputs: mel (B, T_max, n_mels) when layout_bct == 0, (B, n_mels, T_max) otherwise; energy
 * (B, T_max); rows t >= T_b of both are exact zeros; mel_len[b] = T_b int64 (not clamped to
 * T_max; frames >= T_max are not written).  One launch, no workspace, no atomics; a workgroup
 * takes 8 consecutive frames of one utterance.  Returns 0 without a launch when B == 0;
 * FS2_EINVAL, before any launch, for n_fft not a power of two or outside [64, 2048], win_length
 * outside [1, n_fft], hop < 1, n_mels outside [1, 256], T_max < 1, B < 0 or B > 65535, a null
 * pointer, or a filter with a negative entry or running past n_fft / 2 + 1 bins.
 *
 * fs2_energy_minmax: out[b][t] = (e[b][t] - min) / (max - min) for t < min(mel_len[b], T_max),
 * min and max over those frames of utterance b (fp32; NaN when one of them is NaN), one IEEE
 * subtraction and division per frame: 0 / 0 = NaN for a single frame or constant energy, the
 * reference's value; 0 for the padded frames.  energy and out are (B, T_max); out may be energy
 * (in place).  FS2_EINVAL for a null pointer, T_max < 1 or B < 0; 0 without a launch for B == 0.
 * ------------------------------------------------------------------------------------------ */
int fs2_melspec(const float* wav, const int64_t* offsets, int B, const float* window,
                const float* twiddle, const int32_t* bands, const float* band_w, int n_fft,
                int win_length, int hop, int n_mels, int T_max, int layout_bct, int compression,
                float* mel, float* energy, int64_t* mel_len, void* stream);
int fs2_energy_minmax(const float* energy, const int64_t* mel_len, int B, int T_max, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Prosody feature stage (rank_model/preprocess.py:104-168 feature_extraction with
 * _average_by_duration :16-23, remove_outliers :27-31, normalize_field :35-46;
 * fastspeech2/prosody.py drives it).  One field (pitch or energy) of B utterances in G groups
 * takes the four launches below.  Every pointer is DEVICE memory; floats need 4-byte, doubles,
 * int64 and the status words their own 8 / 8 / 4-byte alignment only.  No atomics and no
 * workspace: two runs give the same bits.
 *
 * fs2_prosody_track: utterance b reads the values src[src_start[b] .. src_start[b] + D_b) of
 * src (float64 when src_f64 != 0, else float32; src_start and src_len in elements, B int64
 * each) and the durations dur[dur_off[b] .. dur_off[b+1]) (int64; dur_off B + 1 int64); a
 * duration below 0 counts as 0 (the caller refuses those: the durations are on the device).
 * D_b = min(sum of the durations, src_len[b], trk_off[b+1] - trk_off[b], D_max): nothing is read
 * past an utterance's own src_len and nothing written past its own span of track.  The caller
 * makes the four agree; where they do not, the frames of the span from D_b up to D_max are
 * written as 0, so that fs2_prosody_normalize, which sees the span only, reads nothing that was
 * not written.  In float64:
 *   interpolate != 0 (pitch)  every frame equal to 0 becomes slope * (t - lo) + y_lo with
 *     slope = (y_hi - y_lo) / (hi - lo) between its nearest non-zero neighbours lo < t < hi
 *     (scipy interp1d's expression, each operation rounded once), the first / last non-zero
 *     value before / after them; non-zero frames keep their value;
 *   average != 0  every phoneme with a duration > 0 replaces its frames by their mean, summed
 *     in float64 in frame order and rounded once to float32.
 * track (float64, packed: utterance b at trk_off[b], trk_off B + 1 int64) receives the held
 * values.  ustat (B, 5) float64 = n_clean, mean, M2, q1, q3: the quartiles of np.percentile(x,
 * [25, 75]) (linear: virtual index (n - 1) q, a + (b - a) g, for g >= 0.5 b - (b - a) (1 - g)),
 * and count, mean and sum of squared deviations of the values in [q1 - 1.5 iqr, q3 + 1.5 iqr],
 * summed in a fixed order.  status[b] (int32) = 0, or FS2_PROSODY_NONFINITE (1, a NaN or
 * infinity among the D_b values) | FS2_PROSODY_UNVOICED (2, interpolate and no non-zero frame) |
 * FS2_PROSODY_EMPTY (4, D_b == 0); then track holds the values as read and ustat zeros.
 * One workgroup per utterance, 8 * (D_max rounded up to a power of two) bytes of LDS.
 *
 * fs2_prosody_stats: utterances are ordered by group, group g the utterances group_off[g] ..
 * group_off[g+1] - 1 (G + 1 int64).  gstat (G, 4) float64 = min, max, mean, std; this call
 * writes mean and std: the triples of the utterances with status[u] | status2[u] == 0 (status2
 * may be null: the other field's status words) merged in utterance order by Chan's update,
 * std = sqrt(M2 / n), and 1 where var <= n eps var + (n mean eps)^2 (sklearn's constant
 * feature) or the group has no such utterance (mean 0).
 *
 * fs2_prosody_normalize: z[trk_off[b] + t] = float32((track - mean_g) / std_g), one float64
 * subtraction and division, rounded once; umm (B, 2) float64 = min and max of the float64
 * quotient over the utterance.  An utterance with a status word set gets zeros and (+inf, -inf).
 *
 * fs2_prosody_minmax: writes min and max of gstat from umm over each group's utterances
 * without a status word (+inf, -inf for none).
 *
 * Each returns 0 without a launch for B == 0 (G == 0 for the two per-group calls) and
 * FS2_EINVAL, before any launch, for a null pointer (status2 excepted), B < 0, G < 0, D_max
 * outside [1, 4096], or B > 0 with G < 1 in fs2_prosody_normalize.
 * ------------------------------------------------------------------------------------------ */
#define FS2_PROSODY_NONFINITE 1
#define FS2_PROSODY_UNVOICED 2
#define FS2_PROSODY_EMPTY 4
int fs2_prosody_track(const void* src, int src_f64, const int64_t* src_start,
                      const int64_t* src_len, const int64_t* dur, const int64_t* dur_off,
                      const int64_t* trk_off, int B, int D_max, int interpolate, int average,
                      double* track, double* ustat, int32_t* status, void* stream);
int fs2_prosody_stats(const double* ustat, const int32_t* status, const int32_t* status2,
                      const int64_t* group_off, int G, double* gstat, void* stream);
int fs2_prosody_normalize(const double* track, const int64_t* trk_off, const int32_t* status,
                          const int32_t* status2, const int64_t* group_off, int B, int G,
                          int D_max, const double* gstat, float* z, double* umm, void* stream);
int fs2_prosody_minmax(const double* umm, const int32_t* status, const int32_t* status2,
                       const int64_t* group_off, int G, double* gstat, void* stream);

/* utilities */
int fs2_fill(void* X, int64_t n, float value, int dtype, void* stream);
/* X[i] += alpha * Y[i] over n elements of dtype                                           */
int fs2_add(void* X, const void* Y, int64_t n, float alpha, int dtype, void* stream);
/* dst[i] = src[i] converted, for the four pairs of FS2_F32 / FS2_BF16 (fp32 -> bf16 rounds to
 * nearest even, NaN stays NaN; equal dtypes copy); any other dtype on either side is
 * FS2_EINVAL.  One element per thread: src and dst need only their element's own alignment,
 * no 16-byte alignment and no multiple-of-vector n.  fs2_fill and fs2_add likewise.          */
int fs2_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* Dropout seed base (device-resident, added to every launch's seed argument): HIP-graph
 * replays of a step captured with seed 0 set it to the step's seed first; eager steps leave
 * it 0.  Stream-ordered. */
int fs2_set_dropout_seed(uint32_t seed_base, void* stream);
const char* fs2_version(void);
/* first 16 hex digits of the SHA-256 of the sources the library was built from (csrc/*.hip
 * in name order, csrc/*.h in name order, this header): fastspeech2/_native.py refuses a library
 * whose hash differs from the tree's sources (a stale build)                                */
const char* fs2_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* FS2_HIP_H */
