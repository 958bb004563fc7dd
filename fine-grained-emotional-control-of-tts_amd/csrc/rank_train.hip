// Rank-model training: the HBM-bound pieces of the backward around the extractor's GEMMs,
// attention and LayerNorms (which are fs2_gemm, fs2_attn_bwd / fs2_softmax_bwd, fs2_ln_bwd).
//
//   rank_model/model.py:42-43    GELU + dropout of the FFN, forward and backward
//   rank_model/model.py:103-107  backward of the emotion head (embedding add, mask, classifier)
//   rank_model/model.py:160-164  backward of the time-average pooling and the ranking score
//   rank_model/loss.py:36-55     RankLoss values and their gradients
//
//   gelu_dropout_kernel     Hc = keep * GELU(Z) / (1 - p)   or   dZ = dHc * keep / (1 - p) * GELU'(Z);
//                           16-byte chunks of a row where N is even and the pitches allow, the
//                           rest of the row element by element; the forward may read the GEMM's
//                           fp32 Z beside bf16 activations and keep its rounded copy
//   head_bwd_kernel         dH rows and, per run of HEAD_ROWS frames, fp32 partial sums of dWc
//                           and dEmb over the run; one wave owns 64 * V columns
//   head_bwd_final_kernel   the partial sums added in ascending (sequence, run) order (fp64
//                           accumulator), dEmb by the sequences' emotion ids; dbc over all frames
//   rank_pool_bwd_kernel    dI = gI + (gh + gr * Wp) / length, dWp in ascending b
//   rank_loss_bwd_kernel    rank.hip's loss values plus dhi, dhj, dri, drj; one block
// No atomics: every sum has a fixed order, so a second run gives the same bits.
#include <math.h>

#include <algorithm>

#include "fs2_launch.h"

FS2_SEED_SETTER(fs2_seed_base_rank_train)

namespace {

constexpr int RT_MAX_E = 8;
constexpr int HEAD_ROWS = 16;   // frames per partial sum of the head's parameter gradients

// the erf form of the fs2_gemm epilogue (relu = 2)
__device__ __forceinline__ float gelu_f(float v) {
  return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
}
__device__ __forceinline__ float gelu_grad_f(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) +
         v * expf(-0.5f * v * v) * 0.39894228040143268f;
}

// V consecutive elements of a row of TZ (the activation type, or fp32 beside bf16 activations)
template <typename TZ, int V>
__device__ __forceinline__ void load_run(float* o, const TZ* src) {
  constexpr int W = Vec<TZ>::N;
#pragma unroll
  for (int w = 0; w < V; w += W) vload<TZ>(o + w, src + w);
}

// BWD = 0: out = keep * GELU(z) * scale; BWD = 1: out = g * keep * scale * GELU'(z) (out may be g).
// Item q of a row: q < nvec is the 16-byte chunk (of T) at column q * V, the others are the
// columns from nvec * V on.  The mask index m * N + n does not depend on the pitches.
// TZ = float with T = bf16 (forward only): Z is the GEMM's unrounded fp32 output, so GELU sees
// what the evaluation path's fused epilogue sees; ZA (optional) receives Z rounded to T, which
// is what the backward reads.
template <typename TZ, typename T, int BWD>
__global__ void __launch_bounds__(256) gelu_dropout_kernel(const TZ* Z, long ldz, T* ZA,
                                                           long ldza, const T* G, long ldg, T* O,
                                                           long ldo, int M, int N, int nvec,
                                                           float p, float scale, uint32_t seed,
                                                           uint32_t salt) {
  constexpr int V = Vec<T>::N;
  const int per_row = nvec + (N - nvec * V);
  const long total = (long)M * per_row;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / per_row;
    const int q = (int)(i - m * per_row);
    if (q < nvec) {
      const int n = q * V;
      float z[V], g[V], o[V];
      bool k[V];
      load_run<TZ, V>(z, Z + m * ldz + n);
      if (BWD) vload<T>(g, G + m * ldg + n);
      if (ZA) vstore<T>(ZA + m * ldza + n, z);
      fs2_keep_run<V>(seed, salt, (uint64_t)m * N + n, p, k);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float a = BWD ? g[e] * gelu_grad_f(z[e]) : gelu_f(z[e]);
        o[e] = k[e] ? a * scale : 0.f;
      }
      vstore<T>(O + m * ldo + n, o);
    } else {
      const int n = nvec * V + (q - nvec);
      const float z = to_f(Z[m * ldz + n]);
      if (ZA) ZA[m * ldza + n] = from_f<T>(z);
      const float a = BWD ? to_f(G[m * ldg + n]) * gelu_grad_f(z) : gelu_f(z);
      const bool k = fs2_keep(seed, salt, (uint64_t)m * N + n, p);
      O[m * ldo + n] = from_f<T>(k ? a * scale : 0.f);
    }
  }
}

// Block (run r of sequence b, column group): one wave, lane owns V consecutive columns.
// ws: [B * nrun][E + 1][D] fp32 -- rows 0..E-1 the run's dWc part, row E its dEmb part.
template <typename T, int V>
__global__ void __launch_bounds__(64) head_bwd_kernel(const float* gI, const T* H, long ldh,
                                                      const float* emo_tab, const int64_t* emo,
                                                      int n_emo, const int64_t* lens,
                                                      const float* Wc, int Tt, int D, int E,
                                                      int nrun, T* dH, long lddh, float* ws) {
  const int b = blockIdx.x / nrun, run = blockIdx.x - b * nrun;
  const int d0 = (blockIdx.y * 64 + threadIdx.x) * V;
  if (d0 >= D) return;
  const int64_t len = lens[b], k = emo[b];
  const bool has_emb = k >= 0 && k < n_emo;
  float w[RT_MAX_E][V], em[V], aw[RT_MAX_E][V], ae[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    em[v] = has_emb ? emo_tab[k * D + d0 + v] : 0.f;
    ae[v] = 0.f;
  }
#pragma unroll
  for (int e = 0; e < RT_MAX_E; ++e)
#pragma unroll
    for (int v = 0; v < V; ++v) {
      w[e][v] = e < E ? Wc[(long)e * D + d0 + v] : 0.f;
      aw[e][v] = 0.f;
    }
  const int t0 = run * HEAD_ROWS, t1 = min(t0 + HEAD_ROWS, Tt);
  for (int t = t0; t < t1; ++t) {
    const long m = (long)b * Tt + t;
    float dh[V];
#pragma unroll
    for (int v = 0; v < V; ++v) dh[v] = 0.f;
    if (t < len) {
      float h[V];
      if constexpr (V > 1) {
        vload<T>(h, H + m * ldh + d0);
      } else {
        h[0] = to_f(H[m * ldh + d0]);
      }
#pragma unroll
      for (int e = 0; e < RT_MAX_E; ++e)
        if (e < E) {
          const float g = gI[m * E + e];
#pragma unroll
          for (int v = 0; v < V; ++v) {
            dh[v] += g * w[e][v];
            aw[e][v] += g * (h[v] + em[v]);
          }
        }
#pragma unroll
      for (int v = 0; v < V; ++v) ae[v] += dh[v];
    }
    if constexpr (V > 1) {
      vstore<T>(dH + m * lddh + d0, dh);
    } else {
      dH[m * lddh + d0] = from_f<T>(dh[0]);
    }
  }
  float* o = ws + (long)blockIdx.x * (E + 1) * D + d0;
#pragma unroll
  for (int e = 0; e < RT_MAX_E; ++e)
    if (e < E)
#pragma unroll
      for (int v = 0; v < V; ++v) o[(long)e * D + v] = aw[e][v];
#pragma unroll
  for (int v = 0; v < V; ++v) o[(long)E * D + v] = ae[v];
}

// sum of v over the block's 256 threads, the same value in every thread
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// blocks [0, nb): element i = (row, d) of dWc (rows 0..E-1) and dEmb (rows E..E+n_emo-1);
// block nb: dbc
__global__ void __launch_bounds__(256) head_bwd_final_kernel(const float* ws, const float* gI,
                                                             const int64_t* emo, int n_emo, int B,
                                                             int Tt, int D, int E, int nrun,
                                                             int nb, float* dWc, float* dbc,
                                                             float* dEmb) {
  __shared__ double red[4];
  if ((int)blockIdx.x == nb) {
    // padded frames hold the classifier bias (model.py:106-107), so all B * T frames count
    const long M = (long)B * Tt;
    for (int e = 0; e < E; ++e) {
      double a = 0.0;
      for (long m = threadIdx.x; m < M; m += 256) a += (double)gI[m * E + e];
      a = block_sum_d(a, red);
      if (threadIdx.x == 0) dbc[e] = (float)a;
    }
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)(E + n_emo) * D) return;
  const int row = (int)(i / D), d = (int)(i - (long)row * D);
  const long plane = (long)(E + 1) * D;
  double a = 0.0;
  if (row < E) {
    const float* s = ws + (long)row * D + d;
    for (long u = 0; u < (long)B * nrun; ++u) a += (double)s[u * plane];
    dWc[i] = (float)a;
  } else {
    const int k = row - E;
    const float* s = ws + (long)E * D + d;
    for (int b = 0; b < B; ++b)
      if (emo[b] == k)
        for (int r = 0; r < nrun; ++r) a += (double)s[((long)b * nrun + r) * plane];
    dEmb[(long)k * D + d] = (float)a;   // an emotion no sequence carries: exact zeros
  }
}

__device__ __forceinline__ float pool_bwd_elem(const float* gI, const float* gh, const float* gr,
                                               const float* Wp, const int64_t* length, long TE,
                                               int E, long i) {
  const int b = (int)(i / TE), e = (int)(i % E);
  const float c = (gh[(long)b * E + e] + gr[b] * Wp[e]) / (float)length[b];
  return gI ? gI[i] + c : c;
}

__global__ void __launch_bounds__(256) rank_pool_bwd_kernel(const float* gI, const float* gh,
                                                            const float* gr, const float* h,
                                                            const float* Wp,
                                                            const int64_t* length, int B, int T,
                                                            int E, float* dI, float* dWp) {
  const long TE = (long)T * E, n = (long)B * TE;
  if (blockIdx.x == 0 && (int)threadIdx.x < E) {   // model.py:163: r = h . Wp
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += gr[b] * h[(long)b * E + threadIdx.x];
    dWp[threadIdx.x] = a;
  }
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    f32x4 o;
#pragma unroll
    for (int v = 0; v < 4; ++v) o[v] = pool_bwd_elem(nullptr, gh, gr, Wp, length, TE, E, i + v);
    if (gI) o += *(const f32x4*)(gI + i);
    *(f32x4*)(dI + i) = o;
  } else {
    for (long j = i; j < n; ++j) dI[j] = pool_bwd_elem(gI, gh, gr, Wp, length, TE, E, j);
  }
}

// softmax of one row of logits into p[0..E)
__device__ __forceinline__ void softmax_row(const float* x, int E, float* p) {
  float mx = x[0];
  for (int e = 1; e < E; ++e) mx = fmaxf(mx, x[e]);
  float s = 0.f;
  for (int e = 0; e < E; ++e) s += (p[e] = expf(x[e] - mx));
  for (int e = 0; e < E; ++e) p[e] /= s;
}
// cross entropy of one row (rank.hip's ce_row): NaN for a target outside [0, E)
__device__ __forceinline__ float ce_row(const float* x, int E, int64_t y) {
  if (y < 0 || y >= E) return __builtin_nanf("");
  float mx = x[0];
  for (int e = 1; e < E; ++e) mx = fmaxf(mx, x[e]);
  float s = 0.f;
  for (int e = 0; e < E; ++e) s += expf(x[e] - mx);
  return (mx + logf(s)) - x[y];
}
__device__ __forceinline__ float block_sum_f(float v, double* red) {
  return (float)block_sum_d((double)v, red);
}

__global__ void __launch_bounds__(256) rank_loss_bwd_kernel(
    const float* lam_i, const float* lam_j, const float* hi, const float* hj, const float* ri,
    const float* rj, const int64_t* y_emo, const int64_t* y_neu, int B, int E, float alpha,
    float beta, float* out, float* dhi, float* dhj, float* dri, float* drj) {
  __shared__ double red[4];
  // ---- the values, as rank.hip's rank_loss_kernel computes them
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  float sl[2] = {0.f, 0.f};
  for (int b = threadIdx.x; b < B; b += 256) {
    c[0] += ce_row(hi + (long)b * E, E, y_emo[b]);
    c[1] += ce_row(hi + (long)b * E, E, y_neu[b]);
    c[2] += ce_row(hj + (long)b * E, E, y_emo[b]);
    c[3] += ce_row(hj + (long)b * E, E, y_neu[b]);
    sl[0] += lam_i[b];
    sl[1] += lam_j[b];
  }
  const float inv = 1.f / (float)B;
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = block_sum_f(c[k], red) * inv;
  const float mli = block_sum_f(sl[0], red) * inv, mlj = block_sum_f(sl[1], red) * inv;
  float mix = 0.f, rank = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float li = lam_i[b], lj = lam_j[b];
    mix += (li * c[0] + (1.f - li) * c[1]) + (lj * c[2] + (1.f - lj) * c[3]);
    const float p = 1.f / (1.f + expf(-(ri[b] - rj[b])));
    const float ld = (li - lj + 1.f) / 2.f;
    rank += ld * logf(p + 1e-8f) + (1.f - ld) * logf(1.f - p + 1e-8f);
    {
#pragma clang fp contract(off)
      // ---- gradients of the total, products and sums not contracted.  loss.py:49-51 backwards
      // in autograd's order: the two log terms, then torch.sigmoid's p (1 - p), so a saturated p
      // (1 - p == 0 in fp32) gives exactly 0 as the reference's backward does
      const float up = -(beta * inv);
      const float dp = up * ld / (p + 1e-8f) - up * (1.f - ld) / ((1.f - p) + 1e-8f);
      const float dr = dp * ((1.f - p) * p);
      dri[b] = dr;
      drj[b] = -dr;
      // loss.py:40-44: cross_entropy is the batch mean and the lambdas multiply that scalar, so
      // row b's gradient carries the batch MEAN of the lambdas
      float pi[RT_MAX_E], pj[RT_MAX_E];
      softmax_row(hi + (long)b * E, E, pi);
      softmax_row(hj + (long)b * E, E, pj);
      const int64_t ye = y_emo[b], yn = y_neu[b];
      const float s = alpha * inv;
      for (int e = 0; e < E; ++e) {
        const float oe = e == ye ? 1.f : 0.f, on = e == yn ? 1.f : 0.f;
        dhi[(long)b * E + e] = s * (mli * (pi[e] - oe) + (1.f - mli) * (pi[e] - on));
        dhj[(long)b * E + e] = s * (mlj * (pj[e] - oe) + (1.f - mlj) * (pj[e] - on));
      }
    }
  }
  mix = block_sum_f(mix, red) * inv;
  rank = -(block_sum_f(rank, red) * inv);
  if (threadIdx.x == 0) {
    out[0] = alpha * mix + beta * rank;
    out[1] = mix;
    out[2] = rank;
  }
}

template <typename TZ, typename T, int BWD>
void launch_gelu_dropout(const void* Z, int64_t ldz, void* ZA, int64_t ldza, const void* G,
                         int64_t ldg, void* O, int64_t ldo, int M, int N, float p, uint32_t seed,
                         uint32_t salt, hipStream_t s) {
  constexpr int V = Vec<T>::N;
  // 16-byte chunks need an even element index at every chunk (one hash per pair) and aligned rows
  const bool vec = N % 2 == 0 && ldz % Vec<TZ>::N == 0 && ldo % V == 0 && aligned16(Z) &&
                   aligned16(O) && (!ZA || (ldza % V == 0 && aligned16(ZA))) &&
                   (!BWD || (ldg % V == 0 && aligned16(G)));
  const int nvec = vec ? N / V : 0;
  const long total = (long)M * (nvec + (N - nvec * V));
  // HBM-bound: about eight blocks per CU, the rest of the items by grid stride
  const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 2048);
  hipLaunchKernelGGL((gelu_dropout_kernel<TZ, T, BWD>), dim3(grid), dim3(256), 0, s,
                     (const TZ*)Z, (long)ldz, (T*)ZA, (long)ldza, (const T*)G, (long)ldg, (T*)O,
                     (long)ldo, M, N, nvec, p, 1.f / (1.f - p), seed, salt);
}

template <typename T>
void launch_head_bwd(const float* gI, const void* H, int64_t ldh, const float* emo_tab,
                     const int64_t* emo, int n_emo, const int64_t* lens, const float* Wc, int B,
                     int T_, int D, int E, int nrun, void* dH, int64_t lddh, float* ws,
                     hipStream_t s) {
  constexpr int V = Vec<T>::N;
  const bool vec = D % V == 0 && ldh % V == 0 && lddh % V == 0 && aligned16(H) && aligned16(dH);
  const unsigned gx = (unsigned)(B * nrun);
  if (vec)
    hipLaunchKernelGGL((head_bwd_kernel<T, V>), dim3(gx, nblk(D, 64 * V)), dim3(64), 0, s, gI,
                       (const T*)H, (long)ldh, emo_tab, emo, n_emo, lens, Wc, T_, D, E, nrun,
                       (T*)dH, (long)lddh, ws);
  else
    hipLaunchKernelGGL((head_bwd_kernel<T, 1>), dim3(gx, nblk(D, 64)), dim3(64), 0, s, gI,
                       (const T*)H, (long)ldh, emo_tab, emo, n_emo, lens, Wc, T_, D, E, nrun,
                       (T*)dH, (long)lddh, ws);
}

}  // namespace

extern "C" int fs2_gelu_dropout_fwd(const void* Z, int64_t ldz, int z_fp32, void* Zact,
                                    int64_t ldza, void* Hc, int64_t ldh, int M, int N, float p,
                                    uint32_t seed, uint32_t salt, int dtype, void* stream) {
  if (M < 0 || N < 0 || (dtype != FS2_F32 && dtype != FS2_BF16) || !(p >= 0.f && p < 1.f))
    return FS2_EINVAL;
  if ((long)M * N == 0) return 0;
  if (!Z || !Hc || ldz < N || ldh < N || (Zact && ldza < N)) return FS2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FS2_F32)
    launch_gelu_dropout<float, float, 0>(Z, ldz, Zact, ldza, nullptr, 0, Hc, ldh, M, N, p, seed,
                                         salt, s);
  else if (z_fp32)
    launch_gelu_dropout<float, bf16, 0>(Z, ldz, Zact, ldza, nullptr, 0, Hc, ldh, M, N, p, seed,
                                        salt, s);
  else
    launch_gelu_dropout<bf16, bf16, 0>(Z, ldz, Zact, ldza, nullptr, 0, Hc, ldh, M, N, p, seed,
                                       salt, s);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_gelu_dropout_bwd(const void* dHc, int64_t lddh, const void* Z, int64_t ldz,
                                    void* dZ, int64_t lddz, int M, int N, float p, uint32_t seed,
                                    uint32_t salt, int dtype, void* stream) {
  if (M < 0 || N < 0 || (dtype != FS2_F32 && dtype != FS2_BF16) || !(p >= 0.f && p < 1.f))
    return FS2_EINVAL;
  if ((long)M * N == 0) return 0;
  if (!dHc || !Z || !dZ || lddh < N || ldz < N || lddz < N) return FS2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FS2_BF16)
    launch_gelu_dropout<bf16, bf16, 1>(Z, ldz, nullptr, 0, dHc, lddh, dZ, lddz, M, N, p, seed,
                                       salt, s);
  else
    launch_gelu_dropout<float, float, 1>(Z, ldz, nullptr, 0, dHc, lddh, dZ, lddz, M, N, p, seed,
                                         salt, s);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t fs2_intensity_head_bwd_workspace_floats(int B, int T, int D, int E) {
  if (B <= 0 || T <= 0 || D <= 0 || E <= 0) return 0;
  return (int64_t)B * ((T + HEAD_ROWS - 1) / HEAD_ROWS) * (E + 1) * D;
}

extern "C" int fs2_intensity_head_bwd(const float* gI, const void* H, int64_t ldh,
                                      const float* emo_table, const int64_t* emotions,
                                      int n_emotions, const int64_t* lengths, const float* Wc,
                                      int B, int T, int D, int E, void* dH, int64_t lddh,
                                      float* dWc, float* dbc, float* dEmb, float* workspace,
                                      int dtype, void* stream) {
  if (B < 0 || T < 0 || D < 0 || E < 0 || n_emotions < 0 ||
      (dtype != FS2_F32 && dtype != FS2_BF16))
    return FS2_EINVAL;
  if ((long)B * T * D == 0) return 0;
  if (!gI || !H || !emo_table || !emotions || !lengths || !Wc || !dH || !dWc || !dbc || !dEmb ||
      !workspace || E < 1 || E > RT_MAX_E || ldh < D || lddh < D)
    return FS2_EINVAL;
  const int nrun = (T + HEAD_ROWS - 1) / HEAD_ROWS;
  if ((long)B * nrun > 0x7fffffffL) return FS2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FS2_BF16)
    launch_head_bwd<bf16>(gI, H, ldh, emo_table, emotions, n_emotions, lengths, Wc, B, T, D, E,
                          nrun, dH, lddh, workspace, s);
  else
    launch_head_bwd<float>(gI, H, ldh, emo_table, emotions, n_emotions, lengths, Wc, B, T, D, E,
                           nrun, dH, lddh, workspace, s);
  FS2_CHECK_LAUNCH();
  const int nb = (int)nblk((long)(E + n_emotions) * D);
  hipLaunchKernelGGL(head_bwd_final_kernel, dim3(nb + 1), dim3(256), 0, s, workspace, gI,
                     emotions, n_emotions, B, T, D, E, nrun, nb, dWc, dbc, dEmb);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_rank_pool_bwd(const float* gI, const float* gh, const float* gr,
                                 const float* h, const float* Wp, const int64_t* length, int B,
                                 int T, int E, float* dI, float* dWp, void* stream) {
  if (B < 0 || T < 0 || E < 0) return FS2_EINVAL;
  if ((long)B * E == 0) return 0;
  if (!gh || !gr || !h || !Wp || !length || !dWp || (!dI && T > 0) || E > RT_MAX_E ||
      !aligned16(dI) || !aligned16(gI))
    return FS2_EINVAL;
  const long n = (long)B * T * E;
  hipLaunchKernelGGL(rank_pool_bwd_kernel, dim3(std::max(1u, nblk((n + 3) / 4))), dim3(256), 0,
                     (hipStream_t)stream, gI, gh, gr, h, Wp, length, B, T, E, dI, dWp);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_rank_loss_fwd_bwd(const float* lam_i, const float* lam_j, const float* hi,
                                     const float* hj, const float* ri, const float* rj,
                                     const int64_t* y_emo, const int64_t* y_neu, int B, int E,
                                     float alpha, float beta, float* out, float* dhi, float* dhj,
                                     float* dri, float* drj, void* stream) {
  if (B < 0 || E < 0) return FS2_EINVAL;
  if (B == 0) return 0;
  if (!lam_i || !lam_j || !hi || !hj || !ri || !rj || !y_emo || !y_neu || !out || !dhi || !dhj ||
      !dri || !drj || E < 1 || E > RT_MAX_E)
    return FS2_EINVAL;
  hipLaunchKernelGGL(rank_loss_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lam_i,
                     lam_j, hi, hj, ri, rj, y_emo, y_neu, B, E, alpha, beta, out, dhi, dhj, dri,
                     drj);
  FS2_CHECK_LAUNCH();
  return 0;
}
