// Rank-model evaluation path: the HBM-bound pieces around the IntensityExtractor forward.
//
//   rank_model/model.py:148-153   frame-level mixup of the emotional and the neutral input
//   rank_model/model.py:160-164   time-average pooling and the ranking score
//   rank_model/loss.py:36-55      RankLoss values (forward only)
//   rank_model/inference.py:98-114  per (speaker, emotion) binning of frames sorted by score
//
// The extractor itself (GEMMs, attention, LayerNorm, emotion head) is intensity.hip's path, run
// once over the 2B mixed sequences this file stages.
//   rank_mixup_kernel    emo_X, neu_X fp32 (B,T,C), lambdas (2,B) -> GEMM rows [2*B*T][ldx] in
//                        the activation dtype, zero-padded columns; rows [0, B*T) mixed with
//                        lam_i, rows [B*T, 2*B*T) with lam_j
//   rank_pool_kernel     h[b][e] = sum_{t < T} I[b][t][e] / float(length[b]),
//                        r[b] = sum_e h[b][e] * Wp[e]; one block per sequence
//   rank_loss_kernel     (total, L_mixup, L_rank); one block
//   bucket_means_kernel  mean of bucket k of group g's score-ordered frames; one block per
//                        (group, bucket)
// Every reduction has a fixed order (strided per-thread partial sums, xor butterfly within a
// wave, waves added in index order by one thread) and uses no atomics: the results are the same
// bits run to run.
#include <math.h>

#include "fs2_launch.h"

namespace {

constexpr int RANK_MAX_E = 8;

// model.py:152 as written: two rounded products and one rounded add.  No contraction into an fma,
// so lam == 1 returns emo and lam == 0 returns neu bit for bit.
__device__ __forceinline__ float mixup(float lam, float e, float n) {
#pragma clang fp contract(off)
  const float a = lam * e;
  const float b = (1.f - lam) * n;
  return a + b;
}

template <typename TO>
__global__ void rank_mixup_kernel(const float* emo, const float* neu, const float* lambdas, int B,
                                  int T, int C, TO* X, int ldx, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long m = i / ldx;
  const int c = (int)(i - m * ldx);
  const long BT = (long)B * T;
  const int which = m >= BT;
  const long mm = m - which * BT;
  const int b = (int)(mm / T);
  float v = 0.f;
  if (c < C) v = mixup(lambdas[which * B + b], emo[mm * C + c], neu[mm * C + c]);
  X[i] = from_f<TO>(v);
}

// sum of v over the block's 256 threads, the same value in every thread
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) rank_pool_kernel(const float* I, const int64_t* length,
                                                        const float* Wp, int T, int E, float* h,
                                                        float* r) {
  __shared__ double red[4];
  __shared__ float hs[RANK_MAX_E];
  const int b = blockIdx.x;
  const float* Ib = I + (long)b * T * E;
  double acc[RANK_MAX_E];
#pragma unroll
  for (int e = 0; e < RANK_MAX_E; ++e) acc[e] = 0.0;
  for (int t = threadIdx.x; t < T; t += 256)
#pragma unroll
    for (int e = 0; e < RANK_MAX_E; ++e)
      if (e < E) acc[e] += (double)Ib[(long)t * E + e];
  const float len = (float)length[b];
#pragma unroll
  for (int e = 0; e < RANK_MAX_E; ++e)
    if (e < E) {
      const double s = block_sum_d(acc[e], red);
      if (threadIdx.x == 0) {
        const float v = (float)s / len;   // model.py:160: fp32 sum / length.float()
        hs[e] = v;
        h[(long)b * E + e] = v;
      }
    }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int e = 0; e < E; ++e) s += hs[e] * Wp[e];
    r[b] = s;
  }
}

// cross entropy of one row of logits (log-sum-exp minus the target's logit); NaN for a target
// outside [0, E), which F.cross_entropy rejects
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

__global__ void __launch_bounds__(256) rank_loss_kernel(const float* lam_i, const float* lam_j,
                                                        const float* hi, const float* hj,
                                                        const float* ri, const float* rj,
                                                        const int64_t* y_emo, const int64_t* y_neu,
                                                        int B, int E, float alpha, float beta,
                                                        float* out) {
  __shared__ double red[4];
  // F.cross_entropy's batch means (loss.py:40-43): four scalars
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < B; b += 256) {
    c[0] += ce_row(hi + (long)b * E, E, y_emo[b]);
    c[1] += ce_row(hi + (long)b * E, E, y_neu[b]);
    c[2] += ce_row(hj + (long)b * E, E, y_emo[b]);
    c[3] += ce_row(hj + (long)b * E, E, y_neu[b]);
  }
  const float inv = 1.f / (float)B;
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = block_sum_f(c[k], red) * inv;
  float mix = 0.f, rank = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float li = lam_i[b], lj = lam_j[b];
    // the scalar means times the per-sample lambdas, then the mean over the batch (:40-44)
    mix += (li * c[0] + (1.f - li) * c[1]) + (lj * c[2] + (1.f - lj) * c[3]);
    const float p = 1.f / (1.f + expf(-(ri[b] - rj[b])));
    const float ld = (li - lj + 1.f) / 2.f;
    rank += ld * logf(p + 1e-8f) + (1.f - ld) * logf(1.f - p + 1e-8f);   // :49-51
  }
  mix = block_sum_f(mix, red) * inv;
  rank = -(block_sum_f(rank, red) * inv);
  if (threadIdx.x == 0) {
    out[0] = alpha * mix + beta * rank;
    out[1] = mix;
    out[2] = rank;
  }
}

// Block (g, k).  Group g's utterances are order[grp_off[g] .. grp_off[g+1]) (ascending score);
// cstart[j] is the number of frames before sorted utterance j over the whole sorted list, so the
// group's concatenated frames are positions [cstart[grp_off[g]], cstart[grp_off[g+1]]) and frame
// n of sorted utterance j is row utt_off[order[j]] + n - cstart[j] of ``frames``.
__global__ void __launch_bounds__(256) bucket_means_kernel(const float* frames,
                                                           const int64_t* order,
                                                           const int64_t* cstart,
                                                           const int64_t* utt_off,
                                                           const int64_t* grp_off, int K, int E,
                                                           float* out) {
  __shared__ double red[4];
  const int g = blockIdx.x / K, k = blockIdx.x - g * K;
  const int64_t j0 = grp_off[g], j1 = grp_off[g + 1];
  float* o = out + (long)blockIdx.x * E;
  if (j1 <= j0) {   // empty group: the reference skips it, the bank keeps its zeros
    if (threadIdx.x < E) o[threadIdx.x] = 0.f;
    return;
  }
  const int64_t base = cstart[j0], N = cstart[j1] - base;
  // np.array_split(N, K): the first N % K buckets hold N / K + 1 frames, the rest N / K
  const int64_t q = N / K, rem = N % K;
  const int64_t lo = base + k * q + min<int64_t>(k, rem), cnt = q + (k < rem ? 1 : 0);
  double acc[RANK_MAX_E];
#pragma unroll
  for (int e = 0; e < RANK_MAX_E; ++e) acc[e] = 0.0;
  for (int64_t n = lo + threadIdx.x; n < lo + cnt; n += 256) {
    // last j in [j0, j1) with cstart[j] <= n (utterances of zero frames are passed over)
    int64_t a = j0, z = j1 - 1;
    while (a < z) {
      const int64_t mid = (a + z + 1) >> 1;
      if (cstart[mid] <= n) a = mid; else z = mid - 1;
    }
    const float* f = frames + (utt_off[order[a]] + (n - cstart[a])) * E;
#pragma unroll
    for (int e = 0; e < RANK_MAX_E; ++e)
      if (e < E) acc[e] += (double)f[e];
  }
#pragma unroll
  for (int e = 0; e < RANK_MAX_E; ++e)
    if (e < E) {
      const double s = block_sum_d(acc[e], red);
      // an empty bucket (N < K) is 0 / 0 = NaN: numpy's mean of an empty slice
      if (threadIdx.x == 0) o[e] = (float)(s / (double)cnt);
    }
}

}  // namespace

extern "C" int fs2_rank_mixup_input(const float* emo_X, const float* neu_X, const float* lambdas,
                                    int B, int T, int C, void* X, int ldx, int dtype,
                                    void* stream) {
  if (B < 0 || T < 0 || C < 0 || ldx < 0) return FS2_EINVAL;
  const long n = 2L * B * T * ldx;
  if (n == 0) return 0;
  if (!emo_X || !neu_X || !lambdas || !X || ldx < C) return FS2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(dtype, [&](auto t) {
    using U = decltype(t);
    hipLaunchKernelGGL(rank_mixup_kernel<U>, dim3(nblk(n)), dim3(256), 0, s, emo_X, neu_X,
                       lambdas, B, T, C, (U*)X, ldx, n);
  });
}

extern "C" int fs2_rank_pool(const float* I, const int64_t* length, const float* Wp, int B, int T,
                             int E, float* h, float* r, void* stream) {
  if (B < 0 || T < 0 || E < 0) return FS2_EINVAL;
  if ((long)B * E == 0) return 0;
  if ((!I && T > 0) || !length || !Wp || !h || !r || E > RANK_MAX_E) return FS2_EINVAL;
  hipLaunchKernelGGL(rank_pool_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, I, length, Wp,
                     T, E, h, r);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_rank_loss_fwd(const float* lam_i, const float* lam_j, const float* hi,
                                 const float* hj, const float* ri, const float* rj,
                                 const int64_t* y_emo, const int64_t* y_neu, int B, int E,
                                 float alpha, float beta, float* out, void* stream) {
  if (B < 0 || E < 0) return FS2_EINVAL;
  if (B == 0) return 0;
  if (!lam_i || !lam_j || !hi || !hj || !ri || !rj || !y_emo || !y_neu || !out || E < 1)
    return FS2_EINVAL;
  hipLaunchKernelGGL(rank_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lam_i, lam_j,
                     hi, hj, ri, rj, y_emo, y_neu, B, E, alpha, beta, out);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_bucket_means(const float* frames, const int64_t* order, const int64_t* cstart,
                                const int64_t* utt_off, const int64_t* grp_off, int G, int K,
                                int E, float* out, void* stream) {
  if (G < 0 || K < 0 || E < 0) return FS2_EINVAL;
  if ((long)G * K * E == 0) return 0;
  if (!frames || !order || !cstart || !utt_off || !grp_off || !out || E > RANK_MAX_E ||
      (long)G * K > 0x7fffffffL)
    return FS2_EINVAL;
  hipLaunchKernelGGL(bucket_means_kernel, dim3((unsigned)(G * K)), dim3(256), 0,
                     (hipStream_t)stream, frames, order, cstart, utt_off, grp_off, K, E, out);
  FS2_CHECK_LAUNCH();
  return 0;
}
