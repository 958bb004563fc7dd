// Prosody feature stage: raw F0 / energy tracks -> finished, standardised pitch and energy with
// the per-(speaker, emotion) statistics of stats.json (fastspeech2/prosody.py).
//
//   rank_model/preprocess.py:104-168  feature_extraction (second half), with
//                                     _average_by_duration (:16-23), remove_outliers (:27-31)
//                                     and normalize_field (:35-46)
//
//   prosody_track_kernel      one workgroup per utterance.  D = sum of the durations; the first D
//                             values go into LDS as float64.  Pitch: the zero frames are
//                             interpolated between their voiced neighbours (interp1d's two-point
//                             formula, first / last voiced value outside), a thread per chunk of
//                             ceil(D / 256) frames after two block scans of the chunks' last and
//                             first voiced index.  Optional phoneme averaging: a block scan of
//                             the durations gives every phoneme its span, one thread sums it in
//                             float64, rounds the mean once to float32 and writes it back over
//                             the span.  The held track is stored, then sorted in place in LDS
//                             (bitonic, padded with +inf to a power of two) for the quartiles
//                             of np.percentile's linear method; the values inside the fences
//                             are reduced to (n, mean, M2) by a fixed tree: thread partials in
//                             index order, the wave's xor butterfly, the four waves in order.
//   prosody_stats_kernel      one wave per group: the utterances' triples merged in utterance
//                             order (Chan), std = sqrt(M2 / n), sklearn's constant-feature rule.
//   prosody_normalize_kernel  z = (x - mean_g) / std_g in float64, rounded once to float32;
//                             the utterance's float64 min and max.
//   prosody_minmax_kernel     one wave per group: min and max over its utterances.
//
// No atomics: every sum has one order, so two runs give the same bits.  The float64 products
// and sums whose rounding the reference's numpy arithmetic fixes stay separate operations: the
// whole file is compiled with FMA contraction off.
#include "fs2_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int PR_MAX_D = 4096;   // frames per utterance (fastspeech2/ops.py PROSODY_MAX_D)
constexpr int PR_USTAT = 5;      // n_clean, mean, M2, q1, q3
enum { PR_NONFINITE = 1, PR_UNVOICED = 2, PR_EMPTY = 4 };

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// the sum over a 256-thread block in a fixed order; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();               // the previous use of red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ int flagged(const int32_t* s0, const int32_t* s1, long u) {
  return s0[u] | (s1 ? s1[u] : 0);
}

__device__ __forceinline__ int dur_clamped(const int64_t* dur, long i) {
  const int64_t d = dur[i];
  return (int)min<int64_t>(max<int64_t>(d, 0), PR_MAX_D + 1);
}

__global__ void __launch_bounds__(256)
prosody_track_kernel(const void* __restrict__ src, int src_f64,
                     const int64_t* __restrict__ src_start, const int64_t* __restrict__ src_len,
                     const int64_t* __restrict__ dur, const int64_t* __restrict__ dur_off,
                     const int64_t* __restrict__ trk_off, int D_max, int interpolate, int average,
                     double* track, double* __restrict__ ustat, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double vals[];   // next power of two >= D_max
  __shared__ double red[4];
  __shared__ int sl[256], sf[256], wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  const long p0 = dur_off[b];
  const long P = max<long>(dur_off[b + 1] - p0, 0);
  const long o0 = trk_off[b];

  // D = sum of the (non-negative) durations, then clamped to what may be read and written
  double dsum = 0.0;             // exact: integers far below 2^53
  for (long i = tid; i < P; i += 256) dsum += (double)dur_clamped(dur, p0 + i);
  dsum = block_sum_d(dsum, red);
  const long cap = min<long>(min<long>(max<long>(src_len[b], 0), max<long>(trk_off[b + 1] - o0, 0)),
                             D_max);
  const int D = (int)min<double>(dsum, (double)cap);
  // the utterance's span of track past D (a caller whose lengths disagree): zeros, so that
  // fs2_prosody_normalize, which sees the span only, never reads what was not written
  const int span = (int)min<long>(max<long>(trk_off[b + 1] - o0, 0), D_max);
  for (int t = D + tid; t < span; t += 256) track[o0 + t] = 0.0;

  const long s0 = src_start[b];
  int bad = 0, voiced = 0;
  for (int t = tid; t < D; t += 256) {
    const double v = src_f64 ? ((const double*)src)[s0 + t] : (double)((const float*)src)[s0 + t];
    vals[t] = v;
    bad |= !(fabs(v) <= 1.7976931348623157e308);
    voiced |= v != 0.0;
  }
  bad = __syncthreads_or(bad);
  voiced = __syncthreads_or(voiced);
  const int st = (bad ? PR_NONFINITE : 0) | (interpolate && !voiced && !bad ? PR_UNVOICED : 0) |
                 (D == 0 ? PR_EMPTY : 0);
  if (st) {                      // block-uniform: the values as read, no statistics
    for (int t = tid; t < D; t += 256) track[o0 + t] = vals[t];
    if (tid < PR_USTAT) ustat[b * PR_USTAT + tid] = 0.0;
    if (tid == 0) status[b] = st;
    return;
  }

  if (interpolate) {
    // thread tid owns frames [lo, hi); sl / sf: the last / first voiced frame of the chunks up
    // to / from this one after the scans
    const int chunk = (D + 255) / 256;
    const int lo = min(tid * chunk, D), hi = min(lo + chunk, D);
    int last_v = -1, first_v = D;
    for (int t = lo; t < hi; ++t)
      if (vals[t] != 0.0) {
        last_v = t;
        if (first_v == D) first_v = t;
      }
    sl[tid] = last_v;
    sf[tid] = first_v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int a = tid >= off ? sl[tid - off] : -1;
      const int c = tid + off < 256 ? sf[tid + off] : D;
      __syncthreads();
      sl[tid] = max(sl[tid], a);
      sf[tid] = min(sf[tid], c);
      __syncthreads();
    }
    int prev = tid > 0 ? sl[tid - 1] : -1;
    const int next_out = tid < 255 ? sf[tid + 1] : D;
    // only zero frames are written and only voiced frames are read by index: in place
    for (int t = lo; t < hi; ++t) {
      if (vals[t] != 0.0) {
        prev = t;
        continue;
      }
      int next = next_out;
      for (int u = t + 1; u < hi; ++u)
        if (vals[u] != 0.0) {
          next = u;
          break;
        }
      double y;
      if (prev < 0) y = vals[next];                  // at least one voiced frame exists
      else if (next >= D) y = vals[prev];
      else {
        const double ylo = vals[prev], yhi = vals[next];
        const double slope = (yhi - ylo) / (double)(next - prev);
        y = slope * (double)(t - prev) + ylo;
      }
      vals[t] = y;               // never read again: prev is an index, the search runs over u > t
    }
    __syncthreads();
  }

  if (average) {
    long carry = 0;
    for (long base = 0; base < P; base += 256) {
      const long i = base + tid;
      const int d = i < P ? dur_clamped(dur, p0 + i) : 0;
      int x = d;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      __syncthreads();           // the previous round's reads of wtot
      if (lane == 63) wtot[wave] = x;
      __syncthreads();
      int woff = 0, total = 0;
      for (int w = 0; w < 4; ++w) {
        if (w < wave) woff += wtot[w];
        total += wtot[w];
      }
      const long start = carry + woff + x - d;
      carry += total;
      if (d > 0 && start < D) {  // the spans of different phonemes are disjoint: in place
        const int a = (int)start, e = (int)min<long>(start + d, D);
        double s = 0.0;
        for (int t = a; t < e; ++t) s += vals[t];
        const double m = (double)(float)(s / (double)(e - a));
        for (int t = a; t < e; ++t) vals[t] = m;
      }
    }
    __syncthreads();
  }

  // the held track; each thread reads its own elements back below
  for (int t = tid; t < D; t += 256) track[o0 + t] = vals[t];

  // order statistics: bitonic sort of the next power of two, +inf behind the track
  int N2 = 1;
  while (N2 < D) N2 <<= 1;
  for (int t = D + tid; t < N2; t += 256) vals[t] = INFINITY;
  __syncthreads();
  for (int k = 2; k <= N2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < N2; i += 256) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const double a = vals[i], c = vals[ixj];
          if ((a > c) == ((i & k) == 0)) {
            vals[i] = c;
            vals[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  // np.percentile(x, [25, 75]), method "linear": virtual index (n - 1) q, numpy's _lerp
  double q[2];
  for (int h = 0; h < 2; ++h) {
    const double vi = (double)(D - 1) * (h ? 0.75 : 0.25);
    const int p = (int)vi, nx = min(p + 1, D - 1);
    const double g = vi - (double)p;
    const double a = vals[p], c = vals[nx], diff = c - a;
    q[h] = g >= 0.5 ? c - diff * (1.0 - g) : a + diff * g;
  }
  const double iqr = q[1] - q[0];
  const double f_lo = q[0] - 1.5 * iqr, f_hi = q[1] + 1.5 * iqr;

  double cnt = 0.0, sum = 0.0;
  for (int t = tid; t < D; t += 256) {
    const double v = track[o0 + t];
    if (v >= f_lo && v <= f_hi) {
      cnt += 1.0;
      sum += v;
    }
  }
  cnt = block_sum_d(cnt, red);
  sum = block_sum_d(sum, red);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double m2 = 0.0, c1 = 0.0;     // corrected two-pass: M2 = sum (x - mean)^2 - (sum (x - mean))^2 / n
  for (int t = tid; t < D; t += 256) {
    const double v = track[o0 + t];
    if (v >= f_lo && v <= f_hi) {
      const double dv = v - mean;
      m2 += dv * dv;
      c1 += dv;
    }
  }
  m2 = block_sum_d(m2, red);
  c1 = block_sum_d(c1, red);
  if (cnt > 0.0) m2 = fmax(m2 - c1 * c1 / cnt, 0.0);
  if (tid == 0) {
    double* u = ustat + b * PR_USTAT;
    u[0] = cnt;
    u[1] = mean;
    u[2] = m2;
    u[3] = q[0];
    u[4] = q[1];
    status[b] = 0;
  }
}

__global__ void __launch_bounds__(64)
prosody_stats_kernel(const double* __restrict__ ustat, const int32_t* __restrict__ status,
                     const int32_t* __restrict__ status2, const int64_t* __restrict__ group_off,
                     double* __restrict__ gstat) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const long u0 = group_off[g], u1 = group_off[g + 1];
  double n = 0.0, mean = 0.0, M2 = 0.0;
  for (long base = u0; base < u1; base += 64) {
    const long u = base + lane;
    double nb = 0.0, mb = 0.0, Mb = 0.0;
    if (u < u1 && !flagged(status, status2, u)) {
      nb = ustat[u * PR_USTAT];
      mb = ustat[u * PR_USTAT + 1];
      Mb = ustat[u * PR_USTAT + 2];
    }
    const int cnt = (int)min<long>(64, u1 - base);
    for (int j = 0; j < cnt; ++j) {          // wave-uniform: every lane merges the same triple
      const double bn = __shfl(nb, j, 64), bm = __shfl(mb, j, 64), bM = __shfl(Mb, j, 64);
      if (bn <= 0.0) continue;
      if (n == 0.0) {
        n = bn;
        mean = bm;
        M2 = bM;
        continue;
      }
      const double tot = n + bn, delta = bm - mean;
      mean = mean + delta * (bn / tot);
      M2 = (M2 + bM) + delta * delta * (n * bn / tot);
      n = tot;
    }
  }
  if (lane == 0) {
    const double var = n > 0.0 ? M2 / n : 0.0;
    // sklearn's _is_constant_feature: var <= n eps var + (n mean eps)^2 -> scale 1
    const double eps = 2.220446049250313e-16;
    const double ub = n * eps * var + (n * mean * eps) * (n * mean * eps);
    gstat[g * 4 + 2] = mean;
    gstat[g * 4 + 3] = (n <= 0.0 || var <= ub) ? 1.0 : sqrt(var);
  }
}

__global__ void __launch_bounds__(256)
prosody_normalize_kernel(const double* __restrict__ track, const int64_t* __restrict__ trk_off,
                         const int32_t* __restrict__ status, const int32_t* __restrict__ status2,
                         const int64_t* __restrict__ group_off, int G, int D_max,
                         const double* __restrict__ gstat, float* __restrict__ z,
                         double* __restrict__ umm) {
  __shared__ double smn[4], smx[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  const long o0 = trk_off[b];
  const int D = (int)min<long>(max<long>(trk_off[b + 1] - o0, 0), D_max);
  if (flagged(status, status2, b)) {         // block-uniform
    for (int t = tid; t < D; t += 256) z[o0 + t] = 0.f;
    if (tid == 0) {
      umm[2 * b] = INFINITY;
      umm[2 * b + 1] = -INFINITY;
    }
    return;
  }
  // the group of utterance b: the last g with group_off[g] <= b (every thread, from L2)
  int g0 = 0, g1 = G - 1;
  while (g0 < g1) {
    const int m = (g0 + g1 + 1) >> 1;
    if (group_off[m] <= b) g0 = m;
    else g1 = m - 1;
  }
  const double mean = gstat[g0 * 4 + 2], sd = gstat[g0 * 4 + 3];
  double mn = INFINITY, mx = -INFINITY;
  for (int t = tid; t < D; t += 256) {
    const double zd = (track[o0 + t] - mean) / sd;
    z[o0 + t] = (float)zd;
    mn = fmin(mn, zd);
    mx = fmax(mx, zd);
  }
  mn = wave_min_d(mn);
  mx = wave_max_d(mx);
  if (lane == 0) {
    smn[wave] = mn;
    smx[wave] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    umm[2 * b] = fmin(fmin(smn[0], smn[1]), fmin(smn[2], smn[3]));
    umm[2 * b + 1] = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
  }
}

__global__ void __launch_bounds__(64)
prosody_minmax_kernel(const double* __restrict__ umm, const int32_t* __restrict__ status,
                      const int32_t* __restrict__ status2, const int64_t* __restrict__ group_off,
                      double* __restrict__ gstat) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const long u0 = group_off[g], u1 = group_off[g + 1];
  double mn = INFINITY, mx = -INFINITY;
  for (long u = u0 + lane; u < u1; u += 64)
    if (!flagged(status, status2, u)) {
      mn = fmin(mn, umm[2 * u]);
      mx = fmax(mx, umm[2 * u + 1]);
    }
  mn = wave_min_d(mn);
  mx = wave_max_d(mx);
  if (lane == 0) {
    gstat[g * 4] = mn;
    gstat[g * 4 + 1] = mx;
  }
}

}  // namespace

extern "C" int fs2_prosody_track(const void* src, int src_f64, const int64_t* src_start,
                                 const int64_t* src_len, const int64_t* dur,
                                 const int64_t* dur_off, const int64_t* trk_off, int B, int D_max,
                                 int interpolate, int average, double* track, double* ustat,
                                 int32_t* status, void* stream) {
  if (!src || !src_start || !src_len || !dur || !dur_off || !trk_off || !track || !ustat ||
      !status || B < 0 || D_max < 1 || D_max > PR_MAX_D)
    return FS2_EINVAL;
  if (B == 0) return 0;
  int n2 = 1;
  while (n2 < D_max) n2 <<= 1;
  hipLaunchKernelGGL(prosody_track_kernel, dim3(B), dim3(256), sizeof(double) * n2,
                     (hipStream_t)stream, src, src_f64, src_start, src_len, dur, dur_off, trk_off,
                     D_max, interpolate, average, track, ustat, status);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_prosody_stats(const double* ustat, const int32_t* status,
                                 const int32_t* status2, const int64_t* group_off, int G,
                                 double* gstat, void* stream) {
  if (!ustat || !status || !group_off || !gstat || G < 0) return FS2_EINVAL;
  if (G == 0) return 0;
  hipLaunchKernelGGL(prosody_stats_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, ustat,
                     status, status2, group_off, gstat);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_prosody_normalize(const double* track, const int64_t* trk_off,
                                     const int32_t* status, const int32_t* status2,
                                     const int64_t* group_off, int B, int G, int D_max,
                                     const double* gstat, float* z, double* umm, void* stream) {
  if (!track || !trk_off || !status || !group_off || !gstat || !z || !umm || B < 0 || G < 0 ||
      D_max < 1 || D_max > PR_MAX_D || (B > 0 && G < 1))
    return FS2_EINVAL;
  if (B == 0) return 0;
  hipLaunchKernelGGL(prosody_normalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, track,
                     trk_off, status, status2, group_off, G, D_max, gstat, z, umm);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_prosody_minmax(const double* umm, const int32_t* status,
                                  const int32_t* status2, const int64_t* group_off, int G,
                                  double* gstat, void* stream) {
  if (!umm || !status || !group_off || !gstat || G < 0) return FS2_EINVAL;
  if (G == 0) return 0;
  hipLaunchKernelGGL(prosody_minmax_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, umm,
                     status, status2, group_off, gstat);
  FS2_CHECK_LAUNCH();
  return 0;
}
