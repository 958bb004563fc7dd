// Log-mel front end: waveform -> mel spectrogram and energy, batched over utterances of
// different lengths (fastspeech2/audio.py).
//
//   rank_model/audio_util.py:23-40   get_mel -> speechbrain mel_spectogram(power=1,
//                                    normalized=False, min_max_energy_norm=True, slaney,
//                                    compression=True)
//
//   melspec_kernel        a workgroup takes MEL_F = 8 consecutive frames of one utterance, four
//                         at a time.  The four frames' overlapping samples are read once into
//                         LDS, the reflection applied to the index (clamped into the utterance,
//                         so that no length can make it read outside its own samples).  Two real
//                         frames are packed into one complex n_fft-point transform (z = u0 + i u1),
//                         a radix-2 Stockham FFT between two LDS buffers (natural order in and
//                         out, twiddles from an LDS copy of the host's table), separated into
//                         the two spectra's magnitudes; one wave per frame then forms the band
//                         sums of the mel filters, the frame's energy as a wave reduction, and
//                         the log.  The eight frames' results are staged in LDS and stored
//                         coalesced in either layout.
//   energy_minmax_kernel  (e - min) / (max - min) over an utterance's own frames
//
// No device transcendental but the final log (evaluated in double and rounded once): window,
// twiddles and filter weights are the host's float64 tables rounded once to fp32.  LDS per
// workgroup: 32 * n_fft bytes for the two FFT buffers (the samples live in the second one until
// the first stage overwrites it), 4 * n_fft for the twiddles, the stage.
#include "fs2_launch.h"

namespace {

constexpr int MEL_F = 8;         // frames per workgroup (fastspeech2/ops.py MELSPEC_FRAMES)
constexpr int MEL_R = 4;         // frames per round: two complex transforms
constexpr int MEL_MAX_MELS = 256;

struct MelBands {                // by value in the kernel arguments (2 KiB)
  short start[MEL_MAX_MELS];     // first bin of the filter
  short len[MEL_MAX_MELS];       // its bins
  int off[MEL_MAX_MELS];         // its first weight in the packed weights
};

__global__ void __launch_bounds__(256)
melspec_kernel(const float* __restrict__ wav, const int64_t* __restrict__ offsets,
               const float* __restrict__ window, const float2* __restrict__ twiddle,
               const float* __restrict__ band_w, const MelBands bands, int N, int logN, int hop,
               int n_mels, int T_max, int bct, int compression, float* __restrict__ mel,
               float* __restrict__ energy, int64_t* __restrict__ mel_len) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * MEL_F;
  const long w0 = offsets[b];
  const long L = max<long>(offsets[b + 1] - w0, 0);
  const long Tl = 1 + L / hop;
  const int Tb = (int)min<long>(Tl, T_max);
  if (blockIdx.x == 0 && tid == 0) mel_len[b] = Tl;
  const int rows = min(MEL_F, T_max - t0);
  const int pitch = n_mels | 1;  // odd stage pitch: the transposed read of the bct store

  float2* buf0 = (float2*)lds;                 // [2][N]
  float2* buf1 = buf0 + 2 * N;                 // [2][N]; first the samples of the round
  float2* tw = buf1 + 2 * N;                   // [N / 2]
  float* stage = (float*)(tw + N / 2);         // [MEL_F][pitch]
  float* stage_e = stage + MEL_F * pitch;      // [MEL_F]

  if (t0 < Tb) {
    for (int j = tid; j < N / 2; j += 256) tw[j] = twiddle[j];
    const int hs = min(hop, N);                // frame pitch in the sample buffer
    const int nsmp = (MEL_R - 1) * hs + N;     // <= 4 N floats = buf1
    float* smp = (float*)buf1;
    for (int r = 0; r < MEL_F / MEL_R; ++r) {
      const int tr = t0 + r * MEL_R;           // first frame of the round
      if (tr >= Tb) {                          // block-uniform: the round is all padding
        for (int i = tid; i < MEL_R * pitch; i += 256) stage[r * MEL_R * pitch + i] = 0.f;
        if (tid < MEL_R) stage_e[r * MEL_R + tid] = 0.f;
        continue;
      }
      __syncthreads();                         // the previous round's reads of buf0 / buf1
      // samples of the round's frames; frame f starts at smp[f * hs]
      const long s0 = (long)tr * hop - N / 2;
      for (int j = tid; j < nsmp; j += 256) {
        long i = s0 + j;
        if (hop > N) {                         // frames do not overlap: packed back to back
          const int f = min(j / N, MEL_R - 1);
          i = s0 + (long)f * hop + (j - f * N);
        }
        if (i < 0) i = -i;
        if (i >= L) i = 2 * (L - 1) - i;
        i = min<long>(max<long>(i, 0), L - 1);
        smp[j] = L > 0 ? wav[w0 + i] : 0.f;
      }
      __syncthreads();
      // z = u0 + i u1 of the frame pairs, windowed; a frame past the utterance is zeros
      for (int i = tid; i < 2 * N; i += 256) {
        const int p = i >> logN, n = i & (N - 1);
        const float w = window[n];
        float2 z;
        z.x = tr + 2 * p < Tb ? smp[(2 * p) * hs + n] * w : 0.f;
        z.y = tr + 2 * p + 1 < Tb ? smp[(2 * p + 1) * hs + n] * w : 0.f;
        buf0[i] = z;
      }
      __syncthreads();
      // radix-2 Stockham: stage s reads (t, t + N/2), writes (j, j + p), j = 2t - (t mod p)
      for (int s = 0; s < logN; ++s) {
        const float2* in = (s & 1) ? buf1 : buf0;
        float2* out = (s & 1) ? buf0 : buf1;
        const int p = 1 << s;
        for (int i = tid; i < N; i += 256) {
          const int pr = i >> (logN - 1), t = i & (N / 2 - 1);
          const int k = t & (p - 1);
          const float2 u0 = in[pr * N + t], u1 = in[pr * N + t + N / 2];
          const float2 w = tw[k << (logN - 1 - s)];          // e^{-i pi k / p} = (w.x, -w.y)
          const float vr = u1.x * w.x + u1.y * w.y, vi = u1.y * w.x - u1.x * w.y;
          const int j = pr * N + 2 * t - k;
          out[j] = make_float2(u0.x + vr, u0.y + vi);
          out[j + p] = make_float2(u0.x - vr, u0.y - vi);
        }
        __syncthreads();
      }
      // |X0[k]|, |X1[k]| from Z[k] and Z[N - k]; magnitudes into the other buffer
      const float2* Z = (logN & 1) ? buf1 : buf0;
      float* mag = (float*)((logN & 1) ? buf0 : buf1);       // [2 pairs][2][N / 2 + 1] <= 4 N
      const int nf = N / 2 + 1;
      for (int i = tid; i < 2 * nf; i += 256) {
        const int pr = i / nf, k = i - pr * nf;
        const float2 a = Z[pr * N + k], c = Z[pr * N + ((N - k) & (N - 1))];
        const float xr = 0.5f * (a.x + c.x), xi = 0.5f * (a.y - c.y);
        const float yr = 0.5f * (a.y + c.y), yi = 0.5f * (a.x - c.x);
        mag[(2 * pr) * nf + k] = sqrtf(xr * xr + xi * xi);
        mag[(2 * pr + 1) * nf + k] = sqrtf(yr * yr + yi * yi);
      }
      __syncthreads();
      // wave f: frame tr + f.  Band sums, energy, log
      {
        const int f = wave, t = tr + f;
        const float* mg = mag + f * nf;
        float sq = 0.f;
        for (int m = lane; m < n_mels; m += 64) {
          const int st = bands.start[m], ln = bands.len[m];
          const float* bw = band_w + bands.off[m];
          float acc = 0.f;
          for (int i = 0; i < ln; ++i) acc += bw[i] * mg[st + i];
          sq += acc * acc;
          float v = acc;
          // the log in double, rounded once: the fp32 log adds no error beyond its last bit
          if (compression) v = (float)log((double)(v < 1e-5f ? 1e-5f : v));
          stage[(r * MEL_R + f) * pitch + m] = t < Tb ? v : 0.f;
        }
        sq = wave_sum(sq);
        if (lane == 0) stage_e[r * MEL_R + f] = t < Tb ? sqrtf(sq) : 0.f;
      }
    }
    __syncthreads();
  }
  // stores: rows t0 .. t0 + rows - 1 (< T_max); a block past the utterance writes zeros
  const bool live = t0 < Tb;
  if (!bct) {      // (B, T_max, n_mels): the block's rows are one contiguous run
    float* o = mel + ((long)b * T_max + t0) * n_mels;
    for (int i = tid; i < rows * n_mels; i += 256) {
      const int f = i / n_mels, m = i - f * n_mels;
      o[i] = live ? stage[f * pitch + m] : 0.f;
    }
  } else {         // (B, n_mels, T_max): runs of `rows` frames along t
    float* o = mel + (long)b * n_mels * T_max + t0;
    for (int i = tid; i < MEL_F * n_mels; i += 256) {
      const int m = i / MEL_F, f = i - m * MEL_F;
      if (f < rows) o[(long)m * T_max + f] = live ? stage[f * pitch + m] : 0.f;
    }
  }
  if (tid < rows) energy[(long)b * T_max + t0 + tid] = live ? stage_e[tid] : 0.f;
}

// one workgroup per utterance; in place or out of place
__global__ void __launch_bounds__(256)
energy_minmax_kernel(const float* e, const int64_t* mel_len, int T_max, float* out) {
  __shared__ float smn[4], smx[4], sbad[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = (int)min<int64_t>(max<int64_t>(mel_len[b], 0), T_max);
  const float* eb = e + (long)b * T_max;
  float mn = INFINITY, mx = -INFINITY, bad = 0.f;
  for (int t = tid; t < Tb; t += 256) {
    const float v = eb[t];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    if (v != v) bad = 1.f;       // torch's min / max return NaN when there is one
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  bad = wave_max(bad);
  if (lane == 0) { smn[wave] = mn; smx[wave] = mx; sbad[wave] = bad; }
  __syncthreads();               // also: every read of e above precedes the in-place writes
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  if (sbad[0] + sbad[1] + sbad[2] + sbad[3] > 0.f) mn = mx = __builtin_nanf("");
  const float d = mx - mn;
  float* ob = out + (long)b * T_max;
  for (int t = tid; t < T_max; t += 256) ob[t] = t < Tb ? (eb[t] - mn) / d : 0.f;
}

}  // namespace

extern "C" int fs2_melspec(const float* wav, const int64_t* offsets, int B, const float* window,
                           const float* twiddle, const int32_t* bands, const float* band_w,
                           int n_fft, int win_length, int hop, int n_mels, int T_max,
                           int layout_bct, int compression, float* mel, float* energy,
                           int64_t* mel_len, void* stream) {
  if (n_fft < 64 || n_fft > 2048 || (n_fft & (n_fft - 1)) || win_length < 1 ||
      win_length > n_fft || hop < 1 || n_mels < 1 || n_mels > MEL_MAX_MELS || T_max < 1 ||
      B < 0 || B > 65535)
    return FS2_EINVAL;
  if (!wav || !offsets || !window || !twiddle || !bands || !band_w || !mel || !energy ||
      !mel_len)
    return FS2_EINVAL;
  MelBands mb;
  int off = 0;
  for (int m = 0; m < MEL_MAX_MELS; ++m) {
    const int st = m < n_mels ? bands[2 * m] : 0, ln = m < n_mels ? bands[2 * m + 1] : 0;
    if (st < 0 || ln < 0 || st > n_fft / 2 + 1 || ln > n_fft / 2 + 1 - st) return FS2_EINVAL;
    mb.start[m] = (short)st;
    mb.len[m] = (short)ln;
    mb.off[m] = off;
    off += ln;
  }
  if (B == 0) return 0;
  int logN = 0;
  while ((1 << logN) < n_fft) ++logN;
  const int pitch = n_mels | 1;
  const size_t shmem = (size_t)36 * n_fft + sizeof(float) * (MEL_F * pitch + MEL_F);
  if (shmem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)melspec_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 g((unsigned)((T_max + MEL_F - 1) / MEL_F), (unsigned)B);
  hipLaunchKernelGGL(melspec_kernel, g, dim3(256), shmem, (hipStream_t)stream, wav, offsets,
                     window, (const float2*)twiddle, band_w, mb, n_fft, logN, hop, n_mels, T_max,
                     layout_bct, compression, mel, energy, mel_len);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_energy_minmax(const float* energy, const int64_t* mel_len, int B, int T_max,
                                 float* out, void* stream) {
  if (!energy || !mel_len || !out || T_max < 1 || B < 0) return FS2_EINVAL;
  if (B == 0) return 0;
  hipLaunchKernelGGL(energy_minmax_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, energy,
                     mel_len, T_max, out);
  FS2_CHECK_LAUNCH();
  return 0;
}
