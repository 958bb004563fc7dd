// Batch collate on the GPU: TextMelCollateWithAlignment
// (fastspeech2/dataset.py:62-133) as two scatter kernels over one packed upload.
//
// The host concatenates the B utterances of a batch (the dataset's per-item arrays, in the
// order they arrive) into packed buffers and uploads them once; `order[i]` is the item placed
// at batch row i (descending phoneme length, the collate's torch.sort), so the kernels write
// the padded, sorted tensors directly:
//   collate_phon_kernel   phoneme_padded, duration_padded (B, Tp) int64, zero padded
//   collate_frames_kernel per 64-frame tile of one row: the packed mel (80, T_u) channel-major
//                         tile goes through LDS so that both outputs are written coalesced:
//                         mel_padded (B, Tm, n_mels) (the collate's permute(0, 2, 1), here
//                         contiguous), pitch / energy (B, Tm), and
//                         rank_X (B, n_mels + 2, Tm) = cat(mel, pitch, energy) (:94,116-117)
// HBM-bound byte movement: 4 B x (2 n_mels + 4) per valid frame + the zero padding.
//
// The rank model's pair collate (rank_model/dataset.py:71-115) over a device-resident store:
//   rank_collate_kernel   per 64-frame tile of one row of one output: the (C, T_u) channel-major
//                         item is read along t, transposed in LDS, and the tile's contiguous
//                         frames x C span of emo_X / neu_X (B, T, C) is written along c; frames
//                         past min(emo_len, neu_len) are zeros.  One launch for both outputs.
//
// The FastSpeech2 collate over a device-resident store (fastspeech2/device_store.py):
//   store_collate_kernel  one launch for the whole 12-tuple.  Row b of grid.y; grid.x holds the
//                         row's 64-frame tiles (collate_frames_kernel's LDS transpose, reading
//                         the utterance's (n_mels + 2, T_u) block at its own base), then its
//                         256-phoneme chunks (phoneme / duration padding), then, with a cache,
//                         the 256-float chunks of its cached (n_phon, E) intensity block.
#include "fs2_launch.h"

namespace {

__global__ void collate_phon_kernel(const int32_t* order, const int64_t* off,
                                    const int64_t* phon, const int64_t* dur, int B, int Tp,
                                    int64_t* phon_out, int64_t* dur_out, int64_t* in_len) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * Tp) return;
  const int b = (int)(i / Tp), p = (int)(i - (long)b * Tp);
  const int u = order[b];
  const long o0 = off[u], n = off[u + 1] - o0;
  const bool in = p < n;
  phon_out[i] = in ? phon[o0 + p] : 0;
  dur_out[i] = in ? dur[o0 + p] : 0;
  if (p == 0) in_len[b] = n;
}

constexpr int CT = 64;   // frames per tile

__global__ void __launch_bounds__(256) collate_frames_kernel(
    const int32_t* order, const int64_t* foff, const float* mel, const float* pitch,
    const float* energy, int B, int Tm, int NM, float* mel_out, float* pitch_out,
    float* energy_out, float* rank_out, int64_t* out_len) {
  __shared__ float tile[CT][129];   // [frame][channel], NM <= 128
  const int b = blockIdx.y, t0 = blockIdx.x * CT;
  const int u = order[b];
  const long f0 = foff[u];
  const int T = (int)(foff[u + 1] - f0);
  const float* mu = mel + f0 * NM;   // utterance u: (NM, T) channel-major
  const int NC = NM + 2;
  // rank_X rows: channel c, frames t0..t0+63 (coalesced along t); mel rows staged in LDS
  for (int i = threadIdx.x; i < NC * CT; i += blockDim.x) {
    const int c = i / CT, tl = i - c * CT, t = t0 + tl;
    if (t >= Tm) continue;
    float v = 0.f;
    if (t < T) v = c < NM ? mu[(long)c * T + t] : (c == NM ? pitch[f0 + t] : energy[f0 + t]);
    rank_out[((long)b * NC + c) * Tm + t] = v;
    if (c < NM) tile[tl][c] = v;
    else if (c == NM) pitch_out[(long)b * Tm + t] = v;
    else energy_out[(long)b * Tm + t] = v;
  }
  __syncthreads();
  // mel_padded rows: frame t, channels 0..NM-1 (coalesced along c)
  for (int i = threadIdx.x; i < CT * NM; i += blockDim.x) {
    const int tl = i / NM, c = i - tl * NM, t = t0 + tl;
    if (t < Tm) mel_out[((long)b * Tm + t) * NM + c] = tile[tl][c];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_len[b] = T;
}

constexpr int RC_MAX = 130;   // n_mels + 2, n_mels <= 128

// grid (tiles of T, B, 2): z = 0 the emotional item -> emo_X, z = 1 the neutral one -> neu_X.
// Item bases and pitches are arbitrary (4-byte alignment only), so loads and stores are dwords;
// a wave reads 64 consecutive frames of one channel and writes 64 consecutive floats of the span.
__global__ void __launch_bounds__(256) rank_collate_kernel(
    const float* store, const int64_t* emo_off, const int64_t* emo_len, const int64_t* neu_off,
    const int64_t* neu_len, int T, int C, float* emo_X, float* neu_X, int64_t* length) {
  __shared__ float tile[CT][RC_MAX + 1];   // [frame][channel]; odd pitch: conflict-free columns
  const int b = blockIdx.y, t0 = blockIdx.x * CT, neu = blockIdx.z;
  const long le = emo_len[b] > 0 ? emo_len[b] : 0, ln = neu_len[b] > 0 ? neu_len[b] : 0;
  const long L = min(min(le, ln), (long)T);                 // dataset.py:93 (and the clamp to T)
  const long pitch = neu ? ln : le;
  const float* src = store + (neu ? neu_off[b] : emo_off[b]);
  float* dst = (neu ? neu_X : emo_X) + ((long)b * T + t0) * C;
  const int nf = min(CT, T - t0);                            // frames of this tile
  const int nv = (int)max(0L, min((long)nf, L - t0));        // ... of which valid
  for (int i = threadIdx.x; i < C * CT; i += blockDim.x) {
    const int c = i / CT, tl = i - c * CT;
    if (tl < nv) tile[tl][c] = src[(long)c * pitch + t0 + tl];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nf * C; i += blockDim.x) {
    const int tl = i / C, c = i - tl * C;
    dst[i] = tl < nv ? tile[tl][c] : 0.f;
  }
  if (blockIdx.x == 0 && neu == 0 && threadIdx.x == 0) length[b] = L;
}

// desc: the batch's descriptors, (7, B) row-major int64: float offset, frames, int offset,
// phonemes, speaker, emotion, cache offset (speaker and emotion are not read here).  An
// utterance's floats are its (NM + 2, T_u) channel-major block = cat(mel, pitch, energy); its
// ints are n_phon phoneme ids, then n_phon durations.  Bases are 4-byte aligned only: dword loads.
// grid (nft + npt + nct, B): block-uniform dispatch on blockIdx.x.
__global__ void __launch_bounds__(256) store_collate_kernel(
    const float* fstore, const int64_t* istore, const int64_t* desc, const float* cache, int B,
    int Tp, int Tm, int NM, int E, int nft, int npt, int64_t* phon_out, int64_t* dur_out,
    int64_t* in_len, float* mel_out, float* pitch_out, float* energy_out, float* rank_out,
    int64_t* out_len, float* inten_out) {
  __shared__ float tile[CT][129];   // [frame][channel], NM <= 128
  const int b = blockIdx.y;
  const long n = desc[3L * B + b];
  if ((int)blockIdx.x >= nft + npt) {          // cached intensity rows: (n_phon, E), zeros past
    const long j = (long)((int)blockIdx.x - nft - npt) * blockDim.x + threadIdx.x;
    if (j >= (long)Tp * E) return;
    const long co = desc[6L * B + b];
    inten_out[(long)b * Tp * E + j] = (co >= 0 && j < n * E) ? cache[co + j] : 0.f;
    return;
  }
  if ((int)blockIdx.x >= nft) {                // phonemes and durations, zero padded
    const long p = (long)((int)blockIdx.x - nft) * blockDim.x + threadIdx.x;
    if (p == 0) in_len[b] = n;
    if (p >= Tp) return;
    const int64_t* iu = istore + desc[2L * B + b];
    const bool in = p < n;
    phon_out[(long)b * Tp + p] = in ? iu[p] : 0;
    dur_out[(long)b * Tp + p] = in ? iu[n + p] : 0;
    return;
  }
  const int t0 = blockIdx.x * CT;
  const long T = desc[1L * B + b];
  const float* su = fstore + desc[b];
  const int NC = NM + 2;
  // rank_X rows: channel c, frames t0..t0+63 (coalesced along t); mel rows staged in LDS
  for (int i = threadIdx.x; i < NC * CT; i += blockDim.x) {
    const int c = i / CT, tl = i - c * CT, t = t0 + tl;
    if (t >= Tm) continue;
    const float v = t < T ? su[(long)c * T + t] : 0.f;
    rank_out[((long)b * NC + c) * Tm + t] = v;
    if (c < NM) tile[tl][c] = v;
    else if (c == NM) pitch_out[(long)b * Tm + t] = v;
    else energy_out[(long)b * Tm + t] = v;
  }
  __syncthreads();
  // mel_padded rows: frame t, channels 0..NM-1 (coalesced along c)
  for (int i = threadIdx.x; i < CT * NM; i += blockDim.x) {
    const int tl = i / NM, c = i - tl * NM, t = t0 + tl;
    if (t < Tm) mel_out[((long)b * Tm + t) * NM + c] = tile[tl][c];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_len[b] = T;
}

}  // namespace

extern "C" int fs2_collate_phonemes(const int32_t* order, const int64_t* offsets,
                                    const int64_t* phonemes, const int64_t* durations, int B,
                                    int Tp, int64_t* phoneme_padded, int64_t* duration_padded,
                                    int64_t* input_lengths, void* stream) {
  if ((long)B * Tp == 0) return 0;
  if (!order || !offsets || !phonemes || !durations || !phoneme_padded || !duration_padded ||
      !input_lengths)
    return FS2_EINVAL;
  hipLaunchKernelGGL(collate_phon_kernel, dim3(nblk((long)B * Tp)), dim3(256), 0,
                     (hipStream_t)stream, order, offsets, phonemes, durations, B, Tp,
                     phoneme_padded, duration_padded, input_lengths);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_collate_frames(const int32_t* order, const int64_t* frame_offsets,
                                  const float* mel, const float* pitch, const float* energy,
                                  int B, int Tm, int n_mels, float* mel_padded,
                                  float* pitch_padded, float* energy_padded, float* rank_x,
                                  int64_t* output_lengths, void* stream) {
  if ((long)B * Tm == 0) return 0;
  if (!order || !frame_offsets || !mel || !pitch || !energy || !mel_padded || !pitch_padded ||
      !energy_padded || !rank_x || !output_lengths || n_mels < 1 || n_mels > 128)
    return FS2_EINVAL;
  hipLaunchKernelGGL(collate_frames_kernel, dim3((Tm + CT - 1) / CT, B), dim3(256), 0,
                     (hipStream_t)stream, order, frame_offsets, mel, pitch, energy, B, Tm,
                     n_mels, mel_padded, pitch_padded, energy_padded, rank_x, output_lengths);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_rank_collate(const float* store, const int64_t* emo_off,
                                const int64_t* emo_len, const int64_t* neu_off,
                                const int64_t* neu_len, int B, int T, int C, float* emo_X,
                                float* neu_X, int64_t* length, void* stream) {
  if (B < 0 || T < 0) return FS2_EINVAL;
  if ((long)B * T == 0) return 0;
  if (!store || !emo_off || !emo_len || !neu_off || !neu_len || !emo_X || !neu_X || !length ||
      C < 3 || C > RC_MAX || B > 65535)
    return FS2_EINVAL;
  hipLaunchKernelGGL(rank_collate_kernel, dim3((T + CT - 1) / CT, B, 2), dim3(256), 0,
                     (hipStream_t)stream, store, emo_off, emo_len, neu_off, neu_len, T, C, emo_X,
                     neu_X, length);
  FS2_CHECK_LAUNCH();
  return 0;
}

extern "C" int fs2_store_collate(const float* fstore, const int64_t* istore, const int64_t* desc,
                                 const float* cache, int B, int Tp, int Tm, int n_mels, int E,
                                 int64_t* phoneme_padded, int64_t* duration_padded,
                                 int64_t* input_lengths, float* mel_padded, float* pitch_padded,
                                 float* energy_padded, float* rank_x, int64_t* output_lengths,
                                 float* intensity, void* stream) {
  if (B < 0 || Tp < 0 || Tm < 0) return FS2_EINVAL;
  if ((long)B * Tm == 0) return 0;
  if (!fstore || !istore || !desc || !phoneme_padded || !duration_padded || !input_lengths ||
      !mel_padded || !pitch_padded || !energy_padded || !rank_x || !output_lengths ||
      n_mels < 1 || n_mels > 128 || B > 65535)
    return FS2_EINVAL;
  if (cache && (!intensity || E < 1)) return FS2_EINVAL;
  const int nft = (Tm + CT - 1) / CT;
  const int npt = Tp > 0 ? (Tp + 255) / 256 : 1;      // p == 0 writes input_lengths
  const long nct = cache ? ((long)Tp * E + 255) / 256 : 0;
  if (nft + npt + nct > 0x7fffffffL) return FS2_EINVAL;
  hipLaunchKernelGGL(store_collate_kernel, dim3((unsigned)(nft + npt + nct), B), dim3(256), 0,
                     (hipStream_t)stream, fstore, istore, desc, cache, B, Tp, Tm, n_mels, E, nft,
                     npt, phoneme_padded, duration_padded, input_lengths, mel_padded,
                     pitch_padded, energy_padded, rank_x, output_lengths, intensity);
  FS2_CHECK_LAUNCH();
  return 0;
}
