"""Log-mel front end on the GPU: waveform -> mel spectrogram and energy, batched.

Reference: ``emo_rank_tts/rank_model/audio_util.py::get_mel`` (:23-40), i.e. speechbrain's
``mel_spectogram(power=1, normalized=False, min_max_energy_norm=True, norm="slaney",
mel_scale="slaney", compression=True)`` on one 1-D fp32 waveform.  speechbrain and torchaudio are
not needed; what they compute is restated here:

1. torchaudio ``Spectrogram``: ``torch.stft(y, n_fft, hop, win, hann_window(win) (periodic),
   center=True, pad_mode="reflect", onesided)`` then ``abs()``; ``T = 1 + L // hop``; a window
   shorter than ``n_fft`` is zero-padded centred, ``(n_fft - win) // 2`` zeros on the left;
2. torchaudio ``melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate, "slaney",
   "slaney")`` and ``mel = fb^T |X|``;
3. ``energy = ||mel[:, t]||_2`` before compression, then ``(e - min e) / (max e - min e)`` over
   the utterance's own frames (NaN for one frame or constant energy: the reference's value);
4. ``mel = log(clamp(mel, min=1e-5))``.

All tables (window, twiddles, filterbank) are built here in float64 and rounded once to fp32;
the kernels (csrc/audio.hip: ``fs2_melspec``, ``fs2_energy_minmax``) use no transcendental but
the final ``log``.  A batch is one upload and two launches, whatever the utterance lengths.

What follows it -- the cut to the alignment, pitch interpolation, phoneme averaging, the
outlier-free statistics and the standardised items -- is fastspeech2/prosody.py.  Out of scope
(they stay offline CPU preprocessing): MFA alignment, pyworld pitch, librosa loading /
resampling, G2P.
"""

import math

import numpy as np
import torch

from . import ops

_LOG_STEP = math.log(6.4) / 27.0        # slaney: 27 log-spaced steps per factor 6.4 above 1 kHz
_F_SP = 200.0 / 3.0                     # slaney: linear below 1 kHz, 200/3 Hz per mel
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = 15.0                    # = 1000 / (200 / 3)


def hz_to_mel(f):
    """slaney scale (torchaudio ``_hz_to_mel(mel_scale="slaney")``), float64"""
    f = float(f)
    if f >= _MIN_LOG_HZ:
        return _MIN_LOG_MEL + math.log(f / _MIN_LOG_HZ) / _LOG_STEP
    return f / _F_SP


def mel_to_hz(m):
    """inverse of ``hz_to_mel`` on a float64 array"""
    m = np.asarray(m, np.float64)
    lin = m * _F_SP
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOG_STEP * (m - _MIN_LOG_MEL)), lin)


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate):
    """(n_freqs, n_mels) float64 slaney filterbank with slaney area normalisation."""
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs)
    m_pts = np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2)
    f_pts = mel_to_hz(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]                 # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    return fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]


def stft_window(win_length, n_fft):
    """periodic hann window of ``win_length``, zero-padded centred to ``n_fft``; float64"""
    if win_length > n_fft or win_length < 1:
        raise ValueError(f"win_length {win_length} must be in [1, n_fft = {n_fft}]")
    w = np.zeros(n_fft, np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return w


def twiddles(n_fft):
    """(n_fft // 2, 2) float64: cos and sin of 2 pi j / n_fft for j < n_fft / 2"""
    a = 2.0 * np.pi * np.arange(n_fft // 2) / n_fft
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def band_tables(fb):
    """The filterbank as the kernel reads it: ``bands`` (n_mels, 2) int32 of (first bin, bins)
    per filter -- the hull of its non-zero bins, (0, 0) for an empty filter -- and the hull's
    weights of all filters back to back, float64."""
    bands = np.zeros((fb.shape[1], 2), np.int32)
    packed = []
    for m in range(fb.shape[1]):
        nz = np.flatnonzero(fb[:, m])
        if nz.size:
            bands[m] = (nz[0], nz[-1] - nz[0] + 1)
            packed.append(fb[nz[0]:nz[-1] + 1, m])
    return bands, (np.concatenate(packed) if packed else np.zeros(0, np.float64))


def n_frames(n_samples, hop_length):
    return 1 + n_samples // hop_length


class MelFrontEnd:
    """``MelFrontEnd(**config['audio'], device=...)``: the reference yaml's ``audio:`` keys.
    Holds the device tables; a call runs one upload, one fs2_melspec and one fs2_energy_minmax
    launch for the whole batch."""

    def __init__(self, sampling_rate, hop_length, win_length, n_fft, n_mels, f_min, f_max,
                 device="cuda"):
        if n_fft < 64 or n_fft > 2048 or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft {n_fft} must be a power of two in [64, 2048]")
        if hop_length < 1 or n_mels < 1 or n_mels > 256:
            raise ValueError(f"hop_length {hop_length} must be >= 1 and n_mels {n_mels} in [1, 256]")
        self.sampling_rate, self.hop_length, self.win_length = sampling_rate, hop_length, win_length
        self.n_fft, self.n_mels, self.f_min, self.f_max = n_fft, n_mels, f_min, f_max
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        fb = mel_filterbank(n_fft // 2 + 1, f_min, f_max, n_mels, sampling_rate)
        self.bands, w = band_tables(fb)                          # bands stay on the host
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        self.window = f32(stft_window(win_length, n_fft))
        self.twiddle = f32(twiddles(n_fft))
        self.band_w = f32(w if w.size else np.zeros(1))

    def _pack(self, wavs, lengths):
        """the batch as one packed fp32 buffer + int64 offsets on the device (one upload)"""
        if torch.is_tensor(wavs):
            if wavs.dim() != 2 or lengths is None:
                raise ValueError("a tensor batch is (B, L) with lengths")
            wavs = [wavs[i, :int(n)] for i, n in enumerate(torch.as_tensor(lengths).tolist())]
        elif lengths is not None:
            raise ValueError("lengths go with a (B, L) tensor, not with a list")
        wavs = [w.reshape(-1) for w in wavs]
        lens = [int(w.numel()) for w in wavs]
        for n in lens:
            if n <= self.n_fft // 2:          # torch.stft: reflect padding needs pad < length
                raise ValueError(f"waveform of {n} samples: reflect padding of n_fft / 2 = "
                                 f"{self.n_fft // 2} needs more samples than that")
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        if all(w.device == self.device for w in wavs):
            packed = torch.cat([w.float() for w in wavs])
            return packed, torch.from_numpy(off).to(self.device), lens
        nb = off.nbytes
        host = torch.empty(nb + 4 * int(off[-1]), dtype=torch.uint8)
        host[:nb] = torch.from_numpy(off).view(torch.uint8)
        torch.cat([w.detach().cpu().float() for w in wavs], out=host[nb:].view(torch.float32))
        dev = host.to(self.device)
        return dev[nb:].view(torch.float32), dev[:nb].view(torch.int64), lens

    @torch.no_grad()
    def __call__(self, wavs, lengths=None, layout="btc", compression=True,
                 min_max_energy_norm=True, *, power=1, normalized=False):
        """wavs: list of 1-D waveforms of any lengths, or (B, L) with ``lengths``.  Returns
        (mel, energy, mel_len): mel (B, T_max, n_mels) for "btc" or (B, n_mels, T_max) for "bct",
        energy (B, T_max), both zero past mel_len[b] = 1 + L_b // hop; mel_len int64 (B)."""
        if power != 1 or normalized:
            raise NotImplementedError("only power=1, normalized=False, what the reference's "
                                      "rank_model/audio_util.py:35-36 passes")
        if layout not in ("btc", "bct"):
            raise ValueError(f"layout {layout!r} is not 'btc' or 'bct'")
        packed, offsets, lens = self._pack(wavs, lengths)
        B = len(lens)
        T = max(n_frames(n, self.hop_length) for n in lens)
        shape = (B, T, self.n_mels) if layout == "btc" else (B, self.n_mels, T)
        mel = torch.empty(shape, dtype=torch.float32, device=self.device)
        energy = torch.empty(B, T, dtype=torch.float32, device=self.device)
        mel_len = torch.empty(B, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            ops.melspec(packed, offsets, B, self.window, self.twiddle, self.bands, self.band_w,
                        self.n_fft, self.win_length, self.hop_length, self.n_mels, T,
                        layout == "bct", compression, mel, energy, mel_len)
            if min_max_energy_norm:
                ops.energy_minmax(energy, mel_len, B, T, energy)
        return mel, energy, mel_len


_FRONT_ENDS = {}


def get_mel(y, sampling_rate, hop_length, win_length, n_mels, n_fft, f_min, f_max):
    """rank_model/audio_util.py:23-40 with its signature and return: (mel (n_mels, T), energy
    (T)) of one utterance, on the device ``y`` is on.  A CPU (or numpy) ``y`` is computed on the
    current GPU and returned on the CPU, so preprocess.py:115-116 (``.numpy()``) runs unchanged."""
    y = torch.as_tensor(y, dtype=torch.float32).reshape(-1)
    dev = y.device if y.is_cuda else torch.device("cuda", torch.cuda.current_device())
    key = (sampling_rate, hop_length, win_length, n_fft, n_mels, f_min, f_max, dev)
    fe = _FRONT_ENDS.get(key)
    if fe is None:
        fe = _FRONT_ENDS[key] = MelFrontEnd(sampling_rate, hop_length, win_length, n_fft, n_mels,
                                            f_min, f_max, device=dev)
    mel, energy, _ = fe([y], layout="bct")
    return mel[0].to(y.device), energy[0].to(y.device)
