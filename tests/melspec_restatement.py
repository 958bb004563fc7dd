"""The reference of the log-mel front end (rank_model/audio_util.py:23-40 get_mel, i.e. speechbrain
``mel_spectogram(power=1, normalized=False, min_max_energy_norm=True, norm="slaney",
mel_scale="slaney", compression=True)``), written with ``torch.stft`` and the formulas of
torchaudio's ``Spectrogram`` and ``melscale_fbanks``, in float64 or float32.  Nothing here
imports ``fastspeech2.audio``: the filterbank, the window and the framing are restated.

The error bound
---------------
With u_t the windowed frame t (n_fft samples), X = DFT(u_t) and mel[m, t] = sum_k fb[k, m] |X_k|:
an fp32 FFT of n_fft points has log2(n_fft) butterfly levels, each adding a relative error of
order eps32 to values whose size is at most sum_n |u_t[n]| <= sqrt(n_fft) ||u_t||_2, so

    | |X_k| - |X_k|_64 |  <=  K eps32 log2(n_fft) sqrt(n_fft) ||u_t||_2            for every bin k
    |mel[m, t] - mel64[m, t]|  <=  K eps32 log2(n_fft) sqrt(n_fft) ||u_t||_2 sum_k fb[k, m]

(the filter's own products and sums add at most (bins + 1) eps32 |mel|, far inside the same
expression).  K absorbs the constants of the butterflies, the magnitude and the band sum.  It is
not derived but measured against the reference: on every input of tests/test_melspec_host.py
and tests/test_gpu_melspec.py (CASES and RAGGED below) the FLOAT32 CPU restatement differs from
float64 by at most 0.130 of the K = 1 bound (n_fft 64, the 64-frame item; at most 0.062 at n_fft
1024, 0.037 at 2048; the raw energy uses at most 0.071 of its bound).  The smallest power of two
for which it stays inside is therefore K = 1/4 (0.52 used; 1/8 would be 1.04), doubled once
because a different, equally valid FFT factorisation orders its roundings differently from
torch's:

    K = 1/2

The raw energy e_t = ||mel[:, t]||_2 is bounded by the L2 norm of the frame's mel bounds plus
eps32 e_t.  For the log mel an element with mel64 >= 8 bound is held to bound / (mel64 - bound)
(|log a - log b| <= |a - b| / min(a, b)); smaller elements must be <= 9 bound on both sides.
"""
import math

import numpy as np
import torch

K = 0.5
EPS32 = 2.0 ** -24

REF_AUDIO = dict(sampling_rate=16000, hop_length=256, win_length=1024, n_fft=1024, n_mels=80,
                 f_min=0.0, f_max=8000.0)


def hz_to_mel(f):
    f = float(f)
    if f >= 1000.0:
        return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)
    return f / (200.0 / 3.0)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)),
                    m * (200.0 / 3.0))


def fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """torchaudio melscale_fbanks(norm="slaney", mel_scale="slaney"), float64 (n_freqs, n_mels)"""
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs)
    f_pts = mel_to_hz(np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))
    fb = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        up = (all_freqs - f_pts[m]) / (f_pts[m + 1] - f_pts[m])
        down = (f_pts[m + 2] - all_freqs) / (f_pts[m + 2] - f_pts[m + 1])
        fb[:, m] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (f_pts[m + 2] - f_pts[m]))
    return fb


def linear_mel(y, dtype, *, sampling_rate, hop_length, win_length, n_fft, n_mels, f_min, f_max):
    """(n_mels, T) linear mel and (T) raw energy of one waveform in ``dtype``"""
    y = torch.as_tensor(np.asarray(y)).to(dtype)
    win = torch.hann_window(win_length, periodic=True, dtype=dtype)
    X = torch.stft(y, n_fft, hop_length, win_length, win, center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True).abs()
    fb = torch.from_numpy(fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sampling_rate)).to(dtype)
    mel = torch.matmul(X.transpose(-1, -2), fb).transpose(-1, -2)
    return mel, torch.norm(mel, dim=0)


def minmax(e):
    """speechbrain's min_max_energy_norm on one utterance's frames, in e's dtype"""
    return (e - e.min()) / (e.max() - e.min())


def compress(mel):
    return torch.log(torch.clamp(mel, min=1e-5))


def get_mel(y, dtype, **audio):
    """the reference's return: (log mel (n_mels, T), normalised energy (T))"""
    mel, e = linear_mel(y, dtype, **audio)
    return compress(mel), minmax(e)


def frame_norms(y, *, hop_length, win_length, n_fft, **_):
    """||u_t||_2 of every windowed frame, float64 (T,)"""
    y = np.asarray(y, np.float64)
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    T = 1 + y.size // hop_length
    idx = np.arange(T)[:, None] * hop_length + np.arange(n_fft)[None, :]
    return np.sqrt(((yp[idx] * w[None, :]) ** 2).sum(1))


def mel_bound(y, k=K, **audio):
    """(n_mels, T) float64 bound of |mel - mel64| (the docstring's expression)"""
    n_fft = audio["n_fft"]
    fb = fbanks(n_fft // 2 + 1, audio["f_min"], audio["f_max"], audio["n_mels"],
                audio["sampling_rate"])
    un = frame_norms(y, **audio)
    return k * EPS32 * math.log2(n_fft) * math.sqrt(n_fft) * fb.sum(0)[:, None] * un[None, :]


def energy_bound(bound, e64):
    """(T,) bound of the raw energy given the mel bound (n_mels, T) and the float64 energy"""
    return np.sqrt((bound ** 2).sum(0)) + EPS32 * np.asarray(e64, np.float64)


def wave(seed, n, tone_hz=440.0, tone_amp=0.05, noise_amp=0.1, sample_rate=16000):
    """the tests' input: seeded uniform noise of amplitude ``noise_amp`` plus one tone, fp32"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sample_rate
    y = noise_amp * r.uniform(-1.0, 1.0, n) + tone_amp * np.sin(2 * np.pi * tone_hz * t)
    return y.astype(np.float32)


def check_linear(mel, e, y, audio, k=K):
    """asserts of the linear mel (n_mels, T) and raw energy (T) of a candidate against float64;
    returns (share of the bound used by the mel, by the energy)"""
    m64, e64 = linear_mel(y, torch.float64, **audio)
    m64, e64 = m64.numpy(), e64.numpy()
    bd = mel_bound(y, k, **audio)
    mel, e = np.asarray(mel, np.float64), np.asarray(e, np.float64)
    assert mel.shape == m64.shape and e.shape == e64.shape
    dm, de = np.abs(mel - m64), np.abs(e - e64)
    ebd = energy_bound(bd, e64)
    assert (dm <= bd).all(), f"mel outside the bound: worst share {np.max(dm / bd):.3f}"
    assert (de <= ebd).all(), f"energy outside its bound: worst share {np.max(de / ebd):.3f}"
    return float(np.max(dm / np.maximum(bd, 1e-300))), float(np.max(de / np.maximum(ebd, 1e-300)))


def check_log(logmel, y, audio, k=K):
    """asserts of the log mel (n_mels, T) of a candidate against float64; returns the share of
    elements that was too small to compare (each of those is checked to be small)"""
    m64, _ = linear_mel(y, torch.float64, **audio)
    m64 = m64.numpy()
    bd = mel_bound(y, k, **audio)
    got = np.asarray(logmel, np.float64)
    assert got.shape == m64.shape
    big = m64 >= 8 * bd
    ref = np.log(np.maximum(m64, 1e-5))
    # the clamp is monotone and 1-Lipschitz, so the tolerance of the unclamped logs holds with it
    tol = bd / np.where(big, m64 - bd, 1.0)
    ok = np.abs(got - ref) <= tol
    assert ok[big].all(), f"log mel: worst {np.max(np.abs(got - ref)[big] / tol[big]):.3f} of tol"
    small = ~big
    assert (m64[small] <= 9 * bd[small]).all()
    assert (np.exp(got[small]) <= np.maximum(9 * bd[small], 1e-5 * (1 + 1e-6))).all()
    share = float(small.mean())
    assert share <= 0.01, share
    return share


# ---- the inputs of tests/test_melspec_host.py and tests/test_gpu_melspec.py -----------------------
F = 8                                                  # frames per fs2_melspec workgroup
SMALL = dict(sampling_rate=16000, hop_length=16, win_length=64, n_fft=64, n_mels=8, f_min=0.0,
             f_max=8000.0)
SMALL48 = dict(SMALL, win_length=48)                   # the centred short window
WIDE_HOP = dict(SMALL, hop_length=48)                  # hop > n_fft / 2: one- and two-frame items
SPARSE = dict(SMALL, hop_length=80)                    # hop > n_fft: frames that do not overlap
BIG = dict(REF_AUDIO, n_fft=2048, win_length=2048)     # the largest transform


def _frames(audio, t, extra=0):
    """a length with exactly t frames"""
    return (t - 1) * audio["hop_length"] + extra


# name -> (audio parameters, lengths); every length L > n_fft / 2
CASES = {
    # n_fft / 2 + 1 samples: the two reflections overlap; k hop - 1, k hop, k hop + 1 at k = F
    "small": (SMALL, [33, 127, 128, 129]),
    "small48": (SMALL48, [33, 127, 128, 129]),
    # T_b = F - 1, F, F + 1, 2 F + 1 frames at the reference parameters
    "ref": (REF_AUDIO, [_frames(REF_AUDIO, t, 37) for t in (F - 1, F, F + 1, 2 * F + 1)]),
    "sparse": (SPARSE, [40, _frames(SPARSE, F + 2, 3)]),
    "big": (BIG, [_frames(BIG, F + 2, 300)]),
    # wave and block edges of the energy normalisation: 63, 64, 65 and 257 frames
    "edges": (SMALL, [_frames(SMALL, t, 5) for t in (63, 64, 65, 257)]),
}
# ragged batches (one launch each): T_b = 1, 2, F + 1 and the longest
RAGGED = {
    "ragged_wide": (WIDE_HOP, [40, _frames(WIDE_HOP, F + 1, 3), 50, _frames(WIDE_HOP, 2 * F + 3, 5)]),
    "ragged_ref": (REF_AUDIO, [_frames(REF_AUDIO, 3, 90), _frames(REF_AUDIO, F + 1, 0),
                               _frames(REF_AUDIO, 2 * F + 2, 255)]),
}


def case_waves(name):
    """(audio, list of fp32 waveforms) of a case; seeds follow the case and the position"""
    audio, lens = (CASES.get(name) or RAGGED[name])
    base = sorted(list(CASES) + list(RAGGED)).index(name) * 100
    tone = 440.0 if audio["n_fft"] >= 1024 else 1900.0
    return audio, [wave(base + i, n, tone_hz=tone, sample_rate=audio["sampling_rate"])
                   for i, n in enumerate(lens)]
