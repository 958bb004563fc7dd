"""CPU: the host side of the log-mel front end (fastspeech2/audio.py, fs2_melspec,
fs2_energy_minmax) -- the float64 tables against the formulas' known facts and against
tests/melspec_restatement.py, the restatement's own float32 error inside the bound with the
recorded K, and the refusals before any launch."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import melspec_restatement as MR

REF = MR.REF_AUDIO


def _fb(audio):
    from fastspeech2 import audio as A
    return A.mel_filterbank(audio["n_fft"] // 2 + 1, audio["f_min"], audio["f_max"],
                            audio["n_mels"], audio["sampling_rate"])


def test_filterbank_facts_at_the_reference_size():
    from fastspeech2 import audio as A
    fb = _fb(REF)
    assert fb.shape == (513, 80) and fb.dtype == np.float64 and (fb >= 0).all()
    widths = []
    for m in range(80):
        nz = np.flatnonzero(fb[:, m])
        assert nz.size > 0, f"filter {m} is empty"
        assert (np.diff(nz) == 1).all(), f"filter {m} is not one contiguous band"
        widths.append(nz.size)
    assert min(widths) == 4 and max(widths) == 37
    assert float(A.mel_to_hz(15.0)) == 1000.0 and A.hz_to_mel(1000.0) == 15.0
    assert abs(A.hz_to_mel(500.0) - 7.5) < 1e-14
    assert abs(float(A.mel_to_hz(A.hz_to_mel(6400.0))) - 6400.0) < 1e-9
    area = fb.sum(0) * (16000 / 2) / 512
    assert 0.97 <= area.min() and area.max() <= 1.04, (area.min(), area.max())
    # the restatement's filterbank is written separately from the package's
    assert np.abs(fb - MR.fbanks(513, 0.0, 8000.0, 80, 16000)).max() <= 1e-15


@pytest.mark.parametrize("audio", [REF, MR.SMALL, MR.SMALL48, MR.BIG], ids=["ref", "small",
                                                                          "small48", "big"])
def test_band_tables_reproduce_the_dense_product(audio):
    from fastspeech2 import audio as A
    fb = _fb(audio)
    bands, w = A.band_tables(fb)
    nf = audio["n_fft"] // 2 + 1
    assert bands.dtype == np.int32 and bands.shape == (audio["n_mels"], 2)
    assert (bands[:, 0] >= 0).all() and (bands.sum(1) <= nf).all() and w.size == bands[:, 1].sum()
    X = np.abs(np.random.default_rng(0).standard_normal((nf, 7)))
    dense = fb.T @ X
    got, off = np.zeros_like(dense), 0
    for m, (st, ln) in enumerate(bands):
        got[m] = w[off:off + ln] @ X[st:st + ln]
        off += ln
    assert np.abs(got - dense).max() <= 1e-12


def test_window_and_twiddles():
    from fastspeech2 import audio as A
    w = A.stft_window(1024, 1024)
    assert np.abs(w - torch.hann_window(1024, periodic=True, dtype=torch.float64).numpy()).max() < 1e-15
    w = A.stft_window(48, 64)
    assert (w[:8] == 0).all() and (w[56:] == 0).all() and w[8] == 0 and w[9] > 0
    assert np.abs(w[8:56] - torch.hann_window(48, dtype=torch.float64).numpy()).max() < 1e-15
    tw = A.twiddles(64)
    assert tw.shape == (32, 2) and tw[0, 0] == 1 and tw[0, 1] == 0 and abs(tw[16, 0]) < 1e-16
    assert np.abs(tw[:, 0] ** 2 + tw[:, 1] ** 2 - 1).max() < 1e-15
    with pytest.raises(ValueError):
        A.stft_window(65, 64)


def test_frame_count():
    from fastspeech2 import audio as A
    for name in MR.CASES:
        audio, waves = MR.case_waves(name)
        for y in waves:
            mel, e = MR.linear_mel(y, torch.float64, **audio)
            assert mel.shape == (audio["n_mels"], 1 + y.size // audio["hop_length"])
            assert A.n_frames(y.size, audio["hop_length"]) == mel.shape[1] == e.shape[0]


@pytest.mark.parametrize("name", list(MR.CASES) + list(MR.RAGGED))
def test_float32_restatement_inside_the_bound(name):
    """with the recorded K, and with the K / 2 it was doubled from (the docstring's rule)"""
    audio, waves = MR.case_waves(name)
    for y in waves:
        mel, e = MR.linear_mel(y, torch.float32, **audio)
        sm, se = MR.check_linear(mel.numpy(), e.numpy(), y, audio)
        assert sm <= 0.5 and se <= 0.5
        assert MR.check_log(MR.compress(mel).numpy(), y, audio) == 0.0
        # the inputs keep the linear mel far above the bound
        m64, _ = MR.linear_mel(y, torch.float64, **audio)
        assert (m64.numpy() >= 1000 * MR.mel_bound(y, **audio)).all()


def test_K_is_the_rule_of_the_docstring():
    worst = 0.0
    for name in list(MR.CASES) + list(MR.RAGGED):
        audio, waves = MR.case_waves(name)
        for y in waves:
            m32, _ = MR.linear_mel(y, torch.float32, **audio)
            m64, _ = MR.linear_mel(y, torch.float64, **audio)
            worst = max(worst, float(np.max(np.abs(m32.double().numpy() - m64.numpy())
                                            / MR.mel_bound(y, 1.0, **audio))))
    k0 = 2.0 ** math.ceil(math.log2(worst))
    assert MR.K == 2 * k0, (worst, k0)


def test_one_frame_and_constant_energy_are_nan():
    e = MR.minmax(torch.tensor([0.37], dtype=torch.float32))
    assert e.shape == (1,) and bool(torch.isnan(e).all())
    assert bool(torch.isnan(MR.minmax(torch.full((5,), 2.0))).all())
    audio, waves = MR.case_waves("ragged_wide")
    _, e = MR.get_mel(waves[0], torch.float32, **audio)
    assert e.shape == (1,) and bool(torch.isnan(e).all())


def test_get_mel_signature_is_the_references():
    from fastspeech2 import audio as A
    assert list(inspect.signature(A.get_mel).parameters) == [
        "y", "sampling_rate", "hop_length", "win_length", "n_mels", "n_fft", "f_min", "f_max"]
    assert list(inspect.signature(A.MelFrontEnd.__init__).parameters)[1:] == [
        "sampling_rate", "hop_length", "win_length", "n_fft", "n_mels", "f_min", "f_max", "device"]
    assert set(REF) == set(inspect.signature(A.MelFrontEnd.__init__).parameters) - {"self", "device"}
    import fastspeech2
    from fastspeech2 import ops
    assert ops.MELSPEC_FRAMES == MR.F                 # the tile the tests' lengths are built on
    assert fastspeech2.get_mel is A.get_mel and fastspeech2.MelFrontEnd is A.MelFrontEnd


def test_front_end_refusals():
    from fastspeech2 import audio as A
    for bad in (dict(n_fft=1000), dict(n_fft=32, win_length=32), dict(n_fft=4096),
                dict(win_length=2048), dict(hop_length=0), dict(n_mels=0)):
        with pytest.raises(ValueError):
            A.MelFrontEnd(**dict(REF, **bad), device="cpu")
    fe = A.MelFrontEnd(**REF, device="cpu")          # tables only: no launch on the CPU
    assert fe.window.dtype == torch.float32 and fe.bands.shape == (80, 2)
    with pytest.raises(NotImplementedError, match="audio_util.py:35-36"):
        fe([torch.zeros(2000)], power=2)
    with pytest.raises(NotImplementedError, match="audio_util.py:35-36"):
        fe([torch.zeros(2000)], normalized=True)
    with pytest.raises(ValueError, match="layout"):
        fe([torch.zeros(2000)], layout="tbc")
    with pytest.raises(ValueError, match="reflect"):    # as torch.stft refuses n_fft / 2 >= L
        fe([torch.zeros(2000), torch.zeros(512)])
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(512), 1024, 256, 1024, torch.hann_window(1024), center=True,
                   pad_mode="reflect", return_complex=True)
    with pytest.raises(ValueError, match="lengths"):
        fe(torch.zeros(2, 2000))


def test_export_refusals():
    """every call returns FS2_EINVAL before a launch (no device is touched: the pointers are
    never dereferenced on the device, the band table is host memory)"""
    from fastspeech2 import _native
    lib = _native.load()
    EINVAL, p = -1, 4096
    bands = np.array([[0, 4], [2, 31]], np.int32)
    hb = bands.ctypes.data

    def mel(n_fft=64, win=64, hop=16, n_mels=2, T=4, B=1, wav=p, off=p, win_p=p, tw=p, b=hb,
            bw=p, out=p, e=p, ml=p):
        return lib.fs2_melspec(wav, off, B, win_p, tw, b, bw, n_fft, win, hop, n_mels, T, 0, 1,
                               out, e, ml, None)

    assert mel(B=0) == 0                                  # nothing to do, nothing launched
    for kw in (dict(n_fft=96), dict(n_fft=32, win=32), dict(n_fft=4096), dict(n_fft=0),
               dict(win=65), dict(win=0), dict(hop=0), dict(hop=-3), dict(n_mels=0),
               dict(n_mels=257), dict(T=0), dict(B=-1), dict(B=65536), dict(wav=None),
               dict(off=None), dict(win_p=None), dict(tw=None), dict(b=None), dict(bw=None),
               dict(out=None), dict(e=None), dict(ml=None)):
        assert mel(**kw) == EINVAL, kw
    for bad in ([[0, 4], [3, 31]], [[0, 34], [0, 1]], [[-1, 2], [0, 1]], [[0, -2], [0, 1]],
                [[34, 0], [0, 1]]):
        bb = np.array(bad, np.int32)
        assert mel(b=bb.ctypes.data) == EINVAL, bad
    assert lib.fs2_energy_minmax(p, p, 0, 4, p, None) == 0
    for args in ((None, p, 1, 4, p), (p, None, 1, 4, p), (p, p, 1, 4, None), (p, p, 1, 0, p),
                 (p, p, -1, 4, p)):
        assert lib.fs2_energy_minmax(*args, None) == EINVAL, args
