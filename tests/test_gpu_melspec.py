"""GPU: the log-mel front end -- fs2_melspec and fs2_energy_minmax, each alone through
fastspeech2.ops, against tests/melspec_restatement.py in float64 (pinned on the CPU by
tests/test_melspec_host.py), then MelFrontEnd, get_mel and inference.mel_of on top of them.

Every output sits inside a buffer of 0x5A bytes that must come back untouched around it, and
every float input is followed (the waveforms also preceded) by NaNs, so an over-read shows up
as a wrong value.  The inputs are the restatement's CASES and RAGGED: seeded noise of amplitude
0.1 plus one tone, which keeps every linear mel more than 1000 bounds above zero
(test_float32_restatement_inside_the_bound), so the log comparison leaves nothing out.  The
bound and its K are the restatement's docstring.
"""
import math

import numpy as np
import pytest
import torch

import melspec_restatement as MR

pytestmark = pytest.mark.gpu

TAIL = 64


class Out:
    """an output of ``numel`` elements between ``lead`` and TAIL sentinel elements"""

    def __init__(self, cuda, numel, tdtype, lead=16):
        self.es = torch.empty(0, dtype=tdtype).element_size()
        self.lead, self.numel = lead, numel
        self.raw = torch.full(((lead + numel + TAIL) * self.es,), 0x5A, dtype=torch.uint8,
                              device=cuda)
        self.t = self.raw.view(tdtype)[lead:lead + numel]

    def np(self):
        r = self.raw.cpu()
        a, b = self.lead * self.es, (self.lead + self.numel) * self.es
        assert bool((r[:a] == 0x5A).all()) and bool((r[b:] == 0x5A).all()), "sentinel written"
        return r[a:b].clone().view(self.t.dtype).numpy()


def _in(cuda, arr, lead=0):
    """a device copy of a numpy array between ``lead`` and TAIL elements of NaN (-999 for ints)"""
    arr = np.ascontiguousarray(arr).reshape(-1)
    fillv = np.nan if arr.dtype == np.float32 else -999
    pad = lambda k: np.full(k, fillv, arr.dtype)
    t = torch.from_numpy(np.concatenate([pad(lead), arr, pad(TAIL)]))
    return t.to(cuda)[lead:lead + arr.size]


_TABLES = {}


def _tables(cuda, audio):
    from fastspeech2 import audio as A
    key = tuple(sorted(audio.items()))
    if key not in _TABLES:
        n_fft = audio["n_fft"]
        fb = A.mel_filterbank(n_fft // 2 + 1, audio["f_min"], audio["f_max"], audio["n_mels"],
                              audio["sampling_rate"])
        bands, w = A.band_tables(fb)
        f32 = lambda a: _in(cuda, np.asarray(a, np.float32))
        _TABLES[key] = (f32(A.stft_window(audio["win_length"], n_fft)), f32(A.twiddles(n_fft)),
                        bands, f32(w))
    return _TABLES[key]


def run_melspec(cuda, audio, waves, bct, compression):
    """one fs2_melspec launch; returns mel (B, n_mels, T_max) whatever the layout, raw energy
    (B, T_max), mel_len (B) on the host and the device energy / mel_len for the next kernel"""
    from fastspeech2 import ops
    window, tw, bands, bw = _tables(cuda, audio)
    B, nm, hop = len(waves), audio["n_mels"], audio["hop_length"]
    off = np.zeros(B + 1, np.int64)
    np.cumsum([w.size for w in waves], out=off[1:])
    T = max(1 + w.size // hop for w in waves)
    wav = _in(cuda, np.concatenate(waves), lead=TAIL)
    offsets = _in(cuda, off)
    mel, e, ml = Out(cuda, B * T * nm, torch.float32), Out(cuda, B * T, torch.float32), \
        Out(cuda, B, torch.int64)
    ops.melspec(wav, offsets, B, window, tw, bands, bw, audio["n_fft"], audio["win_length"], hop,
                nm, T, bct, compression, mel.t, e.t, ml.t)
    torch.cuda.synchronize()
    m = mel.np().reshape((B, nm, T) if bct else (B, T, nm))
    return (m if bct else m.transpose(0, 2, 1)), e.np().reshape(B, T), ml.np(), e, ml


def check_batch(cuda, name, bct, parity_log):
    audio, waves = MR.case_waves(name)
    hop = audio["hop_length"]
    lin, e, ml, _, _ = run_melspec(cuda, audio, waves, bct, False)
    log, e2, ml2, _, _ = run_melspec(cuda, audio, waves, bct, True)
    assert e.tobytes() == e2.tobytes() and (ml == ml2).all()
    used = []
    for b, y in enumerate(waves):
        T = 1 + y.size // hop
        assert ml[b] == T
        used.append(MR.check_linear(lin[b, :, :T], e[b, :T], y, audio))
        assert MR.check_log(log[b, :, :T], y, audio) <= 0.01
        # padded rows: exact zeros (+0.0) in the mel of both runs and in the energy
        for pad in (lin[b, :, T:], log[b, :, T:], e[b, T:]):
            assert not pad.view(np.int32).any()
    parity_log[f"melspec_{name}_{'bct' if bct else 'btc'}"] = {
        "mel_share_of_bound": max(u[0] for u in used), "energy_share_of_bound": max(u[1] for u in used)}


@pytest.mark.parametrize("bct", [False, True], ids=["btc", "bct"])
@pytest.mark.parametrize("name", list(MR.CASES))
def test_melspec_single_utterances(cuda, name, bct, parity_log):
    """every length of the case as a launch of its own (T_max = T_b: the tile edges of the grid)"""
    audio, waves = MR.case_waves(name)
    for i, y in enumerate(waves):
        lin, e, ml, _, _ = run_melspec(cuda, audio, [y], bct, False)
        log, _, _, _, _ = run_melspec(cuda, audio, [y], bct, True)
        assert ml[0] == lin.shape[2] == 1 + y.size // audio["hop_length"]
        sm, se = MR.check_linear(lin[0], e[0], y, audio)
        assert MR.check_log(log[0], y, audio) <= 0.01
        parity_log[f"melspec_{name}_{i}_{'bct' if bct else 'btc'}"] = {
            "mel_share_of_bound": sm, "energy_share_of_bound": se}


@pytest.mark.parametrize("bct", [False, True], ids=["btc", "bct"])
@pytest.mark.parametrize("name", list(MR.RAGGED) + ["small", "sparse"])
def test_melspec_ragged_batch(cuda, name, bct, parity_log):
    """one launch over utterances of different lengths: values, mel_len, zero rows, sentinels"""
    check_batch(cuda, name, bct, parity_log)


def _minmax_bits(e_row, T):
    """the float32 restatement on the kernel's own raw energy, zero past T"""
    out = np.zeros_like(e_row)
    out[:T] = MR.minmax(torch.from_numpy(e_row[:T].copy())).numpy()
    return out


@pytest.mark.parametrize("name", ["ragged_wide", "ragged_ref", "edges"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
def test_energy_minmax_bit_for_bit(cuda, name, in_place):
    """T_b = 1 and 2 (ragged_wide), the wave edge 63 / 64 / 65 and 257 frames past the 256-thread
    stride (edges), padded frames left at zero; NaN by NaN-ness"""
    from fastspeech2 import ops
    audio, waves = MR.case_waves(name)
    _, e, ml, e_dev, ml_dev = run_melspec(cuda, audio, waves, False, False)
    B, T = e.shape
    out = e_dev if in_place else Out(cuda, B * T, torch.float32)
    ops.energy_minmax(e_dev.t, ml_dev.t, B, T, out.t)
    torch.cuda.synchronize()
    got = out.np().reshape(B, T)
    for b in range(B):
        ref = _minmax_bits(e[b], int(ml[b]))
        nan = np.isnan(ref)
        assert (np.isnan(got[b]) == nan).all()
        assert (got[b].view(np.int32) == ref.view(np.int32))[~nan].all()
        if ml[b] == 1:
            assert nan[0] and not nan[1:].any()
        if ml[b] >= 2 and not nan.any():
            assert got[b, :ml[b]].min() == 0.0 and got[b, :ml[b]].max() == 1.0
    assert (e_dev.np().reshape(B, T) == e).all() or in_place      # the input is left alone


def test_energy_minmax_constant_and_nan_input(cuda):
    """constant energy is 0 / 0 = NaN; a NaN energy makes the utterance's min and max NaN, as
    torch's do"""
    from fastspeech2 import ops
    e = np.array([[2.5, 2.5, 2.5, 0.0], [1.0, np.nan, 3.0, 4.0], [1.0, 3.0, 2.0, 0.0]], np.float32)
    ml = np.array([3, 4, 3], np.int64)
    out = Out(cuda, 12, torch.float32)
    ops.energy_minmax(_in(cuda, e), _in(cuda, ml), 3, 4, out.t)
    torch.cuda.synchronize()
    got = out.np().reshape(3, 4)
    assert np.isnan(got[0, :3]).all() and got[0, 3] == 0
    assert np.isnan(got[1]).all()
    assert got[2].tolist() == [0.0, 1.0, 0.5, 0.0]


@pytest.mark.parametrize("layout", ["btc", "bct"])
def test_front_end_batch_equals_get_mel(cuda, layout):
    """MelFrontEnd on a list == the per-utterance get_mel, bit for bit (NaN by NaN-ness): the
    batch must not change a value; a (B, L) tensor with lengths gives the same again"""
    from fastspeech2.audio import MelFrontEnd, get_mel
    audio, waves = MR.case_waves("ragged_ref")
    fe = MelFrontEnd(**audio, device=cuda)
    ws = [torch.from_numpy(w) for w in waves]
    mel, energy, mel_len = fe(ws, layout=layout)
    T = [1 + w.numel() // audio["hop_length"] for w in ws]
    assert mel_len.tolist() == T and energy.shape == (3, max(T))
    assert mel.shape == ((3, max(T), 80) if layout == "btc" else (3, 80, max(T)))
    padded = torch.zeros(3, max(w.numel() for w in ws) + 7)
    for i, w in enumerate(ws):
        padded[i, :w.numel()] = w
    mel2, energy2, _ = fe(padded.to(cuda), lengths=[w.numel() for w in ws], layout=layout)
    assert torch.equal(mel, mel2) and torch.equal(energy.nan_to_num(-1), energy2.nan_to_num(-1))
    for i, w in enumerate(ws):
        m1, e1 = get_mel(w.numpy(), **audio)              # numpy in, CPU tensors out
        assert m1.device.type == "cpu" and m1.shape == (80, T[i]) and e1.shape == (T[i],)
        mb = mel[i, :T[i]].t() if layout == "btc" else mel[i, :, :T[i]]
        assert torch.equal(mb.cpu(), m1)
        assert torch.equal(energy[i, :T[i]].cpu(), e1)
        assert not mel[i].cpu().reshape(-1)[T[i] * 80:].any() if layout == "btc" else \
            not mel[i, :, T[i]:].any()
        assert not energy[i, T[i]:].any()
        # and it is the reference's value
        assert MR.check_log(m1.numpy(), waves[i], audio) <= 0.01
        e64 = MR.get_mel(waves[i], torch.float64, **audio)[1]
        assert (e1.double() - e64).abs().max() <= 1e-5
    m_dev, e_dev = get_mel(ws[0].to(cuda), **audio)       # device in, device out
    assert m_dev.is_cuda and e_dev.is_cuda
    assert torch.equal(m_dev.cpu(), get_mel(ws[0], **audio)[0])


def test_all_zero_utterance(cuda):
    from fastspeech2.audio import MelFrontEnd
    fe = MelFrontEnd(**MR.REF_AUDIO, device=cuda)
    mel, energy, mel_len = fe([torch.zeros(2000), torch.from_numpy(MR.wave(1, 1500))], layout="bct")
    T = 1 + 2000 // 256
    assert mel_len.tolist() == [T, 1 + 1500 // 256]
    z = mel[0, :, :T].cpu()
    assert bool((z == z[0, 0]).all()) and abs(float(z[0, 0]) - math.log(1e-5)) <= 1e-6
    assert bool(torch.isnan(energy[0, :T]).all())          # constant (zero) energy: 0 / 0
    raw = fe([torch.zeros(2000)], min_max_energy_norm=False, compression=False)
    assert not raw[0].any() and not raw[1].any()


def test_vocode_mel_of_round_trip_shapes(cuda):
    """mel -> vocode -> mel_of: shapes and lengths (random vocoder weights: no values)"""
    from fastspeech2.audio import MelFrontEnd
    from fastspeech2.inference import mel_of, vocode
    from fastspeech2.vocoder import HifiganGenerator
    torch.manual_seed(0)
    g = HifiganGenerator().to(cuda)
    gen = torch.Generator().manual_seed(3)
    mels = [torch.randn(9, 80, generator=gen) - 4, torch.randn(5, 80, generator=gen) - 4]
    wav, nsamp = vocode(g, mels)
    assert wav.shape == (2, 1, 256 * (9 + 10)) and nsamp == [256 * 9, 256 * 5]
    fe = MelFrontEnd(**MR.REF_AUDIO, device=cuda)
    back, lens = mel_of(wav, nsamp, fe)
    assert lens == [9, 5] and [tuple(m.shape) for m in back] == [(9, 80), (5, 80)]
    assert all(m.is_cuda and bool(torch.isfinite(m).all()) for m in back)
