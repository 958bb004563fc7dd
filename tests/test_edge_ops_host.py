"""CPU checks that pin tests/edge_ops_restatement.py before a GPU test relies on it: each
restatement against torch or the oracle, the bf16 rounding against torch's on the tie and
overflow family, the intensity-head bound against an honest fp32 evaluation, and the entry
points' refusals (FS2_EINVAL before any launch)."""
import ctypes
import fractions
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_ops_restatement as ER


# ---- collate -----------------------------------------------------------------------------------
def _pack(items):
    """order, offsets and packed buffers of a batch, derived as fastspeech2/dataset.py
    (GpuCollate.__call__) derives them"""
    B = len(items)
    input_lengths, ids_sorted_decreasing = torch.sort(
        torch.LongTensor([len(x["phoneme"]) for x in items]), dim=0, descending=True)
    frames = [int(x["mel"].size(1)) for x in items]
    poff = np.zeros(B + 1, dtype=np.int64)
    poff[1:] = np.cumsum([len(x["phoneme"]) for x in items])
    foff = np.zeros(B + 1, dtype=np.int64)
    foff[1:] = np.cumsum(frames)
    cat = lambda k, f: torch.cat([f(x[k]).reshape(-1) for x in items]).numpy()
    return dict(order=ids_sorted_decreasing.to(torch.int32).numpy(), poff=poff, foff=foff,
                phon=cat("phoneme", torch.Tensor.long), dur=cat("duration", torch.Tensor.long),
                mel=cat("mel", torch.Tensor.float), pitch=cat("pitch", torch.Tensor.float),
                energy=cat("energy", torch.Tensor.float), B=B, Tp=int(input_lengths[0]),
                Tm=max(frames), NM=int(items[0]["mel"].size(0)))


def _collate_both(items):
    k = _pack(items)
    ph, du, il = ER.collate_phonemes(k["order"], k["poff"], k["phon"], k["dur"], k["B"], k["Tp"])
    mp, pp, ep, rk, ol = ER.collate_frames(k["order"], k["foff"], k["mel"], k["pitch"],
                                           k["energy"], k["B"], k["Tm"], k["NM"])
    return {"phoneme": ph, "duration": du, "input_lengths": il, "mel": mp, "pitch": pp,
            "energy": ep, "rank_X": rk, "output_lengths": ol}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_collate_restatement_is_the_oracle():
    from oracle.collate_oracle import collate_np
    g = torch.Generator().manual_seed(11)
    items = []
    for i, tp in enumerate((7, 12, 3, 12, 9)):           # a tie: torch.sort decides the order
        d = torch.randint(0, 5, (tp,), generator=g)
        T = max(int(d.sum()), 1)
        items.append({"mel": torch.randn(6, T, generator=g), "pitch": torch.randn(T, generator=g),
                      "energy": torch.randn(T, generator=g), "duration": d,
                      "phoneme": torch.randint(1, 89, (tp,), generator=g),
                      "speaker": torch.tensor(i), "emotion": torch.tensor(i), "text": str(i),
                      "audio_path": f"{i}.wav"})
    got, ref = _collate_both(items), collate_np(items)
    for n, v in got.items():
        assert _same(v, np.ascontiguousarray(ref[n])), n
    assert list(_pack(items)["order"]) != sorted(_pack(items)["order"])


def test_collate_restatement_reproduces_the_golden(golden_dir):
    from oracle.collate_oracle import items_from_golden
    z = np.load(os.path.join(golden_dir, "collate_ref.npz"))
    got = _collate_both(items_from_golden(z))
    for n, v in got.items():
        assert _same(v, np.ascontiguousarray(z["out_" + n])), n


# ---- phoneme average ---------------------------------------------------------------------------
def _avg_case(seed=3, B=3, Tp=9, E=5):
    r = np.random.default_rng(seed)
    durs = r.integers(0, 6, (B, Tp)).astype(np.int64)
    durs[0, 0] = 0
    durs[1, 3:6] = 0
    phon_len = np.array([Tp, Tp - 2, 4][:B], np.int64)
    for b in range(B):
        durs[b, phon_len[b]:] = 0
    T = int(durs.sum(1).max())
    I = r.standard_normal((B, T, E)).astype(np.float32)
    return I, T, E, durs, phon_len, B, Tp


def test_phoneme_average_restatement_is_the_oracle():
    """float64 form == oracle.intensity_oracle.phoneme_average_np; float32 form within the
    derived bound of it and of oracle.fs2_oracle.phoneme_average_intensity (sum d == T per
    utterance or fewer: the reference's domain)"""
    from oracle.fs2_oracle import phoneme_average_intensity
    from oracle.intensity_oracle import phoneme_average_np
    I, T, E, durs, phon_len, B, Tp = _avg_case()
    ref, bound = ER.phoneme_average(I, T, E, durs, phon_len, B, Tp, np.float64)
    assert _same(ref.astype(np.float32), phoneme_average_np(I, durs, phon_len))
    o32 = ER.phoneme_average(I, T, E, durs, phon_len, B, Tp)
    assert o32.dtype == np.float32 and (np.abs(o32 - ref) <= bound).all()
    tor = phoneme_average_intensity(torch.from_numpy(I), torch.from_numpy(durs),
                                    torch.from_numpy(phon_len)).numpy()
    assert (np.abs(tor - ref) <= bound).all()
    assert (bound[durs == 0] == 0).all() and (o32[durs == 0] == 0).all()
    assert 0 < bound.max() < 1e-5


def test_phoneme_average_outside_the_reference_domain():
    """the documented extensions: phon_len clamped to [0, Tp], frames from T on not read, the
    divisor still the full duration"""
    I = np.arange(1, 13, dtype=np.float32).reshape(1, 6, 2)
    durs = np.array([[2, 3, 4, 1]], np.int64)              # sum 10 > T = 6
    out = ER.phoneme_average(I, 6, 2, durs, [9], 1, 4)
    assert out[0, 0].tolist() == [2.0, 3.0]                 # (1+3)/2, (2+4)/2
    assert out[0, 2].tolist() == [np.float32(11) / np.float32(4), 3.0]   # frame 5 only, / 4
    assert out[0, 3].tolist() == [0.0, 0.0] and not np.signbit(out[0, 3]).any()
    assert (ER.phoneme_average(I, 6, 2, durs, [-3], 1, 4) == 0).all()
    nan_tail = np.concatenate([I.reshape(-1), np.full(8, np.nan, np.float32)])
    assert _same(ER.phoneme_average(nan_tail, 6, 2, durs, [4], 1, 4), out)


# ---- intensity head ----------------------------------------------------------------------------
def _head_case(B=3, T=7, D=100, E=5, ldh=104, seed=5):
    r = np.random.default_rng(seed)
    H = r.standard_normal((B * T, ldh)).astype(np.float32)
    tab = r.standard_normal((B + 2, D)).astype(np.float32)
    emo = np.array([B + 1] + list(range(B - 1)), np.int64)
    lens = np.array([0, T, T + 3][:B], np.int64)
    Wc = (r.standard_normal((E, D)) / np.sqrt(D)).astype(np.float32)
    bc = r.standard_normal(E).astype(np.float32)
    return H, ldh, tab, emo, lens, Wc, bc, B, T, D, E


def _head_torch(H, ldh, tab, emo, lens, Wc, bc, B, T, D, E, dtype):
    h = torch.from_numpy(H).to(dtype).view(B, T, ldh)[:, :, :D]
    i_ = h + torch.from_numpy(tab).to(dtype)[torch.from_numpy(emo)].unsqueeze(1)
    mask = torch.arange(T).unsqueeze(0) >= torch.from_numpy(lens).unsqueeze(1)
    i_ = i_.masked_fill(mask.unsqueeze(-1), 0.0)
    lin = torch.nn.Linear(D, E).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(Wc))
        lin.bias.copy_(torch.from_numpy(bc))
        return lin(i_).reshape(B * T, E).numpy()


@pytest.mark.parametrize("D,ldh", [(100, 104), (384, 384), (63, 63)])
def test_intensity_head_restatement_and_bound(D, ldh):
    """float64 form == masked_fill + nn.Linear in torch float64 (to a few float64 ulps of the
    terms: another summation order); torch's fp32 evaluation lies inside the derived bound, and
    one wrong rounding direction's worth of error on every term does not"""
    case = _head_case(D=D, ldh=ldh)
    ref, bound, keep = ER.intensity_head(*case)
    t64 = _head_torch(*case, torch.float64)
    # u = 2^-53 for 2^-24 and a chain of at most D adds for ceil(D/64) + 9 roundings: 2^-29 * 2^6
    assert (np.abs(ref - t64)[keep] <= bound[keep] * 2.0 ** -23).all()
    B, T, E = case[7], case[8], case[10]
    assert keep.reshape(B, T).sum(1).tolist() == [0, T, T]
    assert _same(ref[~keep], np.tile(case[6].astype(np.float64), ((~keep).sum(), 1)))
    assert (bound[~keep] == 0).all() and (bound[keep] > 0).all()
    t32 = _head_torch(*case, torch.float32).astype(np.float64)
    err = np.abs(t32 - ref)
    assert (err <= bound).all() and _same(t32[~keep], ref[~keep])
    print(f"D={D}: torch fp32 at most {float((err[keep] / bound[keep]).max()):.3f} of the bound")
    assert (err[keep] / bound[keep]).max() > 1e-3          # not vacuous: same order as fp32 error
    # a bf16-sized error is far outside it
    assert (bound[keep] < 2.0 ** -9 * np.abs(ref[keep]).max()).all()


# ---- vocoder -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NM,T,pad,ldx", [(2, 80, 23, 5, 80), (1, 80, 1, 5, 88), (3, 7, 4, 0, 8),
                                            (2, 80, 3, 7, 80)])
def test_vocoder_input_restatement_is_replicate_pad(B, NM, T, pad, ldx):
    mel = torch.randn(B, NM, T, generator=torch.Generator().manual_seed(T))
    ref = torch.zeros(B, T + 2 * pad, ldx)
    ref[:, :, :NM] = F.pad(mel, (pad, pad), "replicate").transpose(1, 2)
    got = ER.vocoder_input(mel.numpy(), B, NM, T, pad, ldx, "f32")
    assert _same(got, ref.reshape(-1, ldx).numpy())
    got16 = ER.vocoder_input(mel.numpy(), B, NM, T, pad, ldx, "bf16")
    assert _same(got16.view(np.int16), ref.reshape(-1, ldx).bfloat16().view(torch.int16).numpy())


@pytest.mark.parametrize("slope", [0.1, 0.0])
def test_leaky_relu_restatements_are_torch(slope):
    """Slopes >= 0 only: torch selects by x > 0 and the header by x >= 0, and the two differ
    nowhere for such a slope (IEEE: -0.0 * s = -0.0 and +0.0 * s = +0.0, also for s = 0).  Only a
    negative slope tells them apart at +-0, and no caller passes one."""
    n = 771
    x, b, c = (ER.activation_family(n, s, "f32") for s in (1, 2, 3))
    c[5::9] = -(x[5::9] + b[5::9])                          # sums that cancel exactly
    tx, tb, tc = (torch.from_numpy(v) for v in (x, b, c))
    assert ER.same_bits(ER.leaky_relu(x, slope, "f32"), F.leaky_relu(tx, slope).numpy())
    assert ER.same_bits(ER.mean3_leaky_relu(x, b, c, slope, "f32"),
                        F.leaky_relu(((tx + tb) + tc) / 3, slope).numpy())
    y = ER.leaky_relu(x, slope, "f32")
    z = x == 0
    assert z.sum() >= 4 and (np.signbit(y[z]) == np.signbit(x[z])).all()
    # NaN stays NaN; the only new one is -inf * 0 under slope 0
    assert np.isnan(x).any() and (np.isnan(y) == (np.isnan(x) | ((x == -np.inf) & (slope == 0)))).all()
    # bf16: the fp32 result rounded once more
    xb = ER.activation_family(n, 1, "bf16")
    want = F.leaky_relu(torch.from_numpy(xb), slope).bfloat16().view(torch.int16).numpy()
    assert ER.same_bits16(ER.leaky_relu(xb, slope, "bf16"), want)


# ---- bf16 rounding, add, fill, cast --------------------------------------------------------------
def test_bf16_rne_is_torch_bfloat16():
    fam = ER.rounding_family()
    r = np.random.default_rng(0)
    x = np.concatenate([fam, r.standard_normal(4096).astype(np.float32),
                        r.integers(0, 2 ** 32, 4096, dtype=np.uint32).view(np.float32)])
    got = ER.bf16_rne(x)
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert nan.sum() >= 6
    assert (np.isnan(ER.bf16_to_f32(got)) == nan).all()
    assert (got[~nan] == want[~nan]).all()
    # the family holds what it says it holds
    f = lambda w: np.array([w], np.uint32).view(np.float32)
    assert ER.bf16_rne(f(0x3F808000))[0] == 0x3F80 and ER.bf16_rne(f(0x3F818000))[0] == 0x3F82
    assert ER.bf16_rne(f(0x3F808001))[0] == 0x3F81 and ER.bf16_rne(f(0x3F817FFF))[0] == 0x3F81
    assert ER.bf16_rne(np.float32([ER.FLT_MAX, -ER.FLT_MAX])).tolist() == [0x7F80, 0xFF80]
    assert ER.bf16_rne(f(0x7F7F7FFF))[0] == 0x7F7F and ER.bf16_rne(f(0x7F7F8000))[0] == 0x7F80
    assert ER.bf16_rne(np.float32([0.0, -0.0, np.inf, -np.inf])).tolist() == [0, 0x8000, 0x7F80,
                                                                             0xFF80]
    for w in (0x3F808000, 0x3F818000, 0x7F7F8000, 0x7F7FFFFF, 0x80000000, 0xFF800000):
        assert w in fam.view(np.uint32)
    assert float(ER.bf16_to_f32(np.uint16([0x7F7F]))[0]) == ER.BF16_MAX
    # bf16 -> fp32 -> bf16 is the identity on every non-NaN pattern
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wide = ER.bf16_to_f32(allb)
    ok = ~np.isnan(wide)
    assert (ER.bf16_rne(wide)[ok] == allb[ok]).all()
    tw = torch.from_numpy(allb.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert _same(wide[ok], tw[ok]) and np.isnan(tw[~ok]).all() and (~ok).sum() == 2 * 127
    # subnormals: the restatement rounds them to nearest even as torch does
    sub = ER.subnormal_family()
    assert (np.abs(sub) < ER.FLT_MIN).all() and (sub != 0).all()
    assert _same(ER.bf16_rne(sub).view(np.int16),
                 torch.from_numpy(sub).bfloat16().view(torch.int16).numpy())


@pytest.mark.parametrize("alpha", [1.0, -1.0, 0.37])
def test_add_candidates(alpha):
    """unfused == torch's fp32 x + alpha32*y; fused == the exact sum (rational arithmetic)
    rounded once; for alpha = +-1 the two coincide"""
    r = np.random.default_rng(7)
    n = 600
    x = r.standard_normal(n).astype(np.float32)
    y = r.standard_normal(n).astype(np.float32)
    x[:40] *= np.float32(2.0 ** -20)                        # the product dominates / is dominated
    y[40:80] *= np.float32(2.0 ** -20)
    x[80:90] = -(np.float32(alpha) * y[80:90])              # near cancellation
    unf, fus = ER.add(x, y, alpha, "f32")
    al = np.float32(alpha)
    assert ER.same_bits(unf, (torch.from_numpy(x) + torch.from_numpy(y) * float(al)).numpy())
    Fr = fractions.Fraction
    for i in range(n):
        exact = Fr(float(x[i])) + Fr(float(al)) * Fr(float(y[i]))
        lo, hi = np.nextafter(fus[i], np.float32(-np.inf)), np.nextafter(fus[i], np.float32(np.inf))
        d = abs(exact - Fr(float(fus[i])))
        dl, dh = abs(exact - Fr(float(lo))), abs(exact - Fr(float(hi)))
        assert d <= dl and d <= dh, i
        if d == dl or d == dh:                               # a tie: the even one
            assert int(fus[i:i + 1].view(np.uint32)[0]) & 1 == 0, i
    if abs(alpha) == 1.0:
        assert ER.same_bits(unf, fus)
    else:
        assert 0 < int((unf.view(np.int32) != fus.view(np.int32)).sum()) < n // 2
    u16, f16 = ER.add(ER.bf16_to_f32(ER.bf16_rne(x)), ER.bf16_to_f32(ER.bf16_rne(y)), alpha, "bf16")
    assert u16.dtype == np.uint16 and f16.dtype == np.uint16


def test_fill_and_cast_restatements():
    assert ER.fill(3, 1.0 / 3.0, "f32").tolist() == [np.float32(1.0 / 3.0)] * 3
    assert ER.fill(2, 1.0 / 3.0, "bf16").tolist() == [0x3EAB, 0x3EAB]
    assert ER.fill(1, -0.0, "bf16").tolist() == [0x8000] and ER.fill(1, np.inf, "bf16")[0] == 0x7F80
    x = ER.rounding_family()
    assert ER.same_bits(ER.cast(x, "f32", "f32"), x)
    assert ER.same_bits16(ER.cast(x, "f32", "bf16"), ER.bf16_rne(x))
    b = ER.bf16_rne(x)
    assert ER.same_bits16(ER.cast(b, "bf16", "bf16"), b)
    assert ER.same_bits(ER.cast(b, "bf16", "f32"), ER.bf16_to_f32(b))


def test_intensity_input_restatement():
    B, T, C, ldx = 2, 5, 3, 8
    x = torch.randn(B, T, C)
    ref = torch.zeros(B * T, ldx)
    ref[:, :C] = x.reshape(B * T, C)
    assert _same(ER.intensity_input(x.numpy(), 0, B, T, C, ldx, "f32"), ref.numpy())
    xt = x.transpose(1, 2).contiguous()                     # the collate's (B, C, T)
    assert _same(ER.intensity_input(xt.numpy(), 1, B, T, C, ldx, "f32"), ref.numpy())
    assert _same(ER.intensity_input(xt.numpy(), 1, B, T, C, ldx, "bf16").view(np.int16),
                 ref.bfloat16().view(torch.int16).numpy())


# ---- refusals ----------------------------------------------------------------------------------
def test_edge_entry_points_refuse_before_any_launch():
    """Addresses that are never followed, as in test_adamw_entry_points_refuse_before_any_launch:
    every call here must return FS2_EINVAL (or 0 for a zero-size call) before a launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    EINVAL = -1
    for dt in (N.F32, N.BF16):
        V = 4 if dt == N.F32 else 8
        es = 16 // V
        # fs2_vocoder_input(mel, B, n_mels, T, pad, X, ldx, dtype, stream)
        assert lib.fs2_vocoder_input(p, 2, 80, 4, 1, p, 79, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(p, 2, 80, 0, 1, p, 80, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(p, 2, 80, -1, 2, p, 80, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(p, 2, 80, 4, -1, p, 80, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(None, 2, 80, 4, 1, p, 80, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(p, 2, 80, 4, 1, None, 80, dt, None) == EINVAL
        assert lib.fs2_vocoder_input(p, 0, 80, 4, 1, p, 80, dt, None) == 0
        # fs2_leaky_relu(x, y, n, slope, dtype, stream)
        for n in (V - 1, V + 1, 3 * V + V // 2):
            assert lib.fs2_leaky_relu(p, p, n, 0.1, dt, None) == EINVAL, n
            assert lib.fs2_mean3_leaky_relu(p, p, p, p, n, 0.1, dt, None) == EINVAL, n
        for k in range(2):
            a = [p, p]
            a[k] = p + es                                   # one element off 16-byte alignment
            assert lib.fs2_leaky_relu(*a, 4 * V, 0.1, dt, None) == EINVAL, k
            a[k] = None
            assert lib.fs2_leaky_relu(*a, 4 * V, 0.1, dt, None) == EINVAL, k
        for k in range(4):
            a = [p, p, p, p]
            a[k] = p + es
            assert lib.fs2_mean3_leaky_relu(*a, 4 * V, 0.1, dt, None) == EINVAL, k
            a[k] = p + 8
            assert lib.fs2_mean3_leaky_relu(*a, 4 * V, 0.1, dt, None) == EINVAL, k
            a[k] = None
            assert lib.fs2_mean3_leaky_relu(*a, 4 * V, 0.1, dt, None) == EINVAL, k
        assert lib.fs2_leaky_relu(p, p, 0, 0.1, dt, None) == 0
        assert lib.fs2_mean3_leaky_relu(p, p, p, p, 0, 0.1, dt, None) == 0
        # fs2_intensity_input(x, layout_bct, B, T, C, X, ldx, dtype, stream)
        for bct in (0, 1):
            assert lib.fs2_intensity_input(p, bct, 2, 5, 82, p, 81, dt, None) == EINVAL
            assert lib.fs2_intensity_input(p, bct, 2, 0, 82, p, 88, dt, None) == 0
        # fs2_intensity_head(H, ldh, emo_table, emotions, lengths, Wc, bc, B, T, D, E, I, dtype, s)
        for E in (0, 9, -1):
            assert lib.fs2_intensity_head(p, 64, p, p, p, p, p, 2, 5, 64, E, p, dt, None) == EINVAL
        assert lib.fs2_intensity_head(p, 64, p, p, p, p, p, 0, 5, 64, 5, p, dt, None) == 0
    # fs2_phoneme_average(I, T, E, durations, phon_len, B, Tp, out, stream)
    assert lib.fs2_phoneme_average(p, 10, 5, p, p, 2, 1025, p, None) == EINVAL
    assert lib.fs2_phoneme_average(p, 10, 5, p, p, 2, 4096, p, None) == EINVAL
    assert lib.fs2_phoneme_average(p, 10, 5, p, p, 0, 1024, p, None) == 0
    assert lib.fs2_phoneme_average(p, 10, 0, p, p, 2, 1024, p, None) == 0
    # fs2_collate_frames(order, foff, mel, pitch, energy, B, Tm, n_mels, 5 outputs, stream)
    for nm in (0, 129, -1):
        assert lib.fs2_collate_frames(p, p, p, p, p, 2, 10, nm, p, p, p, p, p, None) == EINVAL
    assert lib.fs2_collate_frames(p, p, p, p, p, 2, 0, 80, p, p, p, p, p, None) == 0
    assert lib.fs2_collate_frames(p, p, p, p, p, 0, 10, 80, p, p, p, p, p, None) == 0
    assert lib.fs2_collate_phonemes(p, p, p, p, 0, 10, p, p, p, None) == 0
    assert lib.fs2_collate_phonemes(p, p, p, p, 2, 10, None, p, p, None) == EINVAL
    # fs2_cast(src, src_dtype, dst, dst_dtype, n, stream)
    for bad in (2, -1):
        for good in (N.F32, N.BF16):
            assert lib.fs2_cast(p, bad, p, good, 16, None) == EINVAL
            assert lib.fs2_cast(p, good, p, bad, 16, None) == EINVAL
        assert lib.fs2_cast(p, bad, p, bad, 16, None) == EINVAL
    assert lib.fs2_cast(p, N.F32, p, N.BF16, 0, None) == 0
    assert lib.fs2_cast(None, N.F32, p, N.BF16, 16, None) == EINVAL
    assert lib.fs2_fill(p, 0, 1.0, N.F32, None) == 0 and lib.fs2_fill(p, 16, 1.0, 2, None) == EINVAL
    assert lib.fs2_add(p, p, 0, 1.0, N.BF16, None) == 0
    assert lib.fs2_add(p, p, 16, 1.0, 2, None) == EINVAL
