"""CPU: the host side of the prosody feature stage (fastspeech2/prosody.py, fs2_prosody_*) --
tests/prosody_restatement.py pinned against the reference's own library calls (scipy's interp1d,
np.percentile, numpy's float32 mean, sklearn's StandardScaler.partial_fit per utterance) on every
case, those libraries' arithmetic inside the derived bounds, the fence condition on the inputs,
the refusals before any launch, and the FeatureSet round trip through FastSpeech2Dataset."""
import json
import os

import numpy as np
import pytest
import torch

import prosody_restatement as PR

NAMES = list(PR.CASES)


def _scipy_track(f0, D):
    """scipy's interp1d through the voiced frames of f0[:D], evaluated at every frame, with the
    library arguments the reference passes (end values outside the voiced range, no error)"""
    from scipy.interpolate import interp1d
    voiced = np.flatnonzero(f0[:D])
    y = f0[voiced]
    return voiced, interp1d(voiced, y, bounds_error=False, fill_value=(y[0], y[-1]))(np.arange(D))


def _numpy_clean(held):
    """numpy's own quartiles of the array as held, and the values inside the restatement's
    fence formula evaluated on them: (q1, q3, mask)"""
    q1, q3 = (np.float64(v) for v in np.percentile(held, (25, 75)))
    lo, hi = PR.fences(q1, q3)
    return q1, q3, np.logical_and(held >= lo, held <= hi)


def _numpy_phoneme_means(values, durs):
    """numpy's mean of every phoneme's frames in the array's own dtype, stored as float32, and
    the frames of every phoneme as float64"""
    ends = np.cumsum(durs)
    means, spans = np.zeros(len(durs), np.float32), []
    for k, (a, e) in enumerate(zip(ends - durs, ends)):
        spans.append(values[a:e].astype(np.float64))
        if e > a:
            means[k] = np.mean(values[a:e])
    return means, spans


def _utterances(name, pa, ea):
    """(i, field, held, expected dict) of every accepted utterance and field of a case"""
    ex = PR.expected(name, pa, ea)
    for i in range(len(ex["D"])):
        if ex["status"][i] == 0:
            for f in (0, 1):
                yield i, f, ex["held"][f][i], ex


@pytest.mark.parametrize("name", NAMES)
def test_interpolation_against_scipy(name):
    pytest.importorskip("scipy.interpolate")
    batch, ex = PR.case(name), PR.expected(name, False, False)
    for i, f0 in enumerate(batch["f0s"]):
        D = ex["D"][i]
        x, st = PR.interpolate(f0, D)
        if st:
            assert st == PR.UNVOICED and not f0[:D].any()
            continue
        voiced, ref = _scipy_track(f0, D)
        assert ref.dtype == np.float64 and ref.shape == x.shape
        assert np.abs(ref - x).max() <= PR.interp_bound(f0, D)
        assert (x[voiced] == f0[voiced]).all()             # voiced frames are kept as they are


def test_one_voiced_frame_is_a_constant_track_in_scipy_too():
    pytest.importorskip("scipy.interpolate")
    pitch = np.array([0, 0, 0, 187.25, 0, 0], np.float64)
    _, ref = _scipy_track(pitch, 6)
    x, st = PR.interpolate(pitch, 6)
    assert st == 0 and (x == 187.25).all() and (ref == 187.25).all()


@pytest.mark.parametrize("pa,ea", PR.AVERAGING)
@pytest.mark.parametrize("name", NAMES)
def test_quartiles_fences_and_clean_mask_against_numpy(name, pa, ea):
    """np.percentile on the array as the reference holds it (float32 when averaged or energy);
    the fence condition with the restatement's fences and with numpy's own; equal masks"""
    for i, f, x, ex in _utterances(name, pa, ea):
        f32 = f == 1 or pa
        held = x.astype(np.float32) if f32 else x
        assert (held.astype(np.float64) == x).all()
        q1, q3, mask = _numpy_clean(held)
        r1, r3 = ex["q"][f][i]
        tol = 4 * PR.U32 * float(np.abs(x).max()) if f32 else 0.0   # numpy's float32 b - a
        assert abs(q1 - r1) <= tol and abs(q3 - r3) <= tol
        assert PR.fence_gap_ok(x, r1, r3), (name, i, f)
        assert PR.fence_gap_ok(x, q1, q3), (name, i, f)
        assert (mask == PR.clean_mask(x, r1, r3)).all()
        assert int(mask.sum()) == ex["n_clean"][f][i] >= 1


@pytest.mark.parametrize("name", NAMES)
def test_averaging_against_numpy_means(name):
    """_average_by_duration: a float32 ``out``; the pitch's float64 mean and the energy's
    float32 mean (numpy accumulates a float32 array in float32) against the restatement"""
    batch, ex = PR.case(name), PR.expected(name, True, True)
    for i in range(len(ex["D"])):
        if ex["status"][i]:
            continue
        D, durs = ex["D"][i], batch["durations"][i]
        pitch = PR.interpolate(batch["f0s"][i], D)[0]
        energy = batch["energies"][i][:D]
        assert energy.dtype == np.float32
        for f, values in ((0, pitch), (1, energy)):
            means, spans = _numpy_phoneme_means(values, durs)
            bound = np.array([0.0 if seg.size == 0 else PR.mean32_bound(seg) if f
                              else float(PR.held32_bound(seg.mean())) for seg in spans])
            ref = np.repeat(means, durs).astype(np.float64)
            got = ex["held"][f][i]
            assert ref.shape == got.shape
            assert (np.abs(ref - got) <= np.repeat(bound, durs)).all()
            assert (got.astype(np.float32).astype(np.float64) == got).all()


@pytest.mark.parametrize("pa,ea", PR.AVERAGING)
@pytest.mark.parametrize("name", ["ragged", "voicing", "constant", "D1", "D5", "D257"])
def test_statistics_and_z_against_sklearn(name, pa, ea):
    """StandardScaler.partial_fit per utterance, as the reference calls it, on the clean values
    as the reference holds them; then normalize_field's arithmetic with sklearn's statistics"""
    StandardScaler = pytest.importorskip("sklearn.preprocessing").StandardScaler
    batch, ex = PR.case(name), PR.expected(name, pa, ea)
    for gname, st in ex["stats"].items():
        idx = [i for i in range(len(ex["D"])) if batch["groups"][i] == gname
               and ex["status"][i] == 0]
        for f in (0, 1):
            f32 = f == 1 or pa
            scaler, zmin, zmax = StandardScaler(), np.inf, -np.inf
            held = [ex["held"][f][i].astype(np.float32) if f32 else ex["held"][f][i] for i in idx]
            for x in held:
                scaler.partial_fit(x[_numpy_clean(x)[2]][:, None])
            mean, std = scaler.mean_[0], scaler.scale_[0]
            N, K, S = ex["pooled"][gname][f]
            assert int(scaler.n_samples_seen_) == N == sum(ex["n_clean"][f][i] for i in idx)
            bm, bs = PR.stat_bounds(N, K, S, st[f][3])
            assert abs(mean - st[f][2]) <= bm and abs(std - st[f][3]) <= bs
            for i, x in zip(idx, held):
                z = (x - mean) / std
                assert z.dtype == np.float64
                z64 = ex["z64"][f][i]
                assert (np.abs(z.astype(np.float32) - z64) <= PR.z_bound(z64, bm, bs, st[f][3])).all()
                zmin, zmax = min(zmin, z.min()), max(zmax, z.max())
            assert abs(zmin - st[f][0]) <= PR.z_bound(st[f][0], bm, bs, st[f][3], f32=False)
            assert abs(zmax - st[f][1]) <= PR.z_bound(st[f][1], bm, bs, st[f][3], f32=False)


def test_constant_track_has_scale_one_and_zero_z():
    ex = PR.expected("constant", False, False)
    for f in (0, 1):
        zmin, zmax, mean, std = ex["stats"]["k"][f]
        assert std == 1.0 and zmin == zmax == 0.0 and mean == (220.0, 0.5)[f]
        assert not ex["z64"][f][0].any()
    ex = PR.expected("voicing", False, False)
    assert ex["rejected"] == [3, 6] and ex["status"][3] == PR.UNVOICED \
        and ex["status"][6] == PR.NONFINITE
    assert sorted(len([g for g in PR.case("voicing")["groups"] if g == n]) for n in "abc") \
        == [1, 2, 7]


def test_flagged_utterance_leaves_the_group_statistics_alone():
    batch = PR.case("voicing")
    keep = [i for i in range(len(batch["groups"])) if i not in (3, 6)]
    sub = {k: [v[i] for i in keep] for k, v in batch.items()}
    a, b = PR.run_batch(batch, True, False), PR.run_batch(sub, True, False)
    assert a["stats"] == b["stats"]


def test_export_refusals():
    """every call returns FS2_EINVAL before a launch (no device is touched)"""
    from fastspeech2 import _native, ops
    lib = _native.load()
    EINVAL, p = -1, 4096
    assert ops.PROSODY_MAX_D == PR.MAX_D
    assert (ops.PROSODY_NONFINITE, ops.PROSODY_UNVOICED, ops.PROSODY_EMPTY) == \
        (PR.NONFINITE, PR.UNVOICED, PR.EMPTY)

    def track(src=p, ss=p, sl=p, dur=p, do=p, to=p, B=1, D_max=16, trk=p, us=p, st=p):
        return lib.fs2_prosody_track(src, 1, ss, sl, dur, do, to, B, D_max, 1, 1, trk, us, st, None)

    assert track(B=0) == 0
    for kw in (dict(src=None), dict(ss=None), dict(sl=None), dict(dur=None), dict(do=None),
               dict(to=None), dict(trk=None), dict(us=None), dict(st=None), dict(B=-1),
               dict(D_max=0), dict(D_max=-5), dict(D_max=4097)):
        assert track(**kw) == EINVAL, kw
    assert track(B=0, D_max=4096) == 0

    def norm(trk=p, to=p, st=p, go=p, B=1, G=1, D_max=16, gs=p, z=p, umm=p):
        return lib.fs2_prosody_normalize(trk, to, st, None, go, B, G, D_max, gs, z, umm, None)

    assert norm(B=0) == 0
    for kw in (dict(trk=None), dict(to=None), dict(st=None), dict(go=None), dict(gs=None),
               dict(z=None), dict(umm=None), dict(B=-1), dict(G=-1), dict(G=0), dict(D_max=0),
               dict(D_max=4097)):
        assert norm(**kw) == EINVAL, kw
    for fn in (lib.fs2_prosody_stats, lib.fs2_prosody_minmax):
        assert fn(p, p, None, p, 0, p, None) == 0
        for args in ((None, p, p, p, 1, p), (p, None, p, p, 1, p), (p, p, p, None, 1, p),
                     (p, p, p, p, 1, None), (p, p, p, p, -1, p)):
            assert fn(*args, None) == EINVAL, args


def test_python_refusals():
    from fastspeech2 import prosody as P
    f0 = [np.full(20, 100.0), np.full(20, 100.0)]
    ok = [[5, 5], [10, 10]]
    assert P.check_alignment(f0, [20, 20], ok).tolist() == [10, 20]
    with pytest.raises(ValueError, match="utterance 1: negative duration -2"):
        P.check_alignment(f0, [20, 20], [[5, 5], [12, -2]])
    with pytest.raises(ValueError, match="utterance 0: the durations sum to 0"):
        P.check_alignment(f0, [20, 20], [[0, 0], [5]])
    with pytest.raises(ValueError, match="utterance 1: the durations sum to 21 frames, the F0"):
        P.check_alignment(f0, [30, 30], [[5], [21]])
    with pytest.raises(ValueError, match="utterance 0: .* the energy 9"):
        P.check_alignment(f0, [9, 20], ok)
    with pytest.raises(ValueError, match="utterance 1: 4097 frames"):
        P.check_alignment([f0[0], np.ones(5000)], [20, 5000], [[5], [4097]])
    assert P.check_alignment([np.ones(5000)], [5000], [[4096]]).tolist() == [4096]
    stage = P.ProsodyStage(True, False, device="cpu")
    e = [np.zeros(20, np.float32)] * 2
    with pytest.raises(ValueError, match="negative duration"):         # before any device use
        stage(f0, e, [[5, 5], [12, -2]], ["a", "a"])
    with pytest.raises(ValueError, match="one entry per utterance"):
        stage(f0, e, ok, ["a"])
    with pytest.raises(ValueError, match="energy_lengths"):
        stage(f0, e, ok, ["a", "a"], energy_lengths=[20, 20])
    with pytest.raises(RuntimeError, match="no CPU path"):              # never an eager fallback
        stage(f0, e, ok, ["a", "a"])
    import fastspeech2
    assert fastspeech2.ProsodyStage is P.ProsodyStage and fastspeech2.FeatureSet is P.FeatureSet
    assert fastspeech2.extract_features is P.extract_features


def _restated_feature_set(name, emotion, pa, ea, n_mels=5, seed=0):
    """build_feature_set on the restatement's tracks (a stub in place of the kernels)"""
    from fastspeech2 import prosody as P
    batch, ex = PR.case(name), PR.expected(name, pa, ea)
    B = len(ex["D"])
    rng = np.random.default_rng(seed)
    phs = ["AA1", "B", "sil", "", "ZH", "sp"]
    mels = [rng.standard_normal((n_mels, ex["D"][i] + 3)).astype(np.float32) for i in range(B)]
    phones = [[phs[k % len(phs)] for k in range(len(batch["durations"][i]))] for i in range(B)]
    meta = [{"speaker": f"spk{batch['groups'][i]}", "emotion": emotion, "audio_id": f"{i:04d}",
             "audio_path": f"/corpus/{i}.wav", "transcript": f" <noise> words {i} ",
             "textgrid_path": f"/tg/{i}.TextGrid"} for i in range(B)]
    z32 = [[None if ex["z64"][f][i] is None else ex["z64"][f][i].astype(np.float32)
            for i in range(B)] for f in (0, 1)]
    stats = {(f"spk{g}", emotion): {"pitch": list(s[0]), "energy": list(s[1])}
             for g, s in ex["stats"].items()}
    fs = P.build_feature_set(mels, z32[0], z32[1], batch["durations"], phones, meta, stats,
                             ex["rejected"], speakers=["spka", "spkb", "spkc"],
                             emotions=["neutral", "angry"], noise_symbol=" <noise> ")
    return fs, mels, z32, ex


def test_feature_set_round_trip_through_the_dataset(tmp_path):
    from fastspeech2.dataset import FastSpeech2Dataset
    fs, mels, z32, ex = _restated_feature_set("voicing", "angry", True, False)
    keep = [i for i in range(10) if i not in ex["rejected"]]
    assert len(fs) == 8 and fs.rejected == [3, 6]
    for k, i in enumerate(keep):
        it = fs[k]
        assert it["mel"].shape == (5, ex["D"][i]) and it["mel"].dtype == torch.float32
        assert np.array_equal(it["mel"].numpy(), mels[i][:, :ex["D"][i]])
        assert it["pitch"].dtype == torch.float32 and it["pitch"].shape == (ex["D"][i],)
        assert np.array_equal(it["pitch"].numpy(), z32[0][i])
        assert np.array_equal(it["energy"].numpy(), z32[1][i])
        assert it["duration"].dtype == torch.int64 and it["phoneme"].dtype == torch.int64
        assert it["text"] == f"words {i}" and it["audio_path"] == f"/corpus/{i}.wav"
        assert int(it["emotion"]) == 1 and int(it["speaker"]) == "abc".index(
            PR.case("voicing")["groups"][i])
    root = str(tmp_path / "pre")
    paths = fs.write(root)
    assert [os.path.relpath(p, root) for p in paths][:2] == [
        os.path.join("spkc", "angry_0000.npz"), os.path.join("spka", "angry_0001.npz")]
    with open(os.path.join(root, "fs2_train.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    ds = FastSpeech2Dataset(root, " <noise> ", ["spka", "spkb", "spkc"], ["neutral", "angry"])
    assert len(ds) == len(fs)
    for k in range(len(fs)):
        a, b = fs[k], ds[k]
        assert set(a) == set(b)
        for key in a:
            if torch.is_tensor(a[key]):
                assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key
            else:
                assert a[key] == b[key], key
    raw = np.load(paths[0], allow_pickle=False)
    assert set(raw.files) == {"phones", "emotion", "speaker", "audio_id", "audio_path",
                              "transcript", "textgrid_path", "mel", "pitch", "energy", "durations"}
    # stats.json: a second call with another emotion merges per speaker (preprocess.py:162-168)
    first = json.load(open(os.path.join(root, "stats.json")))
    assert first == fs.stats and set(first) == {"spka", "spkb", "spkc"}
    assert first["spkc"]["angry"]["pitch"] == list(ex["stats"]["c"][0])
    fs2, _, _, ex2 = _restated_feature_set("voicing", "neutral", False, True)
    more = fs2.write(root)
    assert len(more) == 8 and not set(more) & set(paths) and all(os.path.exists(q) for q in paths)
    both = json.load(open(os.path.join(root, "stats.json")))
    for g in "abc":
        assert both[f"spk{g}"]["angry"] == first[f"spk{g}"]["angry"]
        assert both[f"spk{g}"]["neutral"] == {"pitch": list(ex2["stats"][g][0]),
                                              "energy": list(ex2["stats"][g][1])}
        assert both[f"spk{g}"]["neutral"] != both[f"spk{g}"]["angry"]
