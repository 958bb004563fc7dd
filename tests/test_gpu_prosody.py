"""GPU: the prosody feature stage -- fs2_prosody_track / _stats / _normalize / _minmax, each
alone through fastspeech2.ops, against tests/prosody_restatement.py in float64 (pinned on the CPU
by tests/test_prosody_host.py), then ProsodyStage and extract_features on top of them.

Every output sits inside a buffer of 0x5A bytes that must come back untouched around it, and
every float input is followed by NaNs (ints by -999); the utterances' inputs are longer than D
and packed back to back, so a read past D or past an utterance shows up as a wrong value.  The
cases, their fence condition and the bounds are the restatement's; the observed share of each
bound goes through ``parity_log``.
"""
import numpy as np
import pytest
import torch

import prosody_restatement as PR

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
    fillv = np.nan if arr.dtype.kind == "f" else -999
    pad = lambda k: np.full(k, fillv, arr.dtype)
    t = torch.from_numpy(np.concatenate([pad(lead), arr, pad(TAIL)]))
    return t.to(cuda)[lead:lead + arr.size]


def _cum(v):
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)


class Layout:
    """a batch ordered by group, its offsets on the host and the device"""

    def __init__(self, cuda, batch):
        names = list(dict.fromkeys(batch["groups"]))
        self.order = sorted(range(len(batch["groups"])), key=lambda i: names.index(batch["groups"][i]))
        self.names = names
        self.n, self.G = len(self.order), len(names)
        durs = [np.asarray(batch["durations"][i], np.int64) for i in self.order]
        self.D = np.array([int(d.sum()) for d in durs], np.int64)
        self.trk_off = _cum(self.D)
        self.group_off = _cum(np.bincount([names.index(batch["groups"][i]) for i in self.order],
                                          minlength=self.G))
        self.D_max = int(self.D.max())
        self.dur = _in(cuda, np.concatenate(durs))
        self.dur_off = _in(cuda, _cum([d.size for d in durs]))
        self.trk_off_d = _in(cuda, self.trk_off)
        self.group_off_d = _in(cuda, self.group_off)
        self.src = []
        for key, dt in (("f0s", np.float64), ("energies", np.float32)):
            arrs = [np.asarray(batch[key][i], dt) for i in self.order]      # longer than D
            off = _cum([a.size for a in arrs])
            self.src.append((_in(cuda, np.concatenate(arrs), lead=TAIL), _in(cuda, off[:-1]),
                             _in(cuda, np.array([a.size for a in arrs], np.int64))))


def run_track(cuda, lay, f, averaging):
    from fastspeech2 import ops
    src, start, length = lay.src[f]
    track = Out(cuda, int(lay.trk_off[-1]), torch.float64)
    ustat, status = Out(cuda, lay.n * 5, torch.float64), Out(cuda, lay.n, torch.int32)
    ops.prosody_track(src, start, length, lay.dur, lay.dur_off, lay.trk_off_d, lay.n, lay.D_max,
                      f == 0, averaging, track.t, ustat.t, status.t)
    torch.cuda.synchronize()
    return track, ustat, status


def run_all(cuda, batch, pa, ea):
    """the eight launches in ProsodyStage's order; every output as numpy, per field"""
    from fastspeech2 import ops
    lay = Layout(cuda, batch)
    n, G, total = lay.n, lay.G, int(lay.trk_off[-1])
    tr = [run_track(cuda, lay, f, avg) for f, avg in ((0, pa), (1, ea))]
    gstat = [Out(cuda, G * 4, torch.float64) for _ in (0, 1)]
    z = [Out(cuda, total, torch.float32) for _ in (0, 1)]
    umm = [Out(cuda, n * 2, torch.float64) for _ in (0, 1)]
    for f in (0, 1):
        ops.prosody_stats(tr[f][1].t, tr[f][2].t, tr[1 - f][2].t, lay.group_off_d, G, gstat[f].t)
    for f in (0, 1):
        ops.prosody_normalize(tr[f][0].t, lay.trk_off_d, tr[f][2].t, tr[1 - f][2].t,
                              lay.group_off_d, n, G, lay.D_max, gstat[f].t, z[f].t, umm[f].t)
    for f in (0, 1):
        ops.prosody_minmax(umm[f].t, tr[f][2].t, tr[1 - f][2].t, lay.group_off_d, G, gstat[f].t)
    torch.cuda.synchronize()
    return lay, {"track": [tr[f][0].np() for f in (0, 1)],
                 "ustat": [tr[f][1].np().reshape(n, 5) for f in (0, 1)],
                 "status": [tr[f][2].np() for f in (0, 1)],
                 "gstat": [gstat[f].np().reshape(G, 4) for f in (0, 1)],
                 "z": [z[f].np() for f in (0, 1)], "umm": [umm[f].np().reshape(n, 2) for f in (0, 1)]}


def check_tracks(lay, got, batch, ex, pa, ea, log):
    """held tracks, status, n_clean, quartiles and the utterance triples of both fields"""
    for k, i in enumerate(lay.order):
        a, b = lay.trk_off[k], lay.trk_off[k + 1]
        assert b - a == ex["D"][i]
        st = got["status"][0][k] | got["status"][1][k]
        assert st == ex["status"][i], (i, st)
        for f, avg in ((0, pa), (1, ea)):
            held, x = got["track"][f][a:b], ex["held"][f][i]
            if got["status"][f][k]:
                # the values as read; no statistics
                assert np.array_equal(held, np.asarray(batch[("f0s", "energies")[f]][i],
                                                       np.float64)[:b - a], equal_nan=True)
                assert not got["ustat"][f][k].any()
                continue
            if f == 1 or avg:
                bound = PR.held32_bound(x)
                assert (held.astype(np.float32).astype(np.float64) == held).all()
                key = "held32_share_of_bound"
            else:
                bound = np.full(x.size, PR.interp_bound(batch["f0s"][i], x.size))
                key = "interp_share_of_bound"
            err = np.abs(held - x)
            assert (err <= bound).all(), (i, f)
            log[key] = max(log.get(key, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
            if st:
                continue                       # the other field is flagged: the triple is unused
            n_clean, mean, m2, q1, q3 = got["ustat"][f][k]
            assert n_clean == ex["n_clean"][f][i]                       # integers
            r1, r3 = ex["q"][f][i]
            qb = 8 * PR.U64 * float(np.abs(x).max())    # the lerp: three roundings of <= 2 max|x|
            assert abs(q1 - r1) <= qb and abs(q3 - r3) <= qb
            rn, rmean, rm2 = PR.triple(x)
            S = float(np.abs(x).max())
            bm, _ = PR.stat_bounds(rn, 1, S, 1.0)
            assert abs(mean - rmean) <= bm
            assert abs(m2 - rm2) <= 8 * (rn + 4) * PR.U64 * S * S * rn
            log["utt_mean_share_of_bound"] = max(log.get("utt_mean_share_of_bound", 0.0),
                                                 abs(mean - rmean) / bm)


def check_groups(lay, got, ex, log):
    """mean, std, min, max per group and z per utterance, both fields"""
    for g, name in enumerate(lay.names):
        for f in (0, 1):
            gmin, gmax, mean, std = got["gstat"][f][g]
            if name not in ex["stats"]:
                assert (mean, std) == (0.0, 1.0) and gmin == np.inf and gmax == -np.inf
                continue
            rmin, rmax, rmean, rstd = ex["stats"][name][f]
            N, K, S = ex["pooled"][name][f]
            bm, bs = PR.stat_bounds(N, K, S, rstd)
            assert abs(mean - rmean) <= bm and abs(std - rstd) <= bs
            assert abs(gmin - rmin) <= PR.z_bound(rmin, bm, bs, rstd, f32=False)
            assert abs(gmax - rmax) <= PR.z_bound(rmax, bm, bs, rstd, f32=False)
            log["mean_share_of_bound"] = max(log.get("mean_share_of_bound", 0.0),
                                             abs(mean - rmean) / bm)
            log["std_share_of_bound"] = max(log.get("std_share_of_bound", 0.0),
                                            abs(std - rstd) / bs)
            for k in range(lay.group_off[g], lay.group_off[g + 1]):
                i = lay.order[k]
                z = got["z"][f][lay.trk_off[k]:lay.trk_off[k + 1]]
                if ex["status"][i]:
                    assert not z.view(np.int32).any()                 # +0.0
                    assert got["umm"][f][k].tolist() == [np.inf, -np.inf]
                    continue
                z64 = ex["z64"][f][i]
                zb = PR.z_bound(z64, bm, bs, rstd)
                err = np.abs(z.astype(np.float64) - z64)
                assert (err <= zb).all(), (name, f, i)
                log["z_share_of_bound"] = max(log.get("z_share_of_bound", 0.0),
                                              float((err / zb).max()))


@pytest.mark.parametrize("D", PR.D_EDGES)
def test_each_length_as_a_launch_of_its_own(cuda, D, parity_log):
    """G = 1 with one utterance of exactly D frames: the percentile indices for tiny n, the
    wave, block and power-of-two edges of the reductions and the sort; all four averaging
    combinations; inputs longer than D"""
    batch, log = PR.case(f"D{D}"), {}
    for pa, ea in PR.AVERAGING:
        ex = PR.expected(f"D{D}", pa, ea)
        lay, got = run_all(cuda, batch, pa, ea)
        assert lay.D.tolist() == [D] and ex["rejected"] == []
        check_tracks(lay, got, batch, ex, pa, ea, log)
        check_groups(lay, got, ex, log)
    parity_log[f"prosody_D{D}"] = log


@pytest.mark.parametrize("pa,ea", PR.AVERAGING)
@pytest.mark.parametrize("name", ["ragged", "voicing", "constant"])
def test_batches_against_the_restatement(cuda, name, pa, ea, parity_log):
    """ragged: every length in one launch.  voicing: G = 3 with 1 / 2 / 7 utterances, every
    voicing pattern, zeros in the durations, phonemes across the 64 / 256 frame boundaries, an
    unvoiced and a NaN utterance flagged and left out of their group.  constant: scale 1, z = 0.
    A second run gives the same bits everywhere."""
    batch, ex, log = PR.case(name), PR.expected(name, pa, ea), {}
    lay, got = run_all(cuda, batch, pa, ea)
    check_tracks(lay, got, batch, ex, pa, ea, log)
    check_groups(lay, got, ex, log)
    assert sorted(lay.order[k] for k in range(lay.n)
                  if got["status"][0][k] | got["status"][1][k]) == ex["rejected"]
    if name == "constant":
        for f in (0, 1):
            assert got["gstat"][f][0].tolist() == [0.0, 0.0, (220.0, 0.5)[f], 1.0]
            assert not got["z"][f].view(np.int32).any()
    if name == "voicing":
        assert ex["rejected"] == [3, 6]
    _, again = run_all(cuda, batch, pa, ea)
    for key in got:
        for f in (0, 1):
            assert got[key][f].tobytes() == again[key][f].tobytes(), (key, f)
    parity_log[f"prosody_{name}_{int(pa)}{int(ea)}"] = log


def test_statistics_kernels_alone(cuda, parity_log):
    """fs2_prosody_stats, _normalize and _minmax on the restatement's own triples and tracks:
    G = 3 with 1 / 2 / 7 utterances, two of them flagged through either status array"""
    from fastspeech2 import ops
    batch, ex = PR.case("voicing"), PR.expected("voicing", True, False)
    lay = Layout(cuda, batch)
    n, G = lay.n, lay.G
    ustat, st0, st1 = np.zeros((2, n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k, i in enumerate(lay.order):
        st0[k], st1[k] = ex["status"][i] & PR.UNVOICED, ex["status"][i] & PR.NONFINITE
        for f in (0, 1):
            # a flagged utterance's triple must not be read into the merge: poison it
            ustat[f, k, :3] = (7.0, 1e30, 1e30) if ex["status"][i] else PR.triple(ex["held"][f][i])
    got = {"gstat": [], "z": [], "umm": []}
    s0, s1 = _in(cuda, st0), _in(cuda, st1)
    for f in (0, 1):
        gstat, z = Out(cuda, G * 4, torch.float64), Out(cuda, int(lay.trk_off[-1]), torch.float32)
        umm = Out(cuda, n * 2, torch.float64)
        track = _in(cuda, np.concatenate([ex["held"][f][i] for i in lay.order]))
        ops.prosody_stats(_in(cuda, ustat[f]), s0, s1, lay.group_off_d, G, gstat.t)
        ops.prosody_normalize(track, lay.trk_off_d, s0, s1, lay.group_off_d, n, G, lay.D_max,
                              gstat.t, z.t, umm.t)
        ops.prosody_minmax(umm.t, s0, s1, lay.group_off_d, G, gstat.t)
        torch.cuda.synchronize()
        got["gstat"].append(gstat.np().reshape(G, 4))
        got["z"].append(z.np())
        got["umm"].append(umm.np().reshape(n, 2))
    log = {}
    check_groups(lay, got, ex, log)
    parity_log["prosody_statistics_alone"] = log


def test_span_longer_than_the_source_is_zero_filled(cuda):
    """a caller whose lengths disagree (10 frames of durations and of track, 6 of source): the
    six frames are held, the rest of the span is +0.0, nothing is read past the source"""
    from fastspeech2 import ops
    e = np.arange(1, 7, dtype=np.float32) / 8
    i64 = lambda *v: _in(cuda, np.array(v, np.int64))
    track, ustat, status = Out(cuda, 10, torch.float64), Out(cuda, 5, torch.float64), \
        Out(cuda, 1, torch.int32)
    ops.prosody_track(_in(cuda, e), i64(0), i64(6), i64(4, 6), i64(0, 2), i64(0, 10), 1, 16,
                      False, False, track.t, ustat.t, status.t)
    torch.cuda.synchronize()
    got = track.np()
    assert got[:6].tolist() == e.tolist() and not got[6:].view(np.int64).any()
    assert status.np()[0] == 0 and ustat.np()[0] == 6


def _stage_inputs(cuda, batch, padded):
    if not padded:
        return batch["energies"], None
    lens = [len(e) for e in batch["energies"]]
    e = torch.full((len(lens), max(lens) + 3), float("nan"))
    for i, v in enumerate(batch["energies"]):
        e[i, :lens[i]] = torch.from_numpy(v)
    return e.to(cuda), lens


@pytest.mark.parametrize("padded", [False, True], ids=["list", "padded"])
@pytest.mark.parametrize("pa,ea", [(False, False), (True, True)])
def test_stage_against_the_restatement(cuda, pa, ea, padded, parity_log):
    """ProsodyStage on the voicing case plus an utterance the host skips (one voiced frame in
    the whole F0 track): lengths, status, rejected as integers; statistics and z within their
    bounds; the same bits on a second call"""
    from fastspeech2.prosody import ProsodyStage, HOST_SKIPPED
    batch = PR.merge(PR.case("voicing"), {"f0s": [np.where(np.arange(50) == 7, 130.0, 0.0)],
                                          "energies": [PR.energy_track(np.random.default_rng(1), 50)],
                                          "durations": [np.full(10, 4, np.int64)], "groups": ["a"]})
    ex = PR.run_batch(batch, pa, ea)
    assert ex["rejected"] == [3, 6, 10] and ex["status"][10] == HOST_SKIPPED == PR.HOST_SKIPPED
    stage = ProsodyStage(pa, ea, device=cuda)
    energies, lens = _stage_inputs(cuda, batch, padded)
    res = stage(batch["f0s"], energies, batch["durations"], batch["groups"], energy_lengths=lens)
    assert res.lengths.tolist() == ex["D"] and res.status.tolist() == ex["status"].tolist()
    assert res.rejected == ex["rejected"] and 10 not in res.order.tolist()
    assert res.pitch.dtype == res.energy.dtype == torch.float32 and res.pitch.is_cuda
    assert set(res.stats) == set(ex["stats"]) == {"a", "b", "c"}
    zs, log = (res.pitch.cpu().numpy(), res.energy.cpu().numpy()), {}
    for name, s in res.stats.items():
        for f, key in enumerate(("pitch", "energy")):
            gmin, gmax, mean, std = s[key]
            rmin, rmax, rmean, rstd = ex["stats"][name][f]
            bm, bs = PR.stat_bounds(*ex["pooled"][name][f], rstd)
            assert abs(mean - rmean) <= bm and abs(std - rstd) <= bs
            assert abs(gmin - rmin) <= PR.z_bound(rmin, bm, bs, rstd, f32=False)
            assert abs(gmax - rmax) <= PR.z_bound(rmax, bm, bs, rstd, f32=False)
            for k, i in enumerate(res.order):
                if batch["groups"][i] != name or ex["status"][i]:
                    continue
                z = zs[f][res.offsets[k]:res.offsets[k + 1]].astype(np.float64)
                err, zb = np.abs(z - ex["z64"][f][i]), PR.z_bound(ex["z64"][f][i], bm, bs, rstd)
                assert (err <= zb).all()
                log["z_share_of_bound"] = max(log.get("z_share_of_bound", 0.0),
                                              float((err / zb).max()))
    again = stage(batch["f0s"], energies, batch["durations"], batch["groups"], energy_lengths=lens)
    assert torch.equal(res.pitch, again.pitch) and torch.equal(res.energy, again.energy)
    assert res.stats == again.stats
    parity_log[f"prosody_stage_{int(pa)}{int(ea)}_{'padded' if padded else 'list'}"] = log


def test_extract_features_feeds_the_device_store(cuda):
    """waveforms -> MelFrontEnd -> ProsodyStage -> FeatureSet: the items are the restatement's
    on the front end's own energy, and FS2DeviceStore(feature_set) collates a batch bit-equal
    to GpuCollate on the same items"""
    from fastspeech2.audio import MelFrontEnd
    from fastspeech2.dataset import GpuCollate
    from fastspeech2.device_store import FS2DeviceStore
    from fastspeech2.prosody import extract_features
    audio = dict(sampling_rate=16000, hop_length=64, win_length=256, n_fft=256, n_mels=20,
                 f_min=0.0, f_max=8000.0)
    rng = np.random.default_rng(5)
    frames = [40, 75, 33, 64, 51]
    wavs = [(0.1 * rng.standard_normal(64 * T + 17) + 0.3 * np.sin(np.arange(64 * T + 17) * 0.05))
            .astype(np.float32) for T in frames]
    durations = [PR.durations_of(T - 2, "random", rng) for T in frames]
    f0s = [PR.f0_track(rng, T + 1, "runs") for T in frames]
    f0s[2] = np.zeros(frames[2] + 1)                       # skipped on the host
    phs = ["AA1", "B", "sil", "ZH", "sp"]
    phones = [[phs[k % 5] for k in range(len(d))] for d in durations]
    meta = [{"speaker": "s0" if i < 3 else "s1", "emotion": "happy", "audio_id": str(i),
             "audio_path": f"{i}.wav", "transcript": f"text {i}"} for i in range(5)]
    fs = extract_features(wavs, f0s, durations, phones, meta, audio, True, False, device=cuda)
    assert len(fs) == 4 and fs.rejected == [2] and set(fs.stats) == {"s0", "s1"}
    mel, energy, _ = MelFrontEnd(**audio, device=cuda)([torch.from_numpy(w) for w in wavs],
                                                       layout="bct")
    ex = PR.run_batch({"f0s": f0s, "energies": [energy[i, :frames[i] + 1].cpu().numpy()
                                                for i in range(5)],
                       "durations": durations, "groups": [m["speaker"] for m in meta]}, True, False)
    keep = [0, 1, 3, 4]
    for k, i in enumerate(keep):
        it, D = fs[k], frames[i] - 2
        assert it["mel"].shape == (20, D) and torch.equal(it["mel"], mel[i, :, :D].cpu())
        assert it["pitch"].shape == it["energy"].shape == (D,) and not it["pitch"].is_cuda
        for f, key in enumerate(("pitch", "energy")):
            rstd = ex["stats"][meta[i]["speaker"]][f][3]
            bm, bs = PR.stat_bounds(*ex["pooled"][meta[i]["speaker"]][f], rstd)
            err = np.abs(it[key].numpy().astype(np.float64) - ex["z64"][f][i])
            assert (err <= PR.z_bound(ex["z64"][f][i], bm, bs, rstd)).all()
    store = FS2DeviceStore(fs, device=cuda)
    got = store.collate([2, 0, 3, 1])
    ref = GpuCollate(cuda)([fs[i] for i in (2, 0, 3, 1)])
    for a, b in zip(got, ref):
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a, b)
        else:
            assert a == b
