"""Prosody feature stage at the reference size on 1 MI355X: one corpus slice of 10 (speaker,
emotion) groups of 350 seeded synthetic utterances of 2 to 6 s (16 kHz, hop 256: 126 to 376
frames), F0 tracks with unvoiced runs and phoneme alignments generated on the host, averaging off
(the reference yaml's default):

  a  cpu     what a user runs today, on tracks already in host memory: per utterance
             ``scipy.interpolate.interp1d``, ``np.percentile`` fences, ``StandardScaler
             .partial_fit``, then ``(x - mean) / std`` and its min / max per group, in float64 /
             float32 as the reference holds them.  The three ``.npz`` rewrites per file that the
             reference's ``normalize_field`` adds are left out, so this arm is faster than the
             reference itself;
  b  gpu     ``ProsodyStage.__call__`` on the same host arrays: one upload, eight launches, ended
             by its own read-back of the statistics.

Timed as interleaved pairs (a b a b ...) after warm-up.  Also reported: the eight launches' own
time between device events (inputs resident; the two track kernels also with phoneme averaging
on), the largest difference between the arms' statistics and z, and ``extract_features`` end to end (waveforms in host memory to a
``FeatureSet`` of CPU tensors) against ``MelFrontEnd`` alone on the same waveforms, on a tenth of
the slice.  Not measured: other slice sizes, real F0 tracks, reading or writing files.

    python tools/prosody_bench.py [--pairs 10] [--warmup 2] [--groups 10] [--per-group 350]
Prints one JSON line (and writes it to --out, default profiles/prosody_bench.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))

import numpy as np
import torch

AUDIO = dict(sampling_rate=16000, hop_length=256, win_length=1024, n_fft=1024, n_mels=80,
             f_min=0.0, f_max=8000.0)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def make_slice(G, per_group, seed=0):
    """samples per utterance, F0, energy, durations and group ids"""
    r = np.random.default_rng(seed)
    samples, f0s, ens, durs, groups = [], [], [], [], []
    for g in range(G):
        for _ in range(per_group):
            n = int(r.integers(2 * 16000, 6 * 16000 + 1))
            T = 1 + n // 256
            t = np.arange(T)
            f0 = 170.0 + 60.0 * np.sin(t / 17.0 + r.uniform(0, 6)) + r.uniform(-25, 25, T)
            pos = 0
            while pos < T:                       # unvoiced runs
                k = int(r.integers(3, 40))
                if r.random() < 0.35:
                    f0[pos:pos + k] = 0.0
                pos += k
            f0[int(r.integers(0, T - 1))] = 150.0
            f0[T - 2] = 160.0
            d = []
            while sum(d) < T - 1:
                d.append(int(min(r.integers(1, 24), T - 1 - sum(d))))
            e = np.abs(np.sin(t / 11.0 + r.uniform(0, 3))) * 0.6 + r.uniform(0, 0.4, T)
            samples.append(n)
            f0s.append(f0)
            ens.append(e.astype(np.float32))
            durs.append(np.asarray(d, np.int64))
            groups.append(g)
    return samples, f0s, ens, durs, groups


def inside_fences(track):
    """the values of a track within 1.5 interquartile ranges of numpy's quartiles, as a column"""
    lower, upper = np.percentile(track, (25, 75))
    reach = 1.5 * (upper - lower)
    keep = np.logical_and(track >= lower - reach, track <= upper + reach)
    return track[keep][:, None]


def cpu_arm(f0s, ens, durs, groups):
    """arm a; returns {group: {"pitch": [...], "energy": [...]}} and the float32 z per utterance"""
    from scipy.interpolate import interp1d
    from sklearn.preprocessing import StandardScaler
    stats, zs = {}, [None] * len(f0s)
    for g in dict.fromkeys(groups):
        idx = [i for i in range(len(groups)) if groups[i] == g]
        scalers, held = (StandardScaler(), StandardScaler()), {}
        for i in idx:
            D = int(durs[i].sum())
            voiced = np.flatnonzero(f0s[i][:D])
            y = f0s[i][voiced]
            held[i] = (interp1d(voiced, y, bounds_error=False, fill_value=(y[0], y[-1]))(
                np.arange(D)), ens[i][:D])
            for f in (0, 1):
                scalers[f].partial_fit(inside_fences(held[i][f]))
        out = []
        for f in (0, 1):
            mean, std = scalers[f].mean_[0], scalers[f].scale_[0]
            lo, hi = np.inf, -np.inf
            for i in idx:
                z = (held[i][f] - mean) / std
                lo, hi = min(lo, z.min()), max(hi, z.max())
                zs[i] = (zs[i] or ()) + (z.astype(np.float32),)
            out.append([float(lo), float(hi), float(mean), float(std)])
        stats[g] = {"pitch": out[0], "energy": out[1]}
    return stats, zs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--per-group", type=int, default=350)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prosody_bench needs a GPU: a CPU timing says nothing about it")
    from fastspeech2 import _native, ops
    from fastspeech2.audio import MelFrontEnd
    from fastspeech2.prosody import ProsodyStage, extract_features
    _native.load()
    dev = torch.device("cuda", 0)
    samples, f0s, ens, durs, groups = make_slice(args.groups, args.per_group)
    B = len(f0s)
    stage = ProsodyStage(False, False, device=dev)

    res = {"metric": "F0 / energy tracks in host memory -> standardised tracks and group "
                     "statistics, ms per slice (host clock; the GPU arm ends with its own "
                     "read-back)"}

    def run_b():
        out = stage(f0s, ens, durs, groups)
        torch.cuda.synchronize()
        return out

    # the arms agree
    (sa, za), rb = cpu_arm(f0s, ens, durs, groups), run_b()
    assert rb.rejected == [] and set(rb.stats) == set(sa)
    ds = max(abs(a - b) / max(abs(a), 1e-30) for g in sa for k in ("pitch", "energy")
             for a, b in zip(sa[g][k], rb.stats[g][k]))
    zb = (rb.pitch.cpu().numpy(), rb.energy.cpu().numpy())
    dz = max(float(np.abs(zb[f][rb.offsets[k]:rb.offsets[k + 1]] - za[i][f]).max())
             for k, i in enumerate(rb.order) for f in (0, 1))
    res["max_rel_diff_stats"], res["max_abs_diff_z"] = ds, dz

    for _ in range(args.warmup):
        cpu_arm(f0s, ens, durs, groups)
        run_b()
    ta, tb = [], []
    for _ in range(args.pairs):
        t0 = time.perf_counter()
        cpu_arm(f0s, ens, durs, groups)
        t1 = time.perf_counter()
        run_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    res["a_cpu_ms"], res["b_gpu_ms"] = spread(ta), spread(tb)
    res["ratio_b_over_a"] = spread([b / a for a, b in zip(ta, tb)])

    # the launches' own time: everything resident, device events around the eight launches
    D = np.array([int(d.sum()) for d in durs], np.int64)
    cum = lambda v: torch.from_numpy(np.concatenate([[0], np.cumsum(v)]).astype(np.int64)).to(dev)
    trk_off, dur_off = cum(D), cum([d.size for d in durs])
    group_off = cum(np.bincount(groups, minlength=args.groups))
    dur = torch.from_numpy(np.concatenate(durs)).to(dev)
    lens = torch.from_numpy(D).to(dev)
    src = (torch.from_numpy(np.concatenate([f[:n] for f, n in zip(f0s, D)])).to(dev),
           torch.from_numpy(np.concatenate([e[:n] for e, n in zip(ens, D)])).to(dev))
    total, G, D_max = int(D.sum()), args.groups, int(D.max())
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    track, ustat, umm, gstat = f64(2, total), f64(2, B, 5), f64(2, B, 2), f64(2, G, 4)
    st = torch.empty(2, B, dtype=torch.int32, device=dev)
    z = torch.empty(2, total, dtype=torch.float32, device=dev)
    kt = {"track": [], "stats": [], "normalize": [], "minmax": [], "all": [], "track_averaged": []}
    for it in range(args.warmup + args.pairs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        for f in (0, 1):
            ops.prosody_track(src[f], trk_off[:-1], lens, dur, dur_off, trk_off, B, D_max, f == 0,
                              False, track[f], ustat[f], st[f])
        ev[1].record()
        for f in (0, 1):
            ops.prosody_stats(ustat[f], st[f], st[1 - f], group_off, G, gstat[f])
        ev[2].record()
        for f in (0, 1):
            ops.prosody_normalize(track[f], trk_off, st[f], st[1 - f], group_off, B, G, D_max,
                                  gstat[f], z[f], umm[f])
        ev[3].record()
        for f in (0, 1):
            ops.prosody_minmax(umm[f], st[f], st[1 - f], group_off, G, gstat[f])
        ev[4].record()
        torch.cuda.synchronize()
        # the track kernels with phoneme averaging on (one thread sums a phoneme), on their own
        av = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        av[0].record()
        for f in (0, 1):
            ops.prosody_track(src[f], trk_off[:-1], lens, dur, dur_off, trk_off, B, D_max, f == 0,
                              True, track[f], ustat[f], st[f])
        av[1].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            kt["track_averaged"].append(av[0].elapsed_time(av[1]) * 1e3)
            for k, name in enumerate(("track", "stats", "normalize", "minmax")):
                kt[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
            kt["all"].append(ev[0].elapsed_time(ev[4]) * 1e3)
    res["kernels_us_both_fields"] = {k: spread(v) for k, v in kt.items()}

    # extract_features end to end against MelFrontEnd alone, on a tenth of the slice
    sub = list(range(0, B, 10))
    r = np.random.default_rng(1)
    wavs = [torch.from_numpy((0.1 * r.uniform(-1, 1, samples[i])).astype(np.float32)) for i in sub]
    meta = [{"speaker": f"s{groups[i]}", "emotion": "e", "audio_id": str(i), "audio_path": "",
             "transcript": ""} for i in sub]
    phones = [["AA1"] * durs[i].size for i in sub]
    fe = MelFrontEnd(**AUDIO, device=dev)

    def run_fe():
        out = fe(wavs, layout="bct")
        torch.cuda.synchronize()
        return out

    def run_x():
        return extract_features(wavs, [f0s[i] for i in sub], [durs[i] for i in sub], phones, meta,
                                AUDIO, False, False, device=dev)

    assert len(run_x()) == len(sub)
    run_fe()
    tf, tx = [], []
    for _ in range(max(3, args.pairs // 2)):
        t0 = time.perf_counter()
        run_fe()
        t1 = time.perf_counter()
        run_x()
        t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3)
        tx.append((t2 - t1) * 1e3)
    res["melfrontend_alone_ms"], res["extract_features_ms"] = spread(tf), spread(tx)
    res["extract_features_utterances"] = len(sub)

    res["slice"] = {"groups": G, "utterances": B, "frames": total, "D_max": D_max,
                    "pitch_averaging": False, "energy_averaging": False}
    res["pairs"], res["warmup"] = args.pairs, args.warmup
    res["note"] = ("synthetic F0 and alignments; arm a leaves out the reference's three .npz "
                   "rewrites per file; kernel times between device events include the launches; "
                   "extract_features ends with CPU tensors (mel copied back); not measured: "
                   "other slice sizes, real F0, file I/O")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
