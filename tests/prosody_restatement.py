"""The prosody feature stage restated in numpy float64, with the case tables and the error bounds
the CPU and GPU tests share (tests/test_prosody_host.py pins every function below against scipy,
numpy and sklearn; tests/test_gpu_prosody.py compares the kernels of csrc/prosody.hip with it).

What is restated (emo_rank_tts/rank_model/preprocess.py:104-168): the track is the first
D = sum(durations) frames; pitch is interpolated over its zero frames with the two-point formula
``slope * (t - lo) + y_lo``, ``slope = (y_hi - y_lo) / (hi - lo)``, the first / last voiced value
outside the voiced range, voiced frames untouched; an averaged track holds, per phoneme, the
float64 mean of its frames (summed in frame order) rounded once to float32; energy is float32 to
begin with.  The held values are float64 numbers (exactly float32-representable where the
reference holds float32).  Quartiles are np.percentile's linear method, ``a + (b - a) g`` and
``b - (b - a) (1 - g)`` for ``g >= 0.5`` at the virtual index ``(n - 1) q``; the clean set is
``q1 - 1.5 iqr <= x <= q3 + 1.5 iqr``.  A group's mean and variance are those of its utterances'
pooled clean values (here with math.fsum, i.e. to within one rounding), the scale is
``sqrt(var)``, or 1 under sklearn's constant-feature rule; ``z = (x - mean) / scale``.

Status words: NONFINITE (a NaN or infinity inside D), UNVOICED (pitch without a voiced frame
inside D).  A flagged utterance is left out of both fields' statistics.

Bounds (u64 = 2^-53, u32 = 2^-24; none of them is tuned to the kernels, and the host test shows
that scipy / numpy / sklearn themselves sit inside each):

* interpolated values, ``interp_bound``: the two-point formula is four operations.  With
  M = max |voiced value|: the difference and the quotient give the slope a relative error of
  2 u64, the product 3 u64 on a magnitude of at most 2 M, the sum one more rounding of a result
  of at most M: 7 u64 M for one evaluation.  Two correct evaluations (scipy re-derives voiced
  frames from the segment on their left, this restatement keeps them) differ by at most twice
  that: 16 u64 M.
* float32-held values, ``held32_bound``: two float64 sums of the same frames in different orders
  differ far below a float32 ulp, so their float32 roundings are equal or adjacent: one ulp,
  2^-23 |x|.  numpy's float32 ``mean`` of d energy frames accumulates in float32: (d - 1)
  additions and one division, each u32 of at most max |frame| in any order, plus the final
  rounding this restatement has too: ``mean32_bound`` = (d + 1) u32 max |frame|.
* group mean and std, ``stat_bounds``: N pooled values of magnitude at most S, merged from K
  utterance triples.  Any order of summation is within gamma_(N-1) sum |x| <= N u64 N S of the
  sum, so within N u64 S of the mean; each of the K merges adds a handful of roundings of
  quantities of at most S (mean) or N S^2 (M2).  mean: 2 (N + 4 K) u64 S.  Variance: the
  squared deviations are at most 4 S^2 each with relative error 3 u64 + the mean's share, summed
  in any order: 8 (N + 4 K) u64 S^2; the std inherits it through sqrt: |d std| <= |d var| / std
  (+ one rounding).  This is the gamma_n bound for the merge order; it assumes both sides hold
  the same values, which the held-track comparison establishes first.
* z, ``z_bound``: (x - mean) / std with errors dm, ds in mean and std moves by at most
  (dm + |z| ds) / std (first order, doubled for the second), plus two float64 roundings of |z|,
  plus one float32 rounding u32 |z| (and half the smallest float32 subnormal).  The float64
  minimum and maximum have the same bound without the float32 term.

Fence condition: in every case, no held value may lie within 1e-9 max(|q1|, |q3|, iqr) of a
fence, so that every correct evaluation gives the same clean mask and n_clean is an integer
equality.  One exception is forced by the cases themselves (D = 1, a constant track, one phoneme
spanning D with averaging): when iqr == 0 exactly, both fences equal q1 = q3, which is then one
of the held values copied without arithmetic (a + 0 g), and the values equal to it sit exactly
on the fence in every evaluation; only values at a distance in (0, margin] count as near.
"""
import math

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24
NONFINITE, UNVOICED, EMPTY, HOST_SKIPPED = 1, 2, 4, 8
MAX_D = 4096
D_EDGES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]
SEED = 20


# ------------------------------------------------------------------------------ restatement
def interpolate(f0, D):
    """float64 (D) and the status word"""
    x = np.asarray(f0, np.float64)[:D].copy()
    if not np.isfinite(x).all():
        return x, NONFINITE
    v = np.flatnonzero(x != 0)
    if v.size == 0:
        return x, UNVOICED
    for t in np.flatnonzero(x == 0):
        k = np.searchsorted(v, t)
        if k == 0:
            x[t] = x[v[0]]
        elif k == v.size:
            x[t] = x[v[-1]]
        else:
            lo, hi = v[k - 1], v[k]
            slope = (x[hi] - x[lo]) / np.float64(hi - lo)
            x[t] = slope * np.float64(t - lo) + x[lo]
    return x, 0


def average(x, durations):
    """per phoneme: the float64 mean (frame order) rounded once to float32, repeated"""
    out, idx, D = x.copy(), 0, x.size
    for d in durations:
        d = max(int(d), 0)
        a, e = min(idx, D), min(idx + d, D)
        if e > a:
            s = 0.0
            for v in x[a:e].tolist():
                s += v
            out[a:e] = np.float64(np.float32(np.float64(s) / np.float64(e - a)))
        idx += d
    return out


def held_track(values, durations, pitch, averaging):
    """the values as the reference holds them, float64 (D), and the status word"""
    D = int(np.maximum(np.asarray(durations, np.int64), 0).sum())
    if pitch:
        x, st = interpolate(values, D)
    else:
        x = np.asarray(values, np.float32)[:D].astype(np.float64)
        st = 0 if np.isfinite(x).all() else NONFINITE
    if st == 0 and averaging:
        x = average(x, durations)
    return x, st


def quartiles(x):
    s = np.sort(np.asarray(x, np.float64))
    out = []
    for q in (0.25, 0.75):
        vi = np.float64(s.size - 1) * q
        p = int(math.floor(vi))
        nx = min(p + 1, s.size - 1)
        g = vi - p
        diff = s[nx] - s[p]
        out.append(s[nx] - diff * (1.0 - g) if g >= 0.5 else s[p] + diff * g)
    return np.float64(out[0]), np.float64(out[1])


def fences(q1, q3):
    iqr = q3 - q1
    return q1 - 1.5 * iqr, q3 + 1.5 * iqr


def clean_mask(x, q1, q3):
    lo, hi = fences(q1, q3)
    return (x >= lo) & (x <= hi)


def fence_gap_ok(x, q1, q3):
    """the fence condition of the docstring"""
    iqr = q3 - q1
    margin = 1e-9 * max(abs(q1), abs(q3), iqr)
    for f in fences(q1, q3):
        d = np.abs(x - f)
        near = (d <= margin) & ((d > 0) | (iqr != 0))
        if near.any():
            return False
    return True


def triple(x):
    """(n, mean, M2) of the clean values, to within a rounding"""
    q1, q3 = quartiles(x)
    c = x[clean_mask(x, q1, q3)]
    n = c.size
    mean = math.fsum(c.tolist()) / n
    return float(n), mean, math.fsum(((c - mean) ** 2).tolist())


def scale_of(n, mean, var):
    """sqrt(var), or 1 under sklearn's _is_constant_feature"""
    eps = np.finfo(np.float64).eps
    if n == 0 or var <= n * eps * var + (n * mean * eps) ** 2:
        return 1.0
    return math.sqrt(var)


def group_stats(clean_arrays):
    """(N, mean, var, std) of the pooled values of a group's accepted utterances"""
    pooled = np.concatenate(clean_arrays) if clean_arrays else np.zeros(0)
    n = pooled.size
    if n == 0:
        return 0, 0.0, 0.0, 1.0
    mean = math.fsum(pooled.tolist()) / n
    var = math.fsum(((pooled - mean) ** 2).tolist()) / n
    return n, mean, var, scale_of(n, mean, var)


# ------------------------------------------------------------------------------ bounds
def interp_bound(f0, D):
    x = np.asarray(f0, np.float64)[:D]
    return 16 * U64 * float(np.abs(x).max()) if x.size else 0.0


def held32_bound(x):
    return 2.0 ** -23 * np.abs(x)


def mean32_bound(frames):
    frames = np.asarray(frames, np.float64)
    return (frames.size + 1) * U32 * float(np.abs(frames).max())


def stat_bounds(N, K, S, std):
    """(mean bound, std bound) for N pooled values of magnitude <= S from K utterances"""
    bm = 2 * (N + 4 * K) * U64 * S
    bv = 8 * (N + 4 * K) * U64 * S * S
    return bm, bv / std + 2 * U64 * std


def z_bound(z, bm, bs, std, f32=True):
    z = np.abs(np.asarray(z, np.float64))
    b = 2 * (bm + z * bs) / std + 4 * U64 * z
    return b + (U32 * z + 2.0 ** -150 if f32 else 0.0)


# ------------------------------------------------------------------------------ whole batches
def run_batch(batch, pitch_averaging, energy_averaging):
    """The stage on a batch dict (f0s, energies, durations, groups).  Returns a dict with, per
    utterance, D, status (both fields' bits | HOST_SKIPPED), and per field f in (0 pitch,
    1 energy): held[f][i], q[f][i], n_clean[f][i], z64[f][i]; per group name: stats[name][f] =
    (min, max, mean, std), pooled[name][f] = (N, K, S); rejected."""
    f0s, ens, durs, groups = batch["f0s"], batch["energies"], batch["durations"], batch["groups"]
    B = len(f0s)
    out = {"D": [], "status": np.zeros(B, np.int64), "held": ([], []), "q": ([], []),
           "n_clean": ([], []), "z64": ([None] * B, [None] * B), "stats": {}, "pooled": {}}
    clean = ([None] * B, [None] * B)
    for i in range(B):
        out["D"].append(int(np.maximum(np.asarray(durs[i], np.int64), 0).sum()))
        if np.count_nonzero(f0s[i]) <= 1:
            out["status"][i] = HOST_SKIPPED
        for f, (vals, avg) in enumerate(((f0s[i], pitch_averaging), (ens[i], energy_averaging))):
            x, st = held_track(vals, durs[i], f == 0, avg)
            out["held"][f].append(x)
            if st or out["status"][i] & HOST_SKIPPED:
                out["status"][i] |= st
                out["q"][f].append((0.0, 0.0))
                out["n_clean"][f].append(0)
                continue
            q1, q3 = quartiles(x)
            m = clean_mask(x, q1, q3)
            out["q"][f].append((q1, q3))
            out["n_clean"][f].append(int(m.sum()))
            clean[f][i] = x[m]
    names = list(dict.fromkeys(groups))
    for name in names:
        idx = [i for i in range(B) if groups[i] == name and out["status"][i] == 0]
        if not idx:
            continue
        out["stats"][name], out["pooled"][name] = [], []
        for f in (0, 1):
            N, mean, var, std = group_stats([clean[f][i] for i in idx])
            zmin, zmax = math.inf, -math.inf
            for i in idx:
                z = (out["held"][f][i] - mean) / std
                out["z64"][f][i] = z
                zmin, zmax = min(zmin, float(z.min())), max(zmax, float(z.max()))
            S = max(float(np.abs(clean[f][i]).max()) for i in idx)
            out["stats"][name].append((zmin, zmax, mean, std))
            out["pooled"][name].append((N, len(idx), S))
    out["rejected"] = [i for i in range(B) if out["status"][i]]
    return out


# ------------------------------------------------------------------------------ inputs
def f0_track(rng, L, pattern="runs"):
    """a pyworld-like F0 track: 80-300 Hz where voiced, 0 elsewhere"""
    t = np.arange(L)
    f = 170.0 + 60.0 * np.sin(t / 17.0 + rng.uniform(0, 6)) + rng.uniform(-25, 25, L)
    voiced = np.ones(L, bool)
    if pattern == "edges":
        k = max(1, L // 5)
        voiced[:k] = False
        voiced[L - k:] = False
    elif pattern == "single":    # one voiced frame inside D, another in the spare frames past it
        voiced[:] = False
        voiced[L // 3] = True
        voiced[L - 1] = True
    elif pattern == "alternating":
        voiced[1::2] = False
    elif pattern == "none":
        voiced[:] = False
    elif pattern == "runs":
        pos = 0
        while pos < L:
            n = int(rng.integers(3, 40))
            if rng.random() < 0.35:
                voiced[pos:pos + n] = False
            pos += n
        voiced[int(rng.integers(0, L))] = True
    else:
        assert pattern == "all"
    return np.where(voiced, f, 0.0)


def energy_track(rng, L):
    """a min-max normalised energy: float32 in [0, 1]"""
    e = np.abs(np.sin(np.arange(L) / 11.0 + rng.uniform(0, 3))) * 0.6 + rng.uniform(0, 0.4, L)
    return e.astype(np.float32)


def durations_of(D, kind, rng):
    if kind == "ones":
        return np.ones(D, np.int64)
    if kind == "one":
        return np.array([D], np.int64)
    if kind == "straddle":       # a phoneme across every multiple of 64 (so of 256 as well)
        cuts = sorted({c for k in range(1, D // 64 + 1) for c in (64 * k - 3, 64 * k + 5)
                       if 0 < c < D})
        inner = []
        for a, b in zip([0] + cuts, cuts + [D]):
            if b - a > 12:           # break the long stretches between the straddlers
                mid = a + int(rng.integers(4, b - a - 4))
                inner.append(mid)
        edges = sorted(set([0] + cuts + inner + [D]))
        return np.diff(edges).astype(np.int64)
    assert kind in ("random", "zeros")
    d = []
    while sum(d) < D:
        d.append(int(min(rng.integers(1, 24), D - sum(d))))
    if kind == "zeros":          # zeros at the start, in the middle and at the end
        d = [0, 0] + d[:len(d) // 2] + [0] + d[len(d) // 2:] + [0, 0, 0]
    return np.asarray(d, np.int64)


KINDS = ["ones", "one", "zeros", "straddle", "random"]


def edge_case(D, seed=SEED):
    """one utterance of exactly D frames with 9 / 5 spare input frames (truncation), the
    duration kind and the voicing pattern chosen by D's place in D_EDGES"""
    k = D_EDGES.index(D)
    rng = np.random.default_rng(seed * 1000 + D)
    kind = KINDS[k % len(KINDS)]
    pattern = ["runs", "all", "edges", "alternating"][k % 4] if D > 1 else "all"
    f0 = f0_track(rng, D + 9, pattern)
    if np.count_nonzero(f0[:D]) == 0:
        f0[0] = 200.0
    return {"f0s": [f0], "energies": [energy_track(rng, D + 5)],
            "durations": [durations_of(D, kind, rng)], "groups": ["g"]}


def merge(*batches):
    out = {"f0s": [], "energies": [], "durations": [], "groups": []}
    for b in batches:
        for k in out:
            out[k] += list(b[k])
    return out


def ragged_case():
    """every D of D_EDGES in one launch, one group"""
    return merge(*[edge_case(D) for D in D_EDGES])


def voicing_case(seed=SEED):
    """G = 3 with 1 / 2 / 7 utterances.  Group "c" holds the voicing patterns, an utterance
    without a voiced frame inside D (voiced only past it) and one with a NaN energy, both to be
    flagged; "a" is one utterance; "b" has an exactly constant pitch next to a varying one."""
    rng = np.random.default_rng(seed)
    f0s, ens, durs, groups = [], [], [], []

    def add(g, D, pattern, kind, f0=None, en=None):
        f0s.append(f0_track(rng, D + 3, pattern) if f0 is None else f0)
        ens.append(energy_track(rng, D + 2) if en is None else en)
        durs.append(durations_of(D, kind, rng))
        groups.append(g)

    add("c", 130, "all", "random")
    add("a", 77, "runs", "zeros")
    add("c", 67, "edges", "straddle")
    novoice = np.zeros(90)
    novoice[85:] = 150.0
    add("c", 80, None, "random", f0=novoice)
    add("b", 64, None, "ones", f0=np.full(70, 220.0))
    add("c", 40, "single", "random")
    nan_e = energy_track(rng, 30)
    nan_e[17] = np.nan
    add("c", 25, "all", "random", en=nan_e)
    add("c", 301, "alternating", "straddle")
    add("b", 200, "runs", "random")
    add("c", 9, "all", "one")
    return {"f0s": f0s, "energies": ens, "durations": durs, "groups": groups}


def constant_case():
    """G = 1, one utterance whose pitch and energy are exactly constant: scale 1, z = 0"""
    return {"f0s": [np.full(40, 220.0)], "energies": [np.full(40, 0.5, np.float32)],
            "durations": [np.array([7, 0, 13, 20], np.int64)], "groups": ["k"]}


CASES = {"ragged": ragged_case, "voicing": voicing_case, "constant": constant_case}
for _D in D_EDGES:
    CASES[f"D{_D}"] = (lambda D=_D: edge_case(D))
AVERAGING = [(False, False), (True, False), (False, True), (True, True)]

_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def expected(name, pa, ea):
    key = (name, pa, ea)
    if key not in _CACHE:
        _CACHE[key] = run_batch(case(name), pa, ea)
    return _CACHE[key]
