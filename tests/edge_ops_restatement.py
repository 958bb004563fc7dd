"""Test helper: references of the small kernels that move data into the model and out of it
(csrc/collate.hip, csrc/intensity.hip, csrc/vocoder.hip and fs2_fill / fs2_add / fs2_cast),
in numpy, no GPU.

One function per entry point of include/fs2_hip.h, written from the header's comments and the
reference semantics they cite (the collate's zero padding and permute, masked_fill + classifier,
repeat_interleave + index_add_ + clamp(min=1), F.pad "replicate", F.leaky_relu), as loops over
the *output's* coordinates -- not from the kernels' index arithmetic.  tests/test_edge_ops_host.py
pins every one of them to torch or to the oracle before a GPU test relies on it.

Conventions.  fp32 data is ``np.float32``; bf16 data is its bit pattern in ``np.uint16``
(``bf16_rne`` / ``bf16_to_f32``); ``dtype`` is ``"f32"`` or ``"bf16"``.  numpy rounds every
float32 operation once, never fuses a multiply with an add, and keeps denormals, so a float32
expression here is "each operation rounded once, in this order".

Bounds (u = 2^-24; an fp32 operation returns its exact result times (1 + d), |d| <= u; a factor
SLACK = 1 + 2^-10 covers products of two roundings):

* ``intensity_head``: I = sum_d (h_d + em_d) Wc_d + bc.  A term carries one rounding for h + em
  and one for the product; the lane that owns column d adds ceil(D/64) terms in a chain; six
  shuffle adds join the 64 lanes; one add for the bias; one spare.  Every term therefore passes
  through at most ceil(D/64) + 9 roundings, each relative to a partial sum that is at most
  sum |h + em| |Wc| + |bc| in magnitude:
      |I_fp32 - I_f64| <= (ceil(D/64) + 9) u (sum_d |h + em| |Wc| + |bc|) SLACK.
  A fused multiply-add only removes roundings.
* ``phoneme_average``: a sequential sum of d terms (d - 1 roundings, each relative to a partial
  sum <= sum |I|) and one division: (d + 1) u sum|I| / max(d, 1) SLACK, d the full duration.
"""
import math

import numpy as np

from adamw_restatement import SLACK, U24, same_bits  # noqa: F401  (shared with the AdamW tests)

F32 = np.float32


# ---- bf16 --------------------------------------------------------------------------------------
def bf16_rne(x32):
    """float32 -> bf16 bits (uint16), round to nearest, ties to even.  Inf stays inf, a value
    beyond the largest bf16 plus half an ulp becomes inf, NaN stays (a quiet) NaN."""
    x = np.ascontiguousarray(x32, dtype=F32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        r = np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)
    return r


def bf16_to_f32(bits):
    b = np.ascontiguousarray(bits)
    assert b.dtype in (np.uint16, np.int16)
    b = b.view(np.uint16)
    return (b.astype(np.uint32) << 16).view(F32)


def same_bits16(a, b):
    """bf16 bit patterns equal, NaNs (any payload) in the same places"""
    a, b = np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16)
    assert a.shape == b.shape
    na, nb = np.isnan(bf16_to_f32(a)), np.isnan(bf16_to_f32(b))
    return bool((na == nb).all() and (a[~na] == b[~nb]).all())


def same_out(a, b, dtype):
    return same_bits(a, b) if dtype == "f32" else same_bits16(a, b)


def _store(x32, dtype):
    """an fp32 result as the kernel stores it in ``dtype``"""
    assert dtype in ("f32", "bf16")
    x32 = np.asarray(x32, dtype=F32)
    return x32 if dtype == "f32" else bf16_rne(x32)


# ---- collate -----------------------------------------------------------------------------------
def collate_phonemes(order, offsets, phon, dur, B, Tp):
    """(phoneme_padded, duration_padded, input_lengths): batch row i is item order[i], its
    phonemes / durations at [offsets[u], offsets[u+1]) of the packed arrays, zero padded to Tp"""
    ph = np.zeros((B, Tp), np.int64)
    du = np.zeros((B, Tp), np.int64)
    ln = np.zeros(B, np.int64)
    for i in range(B):
        u = int(order[i])
        a, b = int(offsets[u]), int(offsets[u + 1])
        assert 0 <= b - a <= Tp
        ph[i, :b - a] = phon[a:b]
        du[i, :b - a] = dur[a:b]
        ln[i] = b - a
    return ph, du, ln


def collate_frames(order, foff, mel, pitch, energy, B, Tm, NM):
    """(mel_padded[B,Tm,NM], pitch[B,Tm], energy[B,Tm], rank_x[B,NM+2,Tm], out_len): item u's
    mel is (NM, T_u) channel-major at foff[u]*NM of the packed mel, its pitch / energy at
    foff[u]; mel_padded is the zero-padded mel transposed, rank_x = cat(mel, pitch, energy)"""
    mp = np.zeros((B, Tm, NM), F32)
    pp = np.zeros((B, Tm), F32)
    ep = np.zeros((B, Tm), F32)
    rk = np.zeros((B, NM + 2, Tm), F32)
    ln = np.zeros(B, np.int64)
    for i in range(B):
        u = int(order[i])
        a, b = int(foff[u]), int(foff[u + 1])
        T = b - a
        assert 0 <= T <= Tm
        m = np.asarray(mel[a * NM:b * NM], F32).reshape(NM, T)
        mp[i, :T] = m.T
        pp[i, :T] = pitch[a:b]
        ep[i, :T] = energy[a:b]
        rk[i, :NM, :T] = m
        rk[i, NM, :T] = pitch[a:b]
        rk[i, NM + 1, :T] = energy[a:b]
        ln[i] = T
    return mp, pp, ep, rk, ln


# ---- intensity ---------------------------------------------------------------------------------
def intensity_input(x, bct, B, T, C, ldx, dtype):
    """rank_X (B,T,C), or (B,C,T) with ``bct``, as GEMM rows [B*T][ldx]; columns >= C zero"""
    x = np.asarray(x, F32).reshape(-1)[:B * T * C]
    x = x.reshape(B, C, T).transpose(0, 2, 1) if bct else x.reshape(B, T, C)
    X = np.zeros((B * T, ldx), F32)
    X[:, :C] = x.reshape(B * T, C)
    return _store(X, dtype)


def intensity_head(H, ldh, emo_tab, emo, lens, Wc, bc, B, T, D, E):
    """(ref, bound, keep): ``H`` the stored values of the [B*T][ldh] rows as float32 (a bf16 H
    widened), of which columns < D are used.  ref[m][e] in float64 =
    keep[m] (H[m] + emo_tab[emo[b]]) . Wc[e] + bc[e], keep[m] = t < lens[b] (rows with
    t >= lens[b] are exactly bc); bound[m][e] as derived in the module docstring."""
    H = np.asarray(H, F32).reshape(B * T, ldh)[:, :D].astype(np.float64)
    tab = np.asarray(emo_tab, F32).astype(np.float64)
    Wc = np.asarray(Wc, F32).reshape(E, D).astype(np.float64)
    bc = np.asarray(bc, F32).astype(np.float64)
    ref = np.zeros((B * T, E))
    bound = np.zeros((B * T, E))
    keep = np.zeros(B * T, bool)
    ops = math.ceil(D / 64) + 9
    for b in range(B):
        for t in range(T):
            m = b * T + t
            keep[m] = t < int(lens[b])
            if keep[m]:
                v = H[m] + tab[int(emo[b])]
                ref[m] = Wc @ v + bc
                bound[m] = ops * U24 * (np.abs(Wc) @ np.abs(v) + np.abs(bc)) * SLACK
            else:
                ref[m] = bc
    return ref, bound, keep


def phoneme_average(I, T, E, durs, phon_len, B, Tp, dtype=np.float32):
    """out[b,p,:] = (sum of I[b,t,:] over phoneme p's frames) / max(d[b,p], 1) for
    p < phon_len[b] (clamped to [0, Tp]), +0 elsewhere.  Phoneme p's frames start at
    sum(d[b,:p]); frames from T on are not read, the divisor is still d[b,p].

    float32: the sum in ascending t, each add rounded once, then one division; returns out.
    float64: returns (ref, bound), bound as derived in the module docstring."""
    dtype = np.dtype(dtype).type
    I = np.asarray(I, F32).reshape(-1)[:B * T * E].reshape(B, T, E)
    durs = np.asarray(durs, np.int64).reshape(B, Tp)
    out = np.zeros((B, Tp, E), dtype)
    bound = np.zeros((B, Tp, E))
    for b in range(B):
        n = min(max(int(phon_len[b]), 0), Tp)
        start = 0
        for p in range(n):
            d = int(durs[b, p])
            assert d >= 0
            s = np.zeros(E, dtype)
            sa = np.zeros(E)
            for t in range(start, min(start + d, T)):
                s = s + I[b, t].astype(dtype)
                sa = sa + np.abs(I[b, t].astype(np.float64))
            out[b, p] = s / dtype(max(d, 1))
            bound[b, p] = (d + 1) * U24 * sa / max(d, 1) * SLACK
            start += d
    assert out.dtype == dtype
    return out if dtype is np.float32 else (out, bound)


# ---- vocoder -----------------------------------------------------------------------------------
def vocoder_input(mel, B, NM, T, pad, ldx, dtype):
    """mel (B, NM, T) -> rows [B*(T + 2 pad)][ldx]: ``pad`` copies of the first frame, the T
    frames, ``pad`` copies of the last one; columns >= NM zero"""
    mel = np.asarray(mel, F32).reshape(-1)[:B * NM * T].reshape(B, NM, T)
    X = np.zeros((B, T + 2 * pad, ldx), F32)
    for b in range(B):
        frames = [mel[b, :, 0]] * pad + [mel[b, :, t] for t in range(T)] + [mel[b, :, T - 1]] * pad
        X[b, :, :NM] = np.stack(frames)
    return _store(X.reshape(B * (T + 2 * pad), ldx), dtype)


def _lrelu32(x, slope):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return np.where(x >= 0, x, x * F32(slope)).astype(F32)


def leaky_relu(x, slope, dtype):
    """x >= 0 ? x : x * slope in fp32 (x: the stored values as float32): -0.0 stays -0.0
    (it compares >= 0), NaN stays NaN (it does not, and NaN * slope is NaN)"""
    return _store(_lrelu32(x, slope), dtype)


def mean3_leaky_relu(a, b, c, slope, dtype):
    """leaky_relu(((a + b) + c) / 3, slope), every operation rounded in float32"""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        m = ((a + b) + c) / F32(3)
    assert m.dtype == F32
    return _store(_lrelu32(m, slope), dtype)


# ---- elementwise helpers -----------------------------------------------------------------------
def _round_once(x, p):
    """float32(x + p) rounded once, x float32 and p a float64 that holds a product of two
    float32 exactly.  s = fl64(x + p) and the two-sum error e give x + p = s + e exactly; s is
    moved to round-to-odd (truncate toward zero, set the last bit if inexact), after which the
    rounding of its 53 bits to 24 is the rounding of the exact sum."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        s = x + p
        bv = s - x
        e = (x - (s - bv)) + (p - bv)
    fin = np.isfinite(s) & (e != 0)
    bits = s.view(np.int64).copy()          # sign-magnitude: -1 on the bits moves toward zero
    away = fin & ((e > 0) == (s > 0))       # |exact| > |s|: s is the truncation already
    toward = fin & ~away
    bits[toward] -= 1
    bits[fin] |= 1
    with np.errstate(all="ignore"):
        return bits.view(np.float64).astype(F32)


def add(x, y, alpha, dtype):
    """X += alpha * Y: (unfused, fused).  unfused = x + fl(alpha * y), two fp32 roundings;
    fused = the exact x + alpha * y rounded once to fp32 (a fused multiply-add).  x, y: the
    stored values as float32, alpha rounded to fp32 as the C ABI takes it; a bf16 output is
    bf16_rne of the fp32 result in both."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    al = F32(alpha)
    with np.errstate(all="ignore"):
        unfused = x + al * y
        fused = _round_once(x, np.float64(al) * y.astype(np.float64))
    assert unfused.dtype == F32 and fused.dtype == F32
    return _store(unfused, dtype), _store(fused, dtype)


def fill(n, value, dtype):
    """n elements of ``value`` (rounded to fp32 on the way into the C ABI) in ``dtype``"""
    return _store(np.full(n, F32(value), F32), dtype)


def cast(src, src_dtype, dst_dtype):
    """src (float32, or bf16 bits) converted: bf16 -> fp32 is exact, fp32 -> bf16 is bf16_rne,
    equal dtypes copy the bits"""
    if src_dtype == dst_dtype:
        return np.array(src, copy=True)
    if src_dtype == "bf16":
        return bf16_to_f32(src)
    return bf16_rne(src)


# ---- input families ----------------------------------------------------------------------------
BF16_MAX = float(bf16_to_f32(np.uint16([0x7F7F]))[0])          # 2^127 (2 - 2^-7)
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)


def rounding_family():
    """fp32 values at which a float32 -> bf16 rounding goes wrong: exact ties of both parities
    and both signs, their fp32 neighbours, +-0, +-inf, the largest finite fp32 (-> inf), the
    values from the largest bf16 to half a bf16 ulp above it (the tie goes to inf), the smallest
    normals, NaN.  No fp32 subnormals (``subnormal_family``)."""
    w = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x404A, 0x0080, 0x0081, 0x7F7E, 0x7F7F, 0x7F00, 0x00FF,
               0x3EFF, 0x3F00):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
            w.append((hi << 16) | lo)
    w += [0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0x7F800000, 0x00000000, 0x00800000,
          0x00800001, 0x00808000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]
    w = np.array(w, np.uint32)
    w = np.concatenate([w, w | np.uint32(0x80000000)])
    return w.view(F32).copy()


def subnormal_family():
    """fp32 subnormals, both signs: the extremes, ties of the bf16 subnormal grid and their
    neighbours (recorded, not asserted: what the conversion instruction does with them)"""
    w = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00017FFF, 0x00018000,
         0x00018001, 0x00028000, 0x007F8000, 0x007FFFFF, 0x007F7FFF, 0x00400000, 0x0040FFFF]
    w = np.array(w, np.uint32)
    w = np.concatenate([w, w | np.uint32(0x80000000)])
    return w.view(F32).copy()


def activation_family(n, seed, dtype):
    """n fp32 values (bf16-representable when dtype is bf16): randn with +-0, +-inf, NaN and
    the smallest normals placed at fixed positions of every 8-element vector slot"""
    r = np.random.default_rng([seed, n])
    x = r.standard_normal(n).astype(F32)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MIN, -FLT_MIN, 1.0, -1.0]
    for j, v in enumerate(special):
        x[(j * 7 + 3) % n::max(n // 3, 1) + 11] = v
    k = min(n, len(special))
    x[:k] = special[:k]
    x[n - 1] = -0.0 if n > 1 else x[0]
    if dtype == "bf16":
        x = bf16_to_f32(bf16_rne(x))
    return x
