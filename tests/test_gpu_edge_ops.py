"""GPU: the small kernels that move data into the model and out of it -- fs2_collate_phonemes,
fs2_collate_frames, fs2_intensity_input, fs2_intensity_head, fs2_phoneme_average,
fs2_vocoder_input, fs2_leaky_relu, fs2_mean3_leaky_relu, fs2_fill, fs2_add, fs2_cast -- each
alone, through fastspeech2.ops, against tests/edge_ops_restatement.py (pinned on the CPU by
tests/test_edge_ops_host.py), at the smallest shapes that cross each tile edge.

Everything is compared bit for bit (NaN by NaN-ness), except: the intensity head and the
float64 side of the phoneme average, held to bounds derived from the operation count (the
restatement's docstring), and fs2_add with alpha != +-1, where each element must equal the fused
or the unfused candidate.  Every output is allocated inside a buffer of 0x5A bytes, which must
come back untouched around it; every float input is followed by NaNs, so an over-read shows up
as a wrong value.  No GEMM, attention or LayerNorm kernel is launched here.
"""
import math
import time

import numpy as np
import pytest
import torch

import edge_ops_restatement as ER

pytestmark = pytest.mark.gpu

TAIL = 64                      # sentinel elements after every output, NaN elements after inputs
DTYPES = ["f32", "bf16"]
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _wall_time(parity_log):
    t0 = time.perf_counter()
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        parity_log["edge_ops_wall_seconds"] = {"file": round(time.perf_counter() - t0, 3)}


def _code(dtype):
    from fastspeech2 import _native as N
    return {"f32": N.F32, "bf16": N.BF16}[dtype]


class Out:
    """an output of ``numel`` elements after ``lead`` and before TAIL sentinel elements"""

    def __init__(self, cuda, numel, tdtype, lead=0):
        self.es = torch.empty(0, dtype=tdtype).element_size()
        self.lead, self.numel = lead, numel
        self.raw = torch.full(((lead + numel + TAIL) * self.es,), 0x5A, dtype=torch.uint8,
                              device=cuda)
        self.t = self.raw.view(tdtype)[lead:lead + numel]

    def np(self):
        """the output on the host; asserts the sentinels first"""
        r = self.raw.cpu()
        a, b = self.lead * self.es, (self.lead + self.numel) * self.es
        assert bool((r[:a] == 0x5A).all()) and bool((r[b:] == 0x5A).all()), "sentinel written"
        body = r[a:b].clone()
        if self.t.dtype == torch.bfloat16:
            return body.view(torch.int16).numpy().view(np.uint16)
        return body.view(self.t.dtype).numpy()


def _in(cuda, arr, lead=0):
    """a device copy of a numpy array (float32, bf16 bits as uint16, int64, int32) between
    ``lead`` and TAIL elements of NaN (floats) or -999 (integers)"""
    arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.dtype == np.uint16:
        pad = lambda k: np.full(k, 0x7FC0, np.uint16)
        whole = np.concatenate([pad(lead), arr, pad(TAIL)]).view(np.int16)
        t = torch.from_numpy(whole).view(torch.bfloat16)
    else:
        fillv = np.nan if arr.dtype == np.float32 else -999
        pad = lambda k: np.full(k, fillv, arr.dtype)
        t = torch.from_numpy(np.concatenate([pad(lead), arr, pad(TAIL)]))
    return t.to(cuda)[lead:lead + arr.size]


def _in_dt(cuda, x32, dtype, lead=0):
    """fp32 values as a device input of ``dtype``; returns (tensor, the stored values as fp32)"""
    if dtype == "bf16":
        bits = ER.bf16_rne(x32)
        return _in(cuda, bits, lead), ER.bf16_to_f32(bits).reshape(np.shape(x32))
    x32 = np.ascontiguousarray(x32, np.float32)
    return _in(cuda, x32, lead), x32


def _same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def _rand(r, *shape):
    """randn with a few -0.0 and exact zeros in it: a byte mover must keep the sign bit"""
    x = r.standard_normal(shape).astype(np.float32).reshape(-1)
    x[::13] = -0.0
    x[5::17] = 0.0
    return x.reshape(shape)


# ---- collate -----------------------------------------------------------------------------------
PHON_CASES = {(1, 1): [1], (3, 100): [37, 0, 100], (5, 257): [100, 0, 257, 256, 1]}


@pytest.mark.parametrize("B,Tp", list(PHON_CASES))
def test_collate_phonemes(cuda, B, Tp):
    """256-thread blocks crossed at (5, 257); one item of length 0 (a zero row, in_len 0), one of
    length Tp; the items arrive unsorted, so ``order`` is not the identity"""
    from fastspeech2 import ops
    lens = PHON_CASES[(B, Tp)]
    r = np.random.default_rng(B * 1000 + Tp)
    order = np.argsort(-np.array(lens), kind="stable").astype(np.int32)
    assert B == 1 or list(order) != list(range(B))
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    phon = r.integers(1, 89, off[-1]).astype(np.int64)
    dur = r.integers(0, 10, off[-1]).astype(np.int64)
    po, do, lo = (Out(cuda, n, torch.int64) for n in (B * Tp, B * Tp, B))
    ops.collate_phonemes(_in(cuda, order), _in(cuda, off), _in(cuda, phon), _in(cuda, dur), B, Tp,
                         po.t, do.t, lo.t)
    torch.cuda.synchronize()
    ph, du, ln = ER.collate_phonemes(order, off, phon, dur, B, Tp)
    assert _same_bytes(po.np(), ph) and _same_bytes(do.np(), du) and _same_bytes(lo.np(), ln)
    if B > 1:
        z = list(order).index(lens.index(0))
        assert ln[z] == 0 and not ph[z].any() and ln.max() == Tp


def _frames_case(cuda, NM, Tm, lens, order, seed):
    from fastspeech2 import ops
    B = len(lens)
    r = np.random.default_rng([seed, NM, Tm])
    order = np.array(order, np.int32)
    foff = np.zeros(B + 1, np.int64)
    foff[1:] = np.cumsum(lens)
    nfr = int(foff[-1])
    mel, pitch, energy = _rand(r, nfr * NM), _rand(r, nfr), _rand(r, nfr)
    outs = [Out(cuda, n, torch.float32) for n in (B * Tm * NM, B * Tm, B * Tm, B * (NM + 2) * Tm)]
    lo = Out(cuda, B, torch.int64)
    ops.collate_frames(_in(cuda, order), _in(cuda, foff), _in(cuda, mel), _in(cuda, pitch),
                       _in(cuda, energy), B, Tm, NM, outs[0].t, outs[1].t, outs[2].t, outs[3].t,
                       lo.t)
    torch.cuda.synchronize()
    want = ER.collate_frames(order, foff, mel, pitch, energy, B, Tm, NM)
    got = [o.np() for o in outs] + [lo.np()]
    for name, g, w in zip(("mel", "pitch", "energy", "rank_x", "out_len"), got, want):
        assert _same_bytes(g, w), name
    rk = got[3].reshape(B, NM + 2, Tm)
    assert _same_bytes(rk[:, NM], got[1]) and _same_bytes(rk[:, NM + 1], got[2])
    assert not np.isnan(rk).any()


@pytest.mark.parametrize("Tm", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("NM", [1, 80, 128])
def test_collate_frames(cuda, NM, Tm):
    """the 64-frame tile at 63 / 64 / 65 / 130 frames, one channel, the usual 80 and the LDS
    tile's limit of 128; lengths Tm, 1, min(64, Tm), max(Tm - 1, 1) placed out of order"""
    _frames_case(cuda, NM, Tm, [Tm, 1, min(64, Tm), max(Tm - 1, 1)], [2, 0, 3, 1], 1)


def test_collate_frames_zero_tail_on_every_row(cuda):
    """Tm = max(T_u) + 3, past a tile edge: every row ends in zeros"""
    _frames_case(cuda, 80, 73, [70, 1, 64, 69], [0, 3, 2, 1], 2)


def test_collate_frames_single_item(cuda):
    _frames_case(cuda, 80, 65, [65], [0], 3)


# ---- intensity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,C,ldx", [(2, 5, 82, 88), (1, 1, 3, 8), (3, 37, 82, 82)])
@pytest.mark.parametrize("bct", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_intensity_input(cuda, dtype, bct, B, T, C, ldx):
    from fastspeech2 import ops
    x = _rand(np.random.default_rng([B, T, C, bct]), B * T * C)
    X = Out(cuda, B * T * ldx, TORCH_DT[dtype])
    ops.intensity_input(_in(cuda, x), bct, B, T, C, X.t, ldx, dt=_code(dtype))
    torch.cuda.synchronize()
    want = ER.intensity_input(x, bct, B, T, C, ldx, dtype)
    got = X.np().reshape(B * T, ldx)
    assert _same_bytes(got, want)
    assert not got[:, C:].any()                              # +0 in fp32 and in bf16 bits alike


HEAD_CASES = {  # (B, T, D, E, ldh): lengths
    (3, 7, 384, 5, 384): [0, 7, 10],
    (2, 5, 64, 1, 72): [3, 8],
    (2, 6, 100, 8, 104): [6, 2],
    (1, 9, 63, 3, 63): [4],
}


@pytest.mark.parametrize("B,T,D,E,ldh", list(HEAD_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_intensity_head(cuda, parity_log, dtype, B, T, D, E, ldh):
    """D = 63 leaves a lane idle, D = 100 half of the second round; B*T = 21, 10 and 9 are no
    multiple of the 4 rows of a block; E = 1 and E = 8; lengths 0, T, T + 3 (the clamp) and partial ones
    (the frame at t == len is masked); a different emotion row per utterance, the table's last
    one among them; H's pitch gap, and everything after every input, is NaN"""
    from fastspeech2 import ops
    r = np.random.default_rng([B, T, D, E])
    lens = np.array(HEAD_CASES[(B, T, D, E, ldh)], np.int64)
    n_emo = B + 2
    emo = np.array([1, n_emo - 1, 2][:B] if B > 1 else [n_emo - 1], np.int64)
    H = r.standard_normal((B * T, ldh)).astype(np.float32)
    H[:, D:] = np.nan
    Hd, Hs = _in_dt(cuda, H, dtype)
    tab = r.standard_normal((n_emo, D)).astype(np.float32)
    Wc = (r.standard_normal((E, D)) / math.sqrt(D)).astype(np.float32)
    bc = r.standard_normal(E).astype(np.float32)
    I = Out(cuda, B * T * E, torch.float32)
    ops.intensity_head(Hd, ldh, _in(cuda, tab), _in(cuda, emo), _in(cuda, lens), _in(cuda, Wc),
                       _in(cuda, bc), B, T, D, E, I.t, dt=_code(dtype))
    torch.cuda.synchronize()
    got = I.np().reshape(B * T, E)
    ref, bound, keep = ER.intensity_head(Hs, ldh, tab, emo, lens, Wc, bc, B, T, D, E)
    assert keep.reshape(B, T).sum(1).tolist() == np.minimum(lens, T).tolist()
    assert np.isfinite(got).all(), "a NaN leaked from a pitch gap or from past an input"
    masked = got[~keep]
    assert ER.same_bits(masked, np.tile(bc, (masked.shape[0], 1))), "masked rows are not bc"
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err[keep] / bound[keep]).max())
    print(f"intensity_head {dtype} {(B, T, D, E, ldh)}: max err/bound {ratio:.4f}")
    old = parity_log.setdefault(f"edge_ops_intensity_head_{dtype}", {"err_over_bound": 0.0})
    old["err_over_bound"] = max(old["err_over_bound"], ratio)
    assert (err[keep] <= bound[keep]).all()


def _avg_cases():
    """(B, T, Tp, E) -> (durations, phon_len)"""
    r = np.random.default_rng(17)
    c = {}
    # starts with a zero duration; sum d = 47 > T = 40 with phon_len past Tp; phon_len = 0
    c[(3, 40, 9, 5)] = ([[0, 5, 3, 0, 9, 7, 6, 2, 8], [4, 6, 0, 9, 7, 5, 8, 3, 5],
                         [3, 4, 5, 6, 7, 8, 2, 1, 0]], [9, 14, 0])
    # the whole 1024-entry prefix array; ends with a zero duration; phon_len = Tp and Tp + 5
    d = (r.random((2, 1024)) < 0.25).astype(np.int64)
    d[0, ::97] = 2
    d[0, -1] = 0
    d[1, 500:520] = 0
    assert d.sum(1).max() <= 300
    c[(2, 300, 1024, 5)] = (d, [1024, 1029])
    c[(1, 12, 4, 1)] = ([[4, 0, 8, 0]], [4])                 # ends with a zero duration
    # a run of three zero durations; a zero first and phon_len past Tp
    c[(2, 50, 7, 8)] = ([[6, 0, 0, 0, 9, 20, 15], [0, 10, 1, 12, 0, 20, 7]], [7, 12])
    return c


AVG_CASES = _avg_cases()


@pytest.mark.parametrize("B,T,Tp,E", list(AVG_CASES))
def test_phoneme_average(cuda, B, T, Tp, E):
    from fastspeech2 import ops
    durs, phon_len = AVG_CASES[(B, T, Tp, E)]
    durs = np.array(durs, np.int64).reshape(B, Tp)
    phon_len = np.array(phon_len, np.int64)
    if (B, T, Tp, E) == (3, 40, 9, 5):
        assert durs[1].sum() > T and durs[0].sum() == T
    else:
        assert (durs.sum(1) <= T).all()
    I = np.random.default_rng([B, T, Tp, E]).standard_normal(B * T * E).astype(np.float32)
    out = Out(cuda, B * Tp * E, torch.float32)
    ops.phoneme_average(_in(cuda, I), T, E, _in(cuda, durs), _in(cuda, phon_len), B, Tp, out.t)
    torch.cuda.synchronize()
    got = out.np().reshape(B, Tp, E)
    want = ER.phoneme_average(I, T, E, durs, phon_len, B, Tp)
    ref, bound = ER.phoneme_average(I, T, E, durs, phon_len, B, Tp, np.float64)
    assert np.isfinite(got).all(), "a frame past T (or past I) was read"
    for b in range(B):
        n = min(max(int(phon_len[b]), 0), Tp)
        assert not got[b, n:].view(np.int32).any(), "positions p >= phon_len are not +0.0"
    bad = int((got.view(np.int32) != want.view(np.int32)).sum())
    assert bad == 0, f"{bad} of {got.size} words differ from the fp32 restatement"
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()


# ---- vocoder -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NM,T,pad,ldx", [(2, 80, 23, 5, 80), (1, 80, 1, 5, 88), (3, 7, 4, 0, 8),
                                            (2, 80, 3, 7, 80)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vocoder_input(cuda, dtype, B, NM, T, pad, ldx):
    """one frame; no padding; more padding than frames (replicate, where reflect has no answer)"""
    from fastspeech2 import ops
    mel = _rand(np.random.default_rng([B, NM, T, pad]), B * NM * T)
    rows = B * (T + 2 * pad)
    X = Out(cuda, rows * ldx, TORCH_DT[dtype])
    ops.vocoder_input(_in(cuda, mel), B, NM, T, pad, X.t, ldx, dt=_code(dtype))
    torch.cuda.synchronize()
    got = X.np().reshape(rows, ldx)
    assert _same_bytes(got, ER.vocoder_input(mel, B, NM, T, pad, ldx, dtype))
    assert not got[:, NM:].any()


def _act_inputs(n, dtype):
    """a, b, c for the activations: the special-value family, b shifted by one element so that
    inf meets -inf and NaN meets numbers; sums that cancel exactly (b = -a, c = +-0)"""
    a = ER.activation_family(n, 1, dtype)
    b = np.roll(ER.activation_family(n, 2, dtype), 1)
    c = ER.activation_family(n, 3, dtype)
    k = np.arange(n)
    fin = np.isfinite(a)
    s1, s2 = fin & (k % 5 == 1), fin & (k % 10 == 2)
    b[s1] = -a[s1]
    c[s1] = 0.0
    c[s2] = -0.0
    return a, b, c


def _act_sizes(dtype):
    V = 4 if dtype == "f32" else 8
    return [V, 256 * V, 256 * V + V, 3 * 256 * V - V]


ACT_CASES = [(dt, n) for dt in DTYPES for n in _act_sizes(dt)]


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("dtype,n", ACT_CASES)
def test_leaky_relu(cuda, dtype, n, slope):
    """one vector; one full block; a block and one vector; three blocks less one vector"""
    from fastspeech2 import ops
    a, _, _ = _act_inputs(n, dtype)
    xd, xs = _in_dt(cuda, a, dtype)
    y = Out(cuda, n, TORCH_DT[dtype])
    ops.leaky_relu(xd, y.t, n, slope, dt=_code(dtype))
    torch.cuda.synchronize()
    assert ER.same_out(y.np(), ER.leaky_relu(xs, slope, dtype), dtype)
    if n > 8:
        assert np.isnan(xs).any() and (xs == 0).sum() >= 3 and np.signbit(xs[xs == 0]).any()


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("dtype,n", ACT_CASES)
def test_mean3_leaky_relu(cuda, dtype, n, slope):
    from fastspeech2 import ops
    ins = [_in_dt(cuda, v, dtype) for v in _act_inputs(n, dtype)]
    y = Out(cuda, n, TORCH_DT[dtype])
    ops.mean3_leaky_relu(ins[0][0], ins[1][0], ins[2][0], y.t, n, slope, dt=_code(dtype))
    torch.cuda.synchronize()
    want = ER.mean3_leaky_relu(ins[0][1], ins[1][1], ins[2][1], slope, dtype)
    assert ER.same_out(y.np(), want, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_activations_in_place(cuda, dtype):
    """y == x, and y == a for the mean: the sentinels around the buffer stay, the values are the
    out-of-place ones"""
    from fastspeech2 import ops
    n = _act_sizes(dtype)[2]
    a, b, c = _act_inputs(n, dtype)
    ad, stored = _in_dt(cuda, a, dtype)
    for op in ("lrelu", "mean3"):
        buf = Out(cuda, n, TORCH_DT[dtype])
        buf.t.copy_(ad)
        if op == "lrelu":
            ops.leaky_relu(buf.t, buf.t, n, 0.1, dt=_code(dtype))
            want = ER.leaky_relu(stored, 0.1, dtype)
        else:
            (bd, bs), (cd, cs) = _in_dt(cuda, b, dtype), _in_dt(cuda, c, dtype)
            ops.mean3_leaky_relu(buf.t, bd, cd, buf.t, n, 0.1, dt=_code(dtype))
            want = ER.mean3_leaky_relu(stored, bs, cs, 0.1, dtype)
        torch.cuda.synchronize()
        assert ER.same_out(buf.np(), want, dtype), op


# ---- elementwise helpers -----------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 4 * 70001]


def _cast_source(n, seed):
    x = np.random.default_rng([seed, n]).standard_normal(n).astype(np.float32)
    fam = ER.rounding_family()
    fam = np.roll(fam, -3)                                   # n = 1: a tie (0x3F80 8000)
    k = min(n, fam.size)
    x[:k] = fam[:k]
    if n > 2 * fam.size:
        x[-fam.size:] = fam                                  # and in the last block
    return x


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("src,dst", [("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"),
                                     ("bf16", "bf16")])
def test_cast(cuda, src, dst, n):
    """source and destination one element past a 16-byte boundary; fp32 -> bf16 on exact ties of
    both parities, their neighbours, +-0, +-inf, the overflow to inf, NaN"""
    from fastspeech2 import ops
    sd, stored = _in_dt(cuda, _cast_source(n, 4), src, lead=1)
    out = Out(cuda, n, TORCH_DT[dst], lead=1)
    assert sd.data_ptr() % 16 != 0 and out.t.data_ptr() % 16 != 0
    ops.cast(sd, _code(src), out.t, _code(dst), n)
    torch.cuda.synchronize()
    given = ER.bf16_rne(stored) if src == "bf16" else stored     # bf16: exact, stored is bf16
    want = ER.cast(given, src, dst)
    got = out.np()
    if src == "f32" and dst == "bf16" and n >= 255:
        t = stored.view(np.uint32)
        assert ((t & 0xFFFF) == 0x8000).sum() >= 20 and np.isinf(ER.bf16_to_f32(want)).sum() >= 8
    assert ER.same_out(got, want, dst)


def test_cast_fp32_subnormals_recorded(cuda, parity_log):
    """What fp32 -> bf16 does with fp32 subnormal inputs is recorded, not asserted: the count of
    results that differ from round-to-nearest-even, and how many of those are a signed zero.
    The normal values between them are asserted as everywhere."""
    from fastspeech2 import ops
    sub = ER.subnormal_family()
    x = np.ones(2 * sub.size, np.float32) * np.float32(1.00390625)     # 0x3F808000: a tie
    x[::2] = sub
    out = Out(cuda, x.size, torch.bfloat16, lead=1)
    ops.cast(_in(cuda, x, lead=1), _code("f32"), out.t, _code("bf16"), x.size)
    torch.cuda.synchronize()
    got, want = out.np(), ER.bf16_rne(x)
    assert (got[1::2] == want[1::2]).all()
    diff = got[::2] != want[::2]
    flushed = diff & ((got[::2] & 0x7FFF) == 0)
    print(f"fp32 subnormal -> bf16: {int(diff.sum())} of {sub.size} differ from RNE, "
          f"{int(flushed.sum())} of them flushed to zero")
    parity_log["edge_ops_cast_fp32_subnormal"] = {
        "inputs": int(sub.size), "differ_from_rne": int(diff.sum()),
        "flushed_to_zero": int(flushed.sum())}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fill(cuda, dtype, n):
    from fastspeech2 import ops
    for value in (0.0, -0.0, 1.0 / 3.0, float("inf")):
        out = Out(cuda, n, TORCH_DT[dtype], lead=1)
        ops.fill(out.t, n, value, dt=_code(dtype))
        torch.cuda.synchronize()
        assert _same_bytes(out.np(), ER.fill(n, value, dtype)), value


@pytest.mark.parametrize("alpha", [1.0, -1.0, 0.37])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add(cuda, parity_log, dtype, alpha):
    """X += alpha * Y over four blocks and one element, from unaligned pointers.  alpha = +-1:
    the product is exact and the result is x +- y rounded once, bit for bit.  alpha = 0.37: each
    element is the fused or the unfused candidate; how many took each is recorded."""
    from fastspeech2 import ops
    n = 1025
    r = np.random.default_rng([int(alpha * 100) + 200, n])
    x = r.standard_normal(n).astype(np.float32)
    y = r.standard_normal(n).astype(np.float32)
    x[:64] *= np.float32(2.0 ** -12)
    y[64:128] *= np.float32(2.0 ** -12)
    x[128:160] = -(np.float32(alpha) * y[128:160])           # near cancellation
    x[160], y[161], x[162] = np.inf, np.nan, -0.0
    y[162] = 0.0
    (xd, xs), (yd, ys) = _in_dt(cuda, x, dtype, lead=1), _in_dt(cuda, y, dtype, lead=1)
    out = Out(cuda, n, TORCH_DT[dtype], lead=1)
    out.t.copy_(xd)
    ops.add(out.t, yd, n, alpha, dt=_code(dtype))
    torch.cuda.synchronize()
    got = out.np()
    unf, fus = ER.add(xs, ys, alpha, dtype)
    if abs(alpha) == 1.0:
        assert ER.same_out(unf, fus, dtype)
        assert ER.same_out(got, unf, dtype)
        return
    wide = (lambda v: ER.bf16_to_f32(v)) if dtype == "bf16" else (lambda v: v)
    nan = np.isnan(wide(unf))
    assert (np.isnan(wide(got)) == nan).all() and (np.isnan(wide(fus)) == nan).all()
    eq_u, eq_f = (got == unf) & ~nan, (got == fus) & ~nan
    if dtype == "f32":
        eq_u = (got.view(np.int32) == unf.view(np.int32)) & ~nan
        eq_f = (got.view(np.int32) == fus.view(np.int32)) & ~nan
    counts = {"both": int((eq_u & eq_f).sum()), "fused_only": int((eq_f & ~eq_u).sum()),
              "unfused_only": int((eq_u & ~eq_f).sum()), "neither": int((~eq_u & ~eq_f & ~nan).sum())}
    print(f"fs2_add {dtype} alpha {alpha}: {counts}")
    parity_log[f"edge_ops_add_{dtype}"] = counts
    assert counts["neither"] == 0, counts
