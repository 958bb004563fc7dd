"""Test helper: the references of the AdamW kernels (csrc/optim.hip), no GPU.

``adamw_step`` is one update in numpy from the eight kernel scalars of
``FusedAdamW.begin_step``.  In float64 it is the mathematical reference; in float32 it is the
arithmetic ``adamw_elem`` documents, op for op, one rounding per op and no fused multiply-add
(numpy rounds every float32 op once and keeps float32 denormals).  The scalars are rounded to
fp32 first in both modes, as ctypes ``c_float`` rounds them on the way into the C ABI, so both
modes describe the same operation on the same inputs.

``bounds`` is the per-element error bound of the fp32 arithmetic against the float64 one
(Check B of test_gpu_adamw.py), derived from the op count below -- never from what a kernel
gives.  ``images`` is the expected pair of GEMM weight images of an [O][KW][C] master, written
as index arithmetic from the description of ``w_okc`` in include/fs2_hip.h.  ``build_case``
lays weights and element-wise ranges into flat buffers with un-owned gaps between them.

The error bound.  u = 2^-24; every fp32 op returns its exact result times (1 + d), |d| <= u,
unless the result is denormal (then the error is at most 2^-150 absolute); sums and differences
that land in the denormal range are exact.  With gr = g*gs (1 rounding), M = |m0| + |gr|:

* m, arm w1 < 0.5, ``m0 + w1*(gr - m0)``: the difference carries u|gr| from gr and its own
  u(|gr| + |m0|); the product adds u w1 (|gr| + |m0|); the sum adds u|m'|, |m'| <= |m0| +
  w1 (|gr| + |m0|).  Total u (w1|gr| + 3 w1 M + |m0|) <= u (4 w1 + 1) M <= 3 u M.
  Arm w1 >= 0.5, ``gr - (gr - m0)*(1 - w1)``: 1 - w1 is exact (Sterbenz); the same chain gives
  u (2|gr| + (1 - w1)|gr| + 3 (1 - w1) M) <= 4 u M.  C_M = 4.
* v, ``v0*b2 + (omb2*gr)*gr``, all terms >= 0 so relative errors do not grow: (omb2*gr)*gr
  carries 1 + 1 + 1 + 1 roundings (gr twice), v0*b2 one, the sum one more: C_V = 5, on normal
  v'.  Each of the three products may be denormal: 3 * 2^-150 < 2^-148 absolute on top.
* p, ``p0*decay + (-ss)*(m/denom)``, denom = sqrt(v)/bc2_sqrt + eps: sqrt halves v's 5u and
  adds u (3.5u), the division u, the sum with eps (positive terms) u: denom within 5.5u.  The
  quotient m/denom: dm/denom + (5.5u + u)|m'|/denom <= (C_M + 6.5) u M/denom; times ss adds
  one u: 11.5 u ss M/denom.  p0*decay carries u|p0|, the final sum u|p'| <= u(|p0| + ss M/denom).
  Total u (2|p0| + 12.5 ss M/denom): C_P = 2, C_U = 12.5.  A denormal v moves sqrt(v) by at
  most sqrt(2^-148) = 2^-74, i.e. the update by its 2^-74/(bc2_sqrt*denom) part.

Second-order terms (products of two roundings) are below 2^-20 of the first-order ones; the
bounds carry a factor 1 + 2^-10 for them.  These are absolute bounds in units of 2^-24;
relative ones fail for the reference itself: m cancels in m0 + w1 (gr - m0), so |dm|/|m'|
reaches thousands of ulps, and |dp| hundreds of ulps of p.
"""
import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53
C_M, C_V, C_P, C_U = 4.0, 5.0, 2.0, 12.5
SLACK = 1.0 + 2.0 ** -10
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)      # smallest normal

FAMILIES = ("unit", "spread", "zeros", "huge", "nonfinite")
# (t, betas, grad_scale, weight_decay, lr): t in {1, 2, 1000, 100000}, both lerp arms,
# grad_scale {1, 1/2, 1/3}, weight_decay {0, 1e-2} and lr = 0, every value at least twice
SCALAR_CASES = [
    (1, (0.9, 0.999), 1.0, 1e-2, 1e-3),
    (2, (0.3, 0.9), 0.5, 0.0, 1e-3),
    (1000, (0.9, 0.999), 1.0 / 3.0, 1e-2, 1e-4),
    (100000, (0.3, 0.9), 1.0, 1e-2, 1e-3),
    (1000, (0.3, 0.9), 1.0 / 3.0, 0.0, 0.0),
    (1, (0.3, 0.9), 1.0 / 3.0, 1e-2, 1e-3),
    (100000, (0.9, 0.999), 0.5, 0.0, 1e-3),
    (2, (0.9, 0.999), 1.0, 1e-2, 0.0),
]


def scalars(t, betas=(0.9, 0.999), grad_scale=1.0, weight_decay=1e-2, lr=1e-3, eps=1e-8):
    """The eight kernel scalars of step t, in Python double as torch's single-tensor AdamW
    computes them: (decay_mul, 1-b1, b2, 1-b2, step_size, bc2_sqrt, eps, grad_scale)."""
    b1, b2 = betas
    bc1 = 1 - b1 ** t
    bc2 = 1 - b2 ** t
    return (1 - lr * weight_decay, 1 - b1, b2, 1 - b2, lr / bc1, bc2 ** 0.5, eps, grad_scale)


def adamw_step(p, m, v, g, scal, dtype, scalars_fp32=True):
    """One AdamW update of (p, m, v) by g; returns new (p, m, v) in ``dtype``.  ``scal`` as
    FusedAdamW.begin_step returns it, rounded to fp32 first (``scalars_fp32=False`` keeps the
    doubles: only for the comparison with torch's float64 AdamW, which never rounds them)."""
    dtype = np.dtype(dtype).type
    if scalars_fp32:
        scal = [np.float32(x) for x in scal]
    decay, w1, b2, omb2, ss, bc2s, eps, gs = (dtype(x) for x in scal)
    p, m, v, g = (np.asarray(a).astype(dtype) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        gr = g * gs
        p = p * decay
        if w1 < dtype(0.5):
            m = m + w1 * (gr - m)
        else:
            m = gr - (gr - m) * (dtype(1) - w1)
        v = v * b2 + (omb2 * gr) * gr
        denom = np.sqrt(v) / bc2s + eps
        p = p + (-ss) * (m / denom)
    assert p.dtype == dtype and m.dtype == dtype and v.dtype == dtype
    return p, m, v


def bounds(p0, m0, v0, g, scal, u=U24, denormal=True):
    """(ref, bound, scale): ``ref`` the float64 (p', m', v') of one step, ``bound`` the largest
    |fp32 - ref| the derivation in the module docstring allows per element, ``scale`` what the
    bound's constants multiply (m: u M; v: u v'; p: the bound itself), for reporting an
    observed error in the bound's own units.  ``u`` = 2^-53 with ``denormal=False`` bounds two
    float64 evaluations against each other."""
    ref = adamw_step(p0, m0, v0, g, scal, np.float64)
    s = [float(np.float32(x)) for x in scal]
    _, _, _, _, ss, bc2s, eps, gs = s
    p0, m0, g = (np.asarray(a).astype(np.float64) for a in (p0, m0, g))
    with np.errstate(all="ignore"):
        M = np.abs(m0) + np.abs(g * gs)
        denom = np.sqrt(ref[2]) / bc2s + eps
        q = 2.0 ** -148 if denormal else 0.0
        bm = C_M * u * M * SLACK
        bv = C_V * u * ref[2] * SLACK + q
        upd = ss * M / denom
        bp = u * (C_P * np.abs(p0) + C_U * upd) * SLACK
        if denormal:
            bp = bp + upd * (2.0 ** -74 / bc2s) / denom
    return ref, (bp, bm, bv), (bp, u * M, u * ref[2])


def classify(ref):
    """Element classes of a float64 result: ``fin`` -- p', m', v' all finite and inside fp32's
    range, where Check B applies; ``ovf`` -- finite in float64 but v' beyond fp32 (g*g
    overflows: fp32 gives v = inf, denom = inf and a zero update, p = p0*decay); the rest is
    non-finite in float64 too, and fp32 must give the same infinities and NaNs."""
    p, m, v = ref
    finite = np.isfinite(p) & np.isfinite(m) & np.isfinite(v)
    ovf = finite & (v > 2.0 ** 128)
    fin = finite & (v < 2.0 ** 127) & (np.abs(m) < 2.0 ** 127) & (np.abs(p) < 2.0 ** 127)
    assert not (finite & ~ovf & ~fin).any(), "an input on the edge of fp32's range"
    return fin, ovf, ~finite


def check_b(got, p0, m0, v0, g, scal):
    """Check B.  ``got`` = fp32 (p, m, v).  Returns (violations, figures): violations is a list
    of strings (empty when the bound holds everywhere), figures the observed maxima in the
    bound's units: ``m`` in 2^-24 (|m0| + |gr|) against C_M, ``v`` in 2^-24 v' on normal v'
    against C_V, ``v_denormal`` in 2^-149 absolute, ``p`` as a fraction of its bound."""
    ref, bnd, scale = bounds(p0, m0, v0, g, scal)
    fin, ovf, bad = classify(ref)
    bad_out, figs = [], {"m": 0.0, "v": 0.0, "v_denormal": 0.0, "p": 0.0}
    g32 = [np.asarray(a, dtype=np.float32) for a in got]
    with np.errstate(all="ignore"):
        for name, x, r, b, sc in zip("pmv", g32, ref, bnd, scale):
            err = np.abs(x.astype(np.float64) - r)
            sel = fin if name != "m" else (fin | ovf)
            if not np.isfinite(x[sel]).all():
                bad_out.append(f"{name}: non-finite where the reference is finite")
                continue
            over = sel & (err > b)
            if over.any():
                i = int(np.argmax(np.where(sel, err / np.maximum(b, 1e-300), 0)))
                bad_out.append(f"{name}[{i}]: |err| {err[i]:.3e} > bound {b[i]:.3e} "
                               f"({int(over.sum())} elements)")
            if name == "v":
                normal = sel & (r >= FLT_MIN)
                den = sel & (r < FLT_MIN)
                if normal.any():
                    figs["v"] = float((err[normal] / sc[normal]).max())
                if den.any():
                    figs["v_denormal"] = float(err[den].max() / 2.0 ** -149)
            else:
                nz = sel & (sc > 0)
                if nz.any():
                    figs[name] = float((err[nz] / sc[nz]).max())
                if (sel & (sc == 0) & (err > 0)).any():
                    bad_out.append(f"{name}: an error where the bound is zero")
        # fp32 overflow of g*g: v = +inf, and the update vanishes
        if ovf.any():
            if not (g32[2][ovf] == np.inf).all():
                bad_out.append("v: not +inf where g*g overflows fp32")
            pd = np.abs(g32[0][ovf].astype(np.float64)
                        - np.asarray(p0, np.float64)[ovf] * float(np.float32(scal[0])))
            if (pd > U24 * np.abs(np.asarray(p0, np.float64)[ovf]) * SLACK).any():
                bad_out.append("p: not p0*decay where g*g overflows fp32")
        # non-finite in float64: the same class in fp32 (NaN, or the same infinity)
        for name, x, r in zip("pmv", g32, ref):
            xr, rr = x[bad], r[bad]
            same = (np.isnan(xr) & np.isnan(rr)) | (xr.astype(np.float64) == rr) | np.isfinite(rr)
            if not same.all():
                bad_out.append(f"{name}: another non-finite class than float64")
    return bad_out, figs


def same_bits(a, b):
    """fp32 arrays equal bit for bit, NaNs (any payload) in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~nb]).all())


def make_state(family, n, seed):
    """(p, m, v, g), fp32, of one input family: a random optimiser state, never 'zero moments'"""
    assert family in FAMILIES
    r = np.random.default_rng([seed, FAMILIES.index(family), n])
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    if family == "spread":
        mag = lambda: np.exp(r.uniform(-50, 10, n)) * r.choice([-1.0, 1.0], n)
        p, m, g = f(mag()), f(mag()), f(mag())
        v = f(np.exp(r.uniform(-50, 10, n))) ** 2       # fp32 square: denormal below ~e^-43
        return p, m, f(v), g
    p, m, g = (f(r.standard_normal(n)) for _ in range(3))
    v = f(r.standard_normal(n) ** 2)
    i = np.arange(n)
    if family == "zeros":
        k = r.integers(0, 8, n)                         # bit 0: g, bit 1: m, bit 2: v
        k[: min(n, 8)] = np.arange(min(n, 8))           # all-zero first, every mix after it
        g[(k & 1) == 0] = 0
        m[(k & 2) == 0] = 0
        v[(k & 4) == 0] = 0
        if n > 3:
            g[3] = -0.0
    elif family == "huge":
        big = (i % 2) == 0
        g[big] = f(1e25 * r.uniform(0.5, 2.0, n) * r.choice([-1.0, 1.0], n))[big]
    elif family == "nonfinite":
        for j, val in enumerate((np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf)):
            g[(j * 701 + (n - 1) * (j % 2)) % n] = val
        g[n - 1] = np.nan
    return p, m, v, g


# ---- weight images ---------------------------------------------------------------------------
def images(W, O, C, KW, okc, ldf, ldb):
    """(Wf, Wb, wb_written) of a master W[O][KW][C]: Wf[O][ldf] with element (o, tap j,
    channel c) in column j*C + c, or with bit 3 (C % 64 == 0) in (c/64)*KW*64 + j*64 + c%64,
    and zeros in the columns from KW*C on; Wb[C][ldb] with it in row c, tap position
    jb = KW-1-j with bit 1 (taps reversed) else j, column jb*O + o, or with bit 2
    (O % 64 == 0) (o/64)*KW*64 + jb*64 + o%64.  Wb's columns from KW*O on are not written:
    NaN here, False in ``wb_written``.  (Bit 0 says how the master itself is stored; this
    function always takes [O][KW][C].)"""
    W = np.asarray(W).reshape(O, KW, C)
    assert ldf >= KW * C and ldb >= KW * O
    assert not (okc & 8) or (C % 64 == 0 and ldf == KW * C)
    assert not (okc & 4) or O % 64 == 0
    o, j, c = np.indices((O, KW, C))
    Wf = np.zeros((O, ldf), dtype=W.dtype)
    kf = (c // 64) * (KW * 64) + j * 64 + c % 64 if okc & 8 else j * C + c
    Wf[o, kf] = W
    Wb = np.full((C, ldb), np.nan, dtype=W.dtype)
    written = np.zeros((C, ldb), dtype=bool)
    jb = KW - 1 - j if okc & 2 else j
    col = (o // 64) * (KW * 64) + jb * 64 + o % 64 if okc & 4 else jb * O + o
    Wb[c, col] = W
    written[c, col] = True
    assert written[:, :KW * O].all() and not written[:, KW * O:].any()
    return Wf, Wb, written


# ---- flat layouts ----------------------------------------------------------------------------
class Weight:
    """one GEMM weight of a case: flat offset and the descriptor's fields"""

    def __init__(self, off, O, C, KW, okc, ldf, ldb, wb):
        self.off, self.O, self.C, self.KW, self.okc = off, O, C, KW, okc
        self.ldf, self.ldb, self.wb = ldf, ldb, wb
        self.numel = O * KW * C

    def vector_form(self, bf16=True):
        """the condition under which adamw_prep_tiles_kernel takes its 16-byte form"""
        KC = self.KW * self.C
        return bool(bf16 and self.off % 4 == 0 and KC % 4 == 0 and self.ldf % 4 == 0 and
                    (not self.wb or (self.ldb % 4 == 0 and self.O % 4 == 0)))


class Case:
    def __init__(self, n, weights, ranges, owned):
        self.n, self.weights, self.ranges, self.owned = n, weights, ranges, owned


def build_case(weights=(), ranges=(), seed=0, lead=0):
    """Lay weights, then ranges, into one flat buffer, each after a gap of 1..11 un-owned
    elements.  ``weights``: dicts with O, C, KW, okc and optionally ldf, ldb (default: KW*C
    rounded up to 8; KW*O), wb (False: no Wb), mod (flat offset mod 4, default 0).  ``ranges``:
    (length, mod) pairs, mod = start mod 4 (None: wherever the gap ends).  Returns a Case: total
    size n, the Weight entries, the (start, length) range list and the boolean mask of owned
    elements.  ``lead``: extra un-owned elements in front."""
    r = np.random.default_rng([seed, 77])
    cur, ws, rs = lead, [], []

    def place(mod):
        s = cur + int(r.integers(1, 12))
        if mod is not None:
            s += (mod - s) % 4
        return s

    for w in weights:
        O, C, KW = w["O"], w["C"], w["KW"]
        off = place(w.get("mod", 0))
        ws.append(Weight(off, O, C, KW, w["okc"], w.get("ldf", (KW * C + 7) // 8 * 8),
                         w.get("ldb", KW * O), w.get("wb", True)))
        cur = off + O * KW * C
    for ln, mod in ranges:
        st = place(mod)
        rs.append((st, ln))
        cur = st + ln
    n = cur + int(r.integers(1, 12))
    owned = np.zeros(n, dtype=bool)
    for w in ws:
        assert not owned[w.off:w.off + w.numel].any()
        owned[w.off:w.off + w.numel] = True
    for st, ln in rs:
        assert not owned[st:st + ln].any()
        owned[st:st + ln] = True
    return Case(n, ws, rs, owned)


def expected_tables(case):
    """what ops.weight_prep_table and ops.adamw_ranges_table must compute for a case:
    ([tile0...], [tiles_k...], total_tiles), ([first block...], range_blocks)"""
    t0, t0s, tks = 0, [], []
    for w in case.weights:
        tk = -(-w.ldf // 64)
        t0s.append(t0)
        tks.append(tk)
        t0 += -(-w.O // 64) * tk
    b0, b0s = 0, []
    for _, ln in case.ranges:
        b0s.append(b0)
        b0 += -(-ln // 1024)
    return (t0s, tks, t0), (b0s, b0)


# ---- the fused cases (shared by the host and the GPU tests) ------------------------------------
def _w(O, C, KW, okc, **kw):
    return dict(O=O, C=C, KW=KW, okc=okc, **kw)


MIXED_WEIGHTS = [
    _w(130, 72, 5, 1), _w(136, 72, 9, 3),        # tile edges in both directions
    _w(80, 773, 1, 0),                           # KC odd: the scalar form in bf16 (concat_proj)
    _w(192, 72, 5, 7), _w(128, 128, 3, 15),      # tap-inner Wb; tap-inner Wf as well
    _w(66, 6, 2, 1),                             # quads straddle a tap; O % 4 != 0: scalar form
    _w(68, 8, 3, 1),                             # vector form, O % 64 != 0
    _w(70, 40, 3, 1, wb=False),                  # no Wb
    _w(64, 24, 3, 1, ldf=72 + 128),              # ldf two tiles wider than KC: zero tiles
    _w(72, 20, 3, 1, ldb=3 * 72 + 12),           # Wb columns beyond KW*O: not written
]
RANGE_LENGTHS = [1, 3, 4, 5, 1023, 0, 1024, 1025, 4097, 0]     # an empty one inside, one at the end
MIXED_RANGES = [(ln, (1, 2, 3, None, 0)[i % 5]) for i, ln in enumerate(RANGE_LENGTHS)]
ALIGNED_WEIGHT = _w(68, 8, 3, 1)                 # KC, ldf, ldb, O all multiples of 4


def named_case(name):
    if name == "mixed":
        return build_case(MIXED_WEIGHTS, MIXED_RANGES, seed=1)
    if name == "weights_only":
        return build_case(MIXED_WEIGHTS, (), seed=2)
    if name == "ranges_only":
        return build_case((), MIXED_RANGES, seed=3)
    if name == "table256":                       # the descriptor limit, one tile each
        return build_case([_w(8, 8, 1, i & 1) for i in range(256)], (), seed=4)
    if name == "ranges300":
        r = np.random.default_rng(5)
        return build_case((), [(int(r.integers(0, 40)), None) for _ in range(300)], seed=5)
    if name.startswith("single"):                # one weight of the mixed list alone
        return build_case([MIXED_WEIGHTS[int(name[6:])]], (), seed=6)
    if name.startswith("offset"):                # the aligned weight at flat offset = k (mod 4)
        return build_case([dict(ALIGNED_WEIGHT, mod=int(name[6:]))], (), seed=7)
    raise KeyError(name)
