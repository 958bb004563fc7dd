"""GPU: fs2_adamw and fs2_adamw_prep (csrc/optim.hip) against two anchors.

Check A, exactness: p, m and v equal the fp32 restatement (tests/adamw_restatement.py: the
kernel's documented arithmetic in numpy, one rounding per op, no fused multiply-add) bit for
bit, NaNs in the same places.  Check B: every element is within the derived absolute bound of
the float64 evaluation of the same step (constants from the op count, see the restatement's
docstring; the references themselves are held to it in test_adamw_host.py), so the restatement
cannot repeat a mistake of the kernel unnoticed.  Chains of steps are checked step by step, each
from the kernel's own previous state: as strong as a propagated bound and simpler.

Every buffer sits between guard zones of alternating NaN and finite words (an update of a NaN
stays NaN, so NaN alone would not show a stray *update*); guards, un-owned elements of the flat
buffers and all of ``grad`` must come back bit for bit.  The fused pass is also compared with
the unfused pair fs2_adamw + fs2_weight_prep_batched.  Observed maxima go through ``parity_log``.
"""
import numpy as np
import pytest
import torch

import adamw_restatement as AR

pytestmark = pytest.mark.gpu

G = 64        # guard words on each side: a multiple of 4, so the guarded view stays 16-byte aligned


def _log_max(parity_log, key, figs):
    old = parity_log.setdefault(key, {})
    for k, x in figs.items():
        old[k] = max(old.get(k, 0.0), float(x))


def _guard(n, dtype=torch.float32):
    g = torch.full((n,), float("nan"), dtype=torch.float32)
    g[1::2] = torch.arange(1, n // 2 + 1, dtype=torch.float32) * 0.75 - 7.0
    return g.to(dtype)


def _guarded(x, cuda, shift=0):
    """device buffer [guard | shift words | x | guard]; returns (whole, view of x, host copy of
    whole).  shift = 1 moves x off 16-byte alignment."""
    x = torch.as_tensor(x)
    whole = torch.cat([_guard(G + shift, x.dtype), x.reshape(-1), _guard(G, x.dtype)])
    dev = whole.to(cuda)
    return dev, dev[G + shift:G + shift + x.numel()], whole


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _guards_intact(dev, host, n, shift=0):
    a, b = _bits(dev), _bits(host)
    lo = G + shift
    return bool(torch.equal(a[:lo], b[:lo]) and torch.equal(a[lo + n:], b[lo + n:]))


def _scal(case):
    t, betas, gs, wd, lr = AR.SCALAR_CASES[case]
    return AR.scalars(t, betas, gs, wd, lr)


def _run_adamw(cuda, state, scal, misalign=None):
    """fs2_adamw on guarded copies of (p, m, v, g); checks guards and grad; returns fp32 numpy
    (p, m, v)"""
    from fastspeech2 import ops
    n = state[0].size
    bufs = [_guarded(x, cuda, shift=int(misalign == k)) for k, x in zip("pmvg", state)]
    (_, p, _), (_, m, _), (_, v, _), (_, g, _) = bufs
    assert all((b[1].data_ptr() % 16 == 0) == (misalign != k) for k, b in zip("pmvg", bufs))
    ops.adamw(p, g, m, v, n, *scal)
    torch.cuda.synchronize()
    for k, (dev, _, host) in zip("pmvg", bufs):
        assert _guards_intact(dev, host, n, int(misalign == k)), f"guard of {k} written"
    assert torch.equal(_bits(g), _bits(torch.from_numpy(state[3]))), "grad written"
    return tuple(x.cpu().numpy() for x in (p, m, v))


def _check_a(got, want):
    return [f"{name}: {int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} words "
            f"differ from the fp32 restatement"
            for name, a, b in zip("pmv", got, want) if not AR.same_bits(a, b)]


def _check_step(got, state, scal, parity_log=None, key=None):
    """both checks are evaluated before either is asserted, so a failure says which anchor"""
    p, m, v, g = state
    bad_a = _check_a(got, AR.adamw_step(p, m, v, g, scal, np.float32))
    bad_b, figs = AR.check_b(got, p, m, v, g, scal)
    print(key, figs)
    if parity_log is not None:
        _log_max(parity_log, key, figs)
    assert not bad_a and not bad_b, {"check A": bad_a, "check B": bad_b}


@pytest.mark.parametrize("case", range(len(AR.SCALAR_CASES)))
@pytest.mark.parametrize("family", AR.FAMILIES)
def test_adamw_one_step_from_a_random_state(cuda, parity_log, family, case):
    """n = 4099 (vector kernel + a 3-element tail), every input family x every scalar case:
    t in {1, 2, 1000, 100000}, both lerp arms, grad_scale {1, 1/2, 1/3}, weight_decay {0, 1e-2},
    lr = 0 (p moves by the decay only)."""
    scal = _scal(case)
    state = AR.make_state(family, 4099, 10 + case)
    got = _run_adamw(cuda, state, scal)
    _check_step(got, state, scal, parity_log, f"adamw_kernel_{family}")
    if AR.SCALAR_CASES[case][4] == 0.0:
        decay = np.float32(scal[0])
        keep = ~np.isnan(got[0])
        assert AR.same_bits((state[0] * decay)[keep], got[0][keep])


@pytest.mark.parametrize("misalign", [None, "p", "g", "m", "v"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027, 4099])
def test_adamw_sizes_and_alignment(cuda, n, misalign):
    """n below one quad, at and around the 1024-element block, with a tail; all four pointers
    16-byte aligned, and each in turn one float off so the whole buffer takes the scalar
    kernel.  Families and scalar cases rotate with n so both lerp arms meet both kernels."""
    k = [1, 3, 4, 5, 1023, 1024, 1027, 4099].index(n)
    family = AR.FAMILIES[k % len(AR.FAMILIES)]
    scal = _scal((k + (misalign is not None)) % len(AR.SCALAR_CASES))
    state = AR.make_state(family, n, 50 + k)
    got = _run_adamw(cuda, state, scal, misalign)
    _check_step(got, state, scal)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9)])
@pytest.mark.parametrize("family", ["unit", "spread", "zeros"])
def test_adamw_chain_of_steps(cuda, parity_log, family, betas):
    """four steps from a random state at t = 7, fresh gradients each step, every step checked
    from the kernel's own previous state (both anchors)"""
    n = 1027
    p, m, v, _ = AR.make_state(family, n, 70)
    for k in range(4):
        g = AR.make_state(family, n, 71 + k)[3]
        scal = AR.scalars(7 + k, betas, 0.5, 1e-2, 1e-3)
        got = _run_adamw(cuda, (p, m, v, g), scal)
        _check_step(got, (p, m, v, g), scal, parity_log, f"adamw_kernel_chain_{family}")
        p, m, v = got


# ---- fs2_adamw_prep ---------------------------------------------------------------------------
def _torch_dt(dt):
    return torch.bfloat16 if dt == 1 else torch.float32


class _Fused:
    """device state of one case: the four guarded flat buffers and a guarded image pair per
    weight"""

    def __init__(self, cuda, case, state, dt):
        self.case, self.state, self.dt, self.cuda = case, state, dt, cuda
        self.flat = [_guarded(x, cuda) for x in state]               # p, m, v, g
        self.p, self.m, self.v, self.g = (b[1] for b in self.flat)
        assert all(x.data_ptr() % 16 == 0 for x in (self.p, self.m, self.v, self.g))
        td = _torch_dt(dt)
        self.wf, self.wb = [], []
        for w in case.weights:
            nan = lambda k: torch.full((k,), float("nan"), dtype=td)
            self.wf.append(_guarded(nan(w.O * w.ldf), cuda))
            self.wb.append(_guarded(nan(w.C * w.ldb), cuda) if w.wb else None)

    def entries(self):
        return [(self.p[w.off:w.off + w.numel], w.O, w.C, w.KW, w.okc, f[1], w.ldf,
                 b[1] if b else None, w.ldb)
                for w, f, b in zip(self.case.weights, self.wf, self.wb)]

    def run_fused(self, scal, weights=True, ranges=True):
        from fastspeech2 import ops
        c = self.case
        ent = self.entries()
        wt = ops.weight_prep_table(ent) if weights and ent else (None, 0, 0)
        rt = ops.adamw_ranges_table(c.ranges if ranges else [], self.cuda)
        (t0s, tks, tot), (b0s, blocks) = AR.expected_tables(c)
        assert not (weights and ent) or wt[2] == tot
        assert not ranges or rt[2] == blocks
        ops.adamw_prep(wt, rt, self.p, self.g, self.m, self.v, *scal, dt=self.dt)
        torch.cuda.synchronize()

    def run_unfused(self, scal):
        """fs2_adamw per owned slice, then fs2_weight_prep_batched over the same table"""
        from fastspeech2 import ops
        c = self.case
        for off, n in [(w.off, w.numel) for w in c.weights] + list(c.ranges):
            if n:
                s = slice(off, off + n)
                ops.adamw(self.p[s], self.g[s], self.m[s], self.v[s], n, *scal)
        ent = self.entries()
        if ent:
            table = ops.weight_prep_table(ent)
            ops.weight_prep_batched(*table, dt=self.dt)
        torch.cuda.synchronize()

    def host(self):
        return tuple(x.cpu().numpy() for x in (self.p, self.m, self.v))

    def check(self, scal, owned, parity_log=None, key=None):
        """both anchors on ``owned``, everything else and the guards untouched, grad untouched,
        the images those of the updated p"""
        c, (p0, m0, v0, g0) = self.case, self.state
        got = self.host()
        want = AR.adamw_step(p0, m0, v0, g0, scal, np.float32)
        for name, a, b, old in zip("pmv", got, want, (p0, m0, v0)):
            assert AR.same_bits(a[owned], b[owned]), f"{name}: owned elements differ"
            assert AR.same_bits(a[~owned], old[~owned]), f"{name}: un-owned elements written"
        for name, (dev, _, hostcopy) in zip("pmvg", self.flat):
            assert _guards_intact(dev, hostcopy, c.n), f"guard of {name} written"
        assert torch.equal(_bits(self.g), _bits(torch.from_numpy(g0))), "grad written"
        if owned.any():
            sel = [x[owned] for x in (p0, m0, v0, g0)]
            bad, figs = AR.check_b([x[owned] for x in got], *sel, scal)
            print(key, figs)
            if parity_log is not None:
                _log_max(parity_log, key, figs)
            assert not bad, bad
        return got

    def check_images(self, p_new, which=None):
        td = _torch_dt(self.dt)
        for i, (w, f, b) in enumerate(zip(self.case.weights, self.wf, self.wb)):
            if which is not None and i not in which:
                continue
            W = p_new[w.off:w.off + w.numel]
            Wf, Wb, written = AR.images(W, w.O, w.C, w.KW, w.okc, w.ldf, w.ldb)
            tag = f"weight {i} {(w.O, w.C, w.KW, w.okc)}"
            assert _guards_intact(f[0], f[2], w.O * w.ldf), f"{tag}: Wf guard written"
            want = _bits(torch.from_numpy(Wf).to(td)).reshape(w.O, w.ldf)
            have = _bits(f[1]).reshape(w.O, w.ldf)
            KC = w.KW * w.C
            assert torch.equal(have[:, :KC], want[:, :KC]), f"{tag}: Wf"
            assert not have[:, KC:].any(), f"{tag}: Wf padding columns not zero"
            if not w.wb:
                continue
            assert _guards_intact(b[0], b[2], w.C * w.ldb), f"{tag}: Wb guard written"
            want = _bits(torch.from_numpy(np.nan_to_num(Wb)).to(td)).reshape(w.C, w.ldb)
            have = _bits(b[1]).reshape(w.C, w.ldb)
            old = _bits(b[2][G:G + w.C * w.ldb]).reshape(w.C, w.ldb)
            wr = torch.from_numpy(written)
            assert torch.equal(have[wr], want[wr]), f"{tag}: Wb"
            assert torch.equal(have[~wr], old[~wr]), f"{tag}: Wb columns beyond KW*O written"

    def images_bits(self):
        return [(_bits(f[0]), _bits(b[0]) if b else None) for f, b in zip(self.wf, self.wb)]


def _fused_state(case, family="unit", seed=90):
    return AR.make_state(family, case.n, seed)


SCAL_FUSED = AR.scalars(1000, (0.9, 0.999), 0.5, 1e-2, 1e-3)
SCAL_FUSED_ARM2 = AR.scalars(2, (0.3, 0.9), 1.0 / 3.0, 1e-2, 1e-3)


def _same_as_unfused(cuda, case, state, scal, dt, fused):
    ref = _Fused(cuda, case, state, dt)
    ref.run_unfused(scal)
    for name, a, b in zip("pmv", fused.host(), ref.host()):
        assert AR.same_bits(a, b), f"{name}: fused != fs2_adamw"
    for i, ((f1, b1), (f2, b2)) in enumerate(zip(fused.images_bits(), ref.images_bits())):
        assert torch.equal(f1, f2), f"weight {i}: Wf fused != fs2_weight_prep_batched"
        assert b1 is None or torch.equal(b1, b2), f"weight {i}: Wb"


@pytest.mark.parametrize("dt", [1, 0], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name,family,scal", [
    ("mixed", "unit", SCAL_FUSED), ("mixed", "spread", SCAL_FUSED_ARM2),
    ("weights_only", "unit", SCAL_FUSED_ARM2), ("ranges_only", "spread", SCAL_FUSED),
    ("table256", "unit", SCAL_FUSED), ("ranges300", "unit", SCAL_FUSED_ARM2)],
    ids=["mixed", "mixed_spread_arm2", "weights_only", "ranges_only", "table256", "ranges300"])
def test_adamw_prep_layouts(cuda, parity_log, name, family, scal, dt):
    """One call over a whole layout: the ten weights of MIXED_WEIGHTS (vector and scalar forms,
    every w_okc bit, no Wb, zero padding tiles, an ldb wider than KW*O) and the ranges of every
    edge length with empty ones among them; weights alone (n_ranges = 0), ranges alone (n = 0);
    256 one-tile weights (the descriptor limit: the search's both ends); 300 short ranges."""
    case = AR.named_case(name)
    state = _fused_state(case, family)
    f = _Fused(cuda, case, state, dt)
    f.run_fused(scal)
    got = f.check(scal, case.owned, parity_log, f"adamw_prep_{'bf16' if dt else 'fp32'}_{family}")
    f.check_images(got[0])
    _same_as_unfused(cuda, case, state, scal, dt, f)


@pytest.mark.parametrize("part", ["weights", "ranges"])
def test_adamw_prep_part_of_a_layout(cuda, part):
    """the mixed layout with only its weights in the call (n_ranges = 0), then only its ranges
    (n = 0): the other part's elements are un-owned and stay, its images stay NaN"""
    case = AR.named_case("mixed")
    state = _fused_state(case)
    f = _Fused(cuda, case, state, 1)
    f.run_fused(SCAL_FUSED, weights=part == "weights", ranges=part == "ranges")
    owned = np.zeros(case.n, dtype=bool)
    if part == "weights":
        for w in case.weights:
            owned[w.off:w.off + w.numel] = True
    else:
        for st, ln in case.ranges:
            owned[st:st + ln] = True
    got = f.check(SCAL_FUSED, owned)
    if part == "weights":
        f.check_images(got[0])
    else:
        for (dev, _, hostcopy) in f.wf + [b for b in f.wb if b]:
            assert torch.equal(_bits(dev), _bits(hostcopy)), "an image written with n = 0"


@pytest.mark.parametrize("dt", [1, 0], ids=["bf16", "fp32"])
@pytest.mark.parametrize("i", range(len(AR.MIXED_WEIGHTS)))
def test_adamw_prep_each_weight_alone(cuda, i, dt):
    """every weight of the mixed layout in a call of its own, so a failure names its shape"""
    case = AR.named_case(f"single{i}")
    state = _fused_state(case, "unit", 100 + i)
    f = _Fused(cuda, case, state, dt)
    f.run_fused(SCAL_FUSED_ARM2)
    got = f.check(SCAL_FUSED_ARM2, case.owned)
    f.check_images(got[0])
    _same_as_unfused(cuda, case, state, SCAL_FUSED_ARM2, dt, f)


@pytest.mark.parametrize("dt", [1, 0], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mod", [1, 2, 3])
def test_adamw_prep_flat_offset_not_a_quad(cuda, mod, dt):
    """an aligned weight (KC, ldf, ldb, O multiples of 4) at flat offset = 1, 2, 3 (mod 4) takes
    the scalar form; its parameters, moments and images equal the offset-0 (vector form) run's
    bit for bit"""
    outs = []
    for k in (0, mod):
        case = AR.named_case(f"offset{k}")
        w = case.weights[0]
        assert w.off % 4 == k and w.vector_form(dt == 1) == (k == 0 and dt == 1)
        src = AR.make_state("unit", w.numel, 120)
        state = tuple(np.ascontiguousarray(x) for x in AR.make_state("unit", case.n, 121))
        for dst, s in zip(state, src):
            dst[w.off:w.off + w.numel] = s
        f = _Fused(cuda, case, state, dt)
        f.run_fused(SCAL_FUSED)
        got = f.check(SCAL_FUSED, case.owned)
        f.check_images(got[0])
        sl = slice(w.off, w.off + w.numel)
        outs.append(([x[sl] for x in got], _bits(f.wf[0][1]), _bits(f.wb[0][1])))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert AR.same_bits(a, b)
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_adamw_prep_kw1_layout_bit_is_immaterial(cuda):
    """KW = 1: [O][C][KW] and [O][KW][C] coincide, so w_okc bit 0 clear and set give the same
    parameters, moments and images"""
    outs = []
    for okc in (0, 1):
        case = AR.build_case([dict(O=80, C=773, KW=1, okc=okc), dict(O=68, C=24, KW=1, okc=okc)],
                             seed=8)
        state = _fused_state(case, "unit", 130)
        f = _Fused(cuda, case, state, 1)
        f.run_fused(SCAL_FUSED)
        got = f.check(SCAL_FUSED, case.owned)
        f.check_images(got[0])
        outs.append((got, f.images_bits()))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert AR.same_bits(a, b)
    for (f1, b1), (f2, b2) in zip(outs[0][1], outs[1][1]):
        assert torch.equal(f1, f2) and torch.equal(b1, b2)


@pytest.mark.parametrize("dt", [1, 0], ids=["bf16", "fp32"])
def test_adamw_prep_zero_step_writes_the_images_of_p(cuda, dt):
    """decay 1, step size 0, zero gradient and moments: p comes back bit for bit, m and v stay
    zero, and the images are those of p"""
    case = AR.named_case("mixed")
    p = AR.make_state("unit", case.n, 140)[0]
    z = np.zeros(case.n, dtype=np.float32)
    state = (p, z, z.copy(), z.copy())
    f = _Fused(cuda, case, state, dt)
    scal = (1.0, 0.1, 0.999, 0.001, 0.0, 1.0, 1e-8, 1.0)
    f.run_fused(scal)
    got = f.check(scal, case.owned)
    assert AR.same_bits(got[0], p) and not got[1].any() and not got[2].any()
    f.check_images(p)
