"""GPU parity of the LayerNorm kernels (csrc/norm.hip: fs2_ln_fwd / fs2_ln_bwd) against torch in
float64 with dropout on, at every launched instantiation, the engine's own flag combinations,
ragged row counts, row pitches, misaligned pointers and the edges of the row statistics; plus the
dropout seed base and three row ops (fs2_rowdot_fwd, fs2_mask_rows, fs2_sum_slices).

Reference.  Float64 torch on the same stored input values:

    s = x + r * keep_r / (1 - p_r)
    y = (tanh?)(LN(s) * gamma + beta) * keep_o / (1 - p_o) * row_mask + post_add

with keep_* = ``_keep_np(seed, salt, arange(M*D), p).reshape(M, D)`` (element index row*D + d,
never a pitch).  Where r and s_out are both given the kernels take the statistics from the stored
(rounded) s, so the reference normalises the s_out the kernel wrote; s_out itself is held to "the
float64 s rounded once": |s_out - s| <= half an ulp of s (2^(floor(log2 |s|) - 8) in bf16, 0 in
fp32) plus the fp32 arithmetic that forms it, 2^-21 (|x| + |r| / (1 - p_r)).  Backward: autograd in
float64 through the same expression with the masks as constants, the (s > 0) gate for
relu_gate_in, dr = ds * keep_r / (1 - p_r), dcol = the column sum of the unrounded dr (of ds
without dr).

Metrics.  ``rel`` (max error / max reference) on every output, and on y and ds also a per-row
version (max error in the row / max(row reference max, 0.1 * global reference max): a row zeroed
by row_mask or a small row cannot hide behind the global maximum).  mean / rstd (fp32 in both
modes) per row against float64: |mean - ref| <= 1e-5 * max|s_row|, rstd relative 1e-5.

Bounds.  fp32 mode: 1e-4 on y, 3e-4 on the backward outputs (as test_layernorm_fwd_bwd).  bf16
mode: ``python tests/test_gpu_layernorm.py`` runs, on the CPU, a float64 emulation of every case
below that rounds to bf16 only where the kernels do (s_out, y, ds, dr).  Its largest figures over
all cases: y 3.13e-3 (per row 3.73e-3), ds 2.87e-3 (per row 3.88e-3), dr 3.39e-3 -- up to the
half ulp 2^-8 of a maximum just above a power of two.  The asserted bf16 bound is 1.2e-2 on y and
on every backward output: 3.1x the largest of these (the project's 2e-2 / 6e-2 are the ceiling).
The figures observed on the GPU go through ``parity_log``.

Exact checks.  With p_o > 0 and no post_add, (y != 0) equals keep_o & (row_mask != 0) element
for element (the inputs are nudged until every kept |y| of the reference exceeds 1e-3, asserted).
With p_r > 0, s_out == x bit for bit where keep_r is false and differs everywhere else (|r| >=
0.5, asserted on the reference), and dr == 0 exactly on the dropped positions.  Every output and
the workspace start as NaN, dgamma / dbeta / dcol (which accumulate) as 0.5 / -0.25 / 2.0; every
result is finite; the pitch gaps of y and ds keep their sentinel; a second identical backward is
bit-identical.

Which D launches which instantiation (the dispatch in fs2_ln_fwd / fs2_ln_bwd, product build;
nch = ceil(D / V / 64) with V = 8 bf16 / 4 fp32; the vector kernels need D % V == 0, every pitch
% V == 0 and 16-byte aligned pointers, everything else takes the scalar kernels):

  bf16 D = 8, 80, 384, 512    fwd ln_fwd_rows_kernel<2,true>
                              bwd ln_bwd_rows_kernel<4,false,true>, tanh: ln_bwd_rows_kernel<2,true,true>
  bf16 D = 520, 1024          fwd ln_fwd_vec_kernel<bf16,2>     bwd ln_bwd_vec_kernel<bf16,2>
  bf16 D = 90, 1023           fwd ln_fwd_kernel<bf16>           bwd ln_bwd_kernel<bf16>   (2 / 16 sweeps)
  fp32 D = 8, 256             fwd ln_fwd_vec_kernel<float,1>    bwd ln_bwd_vec_kernel<float,1>
  fp32 D = 260, 512           fwd ln_fwd_vec_kernel<float,2>    bwd ln_bwd_vec_kernel<float,2>
  fp32 D = 516, 1024          fwd ln_fwd_vec_kernel<float,4>    bwd ln_bwd_vec_kernel<float,4>   (nch 3, 4)
  fp32 D = 90, 1023           fwd ln_fwd_kernel<float>          bwd ln_bwd_kernel<float>

seven forward and eight backward, each in test_ln_every_instantiation with p_r = 0.1, p_o = 0.2,
r, s_out, row_mask, dr and all three sums.  A pitch of D + 3 (bf16) / D + 1 (fp32) or a pointer
one element into its buffer sends a vector shape to the scalar kernels (test_ln_pitches_and_
alignment, which also holds the vector and the scalar kernels to each other).

What this found.  No kernel fault: the bf16 figures observed on MI355X (y 3.1e-3, per row 3.7e-3;
ds 2.9e-3, per row 3.9e-3; dr 3.4e-3) are those of the emulation.  On the host, fs2_ln_bwd did
not refuse a null mean / rstd (fs2_ln_fwd did); it does now (tests/test_host.py).  No kernel
changed.  A scratch build whose forward hashes row*ldx + d fails the four pitch cases (first at
the s_out check), one whose forward draws the output mask with another salt fails the exact
zero-pattern check of every case that has it.
"""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_ops import _keep_np, rel

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 3.0
PRE = {"dg": 0.5, "db": -0.25, "dc": 2.0}   # what the accumulating outputs hold before the call
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CODE = {"fp32": 0, "bf16": 1}
TOL_Y = {"fp32": 1e-4, "bf16": 1.2e-2}
TOL_BWD = {"fp32": 3e-4, "bf16": 1.2e-2}
assert TOL_Y["bf16"] <= 2e-2 and TOL_BWD["bf16"] <= 6e-2

FULL = dict(p_r=0.1, p_o=0.2, r=True, row_mask=True, dr=True, parts="gbc")


def _cfg(dt, M, D, **kw):
    c = dict(dt=dt, M=M, D=D, eps=1e-5, tanh=0, p_r=0.0, p_o=0.0, r=False, row_mask=False,
             post_add=False, relu=0, dr=False, parts="gbc", seed=20240, salt_r=11, salt_o=3)
    c.update(kw)
    assert not c["dr"] or c["r"]
    assert c["parts"] in ("gbc", "gb", "c", "")
    return c


@functools.lru_cache(maxsize=8)
def _keep(seed, salt, M, D, p):
    """numpy keep mask (M, D) of one (seed, salt) draw, shared by the cases of a shape"""
    k = _keep_np(seed, salt, np.arange(M * D, dtype=np.uint64), p).reshape(M, D)
    return torch.from_numpy(k)


def _masks(c, dev):
    ko = _keep(c["seed"], c["salt_o"], c["M"], c["D"], c["p_o"]).to(dev) if c["p_o"] > 0 else None
    kr = _keep(c["seed"], c["salt_r"], c["M"], c["D"], c["p_r"]).to(dev) if c["p_r"] > 0 else None
    return ko, kr


# ------------------------------------------------------------------ the float64 reference
def _s64(c, inp, kr):
    s = inp["x"].double()
    if c["r"]:
        rr = inp["r"].double()
        if kr is not None:
            rr = rr * kr / (1 - c["p_r"])
        s = s + rr
    return s


def _y64(c, inp, s, g, b, ko):
    mu = s.mean(1, keepdim=True)
    rstd = ((s - mu).pow(2).mean(1, keepdim=True) + c["eps"]).rsqrt()
    z = (s - mu) * rstd * g + b
    y = torch.tanh(z) if c["tanh"] else z
    if ko is not None:
        y = y * ko / (1 - c["p_o"])
    if c["row_mask"]:
        y = y * inp["rm"].double()[:, None]
    if c["post_add"]:
        y = y + inp["pa"].double()
    return y, mu[:, 0], rstd[:, 0], z


def _bwd64(c, inp, s, ko, kr):
    s = s.detach().clone().requires_grad_(True)
    g = inp["g"].double().requires_grad_(True)
    b = inp["b"].double().requires_grad_(True)
    y, _, _, _ = _y64(c, inp, s, g, b, ko)
    y.backward(inp["dy"].double())
    ds = s.grad
    if c["relu"]:
        ds = ds * (s.detach() > 0)
    out = {"ds": ds, "dg": g.grad, "db": b.grad}
    if c["dr"]:
        out["dr"] = ds * kr / (1 - c["p_r"]) if kr is not None else ds.clone()
    out["dc"] = out.get("dr", ds).sum(0)
    return out


def _round(t64, dt):
    return t64.to(torch.float32).to(TDT[dt])


def _row_rel(got, ref):
    err = (got.double() - ref).abs()
    den = torch.maximum(ref.abs().amax(1), 0.1 * ref.abs().max()).clamp(min=1e-300)
    return (err.amax(1) / den).max().item()


def _kept(c, inp, ko):
    k = ko.clone() if ko is not None else torch.ones(c["M"], c["D"], dtype=torch.bool,
                                                     device=inp["x"].device)
    if c["row_mask"]:
        k &= (inp["rm"] != 0)[:, None]
    return k


# ------------------------------------------------------------------ inputs (made on the CPU)
def _inputs(c, special=None):
    """x, r, dy, post_add (M, D) in the case's dtype, gamma / beta / row_mask fp32, on the CPU.
    |r| >= 0.5; |gamma|, |beta| in [0.5, 1.5).  With p_o > 0 and no post_add, x is nudged by 0.5
    wherever a kept |y| of the reference is below 4e-3, until none is."""
    M, D, tdt = c["M"], c["D"], TDT[c["dt"]]
    gen = torch.Generator().manual_seed(7919 * D + 31 * M + 2 * c["tanh"] + (c["dt"] == "bf16"))

    def randn(*shape):
        return torch.randn(*shape, generator=gen)

    def signed(*shape):
        sign = (torch.rand(*shape, generator=gen) < 0.5).float() * 2 - 1
        return sign * (0.5 + torch.rand(*shape, generator=gen))

    inp = {"x": randn(M, D).to(tdt), "dy": randn(M, D).to(tdt), "g": signed(D), "b": signed(D),
           "pa": randn(M, D).to(tdt)}
    rr = randn(M, D)
    inp["r"] = (torch.where(rr < 0, -1.0, 1.0) * (0.5 + rr.abs())).to(tdt)
    rm = (torch.rand(M, generator=gen) > 0.2).float()
    rm[0] = 1.0
    if M >= 5:
        rm[M // 2] = 0.0
    inp["rm"] = rm
    if special is not None:
        special(inp)
    ko, kr = _masks(c, "cpu")
    if c["r"]:
        assert bool((inp["r"].double().abs() >= 0.5).all())
    if c["p_o"] > 0 and not c["post_add"]:
        kept = _kept(c, inp, ko)
        for _ in range(20):
            s = _s64(c, inp, kr)
            if c["r"]:
                s = _round(s, c["dt"]).double()
            y, _, _, _ = _y64(c, inp, s, inp["g"].double(), inp["b"].double(), ko)
            bad = kept & (y.abs() < 4e-3)
            if not bool(bad.any()):
                break
            inp["x"][bad] = (inp["x"][bad].double() + 0.5).to(tdt)
        else:
            raise AssertionError("could not move every kept y away from 0")
    return inp


# ------------------------------------------------------------------ one forward + two backwards
def _buf(M, D, ld, dtype, fill, gapfill, dev, off=False):
    """(M, ld) view with [:, :D] = fill and the pitch gap = gapfill; ``off``: the view starts one
    element into its (256-byte aligned) allocation"""
    flat = torch.full((M * ld + 8,), gapfill, device=dev, dtype=dtype)
    v = flat[int(off):int(off) + M * ld].view(M, ld)
    assert (v.data_ptr() % 16 != 0) == bool(off)
    v[:, :D] = fill
    return v


def _run(cuda, c, inp, gap=0, off=()):
    """the kernels on one case; every pitched operand has pitch D + gap, the operands named in
    ``off`` start one element into their buffer.  Returns compact clones of every output."""
    from fastspeech2 import ops
    M, D, tdt, code = c["M"], c["D"], TDT[c["dt"]], CODE[c["dt"]]
    ld = D + gap
    d = {k: v.to(cuda) for k, v in inp.items()}

    def pin(name, t):    # an input: NaN in the gap
        b = _buf(M, D, ld, tdt, NAN, NAN, cuda, name in off)
        b[:, :D] = t
        return b

    def pout(name):      # an output: NaN where it is written, the sentinel in the gap
        return _buf(M, D, ld, tdt, NAN, SENTINEL, cuda, name in off)

    x = pin("x", d["x"])
    r = pin("r", d["r"]) if c["r"] else None
    pa = pin("pa", d["pa"]) if c["post_add"] else None
    rm = d["rm"] if c["row_mask"] else None
    y = pout("y")
    s_out = torch.full((M, D), NAN, device=cuda, dtype=tdt) if c["r"] else None
    mean = torch.full((M,), NAN, device=cuda)
    rstd = torch.full((M,), NAN, device=cuda)
    ops.ln_fwd(x, ld, d["g"], d["b"], c["eps"], y, ld, mean, rstd, M, D, dt=code, seed=c["seed"],
               r=r, ldr=ld if c["r"] else 0, p_r=c["p_r"], salt_r=c["salt_r"], s_out=s_out,
               do_tanh=c["tanh"], p_o=c["p_o"], salt_o=c["salt_o"], row_mask=rm, post_add=pa,
               ldp=ld if c["post_add"] else 0)
    assert bool((y[:, D:] == SENTINEL).all()), "forward wrote into the pitch gap of y"
    out = {"y": y[:, :D].clone(), "mean": mean, "rstd": rstd}
    if c["r"]:
        out["s_out"] = s_out
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k

    s_in = pin("s", s_out if c["r"] else d["x"])   # what the backward re-reads, pitched
    dy = pin("dy", d["dy"])
    parts = c["parts"]

    def backward():
        ds = pout("ds")
        dr = torch.full((M, D), NAN, device=cuda, dtype=tdt) if c["dr"] else None
        dg = torch.full((D,), PRE["dg"], device=cuda) if "g" in parts else None
        db = torch.full((D,), PRE["db"], device=cuda) if "b" in parts else None
        dc = torch.full((D,), PRE["dc"], device=cuda) if "c" in parts else None
        ws = torch.full((int(ops.ln_ws(M, D)),), NAN, device=cuda)
        ops.ln_bwd(dy, ld, s_in, ld, mean, rstd, d["g"], d["b"], ds, ld, M, D, dt=code, ws=ws,
                   seed=c["seed"], do_tanh=c["tanh"], p_o=c["p_o"], salt_o=c["salt_o"],
                   row_mask=rm, relu_gate_in=c["relu"], dr=dr, p_r=c["p_r"], salt_r=c["salt_r"],
                   dgamma=dg, dbeta=db, dcol=dc)
        assert bool((ds[:, D:] == SENTINEL).all()), "backward wrote into the pitch gap of ds"
        res = {"ds": ds[:, :D].clone(), "dr": dr, "dg": dg, "db": db, "dc": dc}
        return {k: v for k, v in res.items() if v is not None}

    b1, b2 = backward(), backward()
    for k in b1:
        assert bool(torch.isfinite(b1[k]).all()), k
        assert torch.equal(b1[k], b2[k]), "the backward is not repeatable: " + k
    out.update(b1)
    return out


def _log_max(parity_log, key, figs):
    old = parity_log.setdefault(key, {})
    for k, v in figs.items():
        old[k] = max(old.get(k, 0.0), v)


def _check(c, inp, out, parity_log, key):
    """every output of ``_run`` against float64, the exact zero patterns, the statistics"""
    dt, dev = c["dt"], out["y"].device
    d = {k: v.to(dev) for k, v in inp.items()}
    ko, kr = _masks(c, dev)
    figs = {}
    s = _s64(c, d, kr)
    if c["r"]:
        got = out["s_out"].double()
        slack = 2.0 ** -21 * (d["x"].double().abs() + d["r"].double().abs() / (1 - c["p_r"]))
        if dt == "bf16":   # 8 significant bits: half an ulp of s is 2^(floor(log2 |s|) - 8)
            slack = slack + torch.exp2(torch.floor(torch.log2(s.abs())) - 8)
        assert bool(((got - s).abs() <= slack).all()), "s_out is not s rounded once"
        figs["s_out"] = rel(out["s_out"], s)
        if kr is not None:
            same = out["s_out"] == d["x"]
            assert bool((_round(s, dt) != d["x"])[kr].all()), "the add must change every kept x"
            assert torch.equal(same, ~kr), "s_out == x exactly where the residual was dropped"
        s = got   # the statistics are those of the stored s
    y, mu, rstd, _ = _y64(c, d, s, d["g"].double(), d["b"].double(), ko)
    figs["y"], figs["y_row"] = rel(out["y"], y), _row_rel(out["y"], y)
    figs["mean"] = ((out["mean"].double() - mu).abs() / s.abs().amax(1).clamp(min=1e-300)).max().item()
    figs["rstd"] = ((out["rstd"].double() - rstd).abs() / rstd).max().item()
    if c["p_o"] > 0 and not c["post_add"]:
        kept = _kept(c, d, ko)
        assert float(y[kept].abs().min()) > 1e-3, "a kept y of the reference is too close to 0"
        assert torch.equal(out["y"] != 0, kept), "y != 0 exactly on keep_o & row_mask"
    ref = _bwd64(c, d, s, ko, kr)
    for k in ("ds", "dr", "dg", "db", "dc"):
        if k in out:
            got = out[k].double() - PRE.get(k, 0.0)
            figs[k] = rel(got, ref[k])
    figs["ds_row"] = _row_rel(out["ds"], ref["ds"])
    if c["dr"] and kr is not None:
        assert bool((out["dr"][~kr] == 0).all()), "dr must be 0 where the residual was dropped"
    print(key, {k: v for k, v in c.items() if k not in ("seed", "salt_r", "salt_o")}, figs)
    _log_max(parity_log, key + "_" + dt, figs)
    assert figs["mean"] <= 1e-5 and figs["rstd"] <= 1e-5, figs
    assert figs["y"] < TOL_Y[dt] and figs["y_row"] < TOL_Y[dt], figs
    if "s_out" in figs:
        assert figs["s_out"] < TOL_Y[dt], figs
    for k in ("ds", "ds_row", "dr", "dg", "db", "dc"):
        if k in figs:
            assert figs[k] < TOL_BWD[dt], (k, figs)
    return figs


def _case(cuda, parity_log, key, c, **kw):
    inp = _inputs(c)
    out = _run(cuda, c, inp, **kw)
    _check(c, inp, out, parity_log, key)
    return inp, out


# ------------------------------------------------------------------ the case lists
_VARIANTS = ([("bf16", D) for D in (8, 80, 384, 512, 520, 1024, 90, 1023)] +
             [("fp32", D) for D in (8, 256, 260, 512, 516, 1024, 90, 1023)])
_NPART = [("bf16", 384), ("fp32", 512), ("bf16", 90)]     # rows, vec, scalar
_ENGINE = {
    "postnet_ln3": _cfg("bf16", 37, 80, p_o=0.2, post_add=True, parts="c"),
    "postnet_ln12": _cfg("bf16", 37, 512, tanh=1, p_o=0.2),
    "predictor_ln_256": _cfg("bf16", 37, 256, p_o=0.2, row_mask=True, relu=1),
    "predictor_ln_384": _cfg("bf16", 37, 384, p_o=0.2, row_mask=True, relu=1),
    "fft_norm": _cfg("bf16", 37, 384, r=True, p_r=0.1, dr=True, parts="c"),
}
_ROWS = [(M, D) for D in (384, 1024) for M in (1, 5, 9, 17, 203)]
_PITCH = [("bf16", 384, 3), ("bf16", 1024, 3), ("fp32", 256, 1), ("fp32", 1024, 1)]


def _all_cases():
    """every dropout case of this file (the CPU emulation behind the bf16 bounds runs them all)"""
    for dt, D in _VARIANTS:
        for tanh in (0, 1):
            yield _cfg(dt, 300, D, tanh=tanh, **FULL)
    for dt, D in _NPART:
        for parts in ("gb", "c"):
            yield _cfg(dt, 300, D, **dict(FULL, parts=parts))
    yield from _ENGINE.values()
    for M, D in _ROWS:
        yield _cfg("bf16", M, D, **FULL)
    for dt, D, _ in _PITCH:
        yield _cfg(dt, 37, D, tanh=1, post_add=True, **FULL)


# ------------------------------------------------------------------ 1: every instantiation
@pytest.mark.parametrize("tanh", [0, 1])
@pytest.mark.parametrize("dt,D", _VARIANTS)
def test_ln_every_instantiation(cuda, parity_log, dt, D, tanh):
    """both dropouts, r, s_out, row_mask, dr and all three sums at every D of the docstring's map"""
    _case(cuda, parity_log, "ln_variants", _cfg(dt, 300, D, tanh=tanh, **FULL))


@pytest.mark.parametrize("parts", ["gb", "c"])
@pytest.mark.parametrize("dt,D", _NPART)
def test_ln_partial_sum_variants(cuda, parity_log, dt, D, parts):
    """npart = 2 (dgamma + dbeta) and 1 (dcol alone) on a rows, a vector and a scalar shape; the
    three-sum form is test_ln_every_instantiation"""
    _case(cuda, parity_log, "ln_npart", _cfg(dt, 300, D, **dict(FULL, parts=parts)))


# ------------------------------------------------------------------ 2: the engine's combinations
@pytest.mark.parametrize("name", sorted(_ENGINE))
def test_ln_engine_combinations(cuda, parity_log, name):
    """PostNet ln3 (D = 80, p_o, post_add, dcol), PostNet ln1 / ln2 (D = 512, tanh, p_o), the
    predictors' ln1 / ln2 (p_o, row_mask, the relu gate on the input), the FFT blocks' add & norm
    (r, p_r, s_out, dr, dcol), M = 37"""
    _case(cuda, parity_log, "ln_engine", _ENGINE[name])


# ------------------------------------------------------------------ 3: row counts
@pytest.mark.parametrize("M,D", _ROWS)
def test_ln_row_counts(cuda, parity_log, M, D):
    """partial 8-row forward blocks and their clamped loads, ragged rows per backward block and
    per wave (the rows kernels at D = 384, vec<bf16,2> at D = 1024)"""
    _case(cuda, parity_log, "ln_row_counts", _cfg("bf16", M, D, **FULL))


# ------------------------------------------------------------------ 4: pitches and alignment
@pytest.mark.parametrize("dt,D,odd", _PITCH)
def test_ln_pitches_and_alignment(cuda, parity_log, dt, D, odd):
    """pitch D + 8 (vector kernels) and D + 3 / D + 1 (scalar kernels) with NaN in the gaps of
    x, r, post_add, dy, s and sentinels in the gaps of y, ds (checked in _run); the two agree
    within the bounds; x, then dy, one element into its buffer at pitch D selects the scalar
    kernel: bit-identical to the odd-pitch run of the same values"""
    c = _cfg(dt, 37, D, tanh=1, post_add=True, **FULL)
    inp = _inputs(c)
    vec = _run(cuda, c, inp, gap=8)
    _check(c, inp, vec, parity_log, "ln_pitch_vector")
    sca = _run(cuda, c, inp, gap=odd)
    _check(c, inp, sca, parity_log, "ln_pitch_scalar")
    figs = {k: rel(vec[k], sca[k]) for k in vec}
    _log_max(parity_log, "ln_vector_vs_scalar_" + dt, figs)
    for k, v in figs.items():
        assert v < (TOL_Y[dt] if k in ("y", "s_out", "mean", "rstd") else TOL_BWD[dt]), (k, figs)
    offx = _run(cuda, c, inp, off=("x",))      # scalar forward, vector backward
    for k in ("y", "s_out", "mean", "rstd"):
        assert torch.equal(offx[k], sca[k]), "misaligned x: " + k
    # the scalar forward again (its mean / rstd feed the backward), the backward scalar through dy
    offdy = _run(cuda, c, inp, off=("x", "dy"))
    for k in sca:
        assert torch.equal(offdy[k], sca[k]), "misaligned dy: " + k


# ------------------------------------------------------------------ 5: statistics edges
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("D", [384, 90])
def test_ln_statistics_edges(cuda, parity_log, dt, D):
    """row 0 constant (variance 0: rstd = 1/sqrt(eps), y = beta), row 1 a large common offset
    (1000 + N(0,1) in fp32 -- a one-pass variance loses it; 64 + N(0,1) in bf16, whose spread
    survives the rounding), row 2 of 1e-4-scale values; eps = 1e-6.  dy of rows 0 and 2 is scaled
    by 1e-3 (their rstd is ~1e3) so that every row's ds is of one size."""
    eps = 1e-6
    c = _cfg(dt, 9, D, eps=eps)
    off = 1000.0 if dt == "fp32" else 64.0

    def special(inp):
        x, tdt = inp["x"], TDT[dt]
        x[0] = 3.0
        x[1] = (off + x[1].double()).to(tdt)
        x[2] = (1e-4 * x[2].double()).to(tdt)
        for i in (0, 2):
            inp["dy"][i] = (1e-3 * inp["dy"][i].double()).to(tdt)

    inp = _inputs(c, special)
    assert float(inp["x"][1].double().std()) > 0.5
    out = _run(cuda, c, inp)
    _check(c, inp, out, parity_log, "ln_stats_edges")
    assert abs(out["rstd"][0].item() * math.sqrt(eps) - 1) <= 1e-6
    assert rel(out["y"][0], inp["b"].to(cuda)) < TOL_Y[dt]


# ------------------------------------------------------------------ 6: saturated tanh
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_ln_saturated_tanh(cuda, parity_log, dt):
    """|beta| = 60 on the first quarter of the columns (|z| > 40 in every row) and gamma x 20 on
    the second (|z| reaches 50 on part of each row): y is exactly +-1 where |z| >= 20, the
    backward is finite (checked in _run) and at parity, and the saturated columns add exactly 0
    to dgamma and dbeta (the exp-based gate of the bf16 kernel gives 1 - t^2 = 0 from exp = inf
    and exp = 0)."""
    D, q = 384, 96
    c = _cfg(dt, 37, D, tanh=1)

    def special(inp):
        inp["b"][:q] = torch.sign(inp["b"][:q]) * 60.0
        inp["g"][q:2 * q] *= 20.0

    inp = _inputs(c, special)
    out = _run(cuda, c, inp)
    _check(c, inp, out, parity_log, "ln_saturated_tanh")
    d = {k: v.to(cuda) for k, v in inp.items()}
    _, _, _, z = _y64(c, d, d["x"].double(), d["g"].double(), d["b"].double(), None)
    assert float(z[:, :q].abs().min()) > 40 and float(z[:, q:2 * q].abs().max()) > 50
    sat = z.abs() >= 20
    assert torch.equal(out["y"][sat].double(), torch.sign(z[sat]))
    assert bool((out["dg"][:q] == PRE["dg"]).all()) and bool((out["db"][:q] == PRE["db"]).all())


def test_ln_bf16_tanh_gate_accuracy(cuda, parity_log):
    """the bf16 backward's exp-based gate at |z| ~ 1 against the float64 1 - tanh^2: one row and
    dy = 1, so dbeta[d] is the gate of column d (onto a 2^-10 start value: resolution 3e-8).
    Logged; the bound 1e-5 is far above fp32 arithmetic on z (~2e-7) and far below the bf16 ulp
    of the gradient the gate scales."""
    from fastspeech2 import ops
    D = 512
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, D, generator=gen).to(torch.bfloat16).to(cuda)
    g = (0.5 + torch.rand(D, generator=gen)).to(cuda)
    b = (torch.rand(D, generator=gen) - 0.5).to(cuda)
    y = torch.full((1, D), NAN, device=cuda, dtype=torch.bfloat16)
    mean, rstd = torch.full((1,), NAN, device=cuda), torch.full((1,), NAN, device=cuda)
    ops.ln_fwd(x, D, g, b, 1e-5, y, D, mean, rstd, 1, D, dt=1, do_tanh=1)
    dy = torch.ones(1, D, device=cuda, dtype=torch.bfloat16)
    ds = torch.full((1, D), NAN, device=cuda, dtype=torch.bfloat16)
    dg = torch.zeros(D, device=cuda)
    db = torch.full((D,), 2.0 ** -10, device=cuda)
    ws = torch.full((int(ops.ln_ws(1, D)),), NAN, device=cuda)
    ops.ln_bwd(dy, D, x, D, mean, rstd, g, b, ds, D, 1, D, dt=1, ws=ws, do_tanh=1, dgamma=dg,
               dbeta=db)
    c = _cfg("bf16", 1, D, tanh=1)
    _, _, _, z = _y64(c, {}, x.double(), g.double(), b.double(), None)
    assert 0.9 < float(z.abs().max()) and float(z.abs().median()) > 0.2
    err = ((db.double() - 2.0 ** -10) - (1 - torch.tanh(z[0]) ** 2)).abs().max().item()
    print("bf16 tanh gate", err)
    _log_max(parity_log, "ln_bf16_tanh_gate", {"abs_err": err})
    assert err < 1e-5


# ------------------------------------------------------------------ 7: the dropout seed base
def _with_base(ops, base, fn):
    try:
        ops.set_dropout_seed(base)
        return fn()
    finally:
        ops.set_dropout_seed(0)


def test_seed_base_layernorm(cuda):
    """norm.hip's cell: seed a under base b draws the masks of seed a + b (mod 2^32) under base 0,
    forward and backward, and not those of seed a"""
    from fastspeech2 import ops
    a, b = 0xfffffff0, 0x123
    c = _cfg("bf16", 17, 384, **FULL)
    inp = _inputs(c)
    based = _with_base(ops, b, lambda: _run(cuda, dict(c, seed=a), inp))
    plain = _run(cuda, dict(c, seed=(a + b) & 0xffffffff), inp)
    other = _run(cuda, dict(c, seed=a), inp)
    for k in plain:
        assert torch.equal(based[k], plain[k]), k
    for k in ("y", "s_out", "ds", "dr"):
        assert not torch.equal(based[k], other[k]), k


def test_seed_base_softmax_and_fused_attention(cuda):
    """the same through attention.hip's cell (fs2_softmax_fwd's dropped Pd) and flash.hip's
    (fs2_attn_fwd's out): each translation unit has its own copy of the base"""
    from fastspeech2 import ops
    a, b = 77, 0xffffff00
    B, H, T, dh = 2, 2, 24, 64
    D = H * dh
    gen = torch.Generator().manual_seed(24)
    kp = torch.zeros(B, T, dtype=torch.uint8, device=cuda)
    S = torch.randn(B * H, T, T, generator=gen).to(cuda)
    qkv = (torch.randn(B * T, 3 * D, generator=gen) * 0.5).to(torch.bfloat16).to(cuda)

    def softmax(seed):
        P = torch.full((B * H, T, T), NAN, device=cuda)
        Pd = torch.full((B * H, T, T), NAN, device=cuda)
        ops.softmax_fwd(S, kp, B, H, T, T, T, 0.5, 0.1, seed, 9, P, Pd, dt=0)
        return Pd

    def fused(seed):
        out = torch.full((B * T, D), NAN, device=cuda, dtype=torch.bfloat16)
        lse = torch.full((B * H, T), NAN, device=cuda)
        ops.attn_fwd(qkv, 3 * D, kp, B, H, T, dh, 0.125, 0.1, seed, 5, out, D, lse, dt=1)
        return out

    for fn in (softmax, fused):
        based = _with_base(ops, b, lambda: fn(a))
        plain, other = fn((a + b) & 0xffffffff), fn(a)
        assert bool(torch.isfinite(plain).all())
        assert torch.equal(based, plain), fn.__name__
        assert not torch.equal(based, other), fn.__name__


# ------------------------------------------------------------------ row ops without a direct test
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("M,D,ldu", [(300, 384, 384), (5, 20, 24), (7, 90, 91), (1, 1024, 1024)])
def test_rowdot_fwd(cuda, parity_log, dt, M, D, ldu, scale):
    """y = (u . w + b) * scale against float64: rel 1e-5 in fp32; in bf16 against the float64
    result rounded once, rel 1e-2 (a result on the other side of a tie is one ulp, 2^-8, away)"""
    from fastspeech2 import ops
    tdt = TDT[dt]
    gen = torch.Generator().manual_seed(M + D)
    u = torch.full((M, ldu), NAN, dtype=tdt, device=cuda)
    u[:, :D] = torch.randn(M, D, generator=gen).to(tdt).to(cuda)
    w = torch.randn(D, generator=gen).to(cuda)
    b = torch.randn(1, generator=gen).to(cuda)
    y = torch.full((M + 1,), SENTINEL, dtype=tdt, device=cuda)
    y[:M] = NAN
    ops.rowdot_fwd(u, ldu, w, b, scale, M, D, y, dt=CODE[dt])
    assert float(y[M]) == SENTINEL
    ref = (u[:, :D].double() @ w.double() + b.double()) * float(np.float32(scale))
    if dt == "bf16":
        ref = _round(ref, dt).double()
    err = rel(y[:M], ref)
    _log_max(parity_log, "rowdot_fwd_" + dt, {"y": err})
    assert err < (1e-5 if dt == "fp32" else 1e-2), err


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M,D,ld", [(300, 384, 392), (7, 90, 91), (1, 5, 8)])
def test_mask_rows(cuda, dt, M, D, ld):
    """X *= keep[row] in place: exactly X * keep[:, None], the pitch gap untouched, a NaN in a
    kept row still NaN"""
    from fastspeech2 import ops
    tdt = TDT[dt]
    gen = torch.Generator().manual_seed(M)
    X = torch.full((M, ld), SENTINEL, dtype=tdt, device=cuda)
    X[:, :D] = torch.randn(M, D, generator=gen).to(tdt).to(cuda)
    keep = (torch.rand(M, generator=gen) > 0.4).float().to(cuda)
    keep[0] = 1.0
    X[0, D - 1] = NAN
    want = X[:, :D] * keep[:, None].to(tdt)
    ops.mask_rows(X, ld, keep, M, D, dt=CODE[dt])
    assert bool((X[:, D:] == SENTINEL).all())
    assert bool(torch.isnan(X[0, D - 1])) and bool(torch.isnan(want[0, D - 1]))
    assert torch.equal(torch.nan_to_num(X[:, :D], nan=12345.0), torch.nan_to_num(want, nan=12345.0))


@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("nslices", [1, 3, 5])
@pytest.mark.parametrize("n", [4, 1028, 4 * 70001])
def test_sum_slices(cuda, n, nslices, gap):
    """out (+)= the slices in order, bit-exact against ((out + s0) + s1) + ... in fp32; NaN between
    the slices (stride n + 8), after the last one and in a non-accumulated out is never read"""
    from fastspeech2 import ops
    stride = n + gap
    gen = torch.Generator().manual_seed(n + nslices)
    ws = torch.full((nslices * stride + 8,), NAN, device=cuda)
    sl = torch.randn(nslices, n, generator=gen).to(cuda)
    for i in range(nslices):
        ws[i * stride:i * stride + n] = sl[i]
    for accumulate, start in ((0, NAN), (1, 0.5)):
        out = torch.full((n + 4,), SENTINEL, device=cuda)
        out[:n] = start
        ops.sum_slices(ws, nslices, stride, n, out, accumulate=accumulate)
        want = torch.full((n,), 0.5 if accumulate else 0.0, device=cuda)
        for i in range(nslices):
            want = want + sl[i]
        assert torch.equal(out[:n], want), (accumulate, (out[:n] - want).abs().max().item())
        assert bool((out[n:] == SENTINEL).all())


# ------------------------------------------------------------------ the bf16 rounding budget
def _emulate(c):
    """float64 on the CPU, rounded to the case's dtype only where the kernels round (s_out, y, ds,
    dr): what rounding alone costs on each asserted figure"""
    inp = _inputs(c)
    ko, kr = _masks(c, "cpu")
    dt = c["dt"]
    s = _s64(c, inp, kr)
    if c["r"]:
        s = _round(s, dt).double()
    y, _, _, _ = _y64(c, inp, s, inp["g"].double(), inp["b"].double(), ko)
    ref = _bwd64(c, inp, s, ko, kr)
    figs = {"y": rel(_round(y, dt), y), "y_row": _row_rel(_round(y, dt), y),
            "ds": rel(_round(ref["ds"], dt), ref["ds"]),
            "ds_row": _row_rel(_round(ref["ds"], dt), ref["ds"])}
    if c["dr"]:
        figs["dr"] = rel(_round(ref["dr"], dt), ref["dr"])
    return figs


if __name__ == "__main__":
    worst = {}
    for case in _all_cases():
        if case["dt"] == "bf16":
            for name, fig in _emulate(case).items():
                worst[name] = max(worst.get(name, 0.0), fig)
    print("bf16 rounding alone, largest over the cases:", {k: "%.3g" % v for k, v in worst.items()})
    print("3x:", {k: "%.3g" % (3 * v) for k, v in worst.items()})
