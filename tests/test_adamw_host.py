"""CPU checks around AdamW and the fused weight images: the float64 restatement is torch's
AdamW, the fp32 restatement and torch's own fp32 AdamW meet the float64 bound the kernels are
held to (on every input family the GPU tests use), ``images()`` is the permute expressions of
the weight-prep tests, the two host tables are what the kernels search, and the entry points
refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_restatement as AR

N_HOST = 4099


def _torch_adamw(p, m, v, g, t, betas, wd, lr, dtype, steps=1):
    """``steps`` updates by torch.optim.AdamW (single-tensor path) from step count t-1 and the
    given moments; g: one gradient per step.  Returns the (p, m, v) after each step."""
    P = torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dtype))
    opt = torch.optim.AdamW([P], lr=lr, betas=betas, eps=1e-8, weight_decay=wd, foreach=False)
    opt.state[P] = {"step": torch.tensor(float(t - 1)),
                    "exp_avg": torch.from_numpy(np.array(m)).to(dtype),
                    "exp_avg_sq": torch.from_numpy(np.array(v)).to(dtype)}
    out = []
    for k in range(steps):
        P.grad = torch.from_numpy(np.array(g[k])).to(dtype)
        opt.step()
        st = opt.state[P]
        out.append(tuple(x.detach().clone().numpy() for x in (P, st["exp_avg"], st["exp_avg_sq"])))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9)])
def test_float64_restatement_is_torch_adamw(betas, wd):
    """Four steps from a random state at t = 5, each compared from torch's own previous state.
    Not to the last bit: torch's CPU lerp is one fused multiply-add and its addcdiv divides
    (value*m) by denom where the kernel multiplies value by (m/denom) -- the same number of
    roundings or fewer, in another order.  So both are two evaluations of the same expression
    and differ by at most twice the derived per-element bound with u = 2^-53 (a few float64
    ulps of the terms; measured: well under one bound).  Scalars in double on both sides."""
    steps, t0, lr = 4, 5, 1e-3
    p, m, v, _ = (a.astype(np.float64) for a in AR.make_state("unit", N_HOST, 1))
    r = np.random.default_rng(3)
    gs = [r.standard_normal(N_HOST) for _ in range(steps)]
    got = _torch_adamw(p, m, v, gs, t0, betas, wd, lr, torch.float64, steps)
    worst = 0.0
    for k in range(steps):
        scal = AR.scalars(t0 + k, betas, 1.0, wd, lr)
        mine = AR.adamw_step(p, m, v, gs[k], scal, np.float64, scalars_fp32=False)
        # the bound's scale terms; the fp32 rounding of the scalars inside bounds() moves them
        # by 2^-24 relative, nothing next to the factor 2
        _, bnd, _ = AR.bounds(p, m, v, gs[k], scal, u=AR.U53, denormal=False)
        for a, b, lim in zip(mine, got[k], bnd):
            err = np.abs(a - b)
            assert (err <= 2 * lim).all()
            worst = max(worst, float((err / lim).max()))
        p, m, v = got[k]
    print(f"float64 restatement vs torch: worst {worst:.3f} of the 2^-53 bound")
    assert np.abs(p - AR.make_state("unit", N_HOST, 1)[0]).max() > 1e-3      # it did step


@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9)])
def test_begin_step_scalars(t, betas):
    """FusedAdamW.begin_step returns the scalars the restatement derives, to the last bit"""
    from fastspeech2.optim import FusedAdamW
    opt = FusedAdamW.__new__(FusedAdamW)
    opt.lr, opt.betas, opt.eps, opt.weight_decay = 1e-4, betas, 1e-8, 1e-2
    opt.step_count = t - 1
    got = opt.begin_step(grad_scale=0.5)
    assert opt.step_count == t
    assert got == AR.scalars(t, betas, 0.5, 1e-2, 1e-4)
    assert len(got) == 8 and 0 < got[5] <= 1 and got[4] >= 1e-4


@pytest.mark.parametrize("case", range(len(AR.SCALAR_CASES)))
@pytest.mark.parametrize("family", AR.FAMILIES)
def test_fp32_references_meet_the_float64_bound(family, case, parity_log):
    """Check B on the references themselves, before any kernel is held to it: the fp32
    restatement, and torch's own fp32 CPU AdamW (fed the scaled gradient fl(g*gs), as it has
    no grad_scale), on every input family and every scalar case of the GPU tests."""
    t, betas, gs, wd, lr = AR.SCALAR_CASES[case]
    scal = AR.scalars(t, betas, gs, wd, lr)
    p, m, v, g = AR.make_state(family, N_HOST, 10 + case)
    mine = AR.adamw_step(p, m, v, g, scal, np.float32)
    bad, figs = AR.check_b(mine, p, m, v, g, scal)
    assert not bad, bad
    _log_max(parity_log, f"adamw_ref_fp32_{family}", figs)
    gr = g * np.float32(gs)
    tor = _torch_adamw(p, m, v, [gr], t, betas, wd, lr, torch.float32)[0]
    bad, figs = AR.check_b(tor, p, m, v, g, scal)
    assert not bad, bad
    _log_max(parity_log, f"adamw_torch_fp32_{family}", figs)
    if family == "spread":
        ref = AR.adamw_step(p, m, v, g, scal, np.float64)
        assert ((ref[2] > 0) & (ref[2] < AR.FLT_MIN)).sum() > 20      # v' denormal: reached
    if family == "huge":
        assert np.isinf(mine[2]).sum() >= N_HOST // 2 and not np.isnan(mine[0]).any()
    if family == "nonfinite":
        assert 1 <= np.isnan(mine[0]).sum() <= 8


def _log_max(parity_log, key, figs):
    old = parity_log.setdefault(key, {})
    for k, x in figs.items():
        old[k] = max(old.get(k, 0.0), float(x))


def test_check_b_can_fail():
    """the bound notices one wrong rounding direction's worth of error in each output"""
    scal = AR.scalars(1000)
    p, m, v, g = AR.make_state("unit", 257, 2)
    good = AR.adamw_step(p, m, v, g, scal, np.float32)
    assert not AR.check_b(good, p, m, v, g, scal)[0]
    for k in range(3):
        out = [a.copy() for a in good]
        out[k] *= np.float32(1 + 2.0 ** -19)
        bad, _ = AR.check_b(out, p, m, v, g, scal)
        assert bad and bad[0][0] == "pmv"[k]
    assert not AR.same_bits(good[0], np.nextafter(good[0], np.float32(9)))
    assert AR.same_bits(np.float32([np.nan, -0.0]), np.float32([np.nan, -0.0]))
    assert not AR.same_bits(np.float32([0.0]), np.float32([-0.0]))


# ---- images() ---------------------------------------------------------------------------------
def test_images_reversed_taps_expression():
    """images() == the expressions of test_weight_prep_reversed_taps, on its shape"""
    torch.manual_seed(13)
    O, C, KW = 136, 72, 9
    W = torch.randn(O, KW, C)
    ldf = (KW * C + 7) // 8 * 8
    ref_b = W.flip(1).permute(2, 1, 0).reshape(C, KW * O)
    ref_f = torch.zeros(O, ldf)
    ref_f[:, :KW * C] = W.reshape(O, KW * C)
    Wf, Wb, wr = AR.images(W.numpy(), O, C, KW, 3, ldf, KW * O)
    assert np.array_equal(Wf, ref_f.numpy()) and np.array_equal(Wb, ref_b.numpy()) and wr.all()
    nat = W.permute(2, 1, 0).reshape(C, KW * O)             # bit 1 clear: [c][j*O + o]
    assert np.array_equal(AR.images(W.numpy(), O, C, KW, 1, ldf, KW * O)[1], nat.numpy())


@pytest.mark.parametrize("O,C,KW", [(1536, 384, 9), (192, 72, 5), (128, 40, 3), (256, 128, 9)])
def test_images_tap_inner_expression(O, C, KW):
    """images() == the expressions of test_weight_prep_tap_inner, on its shapes"""
    torch.manual_seed(O + KW)
    W = torch.randn(O, KW, C)
    ldf = (KW * C + 7) // 8 * 8
    okc = 7 | (8 if C % 64 == 0 else 0)
    nat = W.flip(1).permute(2, 1, 0)
    ref_b = nat.reshape(C, KW, O // 64, 64).permute(0, 2, 1, 3).reshape(C, KW * O)
    if okc & 8:
        ref_f = W.view(O, KW, C // 64, 64).permute(0, 2, 1, 3).reshape(O, KW * C)
    else:
        ref_f = torch.zeros(O, ldf)
        ref_f[:, :KW * C] = W.reshape(O, KW * C)
    Wf, Wb, _ = AR.images(W.numpy(), O, C, KW, okc, ldf, KW * O)
    assert np.array_equal(Wf, ref_f.numpy()) and np.array_equal(Wb, ref_b.numpy())


def test_images_padding_and_unwritten_columns():
    W = np.arange(1, 1 + 5 * 2 * 3, dtype=np.float32).reshape(5, 2, 3)
    Wf, Wb, wr = AR.images(W, 5, 3, 2, 1, 8, 13)
    assert (Wf[:, 6:] == 0).all() and (Wf[:, :6] != 0).all()
    assert wr[:, :10].all() and not wr[:, 10:].any() and np.isnan(Wb[:, 10:]).all()
    assert Wf[4, 1 * 3 + 2] == W[4, 1, 2] and Wb[2, 1 * 5 + 4] == W[4, 1, 2]


# ---- build_case and the two host tables ---------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "table256", "ranges300", "offset1", "offset2",
                                  "offset3"])
def test_build_case_layout(name):
    c = AR.named_case(name)
    spans = [(w.off, w.numel) for w in c.weights] + list(c.ranges)
    assert int(c.owned.sum()) == sum(n for _, n in spans)
    assert not c.owned[0] and not c.owned[-1]
    for (s, n), (s2, _) in zip(spans, spans[1:]):
        assert s + n < s2 or n == 0                     # a gap between neighbours
    if name == "mixed":
        assert c.n < 500000
        forms = [w.vector_form() for w in c.weights]
        assert forms == [False, True, False, True, True, False, True, True, True, True]
        assert {s % 4 for s, _ in c.ranges} == {0, 1, 2, 3}
    if name.startswith("offset"):
        assert c.weights[0].off % 4 == int(name[6:]) and not c.weights[0].vector_form()


def _table_fields(raw, n):
    from fastspeech2 import _native as N
    arr = (N.WPrepDesc * n).from_buffer_copy(raw.numpy().tobytes())
    return [arr[i] for i in range(n)]


@pytest.mark.parametrize("name", ["mixed", "table256"])
def test_weight_prep_table(name):
    """tile0 is the ascending prefix sum of ceil(O/64) * tiles_k, tiles_k = ceil(ldf/64),
    total_tiles their sum, and every other field is passed through."""
    from fastspeech2 import ops
    c = AR.named_case(name)
    base = torch.zeros(c.n)
    entries = []
    for w in c.weights:
        Wf = torch.zeros(w.O * w.ldf, dtype=torch.bfloat16)
        Wb = torch.zeros(w.C * w.ldb, dtype=torch.bfloat16) if w.wb else None
        entries.append((base[w.off:w.off + w.numel], w.O, w.C, w.KW, w.okc, Wf, w.ldf, Wb, w.ldb))
    raw, n, total = ops.weight_prep_table(entries)
    (t0s, tks, tot), _ = AR.expected_tables(c)
    assert n == len(c.weights) and total == tot
    ds = _table_fields(raw, n)
    assert [d.tile0 for d in ds] == t0s and [d.tiles_k for d in ds] == tks
    assert all(a < b for a, b in zip(t0s, t0s[1:]))
    for d, w, e in zip(ds, c.weights, entries):
        assert (d.O, d.C, d.KW, d.w_okc, d.ldf, d.ldb) == (w.O, w.C, w.KW, w.okc, w.ldf, w.ldb)
        assert d.W == base.data_ptr() + 4 * w.off and d.Wf == e[5].data_ptr()
        assert (d.Wb or 0) == (e[7].data_ptr() if w.wb else 0)
    if name == "table256":
        assert n == 256 and total == 256


def test_adamw_ranges_table():
    from fastspeech2 import ops
    c = AR.named_case("mixed")
    t, n, blocks = ops.adamw_ranges_table(c.ranges, "cpu")
    _, (b0s, tot) = AR.expected_tables(c)
    assert n == len(c.ranges) and blocks == tot and t.dtype == torch.int64
    rows = t.view(-1, 3).tolist()
    assert [r[:2] for r in rows] == [list(x) for x in c.ranges]
    assert [r[2] for r in rows] == b0s
    # a zero-length range adds no blocks: its successor starts at the same block
    z = [i for i, (_, ln) in enumerate(c.ranges) if ln == 0]
    assert len(z) == 2 and z[-1] == len(c.ranges) - 1
    assert rows[z[0]][2] == rows[z[0] + 1][2] and rows[z[1]][2] == blocks
    assert blocks == sum(-(-ln // 1024) for _, ln in c.ranges) == 5 + 0 + 1 + 2 + 5 + 0
    # an empty list: no ranges, no blocks, and still a tensor to point at
    t, n, blocks = ops.adamw_ranges_table([], "cpu")
    assert (n, blocks) == (0, 0) and t.numel() >= 3


def test_adamw_entry_points_refuse_before_any_launch():
    """Addresses that are never followed, as in test_every_entry_point_refuses_an_unknown_dtype:
    every call here must return before a launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    sc = (1.0, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8, 1.0)

    def prep(descs=p, n=1, tiles=1, ranges=p, nr=1, rb=1, flat=(p, p, p, p), dt=N.BF16):
        return lib.fs2_adamw_prep(descs, n, tiles, ranges, nr, rb, *flat, *sc, dt, None)

    assert prep(n=257) == -1
    assert prep(n=-1) == -1
    assert prep(descs=None) == -1
    assert prep(ranges=None) == -1
    for i in range(4):
        flat = [p] * 4
        flat[i] = None
        assert prep(flat=tuple(flat)) == -1, i
    assert prep(dt=2) == -1
    assert lib.fs2_adamw(None, None, None, None, 0, *sc, None) == 0
    for i in range(4):
        flat = [p] * 4
        flat[i] = None
        assert lib.fs2_adamw(*flat, 16, *sc, None) == -1, i
