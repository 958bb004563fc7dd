"""GPU: rank-model training (csrc/rank_train.hip, ``fastspeech2.rank_train``) against the
reference's own training step (tests/golden/rank_train_ref.npz, made by make_golden_rank_train.py)
and, under dropout and at kernel level, against the float64 restatement
tests/rank_train_restatement.py (pinned to that step in test_rank_train_host.py).

Error is ``rel``: max abs difference over max abs reference, per tensor.

Tolerances.
* Kernels against float64: fp32 1e-5 (a few roundings and an erff / expf of a few ulp, as the
  loss kernel's test allows); activation-typed bf16 outputs 4e-3 = 2^-8, one rounding of the
  result (the inputs are bf16 values, so the float64 reference reads the same numbers); fp32
  parameter gradients 1e-5 in both dtypes; the pooling backward 1e-6 (three roundings) and 1e-5
  for dWp (a sum of B products).
* The loss: values within 1e-6 of ``fs2_rank_loss_fwd``; gradients within 1e-5 of fp32 torch
  autograd of the restated loss on the CPU.
* Whole step, fp32: the 8-tuple and the losses 1e-4 (the evaluation path's bound), every
  parameter gradient 1e-3 (the project's fp32 parity bound; the reference's own fp32 gradients
  are 1.4e-6 from its float64 run).
* Whole step, bf16: gradient cosine >= 0.99 per tensor (the project's bound), I 3e-2 (the
  extractor's bound), and for h, r, the losses and the gradients twice the largest error observed
  on the MI355X (profiles/rank_train_parity_observed.json; BF16_OBS below).
* Training forward at p = 0 against the evaluation forward of the same model: the evaluation
  path's own tolerances (test_gpu_rank.py), fp32 1e-4, bf16 I 3e-2, h 1.5e-3, r 2.8e-3.  The
  engine hands conv1's fp32 output to the GELU kernel and takes the LayerNorm statistics from
  the unrounded residual sum, so at p = 0 both paths compute the same values.
"""
import math

import numpy as np
import pytest
import torch

import rank_restatement as R
import rank_train_restatement as RT

pytestmark = pytest.mark.gpu

NAN = float("nan")
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CODE = {"fp32": 0, "bf16": 1}
TOL_ACT = {"fp32": 1e-5, "bf16": 4e-3}
# largest bf16 errors observed on the MI355X (profiles/rank_train_parity_observed.json); the
# asserted bound is twice each
BF16_OBS = {
    "golden": {"h": 6.85e-4, "r": 9.44e-3, "loss": 1.38e-4, "grad": 1.57e-2},
    "flash_p0.1": {"I": 2.82e-3, "h": 4.29e-4, "r": 1.55e-4, "loss": 3.83e-5, "grad": 1.14e-2},
    "flash_p0.5": {"I": 3.44e-3, "h": 5.39e-4, "r": 2.35e-4, "loss": 1.07e-4, "grad": 1.04e-2},
}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def cosine(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp(min=1e-300)).item()


def _log_max(parity_log, key, figs):
    old = parity_log.setdefault(key, {})
    for k, v in figs.items():
        old[k] = max(old.get(k, 0.0), v)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


@pytest.fixture(scope="module")
def train_ref(golden_dir):
    return RT.load_golden_train(golden_dir)


# ---------------------------------------------------------------------- kernel 1
def _gelu64(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))


def _gelu_grad64(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + \
        z * torch.exp(-z * z / 2) / math.sqrt(2 * math.pi)


def _gelu_inputs(M, N, dt):
    g = torch.Generator().manual_seed(M * 1000 + N)
    z = 2 * torch.randn(M, N, generator=g)
    special = torch.tensor([0.0, 6.0, -6.0])[:min(3, M * N)]
    z.view(-1)[:special.numel()] = special
    return z.to(TDT[dt]), torch.randn(M, N, generator=g).to(TDT[dt])


def _padded(x, ld, cuda):
    buf = torch.full((x.shape[0], ld), NAN, dtype=x.dtype, device=cuda)
    buf[:, :x.shape[1]] = x.to(cuda)
    return buf


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
# (5, 26): 16-byte chunks and a scalar tail in one row; (3, 7): odd N, every element scalar
@pytest.mark.parametrize("M,N", [(1, 2), (7, 24), (33, 128), (5, 1536), (5, 26), (3, 7)])
def test_gelu_dropout_kernel(cuda, parity_log, M, N, dt):
    from fastspeech2 import ops
    seed, salt = 4242, 7
    z, dhc = _gelu_inputs(M, N, dt)
    z64, d64 = z.double(), dhc.double()
    # where GELU(z) is no fp32 zero: not at z = 0, and erff(z / sqrt 2) == -1 in fp32 below -5.4
    nonzero = (z64 != 0) & (z64 > -5)
    worst = {"gelu_fwd": 0.0, "gelu_bwd": 0.0}
    # pitches: N, N + 8 and the next multiple of 8 (aligned rows, with a tail where N is none),
    # N + 1 (rows not 16-byte aligned: no vector access)
    for ld in sorted({N, N + 8, (N + 7) // 8 * 8, N + 1}):
        for p in (0.0, 0.1, 0.5):
            keep = torch.from_numpy(RT.keep_np(seed, salt, np.arange(M * N), p).reshape(M, N))
            assert p == 0 or M * N < 4000 or abs(keep.double().mean().item() - (1 - p)) < 0.06
            Z = _padded(z, ld, cuda)
            Hc = torch.full((M, ld), NAN, dtype=TDT[dt], device=cuda)
            ops.gelu_dropout_fwd(Z, ld, Hc, ld, M, N, p, seed, salt, dt=CODE[dt])
            Hc = Hc.cpu()
            assert torch.isnan(Hc[:, N:]).all()                      # the gaps are not written
            got = Hc[:, :N]
            e = rel(got, _gelu64(z64) * keep / (1 - p))
            worst["gelu_fwd"] = max(worst["gelu_fwd"], e)
            assert e < TOL_ACT[dt], (ld, p, e)
            assert torch.equal((got != 0)[nonzero], keep[nonzero]), (ld, p)   # the mask, exactly
            assert not got[z64 == 0].any()
            G = _padded(dhc, ld, cuda)
            ops.gelu_dropout_bwd(G, ld, Z, ld, G, ld, M, N, p, seed, salt, dt=CODE[dt])  # in place
            G = G.cpu()
            assert torch.isnan(G[:, N:]).all()
            want = d64 * keep / (1 - p) * _gelu_grad64(z64)
            e = rel(G[:, :N], want)
            worst["gelu_bwd"] = max(worst["gelu_bwd"], e)
            assert e < TOL_ACT[dt], (ld, p, e)
            assert not G[:, :N][~keep].any()
            if p == 0.1:              # and out of place at the same pitch (same path): same bits
                dZ = torch.full((M, ld), NAN, dtype=TDT[dt], device=cuda)
                ops.gelu_dropout_bwd(_padded(dhc, ld, cuda), ld, Z, ld, dZ, ld, M, N, p, seed,
                                     salt, dt=CODE[dt])
                assert torch.equal(dZ.cpu()[:, :N], G[:, :N])
    if dt == "bf16":      # Z as the GEMM's fp32 output: GELU of the unrounded value, Z's copy kept
        z32 = 2 * torch.randn(M, N, generator=torch.Generator().manual_seed(N))
        keep = torch.from_numpy(RT.keep_np(seed, salt, np.arange(M * N), 0.1).reshape(M, N))
        for ld in sorted({N, (N + 7) // 8 * 8, N + 1}):
            Hc = torch.full((M, ld), NAN, dtype=TDT[dt], device=cuda)
            Za = torch.full((M, ld), NAN, dtype=TDT[dt], device=cuda)
            ops.gelu_dropout_fwd(_padded(z32, ld, cuda), ld, Hc, ld, M, N, 0.1, seed, salt,
                                 dt=CODE[dt], z_fp32=1, Zact=Za, ldza=ld)
            Hc, Za = Hc.cpu(), Za.cpu()
            assert torch.isnan(Hc[:, N:]).all() and torch.isnan(Za[:, N:]).all()
            assert torch.equal(Za[:, :N], z32.to(TDT[dt]))
            assert rel(Hc[:, :N], _gelu64(z32.double()) * keep / 0.9) < TOL_ACT[dt], ld
    print(f"gelu_dropout {dt} ({M},{N}): {worst}")
    if dt == "bf16":
        _log_max(parity_log, "rank_train_kernels_bf16", worst)


def test_gelu_dropout_seed_base(cuda, request):
    """After fs2_set_dropout_seed(s), seed 0 draws the masks of seed s at base 0."""
    from fastspeech2 import ops
    request.addfinalizer(lambda: ops.set_dropout_seed(0))
    M, N, s, salt, p = 7, 24, 90210, 3, 0.5
    z, _ = _gelu_inputs(M, N, "fp32")
    Z = z.to(cuda)

    def fwd(seed):
        Hc = torch.full((M, N), NAN, device=cuda)
        ops.gelu_dropout_fwd(Z, N, Hc, N, M, N, p, seed, salt, dt=0)
        return Hc.cpu()

    try:
        a, other = fwd(s), fwd(0)
        ops.set_dropout_seed(s)
        b = fwd(0)
    finally:
        ops.set_dropout_seed(0)
    c = fwd(s)
    keep = torch.from_numpy(RT.keep_np(s, salt, np.arange(M * N), p).reshape(M, N))
    live = (z != 0) & (z > -5)
    assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, other)
    assert torch.equal((a != 0)[live], keep[live])


# ---------------------------------------------------------------------- kernel 2
HEAD_CASES = {  # (B, T, D, E): lengths, emotions (two share one where B > 1; one or more unused)
    (1, 1, 32, 5): ([1], [3]),
    (3, 13, 32, 5): ([13, 1, 7], [2, 0, 2]),
    (2, 70, 384, 5): ([70, 1], [4, 4]),
    (2, 300, 128, 8): ([1, 300], [6, 6]),
}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(HEAD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_intensity_head_bwd_kernel(cuda, parity_log, shape, dt):
    from fastspeech2 import ops
    B, T, D, E = shape
    lens, emos = (torch.tensor(v) for v in HEAD_CASES[shape])
    assert 1 in lens and T in lens
    g = torch.Generator().manual_seed(B * T + D)
    gI = torch.randn(B, T, E, generator=g)
    H = torch.randn(B * T, D, generator=g).to(TDT[dt])
    Wc, emb = torch.randn(E, D, generator=g), torch.randn(E, D, generator=g)
    keep = (torch.arange(T)[None] < lens[:, None]).double()[..., None]
    dH64 = (gI.double() @ Wc.double()) * keep
    z64 = (H.double().view(B, T, D) + emb.double()[emos][:, None]) * keep
    want = {"dWc": torch.einsum("bte,btd->ed", gI.double(), z64), "dbc": gI.double().sum((0, 1)),
            "dEmb": torch.zeros(E, D, dtype=torch.float64).index_add_(0, emos, dH64.sum(1))}
    unused = sorted(set(range(E)) - set(emos.tolist()))
    assert unused
    worst = 0.0
    for pad in (0, 8, 1):                      # pitch D + 1: rows not 16-byte aligned, scalar path
        ld = D + pad
        runs = []
        for _ in range(2):
            Hb = _padded(H, ld, cuda)
            dH = torch.full((B * T, ld), NAN, dtype=TDT[dt], device=cuda)
            out = {k: torch.full(v.shape, NAN, device=cuda) for k, v in want.items()}
            ws = torch.full((ops.intensity_head_bwd_ws(B, T, D, E),), NAN, device=cuda)
            ops.intensity_head_bwd(gI.to(cuda), Hb, ld, emb.to(cuda), emos.to(cuda), E,
                                   lens.to(cuda), Wc.to(cuda), B, T, D, E, dH, ld, out["dWc"],
                                   out["dbc"], out["dEmb"], dt=CODE[dt], ws=ws)
            runs.append({"dH": dH.cpu(), **{k: v.cpu() for k, v in out.items()}})
        a, b = runs
        for k in a:
            assert torch.equal(a[k], b[k]) or k == "dH", k            # a second run: same bits
        assert torch.equal(a["dH"][:, :D], b["dH"][:, :D])
        assert torch.isnan(a["dH"][:, D:]).all()
        e = rel(a["dH"][:, :D], dH64.view(B * T, D))
        worst = max(worst, e)
        assert e < TOL_ACT[dt], (pad, e)
        pad_rows = (keep.view(B * T) == 0)
        assert not a["dH"][:, :D][pad_rows].any()
        for k, w in want.items():
            assert rel(a[k], w) < 1e-5, (pad, k, rel(a[k], w))
        assert not a["dEmb"][unused].any()                            # exact zeros
    if dt == "bf16":
        _log_max(parity_log, "rank_train_kernels_bf16", {"head_bwd_dH": worst})


# ---------------------------------------------------------------------- kernel 3
@pytest.mark.parametrize("with_gI", [True, False], ids=["gI", "no_gI"])
@pytest.mark.parametrize("T", [1, 13, 300])
def test_rank_pool_bwd_kernel(cuda, T, with_gI):
    from fastspeech2 import ops
    B, E = 5, 5
    g = torch.Generator().manual_seed(T)
    gI = torch.randn(B, T, E, generator=g) if with_gI else None
    gh, gr = torch.randn(B, E, generator=g), torch.randn(B, generator=g)
    h, Wp = torch.randn(B, E, generator=g), torch.randn(E, generator=g)
    length = torch.tensor([T, 1, max(1, T // 2), T, max(1, T - 1)])
    dI = torch.full((B, T, E), NAN, device=cuda)
    dWp = torch.full((E,), NAN, device=cuda)
    ops.rank_pool_bwd(None if gI is None else gI.to(cuda), gh.to(cuda), gr.to(cuda), h.to(cuda),
                      Wp.to(cuda), length.to(cuda), B, T, E, dI, dWp)
    c = (gh.double() + gr.double()[:, None] * Wp.double()[None]) / length.double()[:, None]
    want = c[:, None, :].expand(B, T, E) + (gI.double() if with_gI else 0.0)
    assert rel(dI, want) < 1e-6
    assert rel(dWp, gr.double() @ h.double()) < 1e-5


# ---------------------------------------------------------------------- kernel 4
def _loss_case(B, E, seed, delta=None):
    g = torch.Generator().manual_seed(seed)
    lam = torch.rand(2, B, generator=g)
    hi, hj = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    ri = torch.randn(B, generator=g)
    rj = ri - delta if delta is not None else torch.randn(B, generator=g)
    y_emo = torch.randint(0, E, (B,), generator=g)
    return lam, [hi, hj, ri, rj], (y_emo, torch.zeros_like(y_emo))


SATURATED = torch.tensor([25., -25., 40., -40., 0.5, 25., -40.])


@pytest.mark.parametrize("case", ["B1", "B7", "equal", "saturated", "B300"])
def test_loss_fwd_bwd_kernel(cuda, case):
    """The cases of test_gpu_rank.py::test_loss_kernel.  Gradients against fp32 torch autograd
    on the CPU of the loss restated with the reference's own ops (torch.sigmoid): where fp32
    saturates (ri - rj = 25, 40) both give exactly 0."""
    from fastspeech2.rank import RankLoss
    from fastspeech2.rank_train import RankTrainLoss
    E = 5
    args = {"B1": (1, E, 1), "B7": (7, E, 2), "B300": (300, E, 3), "equal": (7, E, 4),
            "saturated": (7, E, 5)}[case]
    delta = {"equal": torch.zeros(7), "saturated": SATURATED}.get(case)
    lam, leaves, tg = _loss_case(*args, delta=delta)
    B = args[0]
    lam3 = [l.reshape(B, 1, 1) for l in lam]
    cpu = [t.clone().requires_grad_(True) for t in leaves]
    RT.rank_loss((*lam3, None, None, *cpu), tg, 0.1, 1.0)[0].backward()
    dev = [t.to(cuda).requires_grad_(True) for t in leaves]
    pred = (lam3[0].to(cuda), lam3[1].to(cuda), None, None, *dev)
    tgd = tuple(t.to(cuda) for t in tg)
    got = RankTrainLoss(0.1, 1.0)(pred, tgd)
    vals = RankLoss(0.1, 1.0)(tuple(None if p is None else p.detach() for p in pred), tgd)
    for g_, v in zip(got, vals):
        assert g_.shape == () and torch.isfinite(g_)
        assert abs(g_.item() - v.item()) <= 1e-6 * abs(v.item()), (case, g_.item(), v.item())
    assert got[0].requires_grad and not got[1].requires_grad and not got[2].requires_grad
    got[0].backward()
    for name, d, c in zip(("dhi", "dhj", "dri", "drj"), dev, cpu):
        assert d.grad.shape == c.grad.shape and torch.isfinite(d.grad).all(), name
        e = rel(d.grad, c.grad)
        print(f"rank loss {case} {name}: rel {e:.3e}")
        assert e < 1e-5, (case, name, e)
    if case == "saturated":
        sat = SATURATED >= 25
        assert not dev[2].grad.cpu()[sat].any() and not cpu[2].grad[sat].any()
    assert torch.equal(dev[3].grad, -dev[2].grad)


# ---------------------------------------------------------------------- whole step
def _model(kw, sd, cuda, dt, dropout):
    from fastspeech2.rank_train import TrainableRankModel
    m = TrainableRankModel(**dict(kw, dropout=dropout), act_dtype=TDT[dt])
    m.load_state_dict(sd)
    return m.to(cuda).train()


def _inputs(zt, cuda=None):
    d = {k: torch.from_numpy(zt["in." + k]) for k in
         ("emo_X", "neu_X", "emotions", "length", "lambdas")}
    return d if cuda is None else {k: v.to(cuda) for k, v in d.items()}


def _step(m, inp, alpha, beta, loss_kind, seed):
    from fastspeech2.rank_train import RankTrainLoss
    m.zero_grad()
    pred = m(inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"], lambdas=inp["lambdas"],
             seed=seed)
    tg = (inp["emotions"], torch.zeros_like(inp["emotions"]))
    if loss_kind == "kernel":
        losses = RankTrainLoss(alpha, beta)(pred, tg)
    else:                                     # a loss written in torch on the 8-tuple
        losses = RT.rank_loss(pred, tg, alpha, beta)
    losses[0].backward()
    return pred, losses, {k: p.grad.clone() for k, p in m.named_parameters()}


def _check_step(tag, dt, got, want, parity_log, obs_key=None):
    """got / want: (8-tuple, losses, grads).  fp32: the asserted bounds; bf16: cosine and twice
    the observed figures of BF16_OBS[obs_key]."""
    pred, losses, grads = got
    rpred, rlosses, rgrads = want
    figs = {}
    for name, g_, r_ in zip(RT.NAMES, pred, rpred):
        assert tuple(g_.shape) == tuple(r_.shape), name
        if name.startswith("lam"):
            assert torch.equal(g_.cpu().float(), torch.as_tensor(r_).float())
            continue
        assert g_.dtype == torch.float32
        figs[name[0]] = max(figs.get(name[0], 0.0), rel(g_, r_))
    figs["loss"] = max(abs(l.item() - float(r)) / abs(float(r)) for l, r in zip(losses, rlosses))
    assert set(grads) == set(rgrads)
    gerr = {k: rel(grads[k], rgrads[k]) for k in grads}
    gcos = {k: cosine(grads[k], rgrads[k]) for k in grads}
    figs["grad"] = max(gerr.values())
    figs["grad_cos_min"] = min(gcos.values())
    print(f"rank train {tag} {dt}: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    print(f"rank train {tag} {dt}: worst gradient {max(gerr, key=gerr.get)}")
    _log_max(parity_log, f"rank_train_{tag}_{dt}", {k: v for k, v in figs.items()
                                                    if k != "grad_cos_min"})
    old = parity_log[f"rank_train_{tag}_{dt}"]
    old["grad_cos_min"] = min(old.get("grad_cos_min", 1.0), figs["grad_cos_min"])
    for k in grads:
        assert torch.isfinite(grads[k]).all(), k
    if dt == "fp32":
        for k in ("I", "h", "r", "loss"):
            assert figs[k] < 1e-4, (k, figs[k])
        for k, e in gerr.items():
            assert e < 1e-3, (k, e)
    else:
        obs = BF16_OBS[obs_key]
        assert figs["I"] < (2 * obs["I"] if "I" in obs else 3e-2), figs["I"]
        for k in ("h", "r", "loss", "grad"):
            assert figs[k] < 2 * obs[k], (k, figs[k])
        for k, c in gcos.items():
            assert c >= 0.99, (k, c)


@pytest.mark.parametrize("loss_kind", ["kernel", "torch"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_train_step_matches_reference_golden(cuda, golden, train_ref, parity_log, dt, loss_kind):
    _, kw, sd = golden
    zt = train_ref
    alpha, beta = float(zt["alpha"]), float(zt["beta"])
    m = _model(kw, sd, cuda, dt, 0.0)
    inp = _inputs(zt, cuda)
    got = _step(m, inp, alpha, beta, loss_kind, seed=11)
    want = ([zt["out." + n] for n in RT.NAMES], zt["losses"],
            {k[5:]: zt[k] for k in zt.files if k.startswith("grad.")})
    _check_step("golden", dt, got, want, parity_log, "golden")
    ge = got[2]["intensity_extractor.emotion_embedding.weight"].cpu()
    unused = sorted(set(range(ge.shape[0])) - set(zt["in.emotions"].tolist()))
    assert not ge[unused].any()
    assert m.last_dropout[0] == 11 and len(m.last_dropout[1]) == kw["n_encoder_layers"]
    again = _step(m, inp, alpha, beta, loss_kind, seed=11)       # the same seed: the same bits
    for k in got[2]:
        assert torch.equal(got[2][k], again[2][k]), k
    # .grad accumulates over two backwards, zero_grad() clears it
    pred = m(inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"], lambdas=inp["lambdas"],
             seed=11)
    RT.rank_loss(pred, (inp["emotions"], torch.zeros_like(inp["emotions"])), alpha, beta)[0] \
        .backward()
    k = "intensity_extractor.classifier.weight"
    if loss_kind == "torch":
        assert torch.equal(dict(m.named_parameters())[k].grad, 2 * got[2][k])


def _dropout_case(cuda, parity_log, kw, sd, inp_cpu, dt, p, tag, obs_key, flash):
    m = _model(kw, sd, cuda, dt, p)
    inp = {k: v.to(cuda) for k, v in inp_cpu.items()}
    B, T, _ = inp_cpu["emo_X"].shape
    D, H, L = kw["hidden_dim"], kw["n_heads"], kw["n_encoder_layers"]
    assert m.train_engine().use_flash(T, D // H) == flash
    got = _step(m, inp, 0.1, 1.0, "kernel", seed=None)
    seed, salts = m.last_dropout
    assert len({s for layer in salts for s in layer.values()}) == 4 * L      # one salt per site
    masks = RT.masks_from(seed, salts, 2 * B, H, T, D, p)
    want = RT.train_step_grads(sd, inp_cpu, 0.1, 1.0, H, L, masks=masks, p=p)
    _check_step(tag, dt, got, want, parity_log, obs_key)
    # another step draws another seed, hence other masks
    m(inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"], lambdas=inp["lambdas"])
    assert m.last_dropout[0] != seed and m.last_dropout[1] == salts


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_train_step_dropout_tiny_fp32(cuda, golden, train_ref, parity_log, p):
    """The golden's config and inputs under dropout, fp32, materialised attention."""
    _, kw, sd = golden
    _dropout_case(cuda, parity_log, kw, sd, _inputs(train_ref), "fp32", p, f"tiny_p{p}", None,
                  flash=False)


FLASH_KW = dict(n_mels=14, n_heads=2, n_emotions=5, n_encoder_layers=1, hidden_dim=128,
                kernel_size=9)


@pytest.fixture(scope="module")
def flash_case():
    from fastspeech2.intensity import RankModel
    torch.manual_seed(5)
    sd = {k: v.clone() for k, v in RankModel(**FLASH_KW, dropout=0.1).state_dict().items()}
    g = torch.Generator().manual_seed(6)
    B, T, C = 3, 70, FLASH_KW["n_mels"] + 2
    length = torch.tensor([70, 1, 37])
    emo_X, neu_X = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    for b in range(B):
        emo_X[b, int(length[b]):] = 0.0
        neu_X[b, int(length[b]):] = 0.0
    inp = dict(emo_X=emo_X, neu_X=neu_X, emotions=torch.tensor([2, 4, 2]), length=length,
               lambdas=torch.rand(2, B, generator=g))
    return sd, inp


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_train_step_dropout_flash_bf16(cuda, flash_case, parity_log, p):
    """hidden 128, 2 heads, 1 layer, B=3, T=70, lengths (70, 1, 37): the fused attention forward
    and backward with mask_mode 0 under dropout."""
    sd, inp = flash_case
    _dropout_case(cuda, parity_log, FLASH_KW, sd, inp, "bf16", p, f"flash_p{p}", f"flash_p{p}",
                  flash=True)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_training_forward_without_dropout_is_the_eval_forward(cuda, golden, train_ref, dt):
    _, kw, sd = golden
    inp = _inputs(train_ref, cuda)
    m = _model(kw, sd, cuda, dt, 0.0)
    args = (inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"])
    tr = m(*args, lambdas=inp["lambdas"])
    ev = m.eval()(*args, lambdas=inp["lambdas"])
    assert tr[4].requires_grad and not ev[4].requires_grad
    # at p = 0 the same bits, fp32 and bf16.  The two engines share the attention block
    # (fastspeech2.attention) but not every launch: training runs conv1 into fp32 and then
    # fs2_gelu_dropout_fwd where evaluation has the GELU epilogue, and its LayerNorms take the
    # dropout arguments (bf16: a second call for s), so the equality also rests on those kernels
    # agreeing at p = 0
    for name, a, b in zip(RT.NAMES, tr, ev):
        print(f"train vs eval {dt} {name}: rel {rel(a.detach(), b):.3e}")
        assert torch.equal(a.detach(), b), name


def test_backward_refuses_parameters_changed_since_the_forward(cuda, golden, train_ref):
    """The backward reads the engine's current weight images: after a parameter changed it must
    raise, as torch's version counter does for a saved tensor, and a fresh forward must work."""
    _, kw, sd = golden
    inp = _inputs(train_ref, cuda)
    m = _model(kw, sd, cuda, "fp32", 0.0)
    args = (inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"])
    pred = m(*args, lambdas=inp["lambdas"])
    with torch.no_grad():
        m.intensity_extractor.classifier.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified between"):
        (pred[4].sum() + pred[6].sum()).backward()
    pred = m(*args, lambdas=inp["lambdas"])
    (pred[4].sum() + pred[6].sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ---------------------------------------------------------------------- three optimiser steps
LR = 1e-3


def _restated_steps(sd, inp, H, L, n=3):
    params = RT.leaf_params(sd)
    opt = torch.optim.AdamW(list(params.values()), lr=LR)
    emo = inp["emotions"].long()
    out = []
    for _ in range(n):
        opt.zero_grad()
        pred = RT.train_forward(params, inp["emo_X"], inp["neu_X"], emo, inp["length"],
                                inp["lambdas"], H, L)
        loss = RT.rank_loss(pred, (emo, torch.zeros_like(emo)), 0.1, 1.0)[0]
        loss.backward()
        opt.step()
        out.append(loss.item())
    return out


def test_three_rank_train_steps(cuda, golden, train_ref):
    from fastspeech2.rank import bucketize
    from fastspeech2.rank_train import RankTrainLoss, rank_train_step
    _, kw, sd = golden
    inp = _inputs(train_ref)
    want = _restated_steps(sd, inp, kw["n_heads"], kw["n_encoder_layers"])
    assert want[0] > want[1] > want[2], want             # the learning rate lets the loss fall
    m = _model(kw, sd, cuda, "fp32", 0.0)
    opt = torch.optim.AdamW(m.parameters(), lr=LR)
    crit = RankTrainLoss(0.1, 1.0)
    got = []
    for _ in range(3):
        out = rank_train_step(m, crit, opt, inp)
        assert all(t.shape == () and t.device.type == "cuda" and not t.requires_grad for t in out)
        got.append(out[0])
    got = [t.item() for t in got]
    print("rank train steps: got", got, "want", want)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-3 * abs(b), (got, want)
    assert got[0] > got[1] > got[2], got
    for k, v in m.state_dict().items():
        assert not torch.equal(v.cpu(), sd[k]), k        # every tensor moved
    # the trained model still evaluates and fills a prototype bank
    B = inp["emo_X"].shape[0]
    pred = m.eval()(inp["emo_X"].to(cuda), inp["neu_X"].to(cuda), inp["emotions"].to(cuda),
                    inp["length"].to(cuda), torch.ones(2, B, device=cuda))
    assert all(torch.isfinite(t).all() for t in pred)
    batch = dict(inp, speakers=torch.tensor([0, 1, 0, 1]))
    bank = bucketize(m, [batch], 2, kw["n_emotions"], 3)
    assert bank.shape == (2, kw["n_emotions"], 3, kw["n_emotions"])
    assert np.isfinite(bank[~np.isnan(bank)]).all() and m.training is False
