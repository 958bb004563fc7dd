"""CPU: the rank-model training restatement (tests/rank_train_restatement.py) against the
reference's own training step (tests/golden/rank_train_ref.npz, made by
make_golden_rank_train.py from rank_model/model.py and loss.py), the closed-form loss gradients
that ``fs2_rank_loss_fwd_bwd`` implements, and the host-side behaviour of the new entry points
and of ``fastspeech2.rank_train``.

Tolerance 1e-5 (rtol and atol), as in test_rank_host.py: the same arithmetic in another order
(here float64 against the reference's fp32, whose own distance from float64 is 1.4e-6).
"""
import ctypes

import numpy as np
import pytest
import torch

import rank_restatement as R
import rank_train_restatement as RT


@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


@pytest.fixture(scope="module")
def train_ref(golden_dir):
    return RT.load_golden_train(golden_dir)


def _close(a, b):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=1e-5, atol=1e-5)


def _inputs(zt):
    return {k: torch.from_numpy(zt["in." + k]) for k in
            ("emo_X", "neu_X", "emotions", "length", "lambdas")}


def test_restatement_matches_reference_training_step(golden, train_ref):
    _, kw, sd = golden
    zt = train_ref
    pred, losses, grads = RT.train_step_grads(sd, _inputs(zt), float(zt["alpha"]),
                                              float(zt["beta"]), kw["n_heads"],
                                              kw["n_encoder_layers"])
    for name, got in zip(RT.NAMES, pred):
        assert tuple(got.shape) == zt["out." + name].shape, name
        _close(got, zt["out." + name])
    _close(torch.stack(losses), zt["losses"])
    assert set(grads) == set(sd) == {k[5:] for k in zt.files if k.startswith("grad.")}
    for k, g in grads.items():
        ref = zt["grad." + k]
        assert ref.any(), k
        _close(g, ref)
        assert (g - torch.from_numpy(ref)).abs().max() / np.abs(ref).max() < 1e-5, k
    # the fixture holds what the cases are about: a shared and two unused emotions, a length of
    # 1 and one of T
    ge = zt["grad.intensity_extractor.emotion_embedding.weight"]
    emo = zt["in.emotions"]
    unused = sorted(set(range(ge.shape[0])) - set(emo.tolist()))
    assert len(set(emo.tolist())) < len(emo) and unused and not ge[unused].any()
    assert 1 in zt["in.length"] and zt["in.emo_X"].shape[1] in zt["in.length"]


def test_all_ones_masks_are_the_maskless_forward(golden, train_ref):
    _, kw, sd = golden
    inp = _inputs(train_ref)
    B, T, _ = inp["emo_X"].shape
    D, H, L = kw["hidden_dim"], kw["n_heads"], kw["n_encoder_layers"]
    salts = [dict(attn=4 * i + 1, res1=4 * i + 2, gelu=4 * i + 3, res2=4 * i + 4) for i in range(L)]
    masks = RT.masks_from(77, salts, 2 * B, H, T, D, 0.0)
    assert all(m[k].all() for m in masks for k in m)
    a = RT.train_step_grads(sd, inp, 0.1, 1.0, H, L)
    b = RT.train_step_grads(sd, inp, 0.1, 1.0, H, L, masks=masks, p=0.0)
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k])
    # and real masks drop about p of each site, differently per salt
    masks = RT.masks_from(77, salts, 2 * B, H, T, D, 0.5)
    for m in masks:
        for k, t in m.items():
            assert 0.45 < t.double().mean() < 0.55, k
    assert not torch.equal(masks[0]["res1"], masks[0]["res2"])


def _loss_case(B, E, seed, delta=None):
    g = torch.Generator().manual_seed(seed)
    lam = torch.rand(2, B, generator=g)
    hi, hj = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    ri = torch.randn(B, generator=g)
    rj = ri - delta if delta is not None else torch.randn(B, generator=g)
    y_emo = torch.randint(0, E, (B,), generator=g)
    return lam, hi, hj, ri, rj, y_emo, torch.zeros_like(y_emo)


def closed_form_grads(lam, hi, hj, ri, rj, y_emo, y_neu, alpha, beta, dtype=torch.float64):
    """The formulas of fs2_rank_loss_fwd_bwd's description, in ``dtype``."""
    lam, hi, hj, ri, rj = (t.to(dtype) for t in (lam, hi, hj, ri, rj))
    B, E = hi.shape
    oh = lambda y: torch.nn.functional.one_hot(y, E).to(dtype)

    def dh(h, l):
        s = torch.softmax(h, dim=1)
        return alpha * (l.mean() * (s - oh(y_emo)) + (1 - l.mean()) * (s - oh(y_neu))) / B

    p = torch.sigmoid(ri - rj)
    t = (lam[0] - lam[1] + 1) / 2
    dri = -beta / B * (t / (p + 1e-8) - (1 - t) / (1 - p + 1e-8)) * (p * (1 - p))
    return dh(hi, lam[0]), dh(hj, lam[1]), dri, -dri


def _autograd(loss_fn, c):
    lam, hi, hj, ri, rj, y_emo, y_neu = c
    leaves = [t.clone().requires_grad_(True) for t in (hi, hj, ri, rj)]
    B = hi.shape[0]
    pred = (lam[0].reshape(B, 1, 1), lam[1].reshape(B, 1, 1), torch.zeros(1), torch.zeros(1),
            *leaves)
    loss_fn(pred, (y_emo, y_neu), 0.1, 1.0)[0].backward()
    return [t.grad for t in leaves]


@pytest.mark.parametrize("case", ["B1", "B7", "equal", "B300"])
def test_closed_form_loss_gradients_equal_autograd(case):
    """Float64 closed form against torch autograd of ``rank_restatement.rank_loss`` (fp32), on
    the unsaturated cases of the existing loss test."""
    E = 5
    args = {"B1": (1, E, 1), "B7": (7, E, 2), "B300": (300, E, 3)}.get(case)
    c = _loss_case(*args) if args else _loss_case(7, E, 4, delta=torch.zeros(7))
    want = closed_form_grads(*c, 0.1, 1.0)
    for g, w in zip(_autograd(R.rank_loss, c), want):
        assert g.abs().max() > 0
        assert (g.double() - w).abs().max() <= 1e-5 * w.abs().max()


def test_closed_form_loss_gradients_saturated_fp32():
    """ri - rj of +-25 and +-40: in fp32 sigmoid(25) is exactly 1, and the reference's backward
    (torch.sigmoid's p (1 - p)) is exactly 0 there.  The closed form in fp32 must give the same
    as fp32 autograd of the loss written with torch.sigmoid (rank_train_restatement.rank_loss);
    autograd of rank_restatement's 1 / (1 + exp(-x)) does not (its backward is p^2 exp(-x))."""
    delta = torch.tensor([25., -25., 40., -40., 0.5, 25., -40.])
    c = _loss_case(7, 5, 5, delta=delta)
    want = closed_form_grads(*c, 0.1, 1.0, dtype=torch.float32)
    got = _autograd(RT.rank_loss, c)
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and torch.isfinite(w).all()
        assert (g.double() - w.double()).abs().max() <= 1e-5 * w.double().abs().max()
    sat = delta >= 25
    assert not got[2][sat].any() and not want[2][sat].any()          # exact zeros
    assert _autograd(R.rank_loss, c)[2][sat].abs().min() > 0          # the other formula's


def test_rank_train_kernels_host_validation():
    """Every new entry point returns before any launch: FS2_EINVAL on null pointers, E > 8, a bad
    dtype or p outside [0, 1); 0 on empty work."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    f = lib.fs2_gelu_dropout_fwd      # (Z, ldz, z_fp32, Zact, ldza, Hc, ldh, M, N, p, ...)
    assert f(p, 8, 0, None, 0, p, 8, 0, 8, 0.1, 1, 2, N.F32, None) == 0
    assert f(p, 8, 1, p, 8, p, 8, 4, 0, 0.1, 1, 2, N.BF16, None) == 0
    assert f(None, 8, 0, None, 0, p, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1
    assert f(p, 8, 0, None, 0, None, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1
    assert f(p, 4, 0, None, 0, p, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1      # ldz < N
    assert f(p, 8, 1, p, 4, p, 8, 4, 8, 0.1, 1, 2, N.BF16, None) == -1        # ldza < N
    assert f(p, 8, 0, None, 0, p, 8, 4, 8, 1.0, 1, 2, N.F32, None) == -1      # p = 1
    assert f(p, 8, 0, None, 0, p, 8, 4, 8, -0.1, 1, 2, N.F32, None) == -1
    assert f(p, 8, 0, None, 0, p, 8, 4, 8, float("nan"), 1, 2, N.F32, None) == -1
    assert f(p, 8, 0, None, 0, p, 8, 4, 8, 0.1, 1, 2, 7, None) == -1          # dtype
    assert f(p, 8, 0, None, 0, p, 8, -1, 8, 0.1, 1, 2, N.F32, None) == -1
    b = lib.fs2_gelu_dropout_bwd
    assert b(p, 8, p, 8, p, 8, 0, 8, 0.1, 1, 2, N.F32, None) == 0
    assert b(None, 8, p, 8, p, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1
    assert b(p, 8, None, 8, p, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1
    assert b(p, 8, p, 8, None, 8, 4, 8, 0.1, 1, 2, N.F32, None) == -1
    assert b(p, 8, p, 8, p, 4, 4, 8, 0.1, 1, 2, N.F32, None) == -1      # lddz < N
    assert b(p, 8, p, 8, p, 8, 4, 8, 1.5, 1, 2, N.F32, None) == -1
    assert b(p, 8, p, 8, p, 8, 4, 8, 0.1, 1, 2, 2, None) == -1
    h = lib.fs2_intensity_head_bwd
    assert h(p, p, 32, p, p, 5, p, p, 0, 4, 32, 5, p, 32, p, p, p, p, N.F32, None) == 0
    assert h(p, p, 32, p, p, 5, p, p, 2, 0, 32, 5, p, 32, p, p, p, p, N.BF16, None) == 0
    assert h(None, p, 32, p, p, 5, p, p, 2, 4, 32, 5, p, 32, p, p, p, p, N.F32, None) == -1
    assert h(p, p, 32, p, p, 5, p, p, 2, 4, 32, 5, None, 32, p, p, p, p, N.F32, None) == -1
    assert h(p, p, 32, p, p, 5, p, p, 2, 4, 32, 5, p, 32, p, p, p, None, N.F32, None) == -1
    assert h(p, p, 32, p, p, 5, p, p, 2, 4, 32, 9, p, 32, p, p, p, p, N.F32, None) == -1   # E > 8
    assert h(p, p, 16, p, p, 5, p, p, 2, 4, 32, 5, p, 32, p, p, p, p, N.F32, None) == -1   # ldh < D
    assert h(p, p, 32, p, p, 5, p, p, 2, 4, 32, 5, p, 32, p, p, p, p, 3, None) == -1
    w = lib.fs2_intensity_head_bwd_workspace_floats
    assert w(0, 4, 32, 5) == 0 and w(2, 16, 32, 5) == 2 * 6 * 32 and w(2, 17, 32, 5) == 4 * 6 * 32
    q = lib.fs2_rank_pool_bwd
    assert q(p, p, p, p, p, p, 0, 4, 5, p, p, None) == 0
    assert q(None, p, p, p, p, p, 0, 4, 5, p, p, None) == 0
    assert q(p, None, p, p, p, p, 2, 4, 5, p, p, None) == -1
    assert q(p, p, p, p, p, p, 2, 4, 5, None, p, None) == -1
    assert q(p, p, p, p, p, p, 2, 4, 5, p, None, None) == -1
    assert q(p, p, p, p, p, p, 2, 4, 9, p, p, None) == -1               # E > 8
    assert q(p, p, p, p, p, p, -1, 4, 5, p, p, None) == -1
    l = lib.fs2_rank_loss_fwd_bwd
    assert l(p, p, p, p, p, p, p, p, 0, 5, 0.1, 1.0, p, p, p, p, p, None) == 0
    assert l(p, p, p, p, p, p, p, p, 2, 0, 0.1, 1.0, p, p, p, p, p, None) == -1
    assert l(p, p, p, p, p, p, p, p, 2, 9, 0.1, 1.0, p, p, p, p, p, None) == -1   # E > 8
    assert l(p, p, p, p, p, p, None, p, 2, 5, 0.1, 1.0, p, p, p, p, p, None) == -1
    assert l(p, p, p, p, p, p, p, p, 2, 5, 0.1, 1.0, None, p, p, p, p, None) == -1
    assert l(p, p, p, p, p, p, p, p, 2, 5, 0.1, 1.0, p, p, p, p, None, None) == -1


def test_trainable_model_keys_and_checkpoints(golden):
    from fastspeech2.intensity import RankModel
    from fastspeech2.rank_train import TrainableRankModel
    _, kw, sd = golden
    m, base = TrainableRankModel(**kw), RankModel(**kw)
    assert issubclass(TrainableRankModel, RankModel)
    assert list(m.state_dict()) == list(base.state_dict())
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in base.named_buffers()]
    m.load_state_dict(sd)
    base.load_state_dict(m.state_dict())                 # and back
    for k, v in base.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_training_forward_refuses_cpu_tensors(golden):
    from fastspeech2.rank_train import TrainableRankModel, RankTrainLoss
    _, kw, sd = golden
    m = TrainableRankModel(**kw)
    m.load_state_dict(sd)
    x = torch.zeros(1, 4, kw["n_mels"] + 2)
    args = (x, x, torch.zeros(1, dtype=torch.long), torch.tensor([4]))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.train()(*args)
    with pytest.raises(RuntimeError, match="HIP device"):        # the parent's eval forward
        m.eval()(*args)
    pred = (torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), None, None, torch.zeros(1, 5),
            torch.zeros(1, 5), torch.zeros(1), torch.zeros(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        RankTrainLoss(0.1, 1.0)(pred, (args[2], args[2]))


def test_rank_model_itself_is_unchanged(golden):
    from fastspeech2.intensity import RankModel
    import fastspeech2.rank_train  # noqa: F401  (importing the new module changes nothing)
    _, kw, _ = golden
    m = RankModel(**kw).train()
    x = torch.zeros(1, 4, kw["n_mels"] + 2)
    with pytest.raises(NotImplementedError, match="section 7"):
        m(x, x, torch.zeros(1, dtype=torch.long), torch.tensor([4]))
    assert not hasattr(m, "train_engine")
