"""CPU: the rank-model evaluation path's restatement (tests/rank_restatement.py) against the
reference's own outputs (tests/golden/rank_ref.npz, made by make_golden_rank.py from
rank_model/model.py, loss.py, dataset.py and inference.py::bucketize), and the host-side
behaviour of ``RankModel.forward``.

Tolerance 1e-5 (rtol and atol): the same fp32 torch-CPU arithmetic in another order.
"""
import numpy as np
import pytest
import torch

import rank_restatement as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


def _close(a, b):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=1e-5, atol=1e-5)


def test_restatement_matches_reference_eval_case(golden):
    z, kw, sd = golden
    t = lambda k: torch.from_numpy(z["eval." + k])
    pred = R.rank_forward(sd, t("emo_X"), t("neu_X"), t("emotions"), t("length"), t("lambdas"),
                          kw["n_heads"], kw["n_encoder_layers"])
    names = ("lam_i", "lam_j", "Ii", "Ij", "hi", "hj", "ri", "rj")
    for name, got in zip(names, pred):
        assert tuple(got.shape) == z["eval." + name].shape, name
        _close(got, z["eval." + name])
    assert int(t("length")[-1]) == 1 and torch.isfinite(pred[4]).all()
    losses = R.rank_loss(pred, (t("emotions"), torch.zeros_like(t("emotions"))), 0.1, 1.0)
    _close(torch.stack(losses), z["eval.losses"])
    # the golden's own 8-tuple through the restated loss as well
    losses = R.rank_loss([t(n) for n in names], (t("emotions"), torch.zeros_like(t("emotions"))),
                         0.1, 1.0)
    _close(torch.stack(losses), z["eval.losses"])


def test_restatement_matches_reference_bank(golden):
    z, kw, sd = golden
    batches = R.bank_batches(z)
    n_spk, n_emo, K = len(z["speakers"]), len(z["emotions"]), int(z["bucket_size"])
    assert sum(len(b["length"]) for b in batches) == len(z["bank.raw_speaker"])
    for b in batches:
        B = len(b["length"])
        _, _, I, _, h, _, r, _ = R.rank_forward(sd, b["emo_X"], b["neu_X"], b["emotions"],
                                                b["length"], torch.ones(2, B), kw["n_heads"],
                                                kw["n_encoder_layers"])
        _close(I, b["I"]), _close(h, b["h"]), _close(r, b["r"])
        b["I_restated"], b["r_restated"] = I, r
    ref = z["bank.bank"]
    assert ref.shape == (n_spk, n_emo, K, n_emo)
    for I_key, r_key in (("I", "r"), ("I_restated", "r_restated")):
        bank = R.bank_np(batches, n_spk, n_emo, K, I_key, r_key)
        np.testing.assert_allclose(bank, ref, rtol=1e-5, atol=1e-5, equal_nan=True)
    # the fixture holds what the cases are about: empty groups and a one-utterance group
    groups = np.concatenate([(b["speakers"] * n_emo + b["emotions"]).numpy() for b in batches])
    counts = np.bincount(groups, minlength=n_spk * n_emo)
    assert (counts == 0).any() and (counts == 1).any()
    assert not ref.reshape(n_spk * n_emo, -1)[counts == 0].any()


def test_binning_restatement_edge_cases():
    """Uneven split, ties kept in arrival order, fewer frames than buckets."""
    f = [np.full((2, 1), 1.0), np.full((3, 1), 2.0), np.full((2, 1), 4.0)]
    out = R.bucket_means_np(f, [0.5, 0.5, -1.0], [0, 0, 0], 2, 3)
    # order: utterance 2, then 0, then 1 (tie in arrival order): 4 4 1 | 1 2 | 2 2
    np.testing.assert_allclose(out[0, :, 0], [3.0, 1.5, 2.0])
    assert not out[1].any()
    out = R.bucket_means_np([np.ones((2, 1))], [0.0], [0], 1, 3)
    assert out[0, 0, 0] == 1 and out[0, 1, 0] == 1 and np.isnan(out[0, 2, 0])


def test_rank_kernels_host_validation():
    """The four entry points return before any launch: FS2_EINVAL on null pointers and bad
    sizes, 0 on empty work."""
    import ctypes
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    assert lib.fs2_rank_mixup_input(p, p, p, 0, 4, 16, p, 16, N.F32, None) == 0
    assert lib.fs2_rank_mixup_input(None, p, p, 1, 4, 16, p, 16, N.F32, None) == -1
    assert lib.fs2_rank_mixup_input(p, p, None, 1, 4, 16, p, 16, N.F32, None) == -1
    assert lib.fs2_rank_mixup_input(p, p, p, 1, 4, 16, p, 12, N.F32, None) == -1     # ldx < C
    assert lib.fs2_rank_mixup_input(p, p, p, 1, 4, 16, p, 16, 7, None) == -1         # dtype
    assert lib.fs2_rank_mixup_input(p, p, p, -1, 4, 16, p, 16, N.F32, None) == -1
    assert lib.fs2_rank_pool(p, p, p, 0, 4, 5, p, p, None) == 0
    assert lib.fs2_rank_pool(None, p, p, 1, 4, 5, p, p, None) == -1
    assert lib.fs2_rank_pool(p, p, p, 1, 4, 9, p, p, None) == -1                     # E > 8
    assert lib.fs2_rank_pool(p, p, p, 1, 4, 5, p, None, None) == -1
    assert lib.fs2_rank_loss_fwd(p, p, p, p, p, p, p, p, 0, 5, 0.1, 1.0, p, None) == 0
    assert lib.fs2_rank_loss_fwd(p, p, p, p, p, p, p, p, 2, 0, 0.1, 1.0, p, None) == -1
    assert lib.fs2_rank_loss_fwd(p, p, p, p, p, p, None, p, 2, 5, 0.1, 1.0, p, None) == -1
    assert lib.fs2_rank_loss_fwd(p, p, p, p, p, p, p, p, 2, 5, 0.1, 1.0, None, None) == -1
    assert lib.fs2_bucket_means(p, p, p, p, p, 0, 3, 5, p, None) == 0
    assert lib.fs2_bucket_means(p, p, None, p, p, 2, 3, 5, p, None) == -1
    assert lib.fs2_bucket_means(p, p, p, p, p, 2, 3, 9, p, None) == -1               # E > 8
    assert lib.fs2_bucket_means(p, p, p, p, p, 2, -1, 5, p, None) == -1


def test_rank_model_training_forward_still_refused(golden):
    from fastspeech2.intensity import RankModel
    _, kw, _ = golden
    m = RankModel(**kw).train()
    x = torch.zeros(1, 4, kw["n_mels"] + 2)
    with pytest.raises(NotImplementedError, match="section 7"):
        m(x, x, torch.zeros(1, dtype=torch.long), torch.tensor([4]))


def test_rank_model_eval_forward_refuses_cpu_tensors(golden):
    from fastspeech2.intensity import RankModel
    _, kw, sd = golden
    m = RankModel(**kw)
    m.load_state_dict(sd)
    m.eval()
    x = torch.zeros(1, 4, kw["n_mels"] + 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(x, x, torch.zeros(1, dtype=torch.long), torch.tensor([4]))
