"""CPU checks of the validation path: the C ABI of the forward-only loss (declared, refusing
what ``fs2_loss_fwd_bwd`` refuses, its workspace the restated carve), and ``valid_one_epoch`` /
``fit`` driven by a scripted fake trainer and store (tests/valid_restatement.py), alone and on
two gloo ranks."""
import ctypes
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import loss_restatement as LR
import valid_restatement as VR
from conftest import PKG, ROOT
from test_dp_gloo import _free_port
from test_host import _header_functions


# ---- 1: the C ABI -----------------------------------------------------------------------------
def test_header_declares_the_forward_only_loss():
    """Declared in the header, so test_host's export test holds ``SIGNATURES`` and the library
    to them; and the Python wrappers exist."""
    from fastspeech2 import _native as N
    from fastspeech2 import ops
    declared = _header_functions()
    for name in ("fs2_loss_fwd", "fs2_loss_fwd_workspace_floats"):
        assert name in declared and name in N.SIGNATURES
        assert hasattr(N.load(), name)
    assert callable(ops.loss_fwd) and callable(ops.loss_fwd_ws)


def _desc(B, Tm, NM, dtype=None, buf=None, skip=()):
    """A descriptor whose required pointers point into ``buf`` (host memory: no call that gets as
    far as a launch is made with it) and whose five gradient pointers are null."""
    from fastspeech2 import _native as N
    d = N.LossDesc()
    d.B, d.Tm, d.Tp, d.NM, d.dtype = B, Tm, 8, NM, N.F32 if dtype is None else dtype
    if buf is not None:
        for name in REQUIRED:
            if name not in skip:
                setattr(d, name, ctypes.addressof(buf))
    return d


REQUIRED = ("mel_out", "postnet_out", "log_dur", "pitch_pred", "energy_pred", "mel_tgt", "dur_tgt",
            "pitch_avg", "energy_avg", "mel_len", "phon_len", "loss_out", "workspace")


def test_loss_fwd_host_refusals():
    """Every refusal of fs2_loss_fwd_bwd, before any launch (the pointers are host memory or
    null; a launch would fault), and B = 0 is a no-op with null gradient pointers."""
    from fastspeech2 import _native as N
    f = N.load().fs2_loss_fwd
    buf = (ctypes.c_char * 64)()
    call = lambda d: f(ctypes.byref(d), None)
    assert f(None, None) == -1
    assert call(_desc(2, 10, 80, buf=buf)) == -1        # Tm < 11: the SSIM window does not fit
    assert call(_desc(2, 27, 10, buf=buf)) == -1        # NM < 11
    assert call(_desc(2, 27, 97, buf=buf)) == -1        # NM > 96: the SSIM LDS tiles
    assert call(_desc(2, 27, 80, dtype=7, buf=buf)) == -1   # unknown dtype
    assert call(_desc(2, 27, 80)) == -1                 # a valid shape, every pointer null
    for name in REQUIRED:                               # each required pointer on its own
        assert call(_desc(2, 27, 80, buf=buf, skip=(name,))) == -1, name
    assert call(_desc(0, 27, 80)) == 0                  # empty batch, everything null
    assert call(_desc(0, 27, 80, buf=buf)) == 0
    assert call(_desc(-1, 27, 80, buf=buf)) == 0


def test_loss_fwd_bwd_still_needs_its_gradient_pointers():
    from fastspeech2 import _native as N
    buf = (ctypes.c_char * 64)()
    d = _desc(2, 27, 80, buf=buf)
    assert N.load().fs2_loss_fwd_bwd(ctypes.byref(d), None) == -1
    d.dtype = 7
    assert N.load().fs2_loss_fwd_bwd(ctypes.byref(d), None) == -1


@pytest.mark.parametrize("B,Tm,NM", LR.case_shapes() + [(300, 60, 80), (32, 1000, 80)])
def test_fwd_workspace_size_is_the_carve_without_the_gradient_regions(B, Tm, NM):
    from fastspeech2 import _native as N
    lib = N.load()
    got = lib.fs2_loss_fwd_workspace_floats(B, Tm, NM)
    assert got == VR.fwd_workspace_floats(B, Tm, NM)
    npix = (Tm - 10) * (NM - 10)
    assert lib.fs2_loss_workspace_floats(B, Tm, NM) - got == 3 * B * npix + B * Tm * NM
    assert got - VR.fwd_carve_extent(B, Tm, NM) == 4    # what the carve touches, plus the slack


# ---- 2: valid_one_epoch with fakes ------------------------------------------------------------
def test_valid_one_epoch_order_mean_and_store_flags():
    """Seven utterances in batches of three: [0,1,2], [3,4,5], [6] -- unshuffled, the short last
    batch kept -- and the mean gives every batch the same weight."""
    from fastspeech2.train import valid_one_epoch
    tr, store, ext = VR.FakeTrainer(), VR.FakeStore(7), object()
    tr.model.train()
    got = valid_one_epoch(tr, store, 3, ext)
    assert tr.seen == [[0, 1, 2], [3, 4, 5], [6]]
    assert store.calls == [dict(batch_size=3, shuffle=False, drop_last=False, rank=0,
                                world_size=1, intensity=True, extractor=ext)]
    want = (VR.batch_vector([0, 1, 2]) + VR.batch_vector([3, 4, 5]) + VR.batch_vector([6])) / 3
    assert got.device.type == "cpu" and got.shape == (8,) and torch.equal(got, want)
    assert tr.modes == [False] * 3 and tr.model.training     # eval inside, train restored
    tr.model.eval()
    valid_one_epoch(tr, store, 3, ext)
    assert not tr.model.training                             # an eval model stays in eval


def test_valid_one_epoch_restores_the_mode_after_a_raised_step():
    from fastspeech2.train import valid_one_epoch
    tr = VR.FakeTrainer(raise_at=2)
    tr.model.train()
    with pytest.raises(RuntimeError, match="scripted"):
        valid_one_epoch(tr, VR.FakeStore(7), 3, None)
    assert tr.model.training and tr.modes == [False]


def test_valid_one_epoch_first_batch_hook_and_empty_epoch():
    from fastspeech2.train import valid_one_epoch
    tr, calls = VR.FakeTrainer(), []
    got = valid_one_epoch(tr, VR.FakeStore(7), 3, None,
                          on_first_batch=lambda pred, batch: calls.append((pred, batch)))
    assert len(calls) == 1
    pred, batch = calls[0]
    assert len(pred) == 8 and pred[0] == "prediction0" and batch[0].tolist() == [0, 1, 2]
    plain = valid_one_epoch(VR.FakeTrainer(), VR.FakeStore(7), 3, None)
    assert torch.equal(got, plain)                           # the hook changes no value
    with pytest.raises(ValueError, match="no batch"):
        valid_one_epoch(tr, VR.FakeStore(0), 3, None)


# ---- 3: fit with fakes ------------------------------------------------------------------------
def _fit(script, n_epochs, patience, max_iterations, exp_path=None, n_train=7, on_epoch=None):
    from fastspeech2.train import fit
    tr = VR.FakeTrainer(valid_script=script)
    train, valid = VR.FakeStore(n_train), VR.FakeStore(5)
    hist = fit(tr, train, valid, 3, None, n_epochs, patience, max_iterations, exp_path=exp_path,
               generator=torch.Generator().manual_seed(0), on_epoch=on_epoch)
    return tr, train, valid, hist


def _check_against_model(hist, script, n_epochs, patience, max_iterations, steps_per_epoch):
    ran, best_epoch, best, stopped, _ = VR.fit_model(script, n_epochs, patience, max_iterations,
                                                     steps_per_epoch)
    assert len(hist["train"]) == len(hist["valid"]) == ran
    assert hist["best_epoch"] == best_epoch and hist["stopped"] == stopped
    assert hist["best_valid_loss"] == float(torch.tensor(best, dtype=torch.float32))
    for v, s in zip(hist["valid"], script):
        assert v.shape == (8,) and (float(v[0]) == float(torch.tensor(s)) or s != s)


def test_fit_stops_by_patience_and_keeps_the_best_epochs_weights(tmp_path):
    """improve, improve, then two stalls with patience 2: four epochs, best_model.pth holds the
    parameter after epoch 1's training (2 steps per epoch: 4.0), last_model.pth the last (8.0)."""
    script = [3.0, 2.0, 2.0, 2.5, 1.0, 1.0]
    hooks = []
    tr, train, valid, hist = _fit(script, 6, 2, 10 ** 6, exp_path=str(tmp_path / "exp"),
                                  on_epoch=lambda e, t, v: hooks.append((e, float(t[0]), float(v[0]))))
    _check_against_model(hist, script, 6, 2, 10 ** 6, 2)
    assert hist["stopped"] == "patience" and hist["best_epoch"] == 1 and len(hist["valid"]) == 4
    best = torch.load(tmp_path / "exp" / "best_model.pth", weights_only=True)
    last = torch.load(tmp_path / "exp" / "last_model.pth", weights_only=True)
    assert best["w"].tolist() == [4.0] * 3 and last["w"].tolist() == [8.0] * 3
    assert sorted(os.listdir(tmp_path / "exp")) == ["best_model.pth", "last_model.pth"]
    # the reference's loader flags: train shuffled without the short batch, valid in order with it
    assert all(c["shuffle"] and c["drop_last"] for c in train.calls) and len(train.calls) == 4
    assert all(not c["shuffle"] and not c["drop_last"] for c in valid.calls)
    assert tr.steps == 8 and len(tr.seen) == 4 * 2
    # the hook sees every epoch: the train mean of steps 2e+1, 2e+2 and the scripted loss
    assert hooks == [(e, 2 * e + 1.5, script[e]) for e in range(4)]
    assert tr.model.training                                 # left as train_one_epoch leaves it


def test_fit_stops_by_max_iterations():
    script = [3.0, 2.0, 1.0, 0.5, 0.4]
    tr, _, _, hist = _fit(script, 5, 3, 5, n_train=7)        # 2 steps per epoch: 2, 4, 6 >= 5
    _check_against_model(hist, script, 5, 3, 5, 2)
    assert hist["stopped"] == "max_iterations" and len(hist["valid"]) == 3 and tr.steps == 6
    assert hist["best_epoch"] == 2


def test_fit_runs_to_n_epochs():
    script = [3.0, 2.0, 2.5]
    _, _, _, hist = _fit(script, 3, 5, 10 ** 6)
    _check_against_model(hist, script, 3, 5, 10 ** 6, 2)
    assert hist["stopped"] == "n_epochs" and hist["best_epoch"] == 1


def test_fit_nan_validation_loss_is_no_improvement(tmp_path):
    """NaN < best is false: a NaN epoch counts against the patience and writes no best model,
    also as the very first epoch (best stays inf, best_epoch None)."""
    nan = float("nan")
    script = [2.0, nan, nan, 1.0]
    _, _, _, hist = _fit(script, 4, 2, 10 ** 6, exp_path=str(tmp_path / "a"))
    _check_against_model(hist, script, 4, 2, 10 ** 6, 2)
    assert hist["stopped"] == "patience" and hist["best_epoch"] == 0 and len(hist["valid"]) == 3
    assert torch.load(tmp_path / "a" / "best_model.pth", weights_only=True)["w"].tolist() == [2.0] * 3
    _, _, _, hist = _fit([nan, nan], 2, 5, 10 ** 6, exp_path=str(tmp_path / "b"))
    assert hist["best_epoch"] is None and hist["best_valid_loss"] == float("inf")
    assert os.listdir(tmp_path / "b") == ["last_model.pth"]


def test_fit_rewrites_last_model_every_epoch(tmp_path):
    seen = []

    def on_epoch(epoch, train_vec, valid_vec):
        seen.append(torch.load(tmp_path / "last_model.pth", weights_only=True)["w"][0].item())

    _fit([3.0, 2.0, 1.0], 3, 5, 10 ** 6, exp_path=str(tmp_path), on_epoch=on_epoch)
    assert seen == [2.0, 4.0, 6.0]


def test_fit_without_exp_path_writes_nothing(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch, "save", lambda *a, **k: pytest.fail("torch.save called"))
    _, _, _, hist = _fit([3.0, 2.0], 2, 5, 10 ** 6)
    assert hist["stopped"] == "n_epochs" and os.listdir(tmp_path) == []


# ---- 4: two gloo ranks ------------------------------------------------------------------------
N_UTT, BATCH = 11, 2      # per rank 5 utterances: batches of 2, 2, 1


def _worker(rank, world, port, out_dir):
    import sys
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import valid_restatement as V
    from fastspeech2.train import valid_one_epoch
    tr, store = V.FakeTrainer(), V.FakeStore(N_UTT)
    got = valid_one_epoch(tr, store, BATCH, None)
    torch.save({"vec": got, "seen": tr.seen, "call": store.calls[0]},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_valid_one_epoch_two_gloo_ranks_return_the_global_mean(tmp_path):
    from fastspeech2.device_store import epoch_order
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    out = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world)]
    total, count = torch.zeros(8), 0
    for r in range(world):
        share = [idx.tolist() for idx in epoch_order(N_UTT, BATCH, rank=r, world_size=world)]
        assert out[r]["seen"] == share and len(share) == 3
        assert out[r]["call"]["rank"] == r and out[r]["call"]["world_size"] == world
        for ids in share:
            total += VR.batch_vector(ids)
            count += 1
    assert count == 6
    assert torch.equal(out[0]["vec"], out[1]["vec"])
    assert torch.equal(out[0]["vec"], total / count)
