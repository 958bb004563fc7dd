"""GPU: the validation path -- fs2_loss_fwd (csrc/loss.hip), ``fused_loss(need_grads=False)``,
``eval_loss``, ``FusedTrainer.eval_step``, ``valid_one_epoch`` and ``fit``.

fs2_loss_fwd runs the value path of fs2_loss_fwd_bwd with the gradient work compiled out, so its
seven values are held to test_gpu_loss.py's rule against the same float64 restatement,
``|got - ref64| <= max(8 * e_ref, 64 * 2^-24) * max(1, |ref64|)`` (derived there: the values are
fp32 sums of fp32 arithmetic on the inputs in both dtypes).  The difference to fs2_loss_fwd_bwd's
values on the same inputs is held to the same tolerance; whether the two are bit-equal is
recorded, not asserted (the compiler may contract a product differently once its second use, the
gradient, is gone): ``parity_log`` key ``loss_fwd_<case>_<dtype>``.  No float atomic is left in
the forward-only pass, so two calls must agree bit for bit at every shape.

The launcher passes null gradient pointers; the loss and a workspace of exactly
``fs2_loss_fwd_workspace_floats`` floats lie inside NaN-filled tensors whose 64-element margins
must stay NaN.
"""
import numpy as np
import pytest
import torch

import fs2_store_restatement as S
import loss_restatement as LR
import valid_restatement as VR
from loss_restatement import W_MIXED
from test_gpu_loss import (DTYPES, PLAIN, VAL_FLOOR, _guarded, _intact, _on, launch, reference,
                           same_bits)

pytestmark = pytest.mark.gpu


# ---- fs2_loss_fwd ----------------------------------------------------------------------------
def launch_fwd(dev, inp, dtn, weights, off_bytes=0):
    """One fs2_loss_fwd call with null gradient pointers.  The mel operands start ``off_bytes``
    past a 16-byte boundary.  Returns loss_out[8] on the CPU after checking the guard margins."""
    from fastspeech2 import _native as N
    from fastspeech2 import ops
    dt = DTYPES[dtn]
    B, Tm, NM = inp["mel"].shape
    Tp = inp["ld"].shape[1]
    d = N.LossDesc()
    d.B, d.Tm, d.Tp, d.NM, d.dtype = B, Tm, Tp, NM, N.dtype_code(dt)
    keep = []

    def mel_operand(t, dtype):
        off = off_bytes // torch.empty(0, dtype=dtype).element_size()
        whole, view = _guarded(t.numel(), dtype, dev, off)
        view.copy_(t.reshape(-1).to(dev, dtype))
        assert (view.data_ptr() - off_bytes) % 16 == 0
        keep.append(whole)
        return view.data_ptr()

    def plain(t, dtype):
        t = t.to(dev, dtype).contiguous()
        keep.append(t)
        return t.data_ptr()

    d.mel_out, d.postnet_out = mel_operand(inp["mel"], dt), mel_operand(inp["post"], dt)
    d.mel_tgt = mel_operand(inp["tgt"], torch.float32)
    d.log_dur, d.pitch_pred, d.energy_pred = (plain(inp[k], dt) for k in ("ld", "pp", "pe"))
    d.dur_tgt = plain(inp["dur"], torch.int64)
    d.pitch_avg, d.energy_avg = plain(inp["ap"], torch.float32), plain(inp["ae"], torch.float32)
    d.mel_len, d.phon_len = plain(inp["mel_len"], torch.int64), plain(inp["phon_len"], torch.int64)
    (d.w_ssim, d.w_mel, d.w_post, d.w_dur, d.w_pitch, d.w_energy) = weights
    n_ws = int(ops.loss_fwd_ws(B, Tm, NM))
    assert n_ws == VR.fwd_workspace_floats(B, Tm, NM)
    loss_whole, loss = _guarded(8, torch.float32, dev)
    ws_whole, ws = _guarded(n_ws, torch.float32, dev)
    d.loss_out, d.workspace = loss.data_ptr(), ws.data_ptr()
    assert not d.d_mel_out and not d.d_postnet_out and not d.d_log_dur and not d.d_pitch \
        and not d.d_energy
    ops.loss_fwd(d)
    torch.cuda.synchronize()
    assert _intact(loss_whole, 8), "loss: a guard margin was written"
    assert _intact(ws_whole, n_ws), "workspace: a guard margin was written"
    return loss.cpu()


def check_values(ref, loss, what=""):
    """The seven values against the float64 reference under test_gpu_loss.py's rule; returns
    the worst scaled error."""
    tol = max(ref["bound"], VAL_FLOOR)
    errs = [abs(float(loss[i]) - v) / max(1.0, abs(v)) for i, v in enumerate(ref["vals"])]
    print(f"{what}: val_err {max(errs):.3e} tol {tol:.3e}")
    assert np.isfinite(float(loss[7]))
    for i, v in enumerate(ref["vals"]):
        assert np.isfinite(float(loss[i])) or not np.isfinite(v), LR.LOSS_KEYS[i]
        assert errs[i] <= tol, (what, LR.LOSS_KEYS[i], float(loss[i]), v)
    return max(errs)


def _garbage_pads(x):
    L = int(x["mel_len"][1])
    x["mel"][1, L:] = 1e3
    x["post"][1, L:] = 1e3


# case -> (loss_restatement case, variant, edit of the inputs, byte offset of the mel operands)
VARIANTS = {name: (name, "", None, 0) for name in PLAIN}
VARIANTS.update({
    "align_vector": ("align", "", None, 0),
    "align_scalar": ("align", "", None, 4),            # misaligned operands: the scalar MSE arm
    "short_mel": ("short_mel", "", None, 0),           # mel_len < Tp
    "pads_zero": ("pads", "", None, 0),
    "pads_garbage": ("pads", "garbage", _garbage_pads, 0),
})


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(VARIANTS))
def test_loss_fwd_case(cuda, parity_log, case, dtn):
    """Every shape edge of test_gpu_loss.py's PLAIN cases and its misaligned, mel_len < Tp and
    pad-contents variants: values against float64, two calls bit-equal, and the values of
    fs2_loss_fwd_bwd on the same inputs within the same tolerance (bit equality recorded)."""
    name, variant, edit, off = VARIANTS[case]
    ref = reference(name, dtn, variant=variant, edit=edit)
    tol = max(ref["bound"], VAL_FLOOR)
    first = launch_fwd(cuda, ref["inp"], dtn, W_MIXED, off_bytes=off)
    second = launch_fwd(cuda, ref["inp"], dtn, W_MIXED, off_bytes=off)
    full, _ = launch(cuda, ref["inp"], dtn, W_MIXED, off_bytes=off)
    diff = [abs(float(first[i]) - float(full[i])) / max(1.0, abs(v))
            for i, v in enumerate(ref["vals"])]
    bit_equal = same_bits(first[:7], full[:7])
    err = check_values(ref, first, f"loss_fwd_{case}_{dtn}")
    parity_log[f"loss_fwd_{case}_{dtn}"] = {"val_err": err, "val_tol": tol,
                                            "diff_to_fwd_bwd": max(diff),
                                            "bit_equal_to_fwd_bwd": bit_equal}
    print(f"loss_fwd_{case}_{dtn}: diff to fwd_bwd {max(diff):.3e}, bit-equal {bit_equal}")
    assert same_bits(first, second)
    assert max(diff) <= tol
    assert same_bits(first[7:], full[7:])        # element 7, the SSIM gradient scale, as today


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_loss_fwd_ignores_pad_contents(cuda, dtn):
    """NaN in the pads of mel_out and postnet_out changes no bit of the eight outputs."""
    inp = reference("pads", dtn)["inp"]
    L = int(inp["mel_len"][1])
    zero = dict(inp, mel=inp["mel"].clone(), post=inp["post"].clone())
    nan = dict(inp, mel=inp["mel"].clone(), post=inp["post"].clone())
    for x, v in ((zero, 0.0), (nan, float("nan"))):
        x["mel"][1, L:] = v
        x["post"][1, L:] = v
    assert same_bits(launch_fwd(cuda, zero, dtn, W_MIXED), launch_fwd(cuda, nan, dtn, W_MIXED))


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_fused_loss_without_grads_and_eval_loss(cuda, dtn):
    """``fused_loss(need_grads=False)``: no gradients, the values of the check above.
    ``eval_loss`` on the reference's tuples: the seven keys, the same bits."""
    from fastspeech2.loss import LOSS_KEYS, eval_loss, fused_loss
    ref = reference("weights", dtn)
    g = _on(cuda, ref["inp"], DTYPES[dtn])
    loss, grads = fused_loss(g["mel"], g["post"], g["ld"], g["pp"], g["pe"], g["tgt"], g["dur"],
                             g["ap"], g["ae"], g["mel_len"], g["phon_len"], W_MIXED,
                             need_grads=False)
    assert grads is None and loss.shape == (8,) and loss.dtype == torch.float32
    check_values(ref, loss.cpu(), f"fused_loss_no_grads_{dtn}")
    out = eval_loss((g["mel"], g["post"], g["ld"], g["pp"].unsqueeze(-1), g["ap"].unsqueeze(-1),
                     g["pe"].unsqueeze(-1), g["ae"].unsqueeze(-1), g["mel_len"]),
                    (g["tgt"], g["dur"], None, None, g["mel_len"], g["phon_len"]), W_MIXED)
    assert tuple(out) == LOSS_KEYS == LR.LOSS_KEYS
    for i, k in enumerate(LOSS_KEYS):
        assert out[k].shape == () and not out[k].requires_grad
        assert same_bits(out[k].reshape(1).cpu(), loss[i].reshape(1).cpu()), k


# ---- eval_step -------------------------------------------------------------------------------
def _snapshot(tr):
    m = tr.model
    return dict(flat=m._flat.clone(), params={n: p.detach().clone() for n, p in m.named_parameters()},
                exp_avg=tr.opt.exp_avg.clone(), exp_avg_sq=tr.opt.exp_avg_sq.clone(),
                step_count=tr.opt.step_count, seed=tr.seed, graphs=dict(tr._graphs),
                gflat=m._gflat.clone())


def _assert_unchanged(tr, snap):
    m = tr.model
    assert same_bits(m._flat, snap["flat"]) and same_bits(m._gflat, snap["gflat"])
    for n, p in m.named_parameters():
        assert same_bits(p.detach(), snap["params"][n]), n
    assert same_bits(tr.opt.exp_avg, snap["exp_avg"])
    assert same_bits(tr.opt.exp_avg_sq, snap["exp_avg_sq"])
    assert tr.opt.step_count == snap["step_count"] and tr.seed == snap["seed"]
    assert tr._graphs == snap["graphs"]


def test_eval_step_matches_the_eval_mode_oracle_and_leaves_training_alone(cuda, cfg_all):
    """The full-size fp32 model, B = 2, a ragged batch, dropout rates as configured: the loss of
    ``eval_step`` is ``LossOracle`` on the oracle's eval-mode forward within 1e-4 * max(1, |v|)
    (test_gpu_model.py's tolerance for the same comparison), is the same bits twice, and leaves
    parameters, optimizer and seed as they were, before and after a train step; the next train
    step is the bits of a twin trainer's that never evaluated.  The utterances have at most 32
    frames, the length up to which the train step itself is reproducible (see
    test_gpu_fs2_store.py::test_train_one_epoch_equals_steps_by_hand)."""
    from fastspeech2.synthetic import as_tuple, make_batch
    from fastspeech2.train import FusedTrainer
    from oracle.fs2_oracle import LossOracle
    from test_gpu_model import _pair
    kw = cfg_all["model"]["fastspeech2"]
    assert min(kw[k] for k in ("enc_dropout", "dec_dropout", "postnet_dropout",
                               "variance_predictor_dropout")) > 0
    b = make_batch(B=2, tp_min=6, tp_max=12, t_mel_cap=32, seed=7)
    assert int(b["mel_len"].max()) <= 32 and int(b["mel_len"][0]) != int(b["mel_len"][1])
    bt, inten = as_tuple(b)
    o, m = _pair(cfg_all)
    _, twin = _pair(cfg_all)
    with torch.no_grad():
        po = o(bt[0], bt[1], bt[6], bt[4], bt[5], intensity=inten)
        lo = LossOracle(**cfg_all["loss"])(po, (bt[3], bt[6], bt[4], bt[5], bt[7], bt[2]), 0)
    from fastspeech2.loss import Loss
    weights = Loss(**cfg_all["loss"]).weights
    tr = FusedTrainer(m, loss_weights=weights, lr=1e-4, graph=False)
    tr2 = FusedTrainer(twin, loss_weights=weights, lr=1e-4, graph=False)
    g = [t.cuda() for t in bt]
    gi = inten.cuda()
    m.train()
    twin.train()
    for step in range(2):
        snap = _snapshot(tr)
        first = tr.eval_step(g, gi, mel_len_max=g[3].shape[1]).clone()
        second, preds = tr.eval_step(g, gi, return_predictions=True)
        torch.cuda.synchronize()
        assert same_bits(first, second)
        _assert_unchanged(tr, snap)
        assert m.training                                    # eval_step does not switch modes
        assert len(preds) == 8 and preds[0].shape == g[3].shape
        if step == 0:
            for i, k in enumerate(LR.LOSS_KEYS):
                v = float(lo[k])
                print(f"eval_step {k}: got {float(first[i]):.8g} oracle {v:.8g}")
                assert abs(float(first[i]) - v) <= 1e-4 * max(1.0, abs(v)), k
        l1 = tr.step(g, gi, mel_len_max=g[3].shape[1]).clone()
        l2 = tr2.step(g, gi, mel_len_max=g[3].shape[1]).clone()
        torch.cuda.synchronize()
        assert same_bits(l1, l2), step
        assert same_bits(m._flat, twin._flat), step
        assert tr.seed == tr2.seed == step + 1
        assert tr.opt.step_count == tr2.opt.step_count == step + 1


# ---- valid_one_epoch and fit -----------------------------------------------------------------
PHON = [9, 12, 6, 11, 8, 10]
FRAMES = [81, 90, 36, 77, 52, 64]      # 36 to 90: three to six 16-frame SSIM tiles per utterance


@pytest.fixture(scope="module")
def small(cuda, cfg_all):
    """The six-utterance store of test_train_one_epoch_equals_steps_by_hand with 36 to 90 frames
    (lengths at which the TRAIN step is not run-to-run reproducible), its extractor, and the
    2+2-layer model configuration."""
    from fastspeech2.device_store import FS2DeviceStore
    from fastspeech2.intensity import IntensityExtractor
    items = S.random_items(80, FRAMES, PHON, seed=3)
    store = FS2DeviceStore(items, device=cuda)
    torch.manual_seed(4)
    ext = IntensityExtractor(80, 2, 5, 2, 32, 9, 0.1).to(cuda)
    store.cache_intensity(ext)
    kw = dict(cfg_all["model"]["fastspeech2"], enc_num_layers=2, dec_num_layers=2)
    return store, ext, kw


def _trainer(cuda, kw):
    from fastspeech2.model import FastSpeech2
    from fastspeech2.train import FusedTrainer
    torch.manual_seed(0)
    m = FastSpeech2(**kw, n_speakers=4).to(cuda).train()
    return m, FusedTrainer(m, lr=1e-4, graph=False)


def test_valid_one_epoch_equals_eval_steps_by_hand(cuda, small, parity_log):
    """Batches of four over six utterances -- [0..3] and the short [4, 5], equal weights -- are
    the bits of ``eval_step`` by hand on ``store.collate`` outputs; a second epoch gives the same
    bits; the in-batch extractor (``cached=False``) agrees within 1e-3 * max(1, |v|), the
    tolerance test_gpu_fs2_store.py holds the cached intensity to in fp32."""
    from fastspeech2.train import valid_one_epoch
    store, ext, kw = small
    m, tr = _trainer(cuda, kw)
    snap = _snapshot(tr)
    calls = []
    mean = valid_one_epoch(tr, store, 4, ext,
                           on_first_batch=lambda pred, batch: calls.append((pred, batch)))
    assert m.training and len(calls) == 1
    pred, batch = calls[0]
    assert len(pred) == 8 and pred[0].shape == batch[3].shape and batch[3].shape[0] == 4
    by_hand = []
    for idx in ([0, 1, 2, 3], [4, 5]):
        batch, inten = store.collate(idx, intensity=True, extractor=ext)
        by_hand.append(tr.eval_step(batch, inten, mel_len_max=batch[3].shape[1]).clone())
    want = ((by_hand[0] + by_hand[1]) / 2).cpu()
    assert mean.device.type == "cpu" and mean.shape == (8,) and mean.dtype == torch.float32
    assert torch.isfinite(mean).all()
    assert same_bits(mean, want)
    again = valid_one_epoch(tr, store, 4, ext)
    assert same_bits(mean, again)
    _assert_unchanged(tr, snap)
    live = valid_one_epoch(tr, store, 4, ext, cached=False)
    err = [abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(live[:7], mean[:7])]
    parity_log["valid_epoch_cached_vs_in_batch_fp32"] = {"rel": max(err), "tol": 1e-3}
    print(f"valid_one_epoch cached vs in-batch intensity: {max(err):.3e}")
    assert max(err) <= 1e-3
    m.eval()
    valid_one_epoch(tr, store, 4, ext)
    assert not m.training


def test_fit_two_epochs_and_the_best_checkpoint(cuda, small, tmp_path):
    """Two epochs of the 2+2-layer model with the store as both train and valid set: finite
    vectors, and ``best_model.pth`` loaded through ``inference.load_model`` gives the recorded
    validation vector of the best epoch bit for bit."""
    import os
    from fastspeech2.inference import load_model
    from fastspeech2.train import FusedTrainer, fit, valid_one_epoch
    store, ext, kw = small
    m, tr = _trainer(cuda, kw)
    seen = []
    hist = fit(tr, store, store, 2, ext, n_epochs=2, patience=5, max_iterations=10 ** 6,
               exp_path=str(tmp_path), generator=torch.Generator().manual_seed(1),
               on_epoch=lambda e, t, v: seen.append(e))
    assert seen == [0, 1] and hist["stopped"] == "n_epochs"
    assert len(hist["train"]) == len(hist["valid"]) == 2
    for v in hist["train"] + hist["valid"]:
        assert v.shape == (8,) and v.device.type == "cpu" and torch.isfinite(v).all()
    assert tr.seed == 6 and tr.opt.step_count == 6          # three full batches per epoch
    assert hist["best_epoch"] in (0, 1)
    assert hist["best_valid_loss"] == min(float(v[0]) for v in hist["valid"])
    assert sorted(os.listdir(tmp_path)) == ["best_model.pth", "last_model.pth"]
    loaded = load_model(str(tmp_path / "best_model.pth"), kw, [0, 1, 2, 3], cuda)
    got = valid_one_epoch(FusedTrainer(loaded, lr=1e-4, graph=False), store, 2, ext)
    assert same_bits(got, hist["valid"][hist["best_epoch"]])
    last = load_model(str(tmp_path / "last_model.pth"), kw, [0, 1, 2, 3], cuda)
    got = valid_one_epoch(FusedTrainer(last, lr=1e-4, graph=False), store, 2, ext)
    assert same_bits(got, hist["valid"][1])
