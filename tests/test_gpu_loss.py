"""fs2_loss_fwd_bwd (csrc/loss.hip) against a float64 reference, per term and per utterance.

Reference: ``loss_restatement.loss_forward`` in float64 on the CPU, fed the kernel's inputs (the
bf16-rounded ones in bf16 mode).  test_loss_host.py pins it to ``LossOracle`` in float32.

Metric: for every gradient tensor and every utterance b,
``err_b = max|got[b] - ref64[b]| / max|ref64[b]|``; an utterance whose reference gradient is
identically zero must be all zeros.  Every utterance has to pass.

Bounds, per case:
  * ``e_ref`` is the largest err_b of the float32 ``LossOracle`` against ref64 over all gradients
    and utterances of the case: the reference's own fp32 noise (its sigma = E[x^2] - mu^2
    cancels).  It never touches the kernels.
  * fp32: ``8 * e_ref``.  The kernel is a second, differently ordered fp32 evaluation (separable
    2 x 11 taps instead of 121, block sums, two float atomics per utterance); its error is
    independent of the oracle's.
  * bf16: ``8 * e_ref + 2^-8`` per rounding of a stored gradient: d_post, d_dur, d_pitch and
    d_energy are rounded to bf16 once, d_mel twice (ssim_apply reads it back and adds), so d_mel
    gets ``8 * e_ref + 2^-7``.  bf16 keeps 8 significant bits, so round-to-nearest is off by up to
    2^-8 of a value just above a power of two (2^-9 only just below one); each rounded value is no
    larger than the utterance's maximum, barring cancellation between the MSE and SSIM parts of
    d_mel.  One allowance of 2^-8 for every tensor proved too tight on the GPU: the once-rounded
    tensors reach 3.5e-3 and d_mel 5.7e-3 (profiles/loss_parity_observed.json); 2^-7 is 1.36
    times that.
  * the seven loss values: ``|got - ref64| <= tol * max(1, |ref64|)`` with tol the larger of
    ``8 * e_ref`` and 64 * 2^-24, in both modes: the values are fp32 sums of fp32 arithmetic on
    the (bf16-rounded) inputs, nothing in them is rounded to bf16.  The floor is the worst case
    of a correct fp32 evaluation of a value: a thread adds up to 32 squared errors serially, the
    wave and block trees add 8 levels, then come the chunk sum, the division, the mean over B,
    the weight and the sum of six terms -- under 64 roundings of 2^-24 each; e_ref, taken from
    gradients, says nothing about these sums and is as small as 1e-7 when the SSIM term is off.

The launcher here fills ``LossDesc`` itself: every output and the workspace lie inside NaN-filled
tensors with 64 elements of margin on each side, the workspace is exactly
``fs2_loss_workspace_floats`` floats, and the margins must still be NaN after the call.

Observed figures go through ``parity_log`` (profiles/loss_parity_observed.json).
"""
import numpy as np
import pytest
import torch

import loss_restatement as LR
from loss_restatement import GRAD_KEYS, W_MIXED

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
MARGIN = 64
VAL_FLOOR = 64 * 2.0 ** -24
W_SSIM_ONLY = (0.7, 0.0, 0.0, 0.0, 0.0, 0.0)


# ---- reference, computed once per (case, dtype, weights, variant) ------------------------------
_REF = {}


def reference(name, dtn, weights=W_MIXED, variant="", edit=None):
    """dict(inp, vals, grads, e_ref, bound): CPU inputs of the case (``edit`` changes them for a
    named ``variant``), the float64 values and gradients, the oracle's fp32 noise and the fp32
    bound 8 * e_ref."""
    key = (name, dtn, weights, variant)
    if key not in _REF:
        inp = LR.make_inputs(name, DTYPES[dtn])
        if edit is not None:
            edit(inp)
        vals, grads = LR.run_restatement(inp, weights, torch.float64)
        _, ograds = LR.run_oracle(inp, weights)
        e_ref = LR.worst_error(ograds, grads)
        _REF[key] = dict(inp=inp, vals=vals, grads=grads, e_ref=e_ref, bound=8.0 * e_ref)
    return _REF[key]


# ---- launcher with guards --------------------------------------------------------------------
def _guarded(n, dtype, dev, off=0):
    whole = torch.full((MARGIN + off + n + MARGIN,), float("nan"), dtype=dtype, device=dev)
    return whole, whole[MARGIN + off:MARGIN + off + n]


def _intact(whole, n, off=0):
    return bool(torch.isnan(whole[:MARGIN + off]).all()) and \
        bool(torch.isnan(whole[MARGIN + off + n:]).all())


def launch(dev, inp, dtn, weights, off_bytes=0):
    """One fs2_loss_fwd_bwd call.  The mel operands (mel_out, postnet_out, mel_tgt, d_mel, d_post)
    start ``off_bytes`` past a 16-byte boundary.  Returns (loss_out[8], five gradients) on the
    CPU after checking every guard margin."""
    from fastspeech2 import _native as N
    from fastspeech2 import ops
    dt = DTYPES[dtn]
    B, Tm, NM = inp["mel"].shape
    Tp = inp["ld"].shape[1]
    d = N.LossDesc()
    d.B, d.Tm, d.Tp, d.NM, d.dtype = B, Tm, Tp, NM, N.dtype_code(dt)
    keep, outs = [], {}

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

    def output(name, n, dtype, off=0):
        whole, view = _guarded(n, dtype, dev, off)
        outs[name] = (whole, view, n, off)
        return view.data_ptr()

    d.mel_out, d.postnet_out = mel_operand(inp["mel"], dt), mel_operand(inp["post"], dt)
    d.mel_tgt = mel_operand(inp["tgt"], torch.float32)
    d.log_dur, d.pitch_pred, d.energy_pred = (plain(inp[k], dt) for k in ("ld", "pp", "pe"))
    d.dur_tgt = plain(inp["dur"], torch.int64)
    d.pitch_avg, d.energy_avg = plain(inp["ap"], torch.float32), plain(inp["ae"], torch.float32)
    d.mel_len, d.phon_len = plain(inp["mel_len"], torch.int64), plain(inp["phon_len"], torch.int64)
    (d.w_ssim, d.w_mel, d.w_post, d.w_dur, d.w_pitch, d.w_energy) = weights
    moff = off_bytes // torch.empty(0, dtype=dt).element_size()
    d.loss_out = output("loss", 8, torch.float32)
    d.d_mel_out = output("mel", B * Tm * NM, dt, moff)
    d.d_postnet_out = output("post", B * Tm * NM, dt, moff)
    d.d_log_dur = output("ld", B * Tp, dt)
    d.d_pitch = output("pp", B * Tp, dt)
    d.d_energy = output("pe", B * Tp, dt)
    assert (d.d_mel_out - off_bytes) % 16 == 0 and (d.d_postnet_out - off_bytes) % 16 == 0
    n_ws = int(ops.loss_ws(B, Tm, NM))
    assert n_ws == LR.workspace_floats(B, Tm, NM)
    d.workspace = output("ws", n_ws, torch.float32)
    assert d.workspace % 256 == 0
    ops.loss_fwd_bwd(d)
    torch.cuda.synchronize()
    for name, (whole, _, n, off) in outs.items():
        assert _intact(whole, n, off), f"{name}: a guard margin was written"
    loss = outs["loss"][1].cpu()
    shapes = dict(mel=(B, Tm, NM), post=(B, Tm, NM), ld=(B, Tp), pp=(B, Tp), pe=(B, Tp))
    grads = [outs[k][1].cpu().reshape(shapes[k]) for k in GRAD_KEYS]
    return loss, grads


def grad_bound(ref, k, dtn):
    """8 * e_ref, plus 2^-8 per bf16 rounding of the stored gradient (d_mel is rounded twice)."""
    if dtn == "fp32":
        return ref["bound"]
    return ref["bound"] + (2.0 ** -7 if k == "mel" else 2.0 ** -8)


def check(parity_log, key, ref, loss, grads, dtn):
    """Values and per-utterance gradients against the reference; records the figures first."""
    tol = max(ref["bound"], VAL_FLOOR)
    bounds = {k: grad_bound(ref, k, dtn) for k in GRAD_KEYS}
    val_err = [abs(float(loss[i]) - v) / max(1.0, abs(v)) for i, v in enumerate(ref["vals"])]
    errs = {k: LR.utterance_errors(g, r) for k, g, r in zip(GRAD_KEYS, grads, ref["grads"])}
    worst = LR.worst_error(grads, ref["grads"])
    once = max(max(errs[k]) for k in GRAD_KEYS[1:])
    parity_log[f"loss_{key}_{dtn}"] = {"e_ref": ref["e_ref"], "bound_d_mel": bounds["mel"],
                                       "bound_others": bounds["post"], "err_d_mel": max(errs["mel"]),
                                       "err_others": once, "val_err": max(val_err), "val_tol": tol}
    print(f"loss_{key}_{dtn}: e_ref {ref['e_ref']:.3e} bounds {bounds['mel']:.3e} "
          f"{bounds['post']:.3e} err {worst:.3e} val_err {max(val_err):.3e} tol {tol:.3e} "
          f"per-utterance {errs}")
    assert np.isfinite(float(loss[7]))
    for i, v in enumerate(ref["vals"]):
        assert np.isfinite(float(loss[i])) or not np.isfinite(v), LR.LOSS_KEYS[i]
        assert val_err[i] <= tol, (LR.LOSS_KEYS[i], float(loss[i]), v)
    for k, e in errs.items():
        for b, eb in enumerate(e):
            assert eb <= bounds[k], (k, b, eb, bounds[k])


def same_bits(a, b):
    """Bit-for-bit equality that treats NaN as a value."""
    a, b = a.contiguous(), b.contiguous()
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


# ---- cases -----------------------------------------------------------------------------------
PLAIN = (["weights"] + [f"width_{n}" for n in (11, 13, 64, 74, 81, 84, 96)]
         + [f"time_{t}" for t in (11, 26, 27, 43)]
         + ["chunk_64x128", "chunk_64x129", "chunk_80x103", "long_len", "single"])


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("name", PLAIN)
def test_loss_case(cuda, parity_log, name, dtn):
    """Unequal weights on every shape edge: n_mels 11 (one SSIM column), 64 / 74 (W or OW divides
    256), 81 / 84 (scalar MSE arm), 96 (LDS maximum); Tm giving 1, 16, 17 and 33 SSIM rows with a
    one-frame utterance; Tm * NM exactly one MSE chunk, one frame more, and a boundary inside a
    frame; mel_len > Tm; B = 1."""
    ref = reference(name, dtn)
    loss, grads = launch(cuda, ref["inp"], dtn, W_MIXED)
    check(parity_log, name, ref, loss, grads, dtn)


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hot", range(6))
def test_one_hot_weights(cuda, parity_log, hot, dtn):
    """One weight at a time: the total is that term, the other terms are zero, only that term's
    predictions get a gradient, and loss_out[7] is -w_ssim / (B * npix).  The SSIM-only run
    compares the SSIM gradient with nothing else in d_mel."""
    w = tuple(1.0 if i == hot else 0.0 for i in range(6))
    mixed = reference("weights", dtn)
    ref = reference("weights", dtn, w)
    loss, grads = launch(cuda, ref["inp"], dtn, w)
    k = hot + 1
    assert float(loss[k]) != 0.0 and float(loss[0]) == float(loss[k])
    for j in range(1, 7):
        if j != k:
            assert float(loss[j]) == 0.0, j
    tol = max(mixed["bound"], VAL_FLOOR)     # same inputs: the fp32 noise of the all-terms run
    for i, v in enumerate(ref["vals"]):
        assert abs(float(loss[i]) - v) <= tol * max(1.0, abs(v)), i
    B, Tm, NM = ref["inp"]["mel"].shape
    npix = (Tm - 10) * (NM - 10)
    assert float(loss[7]) == float(np.float32(-w[0]) / np.float32(B * npix))
    live = {0: "mel", 1: "mel", 2: "post", 3: "ld", 4: "pp", 5: "pe"}[hot]
    for name, g in zip(GRAD_KEYS, grads):
        assert bool(g.any()) == (name == live), name
    if hot == 0:
        check(parity_log, "ssim_only", ref, loss, grads, dtn)


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_misaligned_mel_operands(cuda, parity_log, dtn):
    """Mel operands 4 bytes past a 16-byte boundary: the scalar MSE arm at n_mels = 80.  The same
    per-element arithmetic, so the gradients equal the aligned run bit for bit (Tm = 16: one
    ssim_grad block per utterance, no atomic order); the sums are ordered differently."""
    ref = reference("align", dtn)
    loss0, grads0 = launch(cuda, ref["inp"], dtn, W_MIXED)
    loss1, grads1 = launch(cuda, ref["inp"], dtn, W_MIXED, off_bytes=4)
    for k, a, b in zip(GRAD_KEYS, grads0, grads1):
        assert same_bits(a, b), k
    check(parity_log, "align_vector", ref, loss0, grads0, dtn)
    check(parity_log, "align_scalar", ref, loss1, grads1, dtn)


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_mel_length_below_phoneme_axis(cuda, parity_log, dtn):
    """An utterance of 5 phonemes and 12 frames with Tp = 20: the reference slices pitch and
    energy by the MEL length, so they are averaged over [:12] of the phoneme axis -- indices 5 to
    11, past the utterance's phonemes, carry gradient and indices 12 on do not."""
    ref = reference("short_mel", dtn)
    loss, grads = launch(cuda, ref["inp"], dtn, W_MIXED)
    check(parity_log, "short_mel", ref, loss, grads, dtn)
    for g in grads[3:]:
        assert not g[1, 12:].any()
        assert bool((g[1, 5:12] != 0).all())
    assert not grads[2][1, 5:].any()


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_pad_contents_are_ignored(cuda, parity_log, dtn):
    """Only mel_out has zero pads in the model; postnet_out carries bias-driven values there.
    NaN pads in both change no bit of any output, pad gradients are exactly zero, and finite
    garbage in the pads matches the reference fed the same garbage (it masks it)."""
    ref = reference("pads", dtn)
    inp = ref["inp"]
    L = int(inp["mel_len"][1])

    def with_pads(value):
        def edit(x):
            x["mel"][1, L:] = value
            x["post"][1, L:] = value
        return edit

    zero = dict(inp, mel=inp["mel"].clone(), post=inp["post"].clone())
    with_pads(0.0)(zero)
    nan = dict(inp, mel=inp["mel"].clone(), post=inp["post"].clone())
    with_pads(float("nan"))(nan)
    loss0, grads0 = launch(cuda, zero, dtn, W_MIXED)
    loss1, grads1 = launch(cuda, nan, dtn, W_MIXED)
    assert same_bits(loss0, loss1)
    for k, a, b in zip(GRAD_KEYS, grads0, grads1):
        assert same_bits(a, b), k
    assert not grads1[0][1, L:].any() and not grads1[1][1, L:].any()
    check(parity_log, "pads_zero", ref, *launch(cuda, inp, dtn, W_MIXED), dtn)
    garbage = reference("pads", dtn, variant="garbage", edit=with_pads(1e3))
    loss2, grads2 = launch(cuda, garbage["inp"], dtn, W_MIXED)
    check(parity_log, "pads_garbage", garbage, loss2, grads2, dtn)
    assert not grads2[0][1, L:].any() and not grads2[1][1, L:].any()


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_ssim_clamp_gate(cuda, parity_log, dtn):
    """mel_out = -target: 1 - SSIM exceeds 1, the loss is the constant 1 and the SSIM term has no
    gradient, so d_mel is the MSE gradient alone."""
    ref = reference("anti", dtn)
    loss, grads = launch(cuda, ref["inp"], dtn, W_MIXED)
    assert float(loss[1]) == float(np.float32(W_MIXED[0]))
    assert float(loss[7]) == 0.0
    check(parity_log, "anti", ref, loss, grads, dtn)
    only = reference("anti", dtn, W_SSIM_ONLY)
    loss, grads = launch(cuda, only["inp"], dtn, W_SSIM_ONLY)
    assert float(loss[0]) == float(np.float32(W_SSIM_ONLY[0]))
    for g in grads:
        assert not g.any()


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_tied_extrema(cuda, parity_log, dtn):
    """Predictions clamped to [-6, -2.5], SSIM-only weights so the tie split is all there is in
    d_mel.  Utterance 1 is padded: its maximum is the masked-fill zero and the tie count includes
    every pad element.  Utterance 0 is not: its maximum is -2.5 with many real ties."""
    ref = reference("ties", dtn, W_SSIM_ONLY)
    inp = ref["inp"]
    assert int((inp["mel"][0] == -2.5).sum()) > 100 and int((inp["mel"][0] == -6.0).sum()) > 100
    assert float(inp["mel"][1].max()) == 0.0
    loss, grads = launch(cuda, inp, dtn, W_SSIM_ONLY)
    check(parity_log, "ties", ref, loss, grads, dtn)


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_identity(cuda, parity_log, dtn):
    """Predictions equal to the targets and log_dur = log1p(dur): every loss is within the bound
    of 0.  The reference gradients are rounding noise here (1e-18 in d_mel), so the relative
    metric's e_ref is of order 1e9 and admits anything finite; on top of it the gradients of
    bit-equal operands must be exactly zero, and what is left must be small in absolute terms:
    d_mel is -w_ssim / (B * npix) = 3e-4 times X * (2 V + W), where V and W filter -1 / D2 and
    2 / D2 <= 2 / C2 and cancel to a few roundings of 2^-24: under 1e-6.  In fp32 d_dur is
    cd <= 0.4 times the ulp-level difference of two log1p implementations; in bf16 log_dur is
    rounded, d_dur is a real gradient and is held to 2^-8 plus 8 times the oracle's own error on
    that tensor.

    As first written the kernels missed the relative check on d_mel (3.1e9 against
    8 * e_ref = 2.6e9, e_ref 3.2e8: 3.3e-9 of absolute noise around a reference of 1e-18).
    ssim_map_kernel took a^2 + b^2 + C1 and 2ab + C1 separately, an ulp apart under FMA
    contraction, which is 4e-6 in the luminance derivative where the window means are near
    0.007 (next to the pads); it now forms D1 as L1 + (a - b)^2 and the derivatives of cs from
    one shared lum / D2, as autograd does.  Observed since: 9.7e8."""
    ref = reference("identity", dtn)
    loss, grads = launch(cuda, ref["inp"], dtn, W_MIXED)
    for i in range(7):
        assert abs(float(loss[i]) - ref["vals"][i]) <= VAL_FLOOR, i
    for k in (1, 3, 4):
        assert not grads[k].any(), GRAD_KEYS[k]
    assert float(grads[0].float().abs().max()) <= 1e-6
    if dtn == "fp32":
        assert float(grads[2].abs().max()) <= 1e-6
    else:
        _, ograds = LR.run_oracle(ref["inp"], W_MIXED)
        e_dur = max(LR.utterance_errors(ograds[2], ref["grads"][2]))
        for eb in LR.utterance_errors(grads[2], ref["grads"][2]):
            assert eb <= 8 * e_dur + 2.0 ** -8
    check(parity_log, "identity", ref, loss, grads, dtn)     # the relative metric, last


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_two_runs_agree(cuda, parity_log, dtn):
    """Tm = 129 has nine ssim_grad blocks per utterance, each adding S1 and S2 with one atomicAdd:
    everything not downstream of them is bit-identical between two runs, and d_mel stays within
    the bound both times."""
    ref = reference("chunk_64x129", dtn)
    loss0, grads0 = launch(cuda, ref["inp"], dtn, W_MIXED)
    loss1, grads1 = launch(cuda, ref["inp"], dtn, W_MIXED)
    assert same_bits(loss0, loss1)
    for k, a, b in list(zip(GRAD_KEYS, grads0, grads1))[1:]:
        assert same_bits(a, b), k
    check(parity_log, "rerun_a", ref, loss0, grads0, dtn)
    check(parity_log, "rerun_b", ref, loss1, grads1, dtn)


def _on(dev, inp, dt):
    g = {k: v.to(dev) for k, v in inp.items()}
    for k in GRAD_KEYS:
        g[k] = g[k].to(dt)
    return g


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_fused_loss_product_path(cuda, parity_log, dtn):
    """``fastspeech2.loss.fused_loss`` itself (its own allocation of outputs and workspace)."""
    from fastspeech2.loss import fused_loss
    ref = reference("weights", dtn)
    g = _on(cuda, ref["inp"], DTYPES[dtn])
    loss, grads = fused_loss(g["mel"], g["post"], g["ld"], g["pp"], g["pe"], g["tgt"], g["dur"],
                             g["ap"], g["ae"], g["mel_len"], g["phon_len"], W_MIXED)
    check(parity_log, "fused_loss", ref, loss.cpu(), [x.cpu() for x in grads], dtn)


def test_loss_module_scales_and_shapes(cuda):
    """``Loss``: backward is the upstream gradient times the fused gradients (0.5 is exact, and
    Tm = 27 has two ssim_grad blocks per utterance, whose two atomic adds commute), pitch and
    energy keep their (B, Tp, 1) shape, and only total_loss is differentiable."""
    from fastspeech2.loss import Loss, fused_loss
    inp = reference("weights", "fp32")["inp"]
    g = _on(cuda, inp, torch.float32)
    _, want = fused_loss(g["mel"], g["post"], g["ld"], g["pp"], g["pe"], g["tgt"], g["dur"],
                         g["ap"], g["ae"], g["mel_len"], g["phon_len"], W_MIXED)
    w_ssim, w_mel, w_post, w_dur, w_pitch, w_energy = W_MIXED
    crit = Loss(True, w_ssim, w_dur, w_pitch, w_energy, w_mel, w_post)

    def run():
        lv = {k: g[k].clone().requires_grad_(True) for k in GRAD_KEYS}
        lv["pp"] = g["pp"].unsqueeze(-1).clone().requires_grad_(True)
        lv["pe"] = g["pe"].unsqueeze(-1).clone().requires_grad_(True)
        out = crit((lv["mel"], lv["post"], lv["ld"], lv["pp"], g["ap"].unsqueeze(-1), lv["pe"],
                    g["ae"].unsqueeze(-1), g["mel_len"]),
                   (g["tgt"], g["dur"], None, None, g["mel_len"], g["phon_len"]), 0)
        return lv, out

    lv, out = run()
    assert tuple(out) == LR.LOSS_KEYS
    (0.5 * out["total_loss"]).backward()
    B, Tp = g["ld"].shape
    assert lv["pp"].grad.shape == (B, Tp, 1) and lv["pe"].grad.shape == (B, Tp, 1)
    for k, w in zip(GRAD_KEYS, want):
        assert same_bits(lv[k].grad.reshape(w.shape), 0.5 * w), k
    lv, out = run()
    with pytest.raises(NotImplementedError):
        out["mel_loss"].backward()
