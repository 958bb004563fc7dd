"""Test helper: a dtype-generic restatement of ``oracle.fs2_oracle.LossOracle.forward``, the
loss test cases, and the per-utterance error metric.

``LossOracle`` cannot run in float64: it casts its targets with ``.to(torch.float32)`` and
``nn.MSELoss`` refuses the mixed types.  ``loss_forward`` keeps its op order (per-utterance
``mse_loss`` on the same slices, accumulated in utterance order, divided by B, then
``SSIMLoss`` -- which already runs in any float type -- and the weighted sum in the same order)
and casts every float operand to one ``dtype`` instead.  In float32 it is the oracle bit for bit
(test_loss_host.py pins that); in float64 it is the reference of test_gpu_loss.py.

Weights are always in the kernel's order: (ssim, mel, postnet, duration, pitch, energy).
"""
import torch
import torch.nn.functional as F

from oracle.fs2_oracle import LossOracle, SSIMLoss

LOSS_KEYS = ("total_loss", "ssim_loss", "mel_loss", "postnet_mel_loss", "dur_loss",
             "pitch_loss", "energy_loss")
GRAD_KEYS = ("mel", "post", "ld", "pp", "pe")       # the five predictions, in gradient order
W_MIXED = (0.7, 1.3, 0.6, 1.9, 0.8, 1.1)            # ssim, mel, post, dur, pitch, energy
W_ONES = (1.0,) * 6
WIN = 11


def loss_forward(inp, weights, dtype):
    """The seven-entry dict of ``LossOracle.forward`` with every float operand in ``dtype``.
    ``inp``: dict of mel / post (B, Tm, NM), ld / pp / pe / ap / ae (B, Tp), tgt (B, Tm, NM),
    dur (B, Tp) int64, mel_len / phon_len (B,) int64.  The predictions may require grad."""
    c = lambda t: t if t.dtype == dtype else t.to(dtype)
    mel_out, post_out = c(inp["mel"]), c(inp["post"])
    log_dur, pitch, energy = c(inp["ld"]), c(inp["pp"]), c(inp["pe"])
    mel_tgt, pitch_tgt, energy_tgt = c(inp["tgt"]), c(inp["ap"]), c(inp["ae"])
    log_tgt_dur = torch.log1p(inp["dur"].to(dtype))
    mel_len, phon_len = inp["mel_len"], inp["phon_len"]
    w_ssim, w_mel, w_post, w_dur, w_pitch, w_energy = weights
    B = mel_tgt.shape[0]
    for i in range(B):
        L, P = int(mel_len[i]), int(phon_len[i])
        m = F.mse_loss(mel_out[i, :L, :], mel_tgt[i, :L, :])
        pm = F.mse_loss(post_out[i, :L, :], mel_tgt[i, :L, :])
        d = F.mse_loss(log_dur[i, :P], log_tgt_dur[i, :P])
        p = F.mse_loss(pitch[i, :L], pitch_tgt[i, :L])        # phoneme axis, mel length
        e = F.mse_loss(energy[i, :L], energy_tgt[i, :L])
        if i == 0:
            mel_loss, post_loss, dur_loss, pitch_loss, energy_loss = m, pm, d, p, e
        else:
            mel_loss, post_loss = mel_loss + m, post_loss + pm
            dur_loss, pitch_loss, energy_loss = dur_loss + d, pitch_loss + p, energy_loss + e
    ssim_loss = SSIMLoss()(mel_out, mel_tgt, mel_len)
    mel_loss, post_loss = mel_loss / B, post_loss / B
    dur_loss, pitch_loss, energy_loss = dur_loss / B, pitch_loss / B, energy_loss / B
    total = (ssim_loss * w_ssim + mel_loss * w_mel + post_loss * w_post
             + dur_loss * w_dur + pitch_loss * w_pitch + energy_loss * w_energy)
    return {"total_loss": total, "ssim_loss": ssim_loss * w_ssim,
            "mel_loss": mel_loss * w_mel, "postnet_mel_loss": post_loss * w_post,
            "dur_loss": dur_loss * w_dur, "pitch_loss": pitch_loss * w_pitch,
            "energy_loss": energy_loss * w_energy}


def _leaves(inp, dtype):
    out = dict(inp)
    for k in GRAD_KEYS:
        out[k] = inp[k].detach().to(dtype).clone().requires_grad_(True)
    return out


def _finish(out, leaves):
    if out["total_loss"].requires_grad:
        out["total_loss"].backward()
    vals = [float(out[k].detach()) for k in LOSS_KEYS]
    grads = [leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])
             for k in GRAD_KEYS]
    return vals, grads


def run_restatement(inp, weights, dtype):
    """(seven values as python floats, five gradients of total_loss) of the restatement."""
    lv = _leaves(inp, dtype)
    return _finish(loss_forward(lv, weights, dtype), lv)


def run_oracle(inp, weights):
    """The same from the float32 ``LossOracle`` itself."""
    lv = _leaves(inp, torch.float32)
    w_ssim, w_mel, w_post, w_dur, w_pitch, w_energy = weights
    crit = LossOracle(True, w_ssim, w_dur, w_pitch, w_energy, w_mel, w_post)
    out = crit((lv["mel"], lv["post"], lv["ld"], lv["pp"].unsqueeze(-1), lv["ap"].unsqueeze(-1),
                lv["pe"].unsqueeze(-1), lv["ae"].unsqueeze(-1), lv["mel_len"]),
               (lv["tgt"], lv["dur"], None, None, lv["mel_len"], lv["phon_len"]), 0)
    return _finish(out, lv)


def utterance_errors(got, ref):
    """err_b = max|got[b] - ref[b]| / max|ref[b]| for every utterance b (python floats).  An
    utterance whose reference is identically zero must be zero in ``got`` too (-0.0 counts): its
    error is 0.0 then and inf otherwise.  NaN in ``got`` gives NaN, which no bound admits."""
    errs = []
    for b in range(ref.shape[0]):
        g, r = got[b].double().reshape(-1), ref[b].double().reshape(-1)
        top = float(r.abs().max())
        if top == 0.0:
            errs.append(0.0 if torch.equal(g, torch.zeros_like(g)) else float("inf"))
        else:
            d = (g - r).abs()
            errs.append(float("nan") if bool(torch.isnan(d).any()) else float(d.max()) / top)
    return errs


def worst_error(got_grads, ref_grads):
    worst = 0.0
    for g, r in zip(got_grads, ref_grads):
        for e in utterance_errors(g, r):
            if not e <= worst:
                worst = e
    return worst


# ---- cases ------------------------------------------------------------------------------------
# name -> B, Tm, NM, Tp, mel_len and optionally phon (phonemes per utterance) and kind:
#   "anti"     mel_out = -target (SSIM loss clamps at 1)
#   "ties"     predictions clamped to [-6, -2.5]
#   "identity" predictions equal the targets (targets rounded to bf16 so that both dtypes can)
# Durations are mel_len spread over the utterance's phonemes, every one at least 1.
CASES = {
    "weights": dict(B=3, Tm=27, NM=80, Tp=12, mel_len=[27, 20, 12], phon=[12, 9, 7]),
    "time_11": dict(B=3, Tm=11, NM=80, Tp=8, mel_len=[11, 7, 1]),
    "time_26": dict(B=3, Tm=26, NM=80, Tp=8, mel_len=[26, 17, 1]),
    "time_27": dict(B=3, Tm=27, NM=80, Tp=8, mel_len=[27, 18, 1]),
    "time_43": dict(B=3, Tm=43, NM=80, Tp=8, mel_len=[43, 28, 1]),
    "chunk_64x128": dict(B=2, Tm=128, NM=64, Tp=16, mel_len=[128, 100]),
    "chunk_64x129": dict(B=2, Tm=129, NM=64, Tp=16, mel_len=[129, 100]),
    "chunk_80x103": dict(B=2, Tm=103, NM=80, Tp=16, mel_len=[103, 60]),
    "align": dict(B=2, Tm=16, NM=80, Tp=6, mel_len=[16, 9]),
    "short_mel": dict(B=2, Tm=30, NM=80, Tp=20, mel_len=[30, 12], phon=[20, 5]),
    "long_len": dict(B=2, Tm=27, NM=80, Tp=10, mel_len=[32, 20]),
    "pads": dict(B=2, Tm=16, NM=80, Tp=6, mel_len=[16, 9]),
    "anti": dict(B=3, Tm=27, NM=80, Tp=12, mel_len=[27, 20, 12], phon=[12, 9, 7], kind="anti"),
    "anti_small": dict(B=2, Tm=11, NM=11, Tp=6, mel_len=[11, 7], kind="anti"),
    "ties": dict(B=2, Tm=27, NM=80, Tp=10, mel_len=[27, 19], kind="ties"),
    "identity": dict(B=2, Tm=27, NM=80, Tp=10, mel_len=[27, 19], kind="identity"),
    "single": dict(B=1, Tm=27, NM=80, Tp=10, mel_len=[27]),
}
for _nm in (11, 13, 64, 74, 81, 84, 96):
    CASES[f"width_{_nm}"] = dict(B=2, Tm=27, NM=_nm, Tp=10, mel_len=[27, 14])


def case_shapes():
    """Every (B, Tm, NM) the loss tests launch."""
    return sorted({(c["B"], c["Tm"], c["NM"]) for c in CASES.values()})


def make_inputs(name, dtype=torch.float32):
    """CPU float32 inputs of a case, the predictions rounded to ``dtype`` (the kernel's activation
    type): targets randn * 2 - 4 with zeroed pads, mel_out likewise, postnet_out = mel_out + noise
    with its pads left as they fall."""
    c = CASES[name]
    B, Tm, NM, Tp = c["B"], c["Tm"], c["NM"], c["Tp"]
    kind = c.get("kind")
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=gen)
    mel_len = torch.tensor(c["mel_len"], dtype=torch.int64)
    phon = c.get("phon")
    if phon is None:
        phon = [max(1, min(Tp, L) if b == 0 else min(Tp, L) * 3 // 4)
                for b, L in enumerate(c["mel_len"])]
    phon_len = torch.tensor(phon, dtype=torch.int64)
    dur = torch.zeros(B, Tp, dtype=torch.int64)
    for b in range(B):
        L, P = int(mel_len[b]), int(phon_len[b])
        assert 1 <= P <= min(L, Tp)
        dur[b, :P] = L // P
        dur[b, :L % P] += 1
    rows = torch.arange(Tm).view(1, Tm, 1)
    pad = (rows >= mel_len.view(B, 1, 1)).expand(B, Tm, NM)
    tgt = (rn(B, Tm, NM) * 2 - 4)
    if kind == "identity":
        tgt = tgt.bfloat16().float()
    tgt = tgt.masked_fill(pad, 0.0)
    mel = rn(B, Tm, NM) * 2 - 4
    if kind == "ties":
        mel = mel.clamp(-6.0, -2.5)
    post = mel + 0.1 * rn(B, Tm, NM)
    ld, pp, pe, ap, ae = (rn(B, Tp) for _ in range(5))
    if kind == "anti":
        mel = -tgt
    if kind == "identity":
        mel, post = tgt.clone(), tgt.clone()
        ap, ae = ap.bfloat16().float(), ae.bfloat16().float()
        ld, pp, pe = torch.log1p(dur.float()), ap.clone(), ae.clone()
    mel = mel.masked_fill(pad, 0.0)
    mel, post, ld, pp, pe = (t.to(dtype).float() for t in (mel, post, ld, pp, pe))
    return dict(mel=mel, post=post, ld=ld, pp=pp, pe=pe, tgt=tgt, dur=dur, ap=ap, ae=ae,
                mel_len=mel_len, phon_len=phon_len)


# ---- workspace --------------------------------------------------------------------------------
LOSS_CHUNK, MMCH, SSIM_TI = 8192, 16, 16


def carve_extent(B, Tm, NM, base_floats=0):
    """Floats from the workspace start to the end of the last region that the library's carve()
    lays out, for a workspace that starts ``base_floats`` floats past a 16-byte boundary."""
    npix = (Tm - (WIN - 1)) * (NM - (WIN - 1))
    nblk = (Tm - (WIN - 1) + SSIM_TI - 1) // SSIM_TI
    nch = (Tm * NM + LOSS_CHUNK - 1) // LOSS_CHUNK
    w = base_floats
    w += 5 * B              # per_b
    w += 2 * B * nch        # part_mel
    w += 8 * B              # stats
    w += 4 * B * MMCH       # mm_part
    w += 2 * B * MMCH       # cnt_part
    w += 4                  # scal
    w += B * nblk           # ssim_part
    w = (w + 3) // 4 * 4    # dmap starts on a 16-byte boundary
    w += 3 * B * npix       # dmap
    w += B * Tm * NM        # dnmap
    return w - base_floats


def workspace_floats(B, Tm, NM):
    """What a caller must allocate: the regions of carve() plus one whole 16-byte unit for the
    alignment step, whatever the start's phase."""
    npix = (Tm - (WIN - 1)) * (NM - (WIN - 1))
    nblk = (Tm - (WIN - 1) + SSIM_TI - 1) // SSIM_TI
    nch = (Tm * NM + LOSS_CHUNK - 1) // LOSS_CHUNK
    regions = (5 * B + 2 * B * nch + 8 * B + 4 * B * MMCH + 2 * B * MMCH + 4 + B * nblk
               + 3 * B * npix + B * Tm * NM)
    return regions + 4
