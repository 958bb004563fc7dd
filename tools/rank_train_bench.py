"""One rank-model training step at the reference size (parameter.yaml model.rank_model: 6 layers,
hidden 384, 2 heads, k=9; B=8, T=600, dropout 0.1, bf16) on 1 MI355X, random-init weights:

  hip    ``rank_train_step``: ``TrainableRankModel`` forward over the 2B mixed sequences,
         ``RankTrainLoss``, the backward through libfs2_hip.so, ``torch.optim.AdamW``;
  eager  what a user could do before this path existed: the same step written with torch ops
         over a copy of the same parameter containers (``nn.MultiheadAttention``, ``nn.Conv1d``,
         ``nn.LayerNorm`` of ``fastspeech2.intensity``), torch autograd, the same optimiser;
         under ``torch.autocast(bfloat16)`` when the HIP arm runs bf16 activations.

The two are timed as interleaved pairs (A B A B ...) after the warm-up, each step between two
device events; reported are the medians, the median of the per-pair ratios and its range.

    python tools/rank_train_bench.py [--pairs 20] [--warmup 5] [--batch 8] [--frames 600]
Prints one JSON line (and writes it to --out when given).  Reads nothing outside the repository.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))

import torch
import torch.nn.functional as F


def eager_forward(m, emo_X, neu_X, emotions, length, lambdas):
    """rank_model/model.py:138-166 in training mode with torch ops over the containers."""
    ext = m.intensity_extractor
    B, T, _ = emo_X.shape
    lam_i, lam_j = lambdas[0].reshape(B, 1, 1), lambdas[1].reshape(B, 1, 1)
    x = torch.cat([lam_i * emo_X + (1 - lam_i) * neu_X, lam_j * emo_X + (1 - lam_j) * neu_X])
    len2, emo2 = length.repeat(2), emotions.repeat(2)
    pad = torch.arange(T, device=x.device).unsqueeze(0) >= len2.unsqueeze(1)
    h = ext.input_proj(x)
    for layer in ext.fft_block.layers:
        a, _ = layer.self_attn(h, h, h, key_padding_mask=pad, need_weights=False)
        h = layer.norm1(h + layer.dropout(a))
        y = layer.dropout(layer.activation(layer.conv1(h.transpose(1, 2))))
        y = layer.dropout(layer.conv2(y)).transpose(1, 2)
        h = layer.norm2(h + y)
    z = (h + ext.emotion_embedding(emo2).unsqueeze(1)).masked_fill(pad.unsqueeze(-1), 0.0)
    I = ext.classifier(z).float()
    hp = I.sum(dim=1) / len2.unsqueeze(1).float()
    r = m.projector(hp).squeeze(-1)
    return lam_i, lam_j, I[:B], I[B:], hp[:B], hp[B:], r[:B], r[B:]


def eager_loss(pred, targets, alpha, beta):
    """rank_model/loss.py:36-55 with torch ops."""
    lam_i, lam_j, _, _, hi, hj, ri, rj = pred
    y_emo, y_neu = targets
    li, lj = lam_i.reshape(-1), lam_j.reshape(-1)
    mix = (li * F.cross_entropy(hi, y_emo) + (1 - li) * F.cross_entropy(hi, y_neu)
           + lj * F.cross_entropy(hj, y_emo) + (1 - lj) * F.cross_entropy(hj, y_neu)).mean()
    p = torch.sigmoid(ri - rj)
    t = (li - lj + 1) / 2
    rank = -(t * torch.log(p + 1e-8) + (1 - t) * torch.log(1 - p + 1e-8)).mean()
    return alpha * mix + beta * rank, mix, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from fastspeech2 import load_config
    from fastspeech2.rank_train import RankTrainLoss, TrainableRankModel, rank_train_step
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    rc = load_config()["model"]["rank_model"]
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    m = TrainableRankModel(80, rc["n_heads"], 5, rc["n_encoder_layers"], rc["hidden_dim"],
                           rc["kernel_size"], rc["dropout"], act_dtype=dt).cuda().train()
    ref = copy.deepcopy(m).train()
    B, T = a.batch, a.frames
    g = torch.Generator().manual_seed(1)
    length = torch.randint(T // 2, T + 1, (B,), generator=g)
    length[0] = T
    emo_X, neu_X = torch.randn(B, T, 82, generator=g), torch.randn(B, T, 82, generator=g)
    for b in range(B):
        emo_X[b, int(length[b]):] = 0.0
        neu_X[b, int(length[b]):] = 0.0
    batch = dict(emo_X=emo_X.cuda(), neu_X=neu_X.cuda(), length=length.cuda(),
                 emotions=torch.randint(0, 5, (B,), generator=g).cuda(),
                 lambdas=torch.rand(2, B, generator=g).cuda())
    targets = (batch["emotions"], torch.zeros_like(batch["emotions"]))
    crit = RankTrainLoss(0.1, 1.0)
    opt_hip = torch.optim.AdamW(m.parameters(), lr=1e-4)
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-4)

    def hip():
        return rank_train_step(m, crit, opt_hip, batch)[0]

    def eager():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=a.dtype == "bf16"):
            pred = eager_forward(ref, batch["emo_X"], batch["neu_X"], batch["emotions"],
                                 batch["length"], batch["lambdas"])
        loss = eager_loss([t.float() for t in pred], targets, 0.1, 1.0)[0]
        opt_ref.zero_grad()
        loss.backward()
        opt_ref.step()
        return loss.detach()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    eager_error = None
    try:
        for _ in range(a.warmup):
            eager()
        torch.cuda.synchronize()
    except Exception as e:                     # the baseline is optional, the HIP arm is not
        eager_error = f"{type(e).__name__}: {e}"[:200]
    for _ in range(a.warmup):
        l_hip = hip()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.pairs):
        ta.append(timed(hip))
        if eager_error is None:
            tb.append(timed(eager))
    res = {"metric": "rank-model training step (forward, loss, backward, AdamW), ms per step "
                     "between device events",
           "hip_ms_median": statistics.median(ta), "hip_ms_min": min(ta), "pairs": a.pairs,
           "B": B, "T": T, "dtype": a.dtype, "layers": rc["n_encoder_layers"],
           "hidden": rc["hidden_dim"], "dropout": rc["dropout"],
           "hip_loss_after_warmup": l_hip.item(),
           "note": "random-init weights; eager = torch ops and autograd over a copy of the same "
                   "containers" + (", under autocast(bfloat16)" if a.dtype == "bf16" else "")}
    if eager_error is None:
        ratios = [x / y for x, y in zip(ta, tb)]
        res.update(eager_ms_median=statistics.median(tb), eager_ms_min=min(tb),
                   ratio_hip_over_eager_median=statistics.median(ratios),
                   ratio_min=min(ratios), ratio_max=max(ratios))
    else:
        res.update(eager_ms_median=None, eager="not measured", eager_error=eager_error)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
