"""Test helper: a plain torch / numpy restatement of the rank-model evaluation path, written
from the description of the algorithm (rank_model/model.py:138-166 in eval mode, loss.py:36-55,
inference.py:62-118), and the loader of tests/golden/rank_ref.npz.

* forward  -- the mixup, ``oracle.intensity_oracle.extractor_forward`` for each mix, pooling over
  all padded frames divided by the length, the bias-free projector;
* loss     -- restated directly in fp32 torch;
* binning  -- float64 numpy.

test_rank_host.py pins this restatement to the reference's own outputs; test_gpu_rank.py uses
it where the golden file has no case (kernel-level shapes).
"""
import os

import numpy as np
import torch

from oracle.intensity_oracle import extractor_forward


def load_golden(golden_dir):
    """(npz, RankModel kwargs, state dict with every layer's keys) of rank_ref.npz."""
    z = np.load(os.path.join(golden_dir, "rank_ref.npz"))
    kw = {k: (v if k == "dropout" else int(v))
          for k, v in zip(z["cfg_keys"].tolist(), z["cfg_vals"].tolist())}
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    # the file leaves out the layers that equal layer 0 (deep copies of one initialised layer)
    first = "intensity_extractor.fft_block.layers.0."
    for i in range(1, kw["n_encoder_layers"]):
        for k in [k for k in sd if k.startswith(first)]:
            sd.setdefault(k.replace(".layers.0.", f".layers.{i}."), sd[k].clone())
    return z, kw, sd


def bank_batches(z):
    """The reference loader's batches of the bank case, each with the model's I, h, r."""
    keys = ("emo_X", "neu_X", "speakers", "emotions", "length", "I", "h", "r")
    return [{k: torch.from_numpy(z[f"bank.b{i}.{k}"]) for k in keys}
            for i in range(int(z["bank.n_batches"]))]


def rank_forward(sd, emo_X, neu_X, emotions, length, lambdas, n_heads, n_layers):
    """Eval forward from a RankModel state dict: (lam_i, lam_j, Ii, Ij, hi, hj, ri, rj)."""
    pre = "intensity_extractor."
    ext = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    wp = sd["projector.weight"].float().reshape(-1)
    lams, Is, hs, rs = [], [], [], []
    for lam in lambdas.float():
        lam = lam.reshape(-1, 1, 1)
        x = lam * emo_X.float() + (1 - lam) * neu_X.float()
        I = extractor_forward(ext, x, length, emotions, n_heads, n_layers)
        h = I.sum(dim=1) / length.reshape(-1, 1).float()     # ALL T frames over the valid count
        lams.append(lam), Is.append(I), hs.append(h), rs.append(h @ wp)
    return (*lams, *Is, *hs, *rs)


def rank_loss(predictions, targets, alpha, beta):
    """(total, L_mixup, L_rank) in fp32: batch-mean cross entropies weighted per sample by the
    lambdas, and the binary cross entropy of sigmoid(ri - rj) against (lam_i - lam_j + 1) / 2
    with 1e-8 inside the logs."""
    lam_i, lam_j, _, _, hi, hj, ri, rj = [t.float().cpu() for t in predictions]
    y_emo, y_neu = [t.long().cpu().reshape(-1) for t in targets]
    li, lj = lam_i.reshape(-1), lam_j.reshape(-1)

    def ce(h, y):
        return (torch.logsumexp(h, dim=1) - h.gather(1, y[:, None])[:, 0]).mean()

    mix = (li * ce(hi, y_emo) + (1 - li) * ce(hi, y_neu)
           + lj * ce(hj, y_emo) + (1 - lj) * ce(hj, y_neu)).mean()
    p = 1 / (1 + torch.exp(-(ri.reshape(-1) - rj.reshape(-1))))
    t = (li - lj + 1) / 2
    rank = -(t * torch.log(p + 1e-8) + (1 - t) * torch.log(1 - p + 1e-8)).mean()
    return alpha * mix + beta * rank, mix, rank


def bucket_means_np(frames, scores, groups, n_groups, bucket_size):
    """frames: list of (T_i, E) arrays in arrival order; scores (U,) fp32; groups (U,) ids.
    Per group: utterances by ascending score (stable), frames concatenated, split into
    bucket_size runs whose lengths differ by at most one (longer runs first), each averaged in
    float64.  Empty group: zeros.  Empty run: NaN.  Returns (n_groups, bucket_size, E) float64."""
    scores = np.asarray(scores, dtype=np.float32)
    groups = np.asarray(groups)
    E = frames[0].shape[1] if len(frames) else 1
    out = np.zeros((n_groups, bucket_size, E), dtype=np.float64)
    for g in range(n_groups):
        members = sorted((i for i in range(len(frames)) if groups[i] == g),
                         key=lambda i: scores[i])
        if not members:
            continue
        cat = np.concatenate([np.asarray(frames[i], dtype=np.float64) for i in members], axis=0)
        q, rem = divmod(len(cat), bucket_size)
        start = 0
        for k in range(bucket_size):
            n = q + (1 if k < rem else 0)
            out[g, k] = cat[start:start + n].sum(axis=0) / n if n else np.nan
            start += n
    return out


def bank_np(batches, n_speakers, n_emotions, bucket_size, I_key="I", r_key="r"):
    """The (n_spk, n_emo, bucket, n_emo) bank from batches that carry I and r."""
    frames, scores, groups = [], [], []
    for b in batches:
        for i in range(len(b["length"])):
            frames.append(np.asarray(b[I_key][i, :int(b["length"][i])]))
            scores.append(float(b[r_key][i]))
            groups.append(int(b["speakers"][i]) * n_emotions + int(b["emotions"][i]))
    out = bucket_means_np(frames, scores, groups, n_speakers * n_emotions, bucket_size)
    return out.reshape(n_speakers, n_emotions, bucket_size, -1)
