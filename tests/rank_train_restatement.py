"""Test helper: a float64 torch restatement of the rank model's TRAINING forward, written from the
description of the algorithm (rank_model/model.py:8-50 and :138-166 under ``model.train()``,
loss.py:36-55), with an explicit keep mask for each dropout site; gradients come from autograd.
Also a numpy restatement of the two dropout hashes of csrc/fs2_common.h (a copy of its own: the
ones in the existing test files stay where they are) and the loader of
tests/golden/rank_train_ref.npz.

Dropout sites per layer, each ``x * keep / (1 - p)``:
  attn  -- the attention probabilities after the softmax, keep (2B, H, T, T);
  res1  -- the attention block's output before the residual, keep (2B*T, D);
  gelu  -- after the GELU of the FFN, keep (2B*T, 4D);
  res2  -- the conv2 output before the residual, keep (2B*T, D).
The 2B mixed sequences are one batch: the lam_i mixes first, then the lam_j mixes.

test_rank_train_host.py pins this restatement (all-ones masks) to the reference's own training
step; test_gpu_rank_train.py uses it under dropout, with masks built from the engine's recorded
(seed, salts).
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("lam_i", "lam_j", "Ii", "Ij", "hi", "hj", "ri", "rj")
PRE = "intensity_extractor."


def load_golden_train(golden_dir):
    return np.load(os.path.join(golden_dir, "rank_train_ref.npz"))


# ---------------------------------------------------------------------- dropout hashes (numpy)
_M32 = np.uint64(0xffffffff)


def _u(x):
    return np.uint64(x)


def _drop_key(seed, salt):
    h = _u((seed ^ ((salt * 0x9E3779B9) & 0xffffffff)) & 0xffffffff)
    h ^= h >> _u(16)
    h = (h * _u(0x85ebca6b)) & _M32
    h ^= h >> _u(13)
    h = (h * _u(0xc2b2ae35)) & _M32
    h ^= h >> _u(16)
    return int(h) | 1


def keep_np(seed, salt, idx, p):
    """Element dropout (LayerNorm residuals, GELU dropout): element idx is kept iff its 16-bit
    half of the pair hash of idx >> 1 is >= round(p * 65536)."""
    idx = np.asarray(idx).astype(np.uint64)
    if p <= 0:
        return np.ones(idx.shape, dtype=bool)
    pair = idx >> _u(1)
    h = ((pair & _M32) * _u(0x9E3779B1)) & _M32
    h ^= ((pair >> _u(32)) * _u(0x85EBCA77)) & _M32
    h ^= _u(_drop_key(seed, salt))
    h ^= h >> _u(15)
    h = (h * _u(0x2C1B3C6D)) & _M32
    h ^= h >> _u(12)
    h = (h * _u(0x297A2D39)) & _M32
    h ^= h >> _u(15)
    bits = (h >> ((idx & _u(1)) * _u(16))) & _u(0xffff)
    return bits >= _u(int(p * 65536 + 0.5))


def attn_keep_np(seed, salt, rows, keys, p):
    """Attention-probability dropout: rows (R, 1) = (b*H + h)*T + query, keys (1, K)."""
    r, k = np.asarray(rows).astype(np.uint64), np.asarray(keys).astype(np.uint64)
    if p <= 0:
        return np.ones(np.broadcast(r, k).shape, dtype=bool)
    h = ((r * _u(0x9E3779B1)) & _M32) ^ _u(_drop_key(seed, salt))
    h ^= h >> _u(16)
    h = (h * _u(0x7FEB352D)) & _M32
    h ^= h >> _u(15)
    h = (h * _u(0x846CA68B)) & _M32
    h ^= h >> _u(16)
    u = (h + (k >> _u(1)) * _u(0x27D4EB2F)) & _M32
    u ^= u >> _u(15)
    u = ((u & _u(0xffffff)) * _u(0x5BD1E9)) & _M32
    u ^= u >> _u(13)
    bits = (u >> ((k & _u(1)) * _u(16))) & _u(0xffff)
    return bits >= _u(int(p * 65536 + 0.5))


def masks_from(seed, salts, B2, H, T, D, p):
    """The engine's masks of one step: ``salts`` is its per-layer list of
    {"attn", "res1", "gelu", "res2"}.  Index conventions: attention row (b*H + h)*T + q and key;
    row*D + d for the LayerNorm residuals; m*N + n (N = 4D) after the GELU."""
    M = B2 * T
    out = []
    for s in salts:
        rows = np.arange(B2 * H * T)[:, None]
        out.append({
            "attn": torch.from_numpy(attn_keep_np(seed, s["attn"], rows, np.arange(T)[None, :], p)
                                     .reshape(B2, H, T, T)),
            "res1": torch.from_numpy(keep_np(seed, s["res1"], np.arange(M * D), p).reshape(M, D)),
            "gelu": torch.from_numpy(keep_np(seed, s["gelu"], np.arange(M * 4 * D), p)
                                     .reshape(M, 4 * D)),
            "res2": torch.from_numpy(keep_np(seed, s["res2"], np.arange(M * D), p).reshape(M, D)),
        })
    return out


# ---------------------------------------------------------------------- the training forward
def leaf_params(sd, dtype=torch.float64):
    """state dict -> {key: leaf tensor of ``dtype`` that requires grad}"""
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def _conv(x, w, b):
    return F.conv1d(x.transpose(1, 2), w, b, padding=w.shape[-1] // 2).transpose(1, 2)


def train_forward(params, emo_X, neu_X, emotions, length, lambdas, n_heads, n_layers, masks=None,
                  p=0.0):
    """The 8-tuple of the training forward in the dtype of ``params`` (a RankModel state dict of
    tensors, e.g. ``leaf_params``).  ``masks``: per layer {"attn", "res1", "gelu", "res2"} keep
    masks (bool), None = keep everything."""
    g = lambda k: params[PRE + k]
    dt = g("input_proj.weight").dtype
    B, T, _ = emo_X.shape
    B2 = 2 * B
    lam = lambdas.to(dt).reshape(2, B, 1, 1)
    e, n = emo_X.to(dt), neu_X.to(dt)
    x = torch.cat([lam[0] * e + (1 - lam[0]) * n, lam[1] * e + (1 - lam[1]) * n])
    len2, emo2 = length.long().repeat(2), emotions.long().repeat(2)
    pad = torch.arange(T).unsqueeze(0) >= len2.unsqueeze(1)                 # (2B, T)
    drop = lambda t, keep: t if keep is None else t * keep.to(dt).reshape(t.shape) / (1 - p)
    h = x @ g("input_proj.weight").t() + g("input_proj.bias")
    D = h.shape[-1]
    dh = D // n_heads
    for i in range(n_layers):
        q_ = f"fft_block.layers.{i}."
        m = masks[i] if masks is not None else dict(attn=None, res1=None, gelu=None, res2=None)
        qkv = h @ g(q_ + "self_attn.in_proj_weight").t() + g(q_ + "self_attn.in_proj_bias")
        q, k, v = (t.reshape(B2, T, n_heads, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
        pr = drop(torch.softmax(s, dim=-1), m["attn"])
        a = (pr @ v).transpose(1, 2).reshape(B2, T, D)
        a = a @ g(q_ + "self_attn.out_proj.weight").t() + g(q_ + "self_attn.out_proj.bias")
        h = F.layer_norm(h + drop(a, m["res1"]), (D,), g(q_ + "norm1.weight"),
                         g(q_ + "norm1.bias"), 1e-5)
        y = drop(F.gelu(_conv(h, g(q_ + "conv1.weight"), g(q_ + "conv1.bias"))), m["gelu"])
        y = drop(_conv(y, g(q_ + "conv2.weight"), g(q_ + "conv2.bias")), m["res2"])
        h = F.layer_norm(h + y, (D,), g(q_ + "norm2.weight"), g(q_ + "norm2.bias"), 1e-5)
    z = (h + g("emotion_embedding.weight")[emo2].unsqueeze(1)).masked_fill(pad.unsqueeze(-1), 0.0)
    I = z @ g("classifier.weight").t() + g("classifier.bias")
    hp = I.sum(dim=1) / len2.reshape(-1, 1).to(dt)          # ALL T frames over the valid count
    r = hp @ params["projector.weight"].reshape(-1)
    return (lam[0].reshape(B, 1, 1), lam[1].reshape(B, 1, 1), I[:B], I[B:], hp[:B], hp[B:],
            r[:B], r[B:])


def rank_loss(predictions, targets, alpha, beta):
    """(total, L_mixup, L_rank) in the predictions' dtype, differentiable: rank_restatement's
    ``rank_loss`` without its fp32 cast and with ``torch.sigmoid``, the reference's own op
    (loss.py:49).  The values are the same; the backward differs where fp32 saturates: autograd
    of 1 / (1 + exp(-x)) gives p^2 exp(-x), which is 1.4e-11 at x = 25, while torch.sigmoid's
    backward p (1 - p) is exactly 0 there -- and that is what the reference computes."""
    lam_i, lam_j, _, _, hi, hj, ri, rj = predictions
    y_emo, y_neu = [t.long().reshape(-1) for t in targets]
    li, lj = lam_i.reshape(-1), lam_j.reshape(-1)

    def ce(h, y):
        return (torch.logsumexp(h, dim=1) - h.gather(1, y[:, None])[:, 0]).mean()

    mix = (li * ce(hi, y_emo) + (1 - li) * ce(hi, y_neu)
           + lj * ce(hj, y_emo) + (1 - lj) * ce(hj, y_neu)).mean()
    pij = torch.sigmoid(ri.reshape(-1) - rj.reshape(-1))
    t = (li - lj + 1) / 2
    rank = -(t * torch.log(pij + 1e-8) + (1 - t) * torch.log(1 - pij + 1e-8)).mean()
    return alpha * mix + beta * rank, mix, rank


def train_step_grads(sd, inp, alpha, beta, n_heads, n_layers, masks=None, p=0.0,
                     dtype=torch.float64):
    """One forward + backward: (8-tuple, three losses, {key: gradient}) in ``dtype``."""
    params = leaf_params(sd, dtype)
    pred = train_forward(params, inp["emo_X"], inp["neu_X"], inp["emotions"], inp["length"],
                         inp["lambdas"], n_heads, n_layers, masks, p)
    emo = inp["emotions"].long()
    losses = rank_loss(pred, (emo, torch.zeros_like(emo)), alpha, beta)
    losses[0].backward()
    return ([t.detach() for t in pred], [l.detach() for l in losses],
            {k: v.grad for k, v in params.items()})
