"""Rank-model evaluation path downstream of ``RankModel.forward`` (eval mode): the validation
loss values and the emotion-intensity prototype bank that ``fastspeech2.inference`` reads.

Reference (emo_rank_tts/rank_model/):
* ``RankLoss``   -- loss.py:9-55, as ``train.py::validate_one_epoch`` (:71-112) uses it;
* ``bucketize``  -- inference.py:11-119: eval forward with ``lambdas = ones`` over the train
  split, per (speaker, emotion) the utterances sorted by score ``r``, their valid frames
  concatenated and split into ``bucket_size`` buckets, each bucket's mean a prototype.

Everything runs through libfs2_hip.so (``fs2_rank_loss_fwd``, ``fs2_bucket_means``); there is
no CPU path.  Nothing here carries an autograd graph: rank-model training (dropout, backward,
the differentiable loss) is ``fastspeech2.rank_train``.
"""

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from . import ops


class RankLoss(nn.Module):
    """Values of rank_model/loss.py:9-55, forward only.

    ``forward(predictions, targets)`` takes ``RankModel.forward``'s 8-tuple and
    ``targets = (y_emo, y_neu)`` (int64 class ids, (B,)) and returns ``(loss, L_mixup, L_rank)``
    as 0-d fp32 tensors on the device.  The result carries NO autograd graph: it is for
    validation, not for training.

    As in the reference, ``F.cross_entropy`` is the batch-mean scalar, multiplied by the
    per-sample lambda before the final mean; the rank term is the binary cross entropy of
    ``sigmoid(ri - rj)`` against ``(lam_i - lam_j + 1) / 2`` with ``log(p + 1e-8)``."""

    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha = alpha
        self.beta = beta

    @torch.no_grad()
    def forward(self, predictions, targets):
        y_emo, y_neu = targets
        lam_i, lam_j, _, _, hi, hj, ri, rj = predictions
        if hi.device.type != "cuda":
            raise RuntimeError("RankLoss runs only on the HIP device (libfs2_hip.so); there is "
                               "no CPU path")
        N.load()
        dev = hi.device
        B, E = hi.shape
        f = lambda t, *shape: t.detach().to(device=dev, dtype=torch.float32).reshape(*shape) \
            .contiguous()
        y = lambda t: t.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
        out = torch.zeros(3, dtype=torch.float32, device=dev)
        ops.rank_loss_fwd(f(lam_i, B), f(lam_j, B), f(hi, B, E), f(hj, B, E), f(ri, B), f(rj, B),
                          y(y_emo), y(y_neu), B, E, float(self.alpha), float(self.beta), out)
        return out[0], out[1], out[2]


def bucket_means(frames, utt_len, scores, groups, n_groups, bucket_size):
    """rank_model/inference.py:98-114 for utterances kept in arrival order.

    frames (N_total, E) fp32: the utterances' valid frames one after another; utt_len (U,) int64
    frames per utterance; scores (U,) fp32; groups (U,) int64 group id in [0, n_groups).  All on
    the HIP device.  Returns (n_groups, bucket_size, E) fp32 on the device.

    Within a group the utterances are ordered by score, ascending and stable in arrival order
    (Python's ``list.sort`` on the reference's fp32 scores); the group's concatenated frames are
    split as ``np.array_split`` does and each bucket is averaged (fp64 sums in a fixed order).
    An empty group gives zeros (the reference skips it).  A bucket with no frames (a group of
    fewer frames than buckets) gives NaN, numpy's mean of an empty slice."""
    N.load()
    dev = frames.device
    if dev.type != "cuda":
        raise RuntimeError("bucket_means runs only on the HIP device (libfs2_hip.so)")
    G, K = int(n_groups), int(bucket_size)
    if G < 1 or K < 1:
        raise ValueError("n_groups and bucket_size must be positive")
    frames = frames.to(torch.float32).contiguous()
    E = frames.shape[1]
    i64 = lambda t: t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    utt_len, groups = i64(utt_len), i64(groups)
    scores = scores.to(device=dev, dtype=torch.float32).reshape(-1)
    U = utt_len.numel()
    if scores.numel() != U or groups.numel() != U:
        raise ValueError("utt_len, scores and groups must have one entry per utterance")
    out = torch.empty(G, K, E, dtype=torch.float32, device=dev)
    if U == 0:
        return out.zero_()
    if bool(((groups < 0) | (groups >= G)).any()) or bool((utt_len < 0).any()):
        raise ValueError("group id outside [0, n_groups) or negative utterance length")
    if int(utt_len.sum()) != frames.shape[0]:
        raise ValueError("frames must hold exactly sum(utt_len) rows")
    # order: by group, within a group by score, ties in arrival order (two stable sorts)
    by_score = torch.sort(scores, stable=True).indices
    order = by_score[torch.sort(groups[by_score], stable=True).indices].contiguous()
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    utt_off = torch.cat([zero, torch.cumsum(utt_len, 0)[:-1]]).contiguous()
    cstart = torch.cat([zero, torch.cumsum(utt_len[order], 0)]).contiguous()
    grp_off = torch.cat([zero, torch.cumsum(torch.bincount(groups, minlength=G), 0)]).contiguous()
    if frames.shape[0] == 0:
        frames = torch.zeros(1, max(E, 1), dtype=torch.float32, device=dev)
    ops.bucket_means(frames, order, cstart, utt_off, grp_off, G, K, E, out)
    return out


class PrototypeBank:
    """Device-side storage of rank_model/inference.py:59-89 and the binning of :93-114.

    ``add(I, r, speakers, emotions, length)`` appends each utterance's valid frames
    ``I[i, :length[i]]`` and its score ``r[i]`` under group (speakers[i], emotions[i]);
    ``finalize()`` returns the (n_speakers, n_emotions, bucket_size, n_emotions) fp32 numpy
    array that ``fastspeech2.inference.get_intensity_rep`` reads (see ``bucket_means`` for the
    empty-group and empty-bucket values)."""

    def __init__(self, n_speakers, n_emotions, bucket_size):
        self.n_speakers, self.n_emotions, self.bucket_size = n_speakers, n_emotions, bucket_size
        self._frames, self._len, self._r, self._group = [], [], [], []

    def add(self, I, r, speakers, emotions, length):
        if I.device.type != "cuda":
            raise RuntimeError("PrototypeBank keeps its storage on the HIP device")
        dev = I.device
        B, T, E = I.shape
        if E != self.n_emotions:
            raise ValueError(f"I has {E} classes, the bank {self.n_emotions}")
        length = length.to(device=dev, dtype=torch.int64).reshape(B).clamp(0, T)
        valid = torch.arange(T, device=dev).unsqueeze(0) < length.unsqueeze(1)
        self._frames.append(I.detach().float()[valid])              # (sum length, E), row order
        self._len.append(length)
        self._r.append(r.detach().to(device=dev, dtype=torch.float32).reshape(B))
        spk = speakers.to(device=dev, dtype=torch.int64).reshape(B)
        emo = emotions.to(device=dev, dtype=torch.int64).reshape(B)
        if bool(((spk < 0) | (spk >= self.n_speakers) | (emo < 0) | (emo >= self.n_emotions))
                .any()):
            raise ValueError("speaker or emotion id outside the bank")
        self._group.append(spk * self.n_emotions + emo)

    def finalize(self):
        shape = (self.n_speakers, self.n_emotions, self.bucket_size, self.n_emotions)
        if not self._frames:
            return np.zeros(shape, dtype=np.float32)
        out = bucket_means(torch.cat(self._frames), torch.cat(self._len), torch.cat(self._r),
                           torch.cat(self._group), self.n_speakers * self.n_emotions,
                           self.bucket_size)
        return out.cpu().numpy().reshape(shape)


@torch.no_grad()
def bucketize(model, batches, n_speakers, n_emotions, bucket_size):
    """rank_model/inference.py:62-118: the intensity prototype bank of a trained ``RankModel``.

    ``batches`` is an iterable of the rank collate's dicts (``emo_X``, ``neu_X`` (B, T,
    n_mels+2), ``speakers``, ``emotions``, ``length``), as
    ``fastspeech2.rank_dataset.RankDeviceStore.batches(8)`` yields them; ``model`` is on the HIP device and is
    run in eval mode with ``lambdas = ones`` (the unmixed emotional input).  Returns the
    (n_speakers, n_emotions, bucket_size, n_emotions) fp32 numpy array; ``np.save`` it and pass
    the path (or the array) to ``fastspeech2.inference.get_intensity_rep``.

    The scores depend on each batch's padded length (see ``RankModel.forward``), so the same
    batching as the reference's loader (batch_size=8, unshuffled) reproduces its bank."""
    dev = next(model.parameters()).device
    bank = PrototypeBank(n_speakers, n_emotions, bucket_size)
    was_training = model.training
    model.eval()
    try:
        for batch in batches:
            emo_X, neu_X = batch["emo_X"].to(dev), batch["neu_X"].to(dev)
            emo_ids, length = batch["emotions"].to(dev), batch["length"].to(dev)
            lambdas = torch.ones(2, emo_X.shape[0], device=dev)
            _, _, I, _, _, _, r, _ = model(emo_X, neu_X, emo_ids, length, lambdas)
            bank.add(I, r, batch["speakers"], emo_ids, length)
    finally:
        model.train(was_training)
    return bank.finalize()
