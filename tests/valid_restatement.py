"""Test helper for the validation path: the forward-only loss workspace restated from
``loss_restatement``, a pure-Python model of ``fastspeech2.train.fit``'s epoch loop, and the
scripted fake trainer / store the host tests drive ``valid_one_epoch`` and ``fit`` with.
"""
import torch

import loss_restatement as LR


# ---- workspace --------------------------------------------------------------------------------
def grad_regions(B, Tm, NM):
    """Floats of the two regions only the gradient pass uses: dmap [3][B][npix], dnmap
    [B][Tm][NM]."""
    npix = (Tm - (LR.WIN - 1)) * (NM - (LR.WIN - 1))
    return 3 * B * npix + B * Tm * NM


def fwd_workspace_floats(B, Tm, NM):
    """fs2_loss_fwd_workspace_floats: ``loss_restatement.workspace_floats`` without dmap and
    dnmap, with the same 16-byte unit of slack."""
    return LR.workspace_floats(B, Tm, NM) - grad_regions(B, Tm, NM)


def fwd_carve_extent(B, Tm, NM):
    """Floats the forward-only carve can touch: every region of ``carve_extent`` up to
    ssim_part, no alignment step after it."""
    nblk = (Tm - (LR.WIN - 1) + LR.SSIM_TI - 1) // LR.SSIM_TI
    nch = (Tm * NM + LR.LOSS_CHUNK - 1) // LR.LOSS_CHUNK
    return 5 * B + 2 * B * nch + 8 * B + 4 * B * LR.MMCH + 2 * B * LR.MMCH + 4 + B * nblk


# ---- the fit loop -----------------------------------------------------------------------------
def fit_model(valid_losses, n_epochs, patience, max_iterations, steps_per_epoch):
    """train.py:244-264 on a list of validation losses (one per epoch, in order).  Returns
    (epochs run, best_epoch, best_valid_loss, stopped, epochs at which best_model is written)."""
    best, best_epoch, stalled, global_step = float("inf"), None, 0, 0
    stopped, ran, saved = "n_epochs", 0, []
    for epoch in range(n_epochs):
        val = valid_losses[epoch]
        ran += 1
        if val < best:
            stalled, best, best_epoch = 0, val, epoch
            saved.append(epoch)
        else:
            stalled += 1
            if stalled >= patience:
                stopped = "patience"
                break
        global_step += steps_per_epoch
        if global_step >= max_iterations:
            stopped = "max_iterations"
            break
    return ran, best_epoch, best, stopped, saved


# ---- fakes ------------------------------------------------------------------------------------
class FakeModel(torch.nn.Module):
    """One parameter, so that a checkpoint tells which epoch wrote it."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))


class FakeStore:
    """``len`` and ``batches`` of ``FS2DeviceStore`` on the host: a batch is a tuple whose
    element 3 has the frame axis ``train_one_epoch`` / ``valid_one_epoch`` read, and whose
    element 0 holds the utterance indices.  Records every ``batches`` call."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def batches(self, batch_size, shuffle=False, generator=None, drop_last=False, rank=0,
                world_size=1, intensity=False, extractor=None):
        from fastspeech2.device_store import epoch_order
        self.calls.append(dict(batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                               rank=rank, world_size=world_size, intensity=intensity,
                               extractor=extractor))
        for idx in epoch_order(self.n, batch_size, shuffle, generator, drop_last, rank,
                               world_size):
            ids = torch.as_tensor(idx, dtype=torch.int64)
            batch = (ids, None, None, torch.zeros(len(ids), 7, 2)) + (None,) * 8
            inten = torch.zeros(len(ids), 1, 5)
            yield (batch, inten) if intensity else batch


def batch_vector(ids):
    """The fake loss vector of a batch: distinct for every set of utterances, and not
    proportional to the batch size (a mean weighted by size would differ)."""
    ids = [int(i) for i in ids]
    v = torch.arange(8, dtype=torch.float32) * 0.125
    return v + float(sum((i + 1) ** 2 for i in ids)) + 0.5 * len(ids)


class FakeTrainer:
    """``step`` / ``eval_step`` of ``FusedTrainer`` with scripted results.  ``valid_script`` is
    the total validation loss per epoch (every batch of an epoch returns it, so the epoch mean
    is that number); without it ``eval_step`` returns ``batch_vector``.  A train step adds 1 to
    the model's parameter; ``raise_at`` makes the n-th ``eval_step`` raise."""

    def __init__(self, valid_script=None, raise_at=None):
        self.model = FakeModel()
        self.valid_script, self.raise_at = valid_script, raise_at
        self.seen, self.modes, self.steps, self.epoch, self.evals = [], [], 0, -1, 0
        self._stepped = True

    def step(self, batch, intensity, mel_len_max=None):
        assert self.model.training
        with torch.no_grad():
            self.model.w.add_(1.0)
        self.steps += 1
        self._stepped = True
        return torch.full((8,), float(self.steps))

    def eval_step(self, batch, intensity, mel_len_max=None, return_predictions=False):
        if self._stepped:                           # first evaluation after training: next epoch
            self.epoch, self._stepped = self.epoch + 1, False
        self.evals += 1
        if self.raise_at is not None and self.evals == self.raise_at:
            raise RuntimeError("scripted failure")
        self.modes.append(self.model.training)
        self.seen.append([int(i) for i in batch[0]])
        assert mel_len_max == batch[3].shape[1]
        if self.valid_script is not None:
            loss = torch.zeros(8)
            loss[0] = self.valid_script[self.epoch]
        else:
            loss = batch_vector(batch[0])
        preds = tuple(f"prediction{i}" for i in range(8))
        return (loss, preds) if return_predictions else loss
