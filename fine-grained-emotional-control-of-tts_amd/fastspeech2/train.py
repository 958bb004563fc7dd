"""Train step (emo_rank_tts/fastspeech2/train.py:54-109, 232) and its data-parallel form.

* ``train_step`` is the reference loop body verbatim in structure -- model forward ->
  ``Loss`` -> ``optim.zero_grad()`` -> ``loss['total_loss'].backward()`` -> ``optim.step()``
  (train.py:72-81) -- and works with ``torch.optim.AdamW`` or ``FusedAdamW``.
* ``FusedTrainer`` is the same step without autograd bookkeeping: engine forward, fused loss,
  engine backward into the flat gradient buffer, a bucketed RCCL all-reduce (SUM, averaged in
  the optimizer) launched per bucket as soon as the backward has produced it; the fused AdamW
  of the decoder / mel-linear / PostNet parameters runs on the aux stream during the encoder
  backward (one process: right after the decoder; DP: once their buckets are reduced), the
  rest after the backward (DP: after the last bucket).  One process per GPU, ``torch.distributed`` with the nccl (= RCCL) backend.
* ``valid_one_epoch`` (train.py:112-165) and ``fit`` (train.py:244-264) are the other half of
  the reference's ``train()``: the validation mean over ``FusedTrainer.eval_step`` (eval-mode
  forward + the forward-only loss ``fs2_loss_fwd``), and the epoch loop with early stopping,
  ``last_model.pth`` / ``best_model.pth`` and ``max_iterations``.
"""

import os

import torch
import torch.distributed as dist

from . import ops
from .device_store import epoch_order
from .intensity import get_intensity_representation
from .loss import fused_loss
from .optim import FusedAdamW


def train_step(model, criterion, optim, batch, intensity, epoch=0):
    """train.py:60-81 loop body (intensity given as an input)."""
    (phoneme, spk_ids, phon_len, mel_tgt, pitch_tgt, energy_tgt, duration_tgt, mel_len) = batch[:8]
    predictions = model(phoneme, spk_ids, duration_tgt, pitch_tgt, energy_tgt, intensity=intensity)
    targets = (mel_tgt, duration_tgt, pitch_tgt, energy_tgt, mel_len, phon_len)
    loss = criterion(predictions, targets, epoch)
    optim.zero_grad()
    loss["total_loss"].backward()
    optim.step()
    return predictions, loss


def train_one_epoch(trainer, store, batch_size, extractor, shuffle=True, generator=None,
                    drop_last=False, cached=True):
    """The body of the reference's ``train_one_epoch`` (train.py:60-81) without logging, over a
    ``FS2DeviceStore``: per batch the intensity input, then ``trainer.step``.  ``cached=True``
    takes the intensity from ``store.collate(..., intensity=True)`` (the store's cache, which
    ``store.cache_intensity(extractor)`` must have filled); ``cached=False`` runs
    ``get_intensity_representation`` on every batch as the reference does.  The loss vectors
    are summed on the device and copied back once: returns their mean over the epoch's steps
    (the reference's ``epoch_avg_loss``) as a host tensor.  Under data parallelism (an
    initialised ``torch.distributed``) each rank takes its share of ``epoch_order``; a shuffled
    epoch then needs a ``generator`` seeded alike on every rank."""
    rank, world = 0, 1
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    if world > 1 and shuffle and generator is None:
        raise ValueError("a shuffled epoch under data parallelism needs a generator seeded alike "
                         "on every rank")
    trainer.model.train()
    total, steps = None, 0
    for item in store.batches(batch_size, shuffle=shuffle, generator=generator,
                              drop_last=drop_last, rank=rank, world_size=world,
                              intensity=cached, extractor=extractor if cached else None):
        if cached:
            batch, intensity = item
        else:
            batch, intensity = item, get_intensity_representation(extractor, item)
        loss = trainer.step(batch, intensity, mel_len_max=batch[3].shape[1])
        total = loss.clone() if total is None else total.add_(loss)
        steps += 1
    if total is None:
        raise ValueError("the epoch has no batch")
    return (total / steps).cpu()


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def valid_one_epoch(trainer, store, batch_size, extractor, cached=True, on_first_batch=None):
    """The reference's ``valid_one_epoch`` (train.py:112-165) without logging, over a
    ``FS2DeviceStore``: the store's order, the short last batch kept, per batch the intensity
    input (as in ``train_one_epoch``) and ``trainer.eval_step``.  The model is in ``eval()`` for
    the epoch and gets its previous mode back afterwards, also when a step raises.  The loss
    vectors are summed on the device and copied back once; returns the sum divided by the
    number of batches (every batch weighs the same, the reference's ``/ len(dataloader)``) as a
    host tensor.  Under data parallelism each rank takes its share of ``epoch_order`` and the
    sum and the batch count are all-reduced before the division, so every rank returns the same
    vector.  ``on_first_batch(predictions, batch)`` is called once with the first batch's
    8-tuple of predictions: the place for the reference's sample synthesis and plots."""
    rank, world = _rank_world()
    model = trainer.model
    was_training = model.training
    model.eval()
    total, steps = None, 0
    try:
        for item in store.batches(batch_size, shuffle=False, drop_last=False, rank=rank,
                                  world_size=world, intensity=cached,
                                  extractor=extractor if cached else None):
            if cached:
                batch, intensity = item
            else:
                batch, intensity = item, get_intensity_representation(extractor, item)
            mlm = batch[3].shape[1]
            if steps == 0 and on_first_batch is not None:
                loss, predictions = trainer.eval_step(batch, intensity, mel_len_max=mlm,
                                                      return_predictions=True)
                on_first_batch(predictions, batch)
                del predictions
            else:
                loss = trainer.eval_step(batch, intensity, mel_len_max=mlm)
            total = loss.clone() if total is None else total.add_(loss)
            steps += 1
    finally:
        model.train(was_training)
    if total is None:         # epoch_order gives every rank the same count: all ranks raise alike
        raise ValueError("the epoch has no batch")
    if world == 1:
        return (total / steps).cpu()
    count = torch.tensor([steps], dtype=torch.int64, device=total.device)
    dist.all_reduce(total, op=dist.ReduceOp.SUM)
    dist.all_reduce(count, op=dist.ReduceOp.SUM)
    return (total / count.to(total.dtype)).cpu()


def fit(trainer, train_store, valid_store, batch_size, extractor, n_epochs, patience,
        max_iterations, exp_path=None, generator=None, cached=True, on_epoch=None):
    """The reference's epoch loop (train.py:244-264).  Per epoch: ``train_one_epoch`` with the
    reference loader's flags (shuffled, last short batch dropped), ``last_model.pth`` (:107),
    ``valid_one_epoch``; ``val < best`` (a NaN never improves) resets the patience count and
    writes ``best_model.pth``, anything else increments it and stops the loop at ``patience``;
    then the global step grows by the epoch's train batches and the loop stops at
    ``max_iterations``.  Checkpoints are ``torch.save(model.state_dict())`` into ``exp_path``
    (``inference.load_model`` reads them), written by rank 0 only; without ``exp_path`` nothing
    is written.  ``on_epoch(epoch, train_vec, valid_vec)`` is the logging hook.

    Returns ``dict(train=[...], valid=[...], best_epoch, best_valid_loss, stopped)`` with the
    per-epoch host loss vectors and ``stopped`` one of "patience", "max_iterations", "n_epochs".
    Under data parallelism every rank sees the same validation vector and stops alike."""
    rank, world = _rank_world()
    model = trainer.model
    save = exp_path is not None and rank == 0
    if save:
        os.makedirs(exp_path, exist_ok=True)
    steps_per_epoch = len(epoch_order(len(train_store), batch_size, drop_last=True, rank=rank,
                                      world_size=world))
    hist = {"train": [], "valid": [], "best_epoch": None, "best_valid_loss": float("inf"),
            "stopped": "n_epochs"}
    global_step, stalled = 0, 0
    for epoch in range(n_epochs):
        train_vec = train_one_epoch(trainer, train_store, batch_size, extractor, shuffle=True,
                                    generator=generator, drop_last=True, cached=cached)
        if save:
            torch.save(model.state_dict(), os.path.join(exp_path, "last_model.pth"))
        valid_vec = valid_one_epoch(trainer, valid_store, batch_size, extractor, cached=cached)
        hist["train"].append(train_vec)
        hist["valid"].append(valid_vec)
        if on_epoch is not None:
            on_epoch(epoch, train_vec, valid_vec)
        val = float(valid_vec[0])
        if val < hist["best_valid_loss"]:
            stalled = 0
            hist["best_valid_loss"], hist["best_epoch"] = val, epoch
            if save:
                torch.save(model.state_dict(), os.path.join(exp_path, "best_model.pth"))
        else:
            stalled += 1
            if stalled >= patience:
                hist["stopped"] = "patience"
                break
        global_step += steps_per_epoch
        if global_step >= max_iterations:
            hist["stopped"] = "max_iterations"
            break
    return hist


class GradBucketer:
    """Bucketed all-reduce of a flat gradient buffer, overlapped with the backward.

    ``ranges`` are the model's (tag, start, end) backward groups in completion order; they
    are merged into contiguous buckets of at least ``bucket_bytes``.  ``ready(tag, streams)``
    is called by the backward when a group's gradients are queued; a bucket is reduced (async,
    SUM) once its last group is ready.  The reduction is issued from a communication stream
    that first waits (stream-ordered events, no host sync) on every stream in ``streams`` that
    may still be writing gradients -- the main stream and the weight-gradient side stream --
    so neither the host nor the main stream waits for it.  ``finish()`` makes the current
    stream wait for every outstanding reduction.
    """

    def __init__(self, flat, ranges, bucket_bytes=32 << 20, group=None):
        self.flat, self.group = flat, group
        self.comm = torch.cuda.Stream(flat.device) if flat.is_cuda else None
        self.buckets = []          # [(start, end, last_tag)]
        cur = None
        for tag, s, e in ranges:
            if cur is None:
                cur = [s, e, tag]
            else:
                cur[1], cur[2] = e, tag
            if (cur[1] - cur[0]) * flat.element_size() >= bucket_bytes:
                self.buckets.append(tuple(cur))
                cur = None
        if cur is not None:
            self.buckets.append(tuple(cur))
        self.by_tag = {}
        for i, (_, _, tag) in enumerate(self.buckets):
            self.by_tag.setdefault(tag, []).append(i)
        self.handles = {}          # bucket index -> async all-reduce work
        self.launched = set()
        self.late_end = 0          # set_late(): flat end of the parameters updated early

    def _reduce(self, i, streams):
        s, e, _ = self.buckets[i]
        if self.comm is None:
            self.handles[i] = dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM,
                                              group=self.group, async_op=True)
        else:
            for st in streams or [torch.cuda.current_stream(self.flat.device)]:
                self.comm.wait_stream(st)
            with torch.cuda.stream(self.comm):
                self.handles[i] = dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM,
                                                  group=self.group, async_op=True)
        self.launched.add(i)

    # -- the late parameters' AdamW under DP (FusedTrainer.step): the decoder / mel-linear /
    # PostNet gradients occupy the front of the flat buffer (backward-completion order); once
    # every bucket that holds any of them is reduced, their update may run on the engine's aux
    # stream during the encoder backward, as the one-process step does
    def set_late(self, end):
        self.late_end = int(end)

    def late_launched(self):
        return self.late_end > 0 and all(i in self.launched for i, (s, _, _) in
                                         enumerate(self.buckets) if s < self.late_end)

    def wait_late(self, stream):
        """make ``stream`` wait (stream-ordered) for the all-reduce of every bucket that holds
        late gradients"""
        with torch.cuda.stream(stream):
            for i, (s, _, _) in enumerate(self.buckets):
                if s < self.late_end:
                    self.handles[i].wait()

    def ready(self, tag, streams=None):
        for i in self.by_tag.get(tag, []):
            if i not in self.launched:
                self._reduce(i, streams)

    def finish(self, streams=None):
        for i in range(len(self.buckets)):
            if i not in self.launched:   # groups that never reported (defensive)
                self._reduce(i, streams)
        for h in self.handles.values():
            h.wait()
        if self.comm is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self.comm)
        self.handles, self.launched = {}, set()


# opt-in: measured slower on ROCm 7 / MI355X (bench A/B, profiles/r02_graph_ab.txt: B=32 21.88 ms
# eager vs 22.16 ms graph, B=16 14.02 vs 14.46 ms; GPU-idle time per step 0.63 ms eager vs
# 1.50 ms graph): the replayed multi-stream graph leaves more gaps between kernels than the
# eager launches, whose host issue time (8-12 ms/step) is already below the GPU time
_GRAPH = os.environ.get("FS2_GRAPH", "0") not in ("", "0")


class _StepGraph:
    """One captured forward + loss + backward for a fixed batch shape.

    The graph owns static copies of the batch tensors (refreshed by a device copy per step, so
    a caller may hand in a new batch of the same shape every step), the loss vector it writes,
    and every intermediate (torch's graph-private memory pool).  Launch arguments are frozen at
    capture, so the dropout seed is captured as 0 and each replay first writes the step's seed
    into the kernels' device-resident seed base (``ops.set_dropout_seed``); AdamW, whose bias
    corrections change every step, runs eagerly after the replay."""

    def __init__(self, trainer, batch, intensity, mel_len_max):
        self.static = [t.clone() for t in batch[:8]] + [intensity.clone()]
        self.mel_len_max = mel_len_max
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            # one eager pass on the capture stream: workspaces and lazily built tables exist
            # before capture, as torch.cuda.graphs recommends
            trainer.forward_backward(self.static[:8], self.static[8], mel_len_max, seed=0)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=s):
            self.loss = trainer.forward_backward(self.static[:8], self.static[8], mel_len_max,
                                                 seed=0)
        torch.cuda.synchronize()

    def replay(self, batch, intensity, seed):
        for dst, src in zip(self.static, list(batch[:8]) + [intensity]):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        ops.set_dropout_seed(seed)
        self.graph.replay()
        ops.set_dropout_seed(0)
        return self.loss


class FusedTrainer:
    """One optimiser step of the FastSpeech2 train path on this rank's shard of the batch.

    ``graph=True`` (or FS2_GRAPH=1 on one rank) replays forward + loss + backward as a captured
    HIP graph per batch shape: one host launch instead of ~500 ctypes calls per step.  Off by
    default: measured slower than the eager launches on this stack (see ``_GRAPH``)."""

    def __init__(self, model, loss_weights=(1.0,) * 6, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, bucket_bytes=32 << 20, graph=None):
        self.model = model
        self.eng = model.engine()
        self.opt = FusedAdamW(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.weights = tuple(float(w) for w in loss_weights)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.bucketer = None
        if self.world > 1:
            self.bucketer = GradBucketer(model._gflat, model.group_ranges(), bucket_bytes)
            self.eng.on_grads_ready = self.bucketer.ready
            # the late parameters' AdamW runs inside the backward once their buckets are
            # reduced (engine.dp_late), as the one-process step's does after the decoder
            self.bucketer.set_late(self.eng.late_param_end())
            self.eng.dp_late = (self.bucketer.late_launched, self.bucketer.wait_late)
        self.seed = 0
        # DP steps stay eager: their bucketed all-reduces are issued from the backward hooks,
        # and a captured step would record none of them (its warm-up pass already fired every
        # bucket), so graph replay is refused there rather than silently unreduced
        if graph and self.world > 1:
            raise ValueError("FusedTrainer(graph=True) needs world size 1")
        self.use_graph = (self.world == 1 and _GRAPH) if graph is None else bool(graph)
        self._graphs = {}
        self._torn = False         # a failed split step left the optimizer half-applied

    def _graph_for(self, batch, intensity, mel_len_max):
        key = tuple(tuple(t.shape) for t in batch[:8]) + (tuple(intensity.shape), mel_len_max)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 4:          # shape buckets kept resident
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[key] = _StepGraph(self, batch, intensity, mel_len_max)
        return g

    def forward_backward(self, batch, intensity, mel_len_max=None, seed=None):
        """Forward + fused loss + backward of this rank's shard; the gradients are left in the
        model's flat buffer (with DP on, their bucket all-reduces are queued as the backward
        produces them).  Returns the loss vector."""
        (phoneme, spk_ids, phon_len, mel_tgt, pitch_tgt, energy_tgt, duration_tgt, mel_len) = batch[:8]
        m = self.model
        m._gflat.zero_()
        out, ctx = self.eng.forward(phoneme, spk_ids, duration_tgt, pitch_tgt, energy_tgt,
                                    intensity=intensity, training=True,
                                    seed=self.seed if seed is None else seed,
                                    mel_len_max=mel_len_max if mel_len_max is not None
                                    else mel_tgt.shape[1])
        mel, post, pd, pp, avg_p, pe, avg_e, _ = out
        loss, grads = fused_loss(mel, post, pd, pp.view(pd.shape), pe.view(pd.shape), mel_tgt,
                                 duration_tgt, avg_p.view(pd.shape), avg_e.view(pd.shape), mel_len,
                                 phon_len, self.weights)
        self.eng.backward(ctx, *grads)
        return loss

    def eval_step(self, batch, intensity, mel_len_max=None, return_predictions=False):
        """One validation batch (train.py:118-135): the eval-mode forward (no dropout, seed 0)
        with the targets teacher-forced, then the forward-only fused loss.  Returns the 8-float
        device loss vector, with ``return_predictions`` also the forward's 8-tuple.  Nothing of
        the training state is touched -- the dropout seed, the gradient buffer, the optimizer,
        the parameters, the captured step graphs -- and there is no host sync."""
        (phoneme, spk_ids, phon_len, mel_tgt, pitch_tgt, energy_tgt, duration_tgt, mel_len) = batch[:8]
        with torch.no_grad():
            out, ctx = self.eng.forward(phoneme, spk_ids, duration_tgt, pitch_tgt, energy_tgt,
                                        intensity=intensity, training=False, seed=0,
                                        mel_len_max=mel_len_max if mel_len_max is not None
                                        else mel_tgt.shape[1])
            del ctx             # nothing runs backward: the saved activations go back at once
            mel, post, pd, pp, avg_p, pe, avg_e, _ = out
            loss, _ = fused_loss(mel, post, pd, pp.view(pd.shape), pe.view(pd.shape), mel_tgt,
                                 duration_tgt, avg_p.view(pd.shape), avg_e.view(pd.shape),
                                 mel_len, phon_len, self.weights, need_grads=False)
        return (loss, out) if return_predictions else loss

    def apply(self):
        """Wait for the gradient all-reduce (stream-ordered) and run AdamW with the 1/N mean."""
        if self.bucketer is not None:
            self.bucketer.finish(self.eng.grad_streams())
        self.opt.step(grad_scale=1.0 / self.world)

    def step(self, batch, intensity, mel_len_max=None):
        self.seed += 1
        if self.use_graph:
            if self.world > 1:
                raise RuntimeError("FusedTrainer: graph replay under data parallelism is not "
                                   "supported (the bucket all-reduces are issued from the "
                                   "backward hooks); use the eager step")
            mlm = mel_len_max if mel_len_max is not None else batch[3].shape[1]
            loss = self._graph_for(batch, intensity, mlm).replay(batch, intensity, self.seed)
        else:
            # the AdamW scalars are fixed before the backward, which updates the decoder /
            # PostNet parameters on the aux stream during the encoder backward (under DP once
            # the all-reduce of their gradient buckets is done, GradBucketer.wait_late)
            if self._torn:
                raise RuntimeError("FusedTrainer: an earlier step failed after the decoder / "
                                   "PostNet half of its AdamW update was applied; the optimizer "
                                   "state is inconsistent -- restore it from a checkpoint")
            split = self.opt.fused_images()
            if split:
                scal = self.opt.begin_step(1.0 / self.world)
                self.eng.adam_split = (self.opt, scal)
            try:
                loss = self.forward_backward(batch, intensity, mel_len_max)
            except BaseException:
                if split:
                    if self.eng._adam_late_done:
                        # the late parameters are already updated (aux stream): the step cannot
                        # be undone, and retrying it in place would update them twice
                        self._torn = True
                    else:    # nothing applied: undo the step count, the step may be retried
                        self.opt.step_count -= 1
                    self.eng._adam_late_done = False
                raise
            finally:
                self.eng.adam_split = None
            if split:
                if self.bucketer is not None:
                    self.bucketer.finish(self.eng.grad_streams())
                self.eng.adamw_step_split(self.opt, scal)
                return loss
        self.apply()
        return loss
