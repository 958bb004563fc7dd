"""FastSpeech2 data path with the whole preprocessed set resident on the device: a batch is an
index list, and the frozen IntensityExtractor's input is served from a per-utterance cache.

Reference: emo_rank_tts/fastspeech2/dataset.py (``FastSpeech2Dataset`` :11-58,
``TextMelCollateWithAlignment`` :62-133) and fastspeech2/train.py:16-51,60-81.

``FS2DeviceStore`` reads every ``.npz`` of a ``FastSpeech2Dataset`` once and keeps

* ``buffer``   one fp32 device buffer: per utterance its (n_mels + 2, T_u) channel-major block
  ``cat(mel, pitch, energy)``, blocks back to back (the layout of ``RankDeviceStore.buffer``;
  bases are only 4-byte aligned);
* ``ibuffer``  one int64 device buffer: per utterance its phoneme ids, then its durations;
* ``table`` / ``table_d``  the descriptor table, (7, n) int64 on the host (numpy) and on the
  device, rows ``float offset, frames, int offset, phonemes, speaker, emotion, cache offset``;
* ``text`` / ``audio_path``  the host lists.

``store.collate(indices)`` is ``GpuCollate()([dataset[i] for i in indices])`` bit for bit: the
sort order comes from the host table through the reference's own ``torch.sort`` call, the index
list (already in batch-row order) is the only upload, and one ``fs2_store_collate`` launch
writes every padded tensor.

The intensity cache (``cache_intensity`` / ``collate(..., intensity=True)``) rests on the
R-frame rule.  The extractor's output on an utterance's valid frames depends on the padded
frames that follow it only through the zero-padded convolutions: the padded rows are not zero
after attention and LayerNorm and leak into the valid tail, one ``kernel_size // 2`` per
convolution, ``R = n_layers * 2 * (kernel_size // 2)`` frames in all; attention (padded keys
masked) then spreads the change over the whole utterance.  Beyond R padded frames nothing
changes, and rows of a batch do not see each other.  So an utterance's in-batch value is a
function of its own content and of ``min(T_max - frames, R)``: a value computed once with at
least R padded frames is the in-batch value of every row with ``T_max - frames >= R``, and only
the rows within R frames of the batch's longest go through the extractor, at the batch's own
``T_max``.  (CPU evidence, the reference's extractor at 6 layers / hidden 384 / k = 9, one
utterance of 150 frames: 0 against >= 48 padded frames differ by 0.3 relative; 48 against 300
give the same bits; 47 against 48 still differ in the 7th digit; tests/test_fs2_store_host.py
repeats this with the oracle on a small config.)

There is no CPU path: a non-HIP device is refused.
"""

import numpy as np
import torch

from . import _native as N
from . import ops
from .intensity import phoneme_average

__all__ = ["FS2DeviceStore", "recompute_rows", "epoch_order", "extractor_reach"]

# rows of the descriptor table
F_OFF, FRAMES, I_OFF, PHONEMES, SPEAKER, EMOTION, C_OFF = range(7)


def _hip_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs only on the HIP device (libfs2_hip.so); there is no CPU "
                           "path")
    return dev


def _upload(t, dev):
    return t.pin_memory().to(dev, non_blocking=True)


def extractor_reach(extractor):
    """R = n_layers * 2 * (kernel_size // 2): the frames the extractor's 2 * n_layers zero-padded
    convolutions carry a padded frame's value back into the valid ones."""
    return int(extractor.n_layers) * 2 * (int(extractor.kernel) // 2)


def recompute_rows(frames_sorted, R):
    """The batch rows whose in-batch intensity is not the cached one: those with fewer than R
    padded frames, ``max(frames) - frames[i] < R``.  For R > 0 the longest row is always one."""
    frames = [int(f) for f in frames_sorted]
    Tm = max(frames) if frames else 0
    return [i for i, f in enumerate(frames) if Tm - f < R]


def epoch_order(n, batch_size, shuffle=False, generator=None, drop_last=False, rank=0,
                world_size=1):
    """The index arrays of one epoch's batches, a pure host function.

    ``shuffle=False``: 0, 1, 2, ... in runs of ``batch_size``, the reference loader's order.
    ``shuffle=True`` takes one ``torch.randperm(n, generator=generator)``; it is a uniform shuffle
    but is NOT pinned to the draws of ``DataLoader``'s ``RandomSampler``.  With ``world_size > 1``
    every rank must pass the same generator state: the order is cut to ``n // world_size *
    world_size`` entries and rank r takes every ``world_size``-th of them from the r-th on
    (DistributedSampler's interleaving, cutting the tail where it pads), so the ranks' sets are
    disjoint and of equal size; with ``drop_last`` every rank gets the same number of full
    batches, else the same number of batches with an equally short last one."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside world size {world_size}")
    order = torch.randperm(n, generator=generator).numpy() if shuffle \
        else np.arange(n, dtype=np.int64)
    if world_size > 1:
        order = order[:n // world_size * world_size][rank::world_size]
    out = []
    for start in range(0, len(order), batch_size):
        idx = order[start:start + batch_size]
        if drop_last and idx.size < batch_size:
            break
        out.append(idx)
    return out


# names and dtypes of the tensors ``out=`` supplies, in the 12-tuple's order
_OUT = ("phoneme", "input_lengths", "mel", "pitch", "energy", "duration", "output_lengths",
        "rank_X")


class FS2DeviceStore:
    """Every utterance of a ``FastSpeech2Dataset`` on the device (see the module docstring).

    ``max_bytes``: raise ``ValueError`` before anything is allocated on the device when the two
    packed buffers together would be larger.  Utterances without frames or phonemes, and items
    whose pitch / energy / duration lengths disagree with mel / phoneme, are refused."""

    _CHUNK = 8 << 20      # floats per upload while filling the buffer

    def __init__(self, dataset, device="cuda", max_bytes=None):
        self.device = _hip_device(device, "FS2DeviceStore")
        N.load()
        n = len(dataset)
        farrays, iarrays, ftotal, itotal = [], [], 0, 0
        table = np.empty((7, n), dtype=np.int64)
        self.text, self.audio_path = [], []
        self.n_mels = None
        for i in range(n):
            it = dataset[i]
            mel = it["mel"].float().numpy()
            if mel.ndim != 2:
                raise ValueError(f"utterance {i}: mel of shape {mel.shape}, expected (n_mels, T)")
            if self.n_mels is None:
                self.n_mels = mel.shape[0]
            T = mel.shape[1]
            pitch = it["pitch"].float().numpy().reshape(-1)
            energy = it["energy"].float().numpy().reshape(-1)
            phon = it["phoneme"].long().numpy().reshape(-1)
            dur = it["duration"].long().numpy().reshape(-1)
            if mel.shape[0] != self.n_mels or not 1 <= self.n_mels <= 128:
                raise ValueError(f"utterance {i}: mel of shape {mel.shape}, the set has "
                                 f"{self.n_mels} mel channels (1..128)")
            if T < 1 or phon.size < 1:
                raise ValueError(f"utterance {i}: {T} frames and {phon.size} phonemes; an empty "
                                 "utterance cannot be collated")
            if pitch.size != T or energy.size != T or dur.size != phon.size:
                raise ValueError(f"utterance {i}: pitch {pitch.size} / energy {energy.size} "
                                 f"frames against mel's {T}, {dur.size} durations against "
                                 f"{phon.size} phonemes")
            table[:, i] = (ftotal, T, itotal, phon.size, int(it["speaker"]), int(it["emotion"]),
                           -1)
            farrays.append(np.concatenate([mel.reshape(-1), pitch, energy]))
            iarrays.append(np.concatenate([phon, dur]))
            ftotal += farrays[-1].size
            itotal += iarrays[-1].size
            self.text.append(it["text"])
            self.audio_path.append(it["audio_path"])
        self.nbytes = 4 * ftotal + 8 * itotal
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError(f"the packed store needs {self.nbytes} bytes, max_bytes is "
                             f"{max_bytes}")
        self.table = table
        self.buffer = torch.empty(max(ftotal, 1), dtype=torch.float32, device=self.device)
        start, off = 0, 0
        while start < n:                                # a few utterances per upload
            stop, size = start, 0
            while stop < n and (stop == start or size + farrays[stop].size <= self._CHUNK):
                size += farrays[stop].size
                stop += 1
            self.buffer[off:off + size].copy_(
                torch.from_numpy(np.concatenate(farrays[start:stop])))
            start, off = stop, off + size
        ints = np.concatenate(iarrays) if n else np.zeros(1, dtype=np.int64)
        self.ibuffer = torch.from_numpy(ints).to(self.device)
        self.table_d = torch.from_numpy(table).to(self.device)
        self.cache = None             # (sum of phonemes, E) fp32 once cache_intensity has run
        self.reach = None             # R of the cached extractor
        self._cache_key = None

    def __len__(self):
        return self.table.shape[1]

    # ------------------------------------------------------------------ collate
    def _sorted(self, indices):
        """The batch's utterance indices in batch-row order (the reference's descending
        ``torch.sort`` of the phoneme lengths), Tp and Tm, all from the host table."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError("an empty batch")
        if idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"utterance index out of range for {len(self)} utterances")
        input_lengths, ids_sorted_decreasing = torch.sort(
            torch.LongTensor(self.table[PHONEMES, idx].tolist()), dim=0, descending=True)
        rows = idx[ids_sorted_decreasing.numpy()]
        return rows, int(input_lengths[0]), int(self.table[FRAMES, idx].max())

    def _outputs(self, B, Tp, Tm, E, out):
        dev, NM = self.device, self.n_mels
        spec = [((B, Tp), torch.int64), ((B,), torch.int64), ((B, Tm, NM), torch.float32),
                ((B, Tm), torch.float32), ((B, Tm), torch.float32), ((B, Tp), torch.int64),
                ((B,), torch.int64), ((B, NM + 2, Tm), torch.float32)]
        if E:
            spec.append(((B, Tp, E), torch.float32))
        if out is None:
            return [torch.empty(*shape, dtype=dt, device=dev) for shape, dt in spec]
        out = list(out)
        if len(out) != len(spec):
            raise ValueError(f"out: expected {len(spec)} tensors ({', '.join(_OUT)}"
                             f"{', intensity' if E else ''}), got {len(out)}")
        for t, (shape, dt) in zip(out, spec):
            if tuple(t.shape) != shape or t.dtype != dt or t.device.type != "cuda" \
                    or not t.is_contiguous():
                raise ValueError(f"out: expected a contiguous {dt} device tensor of shape {shape}")
        return out

    def _launch(self, desc, B, Tp, Tm, out, E=0):
        o = self._outputs(B, Tp, Tm, E, out)
        ops.store_collate(self.buffer, self.ibuffer, desc, self.cache if E else None, B, Tp, Tm,
                          self.n_mels, E, o[0], o[5], o[1], o[2], o[3], o[4], o[7], o[6],
                          o[8] if E else None)
        return o

    def collate(self, indices, out=None, intensity=False, extractor=None):
        """The 12-tuple of ``GpuCollate()([dataset[i] for i in indices])``, bit for bit
        (``labels`` / ``wavs`` host lists in sorted order).  The index list, in batch-row order,
        is the only upload; nothing is copied back and nothing synchronises.  Repeated indices
        are legal.  ``out``: the eight device tensors to write into, in the tuple's order
        (phoneme, input_lengths, mel, pitch, energy, duration, output_lengths, rank_X), with
        ``intensity=True`` a ninth (B, Tp, E).

        ``intensity=True`` (after ``cache_intensity(extractor)``) returns ``(batch, intensity)``,
        intensity (B, Tp, E) fp32 = ``get_intensity_representation(extractor, batch)`` up to
        rounding: rows with at least R padded frames take their cached block inside the collate
        kernel, the others (``recompute_rows``) go through ``extractor`` as one sub-batch at the
        batch's own Tm."""
        rows, Tp, Tm = self._sorted(indices)
        B = rows.size
        redo = []
        if intensity:
            self._check_cache(extractor)
            redo = recompute_rows(self.table[FRAMES, rows], self.reach)
        up = _upload(torch.from_numpy(np.concatenate([rows, np.asarray(redo, dtype=np.int64)])),
                     self.device)
        desc = self.table_d.index_select(1, up[:B])
        E = self.cache.shape[1] if intensity else 0
        o = self._launch(desc, B, Tp, Tm, out, E)
        batch = (o[0], desc[SPEAKER], o[1], o[2], o[3], o[4], o[5], o[6],
                 [self.text[i] for i in rows], [self.audio_path[i] for i in rows], o[7],
                 desc[EMOTION])
        if not intensity:
            return batch
        if redo:
            sel = up[B:]
            with torch.no_grad():
                I = extractor(o[7].index_select(0, sel), o[6].index_select(0, sel),
                              desc[EMOTION].index_select(0, sel), layout="BCT")
                o[8].index_copy_(0, sel, phoneme_average(I, o[5].index_select(0, sel),
                                                         o[1].index_select(0, sel)))
        return batch, o[8]

    # ------------------------------------------------------------------ intensity cache
    @staticmethod
    def _extractor_key(extractor):
        return (id(extractor), extractor.act_dtype,
                tuple((p.data_ptr(), p._version) for p in extractor.parameters()))

    def _check_cache(self, extractor):
        if extractor is None:
            raise ValueError("collate(intensity=True) needs extractor=")
        if self.cache is None:
            raise RuntimeError("no intensity cache: call store.cache_intensity(extractor) first")
        if self._extractor_key(extractor) != self._cache_key:
            raise RuntimeError("the intensity cache was computed with other extractor parameters "
                               "(they changed, moved, or this is another extractor): call "
                               "store.cache_intensity(extractor) again")

    def cache_intensity(self, extractor, batch_size=32):
        """Run the frozen extractor once per utterance (eval mode, ``no_grad``) and keep each
        utterance's ``phoneme_average``d (n_phon, E) block in ``cache``.  Utterances go through
        in groups of ``batch_size`` (longest first) padded to ``max(frames in the group) + R``,
        so every row has at least R padded frames.  The extractor's parameter versions are
        recorded; a later ``collate(intensity=True)`` with changed parameters raises."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        R = extractor_reach(extractor)
        E = int(extractor.n_emotions)
        n = len(self)
        table = self.table.copy()
        table[C_OFF] = E * (np.cumsum(table[PHONEMES]) - table[PHONEMES])
        cache = torch.empty(max(int(table[PHONEMES].sum()), 1), E, dtype=torch.float32,
                            device=self.device)
        flat = cache.view(-1)
        by_frames = np.argsort(-table[FRAMES], kind="stable")
        was_training = extractor.training
        extractor.eval()
        try:
            with torch.no_grad():
                for start in range(0, n, batch_size):
                    rows, Tp, Tm = self._sorted(by_frames[start:start + batch_size])
                    B = rows.size
                    desc = self.table_d.index_select(1, _upload(torch.from_numpy(rows),
                                                                self.device))
                    o = self._launch(desc, B, Tp, Tm + R, None)
                    I = extractor(o[7], o[6], desc[EMOTION], layout="BCT")
                    rep = phoneme_average(I, o[5], o[1])
                    for b, u in enumerate(rows):
                        k, c0 = int(table[PHONEMES, u]), int(table[C_OFF, u])
                        flat[c0:c0 + k * E].copy_(rep[b, :k].reshape(-1))
        finally:
            extractor.train(was_training)
        self.table = table
        self.table_d = torch.from_numpy(table).to(self.device)
        self.cache, self.reach = cache, R
        self._cache_key = self._extractor_key(extractor)

    # ------------------------------------------------------------------ epochs
    def batches(self, batch_size, shuffle=False, generator=None, drop_last=False, rank=0,
                world_size=1, intensity=False, extractor=None):
        """Yields what ``collate`` returns for the batches of ``epoch_order``, in that order."""
        for idx in epoch_order(len(self), batch_size, shuffle, generator, drop_last, rank,
                               world_size):
            yield self.collate(idx, intensity=intensity, extractor=extractor)
