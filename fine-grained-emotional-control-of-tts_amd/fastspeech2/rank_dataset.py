"""Rank-model data path: the reference's pair dataset, its collate on the GPU, and a
device-resident store of the whole preprocessed set.

Reference: emo_rank_tts/rank_model/dataset.py
* ``FineGrainedDataset`` -- :8-68: ``{split}.txt`` holds ``speaker|emotion|emo_id|neu_id`` lines;
  an item is the pair ``{speaker}/{emotion}_{emo_id}.npz`` / ``{speaker}/neutral_{neu_id}.npz``,
  each as X = concatenate([mel, pitch[None], energy[None]]), float32 (n_mels + 2, T), with the
  speaker's and the emotion's index.
* ``collate_fn`` -- :71-115: every pair is truncated to the shorter of its two recordings (:93-97)
  and zero-padded to ``max_T``, the maximum over ALL untruncated lengths of the batch (:76-77), so
  ``max_T`` can exceed every ``length[i]``; returned as (B, max_T, n_mels + 2).
  ``RankModel.forward`` sums the classifier bias over all ``max_T`` frames, so ``max_T`` is part
  of the arithmetic and is reproduced exactly.

``RankGpuCollate`` is the drop-in for ``collate_fn``: one packed fp32 upload of the batch's
distinct arrays, one packed int64 upload of the descriptors, then ``fs2_rank_collate`` truncates,
transposes and pads on the device.  ``RankDeviceStore`` uploads every distinct file of a dataset
once; a batch is then its index list, and ``store.batches(...)`` replaces the ``DataLoader`` of
rank_model/train.py:19-43 and rank_model/inference.py:53-89.

The .npz files are read with ``allow_pickle=False`` (string fields are unicode arrays and load
without pickling).  There is no CPU path: a non-HIP device is refused.
"""

import os
import weakref

import numpy as np
import torch

from . import _native as N
from . import ops

__all__ = ["FineGrainedDataset", "RankGpuCollate", "RankDeviceStore", "load_rank_x"]


def load_rank_x(path):
    """``_prepare_X`` (dataset.py:56-68) of one .npz: float32 (n_mels + 2, T), C-contiguous."""
    with np.load(path, allow_pickle=False) as data:
        mel, pitch, energy = data["mel"], data["pitch"], data["energy"]
    X = np.concatenate([mel, pitch.reshape((1, -1)), energy.reshape((1, -1))], axis=0)
    return np.ascontiguousarray(X, dtype=np.float32)


class FineGrainedDataset(torch.utils.data.Dataset):
    """dataset.py:8-68 (same constructor and item dict).

    Lines of one speaker share neutral recordings: while an item that holds a file's array is
    alive, another item naming the same file gets the same (read-only) array object, which is
    how ``RankGpuCollate`` recognises a shared recording within a batch."""

    def __init__(self, preprocessed_path, speakers, emotions, split="train"):
        super().__init__()
        self.split = split
        self.preprocessed_path = preprocessed_path
        self.speakers = speakers
        self.emotions = emotions
        self.emo_audio_id, self.neu_audio_id, self.speaker, self.emotion = [], [], [], []
        with open(os.path.join(preprocessed_path, f"{split}.txt")) as f:
            for line in f.readlines():
                if not line.strip():
                    continue
                speaker, emotion, emo_audio_id, neu_audio_id = line.strip().split("|")
                self.emo_audio_id.append(emo_audio_id)
                self.neu_audio_id.append(neu_audio_id)
                self.speaker.append(speaker)
                self.emotion.append(emotion)
        self._live = weakref.WeakValueDictionary()

    def __len__(self):
        return len(self.emo_audio_id)

    def paths(self, idx):
        """(emotional .npz, neutral .npz) of line ``idx`` (dataset.py:39-41)."""
        base = os.path.join(self.preprocessed_path, self.speaker[idx])
        return (os.path.join(base, f"{self.emotion[idx]}_{self.emo_audio_id[idx]}.npz"),
                os.path.join(base, f"neutral_{self.neu_audio_id[idx]}.npz"))

    def ids(self, idx):
        """(speaker index, emotion index) of line ``idx`` (dataset.py:46-47)."""
        return self.speakers.index(self.speaker[idx]), self.emotions.index(self.emotion[idx])

    def _load(self, path):
        X = self._live.get(path)
        if X is None:
            X = load_rank_x(path)
            X.setflags(write=False)
            self._live[path] = X
        return X

    def __getitem__(self, idx):
        emo_path, neu_path = self.paths(idx)
        speaker_id, emotion_id = self.ids(idx)
        return {"emo_X": self._load(emo_path), "neu_X": self._load(neu_path),
                "speaker": speaker_id, "emotion": emotion_id}


def _hip_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs only on the HIP device (libfs2_hip.so); there is no CPU "
                           "path")
    return dev


def _upload(t, dev):
    return t.pin_memory().to(dev, non_blocking=True)


def _as_item(x):
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"a rank item is (n_mels + 2, T), got shape {x.shape}")
    return x


def _collate_into(store, desc, B, T, C, dev, out):
    """desc (>= 4, B) int64 on the device: rows emo_off, emo_len, neu_off, neu_len."""
    if out is None:
        emo_X = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        neu_X = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        length = torch.empty(B, dtype=torch.int64, device=dev)
    else:
        emo_X, neu_X, length = out
        for t, shape, dt in ((emo_X, (B, T, C), torch.float32), (neu_X, (B, T, C), torch.float32),
                             (length, (B,), torch.int64)):
            if tuple(t.shape) != shape or t.dtype != dt or t.device.type != "cuda" \
                    or not t.is_contiguous():
                raise ValueError(f"out: expected a contiguous {dt} device tensor of shape {shape}")
    if T == 0:
        length.zero_()        # every item is empty: the kernel has nothing to launch
    ops.rank_collate(store, desc[0], desc[1], desc[2], desc[3], B, T, C, emo_X, neu_X, length)
    return emo_X, neu_X, length


class RankGpuCollate:
    """Drop-in for ``collate_fn`` (dataset.py:71-115) producing device tensors: the dict
    ``emo_X``, ``neu_X`` (B, T, n_mels + 2) fp32, ``speakers``, ``emotions``, ``length`` (B,)
    int64, with T the maximum over all untruncated lengths of the batch.

    Two uploads per batch (the packed fp32 items, each distinct array once -- items that hold
    the same ``neu_X`` object, as ``FineGrainedDataset`` returns for a shared file, are packed
    once; the packed int64 descriptors) and one kernel; T comes from the item shapes, nothing is
    copied back.  The collate runs in the calling process on the device: as a ``DataLoader``'s
    ``collate_fn`` it works only with ``num_workers=0``.

    ``out=(emo_X, neu_X, length)`` writes into tensors the caller allocated."""

    def __init__(self, device="cuda"):
        self.device = _hip_device(device, "RankGpuCollate")

    def __call__(self, batch, out=None):
        N.load()
        B = len(batch)
        if B == 0:
            raise ValueError("an empty batch")
        pairs = [(_as_item(it["emo_X"]), _as_item(it["neu_X"])) for it in batch]
        C = pairs[0][0].shape[0]
        packed, where, total = [], {}, 0
        desc = np.empty((6, B), dtype=np.int64)
        for b, pair in enumerate(pairs):
            for k, x in enumerate(pair):
                if x.shape[0] != C:
                    raise ValueError(f"item {b}: {x.shape[0]} channels, the batch has {C}")
                if id(x) not in where:                 # alive in ``pairs``: ids are distinct
                    where[id(x)] = total
                    packed.append(np.ascontiguousarray(x, dtype=np.float32).reshape(-1))
                    total += x.size
                desc[2 * k, b], desc[2 * k + 1, b] = where[id(x)], x.shape[1]
            desc[4, b], desc[5, b] = int(batch[b]["speaker"]), int(batch[b]["emotion"])
        T = int(max(desc[1].max(), desc[3].max()))                         # dataset.py:76-77
        dev = self.device
        flts = torch.from_numpy(np.concatenate(packed)) if total else torch.zeros(1)
        store = _upload(flts, dev)
        desc_d = _upload(torch.from_numpy(desc), dev)
        emo_X, neu_X, length = _collate_into(store, desc_d, B, T, C, dev, out)
        return {"emo_X": emo_X, "neu_X": neu_X, "speakers": desc_d[4], "emotions": desc_d[5],
                "length": length}


class RankDeviceStore:
    """Every distinct .npz a ``FineGrainedDataset`` names, loaded once and packed into one fp32
    device buffer (``buffer``: the (C, T_u) channel-major arrays back to back, in order of first
    use), with the per-line tables ``emo_off, emo_len, neu_off, neu_len, speaker, emotion`` on
    the host (``table``, (6, lines) int64 numpy) and on the device (``table_d``).

    ``max_bytes``: raise ``ValueError`` before anything is allocated on the device when the
    packed buffer would be larger."""

    _CHUNK = 8 << 20      # floats per upload while filling the buffer

    def __init__(self, dataset, device="cuda", max_bytes=None):
        self.device = _hip_device(device, "RankDeviceStore")
        N.load()
        n = len(dataset)
        arrays, where, total = [], {}, 0
        table = np.empty((6, n), dtype=np.int64)
        self.n_channels = None
        for i in range(n):
            for k, path in enumerate(dataset.paths(i)):
                if path not in where:
                    x = load_rank_x(path)
                    if self.n_channels is None:
                        self.n_channels = x.shape[0]
                    if x.shape[0] != self.n_channels:
                        raise ValueError(f"{path}: {x.shape[0]} channels, the set has "
                                         f"{self.n_channels}")
                    where[path] = (total, x.shape[1])
                    arrays.append(x.reshape(-1))
                    total += x.size
                table[2 * k, i], table[2 * k + 1, i] = where[path]
            table[4, i], table[5, i] = dataset.ids(i)
        self.n_files = len(where)
        self.nbytes = 4 * total
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError(f"the packed store needs {self.nbytes} bytes, max_bytes is "
                             f"{max_bytes}")
        self.table = table
        self.buffer = torch.empty(max(total, 1), dtype=torch.float32, device=self.device)
        start, off = 0, 0
        while start < len(arrays):                     # a few files per upload, in packing order
            stop, size = start, 0
            while stop < len(arrays) and (stop == start or size + arrays[stop].size <= self._CHUNK):
                size += arrays[stop].size
                stop += 1
            self.buffer[off:off + size].copy_(torch.from_numpy(np.concatenate(arrays[start:stop])))
            start, off = stop, off + size
        self.table_d = torch.from_numpy(table).to(self.device)

    def __len__(self):
        return self.table.shape[1]

    def collate(self, indices, out=None):
        """The dict of ``RankGpuCollate([dataset[i] for i in indices])``, bit for bit.  The
        index list is the only upload; the descriptors are gathered from the device tables and T
        comes from the host tables."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        B = idx.size
        if B == 0:
            raise ValueError("an empty batch")
        if idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"line index out of range for {len(self)} lines")
        T = int(max(self.table[1, idx].max(), self.table[3, idx].max()))    # dataset.py:76-77
        desc = self.table_d.index_select(1, _upload(torch.from_numpy(idx), self.device))
        emo_X, neu_X, length = _collate_into(self.buffer, desc, B, T, self.n_channels,
                                             self.device, out)
        return {"emo_X": emo_X, "neu_X": neu_X, "speakers": desc[4], "emotions": desc[5],
                "length": length}

    def batches(self, batch_size, shuffle=False, generator=None, drop_last=False):
        """Yields the collated dicts in ``DataLoader`` order.  ``shuffle=False`` is exactly the
        reference loader's order (lines 0, 1, 2, ... in runs of ``batch_size``, the last one
        short unless ``drop_last``).  ``shuffle=True`` takes one
        ``torch.randperm(len, generator=generator)`` per call; it is a uniform shuffle but is
        NOT pinned to the draws of ``DataLoader``'s ``RandomSampler``."""
        n = len(self)
        order = torch.randperm(n, generator=generator).numpy() if shuffle else np.arange(n)
        for start in range(0, n, batch_size):
            idx = order[start:start + batch_size]
            if drop_last and idx.size < batch_size:
                return
            yield self.collate(idx)
