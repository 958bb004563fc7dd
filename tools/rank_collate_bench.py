"""Rank-model pair collate at the reference size (C = 82, recordings of up to 600 frames, B = 8:
rank_model/parameter.yaml's training batch size and inference.py:55's) on 1 MI355X, synthetic
items, 5 neutral recordings shared among each speaker's lines:

  host    what a user must write without this path: a numpy restatement of ``collate_fn``
          (rank_model/dataset.py:71-115: pad on the host, permute) and ``.to(device)`` of its
          five tensors;
  gpu     ``RankGpuCollate``: two packed uploads of the batch's distinct arrays and descriptors,
          ``fs2_rank_collate`` on the device;
  store   ``RankDeviceStore.collate(indices)``: the set is resident, a batch uploads its indices.

The three are timed as interleaved triples (A B C A B C ...) over a cycle of batches, each call
ended by a device synchronise, items already in host memory (no file reads in any arm).
Reported are the medians, the median and range of the per-triple ratios gpu/host and store/host,
and the kernel's own time between device events.  The outputs of the three arms are compared
bit for bit first.

    python tools/rank_collate_bench.py [--triples 60] [--warmup 5] [--batch 8] [--frames 600]
Prints one JSON line (and writes it to --out when given).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))

import numpy as np
import torch

SPEAKERS = ["spk_a", "spk_b", "spk_c", "spk_d"]
EMOTIONS = ["neutral", "amused", "angry", "disgusted", "sleepy"]
N_NEUTRAL, PER_GROUP = 5, 4


def write_dataset(root, n_mels, t_min, t_max, rng):
    def put(path):
        T = int(rng.integers(t_min, t_max + 1))
        np.savez(path, mel=rng.standard_normal((n_mels, T)).astype(np.float32),
                 pitch=rng.standard_normal(T).astype(np.float32),
                 energy=rng.standard_normal(T).astype(np.float32))

    lines = []
    for spk in SPEAKERS:
        os.makedirs(os.path.join(root, spk))
        for n in range(N_NEUTRAL):
            put(os.path.join(root, spk, f"neutral_{n}.npz"))
        for emo in EMOTIONS[1:]:
            for n in range(PER_GROUP):
                put(os.path.join(root, spk, f"{emo}_{n}.npz"))
                lines.append(f"{spk}|{emo}|{n}|{int(rng.integers(0, N_NEUTRAL))}")
    lines = [lines[i] for i in rng.permutation(len(lines))]
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def host_collate(batch):
    """dataset.py:71-115 restated in numpy: (B, C, max_T) zero-padded, returned permuted."""
    B, C = len(batch), batch[0]["emo_X"].shape[0]
    max_T = max(max(it["emo_X"].shape[1], it["neu_X"].shape[1]) for it in batch)
    emo_X = np.zeros((B, C, max_T), dtype=np.float32)
    neu_X = np.zeros((B, C, max_T), dtype=np.float32)
    length = torch.empty(B, dtype=torch.int64)
    for b, it in enumerate(batch):
        n = min(it["emo_X"].shape[1], it["neu_X"].shape[1])
        emo_X[b, :, :n] = it["emo_X"][:, :n]
        neu_X[b, :, :n] = it["neu_X"][:, :n]
        length[b] = n
    return {"emo_X": torch.from_numpy(emo_X).permute(0, 2, 1),
            "neu_X": torch.from_numpy(neu_X).permute(0, 2, 1),
            "speakers": torch.LongTensor([it["speaker"] for it in batch]),
            "emotions": torch.LongTensor([it["emotion"] for it in batch]),
            "length": length}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from fastspeech2 import load_config, ops
    from fastspeech2.rank_dataset import FineGrainedDataset, RankDeviceStore, RankGpuCollate
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    n_mels = load_config()["audio"]["n_mels"]
    dev = torch.device("cuda")
    B = a.batch
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, n_mels, a.frames // 2, a.frames, np.random.default_rng(0))
        ds = FineGrainedDataset(root, SPEAKERS, EMOTIONS)
        items = [ds[i] for i in range(len(ds))]          # held: shared files are shared objects
        store = RankDeviceStore(ds, device=dev)
    collate = RankGpuCollate(dev)
    n = len(items)
    batches = [list(range(s, s + B)) for s in range(0, n - B + 1, B)]
    keys = ("emo_X", "neu_X", "speakers", "emotions", "length")

    def host(idx):
        return {k: v.to(dev) for k, v in host_collate([items[i] for i in idx]).items()}

    def gpu(idx):
        return collate([items[i] for i in idx])

    def resident(idx):
        return store.collate(idx)

    for idx in batches:                                   # the three arms agree bit for bit
        ra, rb, rc = host(idx), gpu(idx), resident(idx)
        for k in keys:
            assert ra[k].dtype == rb[k].dtype == rc[k].dtype and ra[k].shape == rb[k].shape, k
            assert torch.equal(ra[k], rb[k]) and torch.equal(rb[k], rc[k]), k

    def timed(fn, idx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(idx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for i in range(a.warmup):
        for fn in (host, gpu, resident):
            fn(batches[i % len(batches)])
    ta, tb, tc = [], [], []
    for i in range(a.triples):
        idx = batches[i % len(batches)]
        ta.append(timed(host, idx))
        tb.append(timed(gpu, idx))
        tc.append(timed(resident, idx))
    rb_, rc_ = [y / x for x, y in zip(ta, tb)], [y / x for x, y in zip(ta, tc)]

    # the kernel alone, between device events, on the resident store's descriptors
    idx = batches[0]
    T = int(max(store.table[1, idx].max(), store.table[3, idx].max()))
    desc = store.table_d.index_select(1, torch.tensor(idx, device=dev))
    C = store.n_channels
    emo_X, neu_X = torch.empty(B, T, C, device=dev), torch.empty(B, T, C, device=dev)
    length = torch.empty(B, dtype=torch.int64, device=dev)
    kt = []
    for i in range(a.warmup + a.triples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.rank_collate(store.buffer, desc[0], desc[1], desc[2], desc[3], B, T, C, emo_X, neu_X,
                         length)
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            kt.append(e0.elapsed_time(e1) * 1e3)
    valid = int(length.sum())
    res = {"metric": "rank-model pair collate, ms per batch (host clock around a synchronised "
                     "call; items in host memory)",
           "host_ms_median": statistics.median(ta), "gpu_ms_median": statistics.median(tb),
           "store_ms_median": statistics.median(tc),
           "host_ms_min": min(ta), "gpu_ms_min": min(tb), "store_ms_min": min(tc),
           "ratio_gpu_over_host_median": statistics.median(rb_),
           "ratio_gpu_over_host_min": min(rb_), "ratio_gpu_over_host_max": max(rb_),
           "ratio_store_over_host_median": statistics.median(rc_),
           "ratio_store_over_host_min": min(rc_), "ratio_store_over_host_max": max(rc_),
           "kernel_us_median": statistics.median(kt), "kernel_us_min": min(kt),
           "kernel_batch": {"B": B, "T": T, "C": C, "valid_frames": valid,
                            "bytes_moved": 4 * C * 2 * (valid + B * T)},
           "triples": a.triples, "B": B, "C": C, "frames_max": a.frames, "lines": n,
           "files": store.n_files, "store_bytes": store.nbytes, "batches_in_cycle": len(batches),
           "outputs_bit_identical": True,
           "note": "synthetic items, 5 neutral recordings shared per speaker; the kernel's time "
                   "between device events includes the launch"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
