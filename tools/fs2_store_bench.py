"""FastSpeech2 batch assembly and intensity input at the reference size (n_mels 80, B = 32,
100-200 phonemes of 1-9 frames each, the reference extractor: parameter.yaml model.rank_model)
on 1 MI355X, a seeded synthetic set written as the reference's preprocessed files:

  a  host    ``GpuCollate`` on host item dicts (items already in host memory: no file reads)
             + ``get_intensity_representation`` (the extractor on all B rows);
  b  store   ``FS2DeviceStore.collate(indices)`` + ``get_intensity_representation``;
  c  cached  ``FS2DeviceStore.collate(indices, intensity=True)``: the cached blocks gathered
             in the collate kernel, the extractor only on the rows within R frames of the
             batch's longest.

The three are timed as interleaved triples (a b c a b c ...) over a cycle of batches, each arm
ended by a device synchronise.  First the 12-tuples of a and b are compared bit for bit and arm
c's intensity against arm b's (relative error, max |c - b| / max |b| per batch).  Reported: the
medians, the median and range of the per-triple ratios b/a, c/b and c/a, the rows recomputed
per batch, and the store kernel's own time (with the cache gather) between device events.
Not measured: reading the .npz files, ``DataLoader`` workers, more than one GPU.

    python tools/fs2_store_bench.py [--triples 60] [--warmup 5] [--batch 32] [--utterances 256]
                                    [--dtype bfloat16|float32] [--out FILE]
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
EMOTIONS = ["Neutral", "Angry", "Happy", "Sad", "Surprise"]
TENSORS = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11)       # the 12-tuple's device tensors


def write_dataset(root, n, n_mels, rng, tokens):
    paths = []
    for i in range(n):
        tp = int(rng.integers(100, 201))
        dur = rng.integers(1, 10, tp)
        T = int(dur.sum())
        path = os.path.join(root, f"utt_{i}.npz")
        np.savez(path, mel=rng.standard_normal((n_mels, T)).astype(np.float32),
                 pitch=rng.standard_normal(T).astype(np.float32),
                 energy=rng.standard_normal(T).astype(np.float32), durations=dur,
                 phones=np.array([tokens[int(p)] for p in rng.integers(1, 85, tp)]),
                 speaker=np.array(SPEAKERS[i % 4]), emotion=np.array(EMOTIONS[i % 5]),
                 transcript=np.array(f"utterance {i}"), audio_path=np.array(f"{i}.wav"))
        paths.append(path)
    with open(os.path.join(root, "fs2_train.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from fastspeech2 import load_config, ops
    from fastspeech2.dataset import FastSpeech2Dataset, GpuCollate, VALID_TOKENS
    from fastspeech2.device_store import FS2DeviceStore, recompute_rows
    from fastspeech2.intensity import IntensityExtractor, get_intensity_representation
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    cfg = load_config()
    n_mels, rc = cfg["audio"]["n_mels"], cfg["model"]["rank_model"]
    dev = torch.device("cuda")
    B = a.batch
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, a.utterances, n_mels, np.random.default_rng(0), VALID_TOKENS)
        ds = FastSpeech2Dataset(root, " [noise] ", SPEAKERS, EMOTIONS)
        items = [ds[i] for i in range(len(ds))]
        store = FS2DeviceStore(ds, device=dev)
    torch.manual_seed(0)
    ext = IntensityExtractor(n_mels, rc["n_heads"], len(EMOTIONS), rc["n_encoder_layers"],
                             rc["hidden_dim"], rc["kernel_size"], rc["dropout"],
                             act_dtype=getattr(torch, a.dtype)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store.cache_intensity(ext, batch_size=B)
    torch.cuda.synchronize()
    cache_ms = (time.perf_counter() - t0) * 1e3
    collate = GpuCollate(dev)
    order = torch.randperm(len(items), generator=torch.Generator().manual_seed(1)).tolist()
    batches = [order[s:s + B] for s in range(0, len(order) - B + 1, B)]

    def host(idx):
        batch = collate([items[i] for i in idx])
        return batch, get_intensity_representation(ext, batch)

    def resident(idx):
        batch = store.collate(idx)
        return batch, get_intensity_representation(ext, batch)

    def cached(idx):
        return store.collate(idx, intensity=True, extractor=ext)

    errs, redo = [], []
    for idx in batches:
        (ba, _), (bb, ib), (bc, ic) = host(idx), resident(idx), cached(idx)
        for k in TENSORS:
            assert ba[k].dtype == bb[k].dtype and ba[k].shape == bb[k].shape, k
            assert torch.equal(ba[k], bb[k]) and torch.equal(bb[k], bc[k]), k
        assert ba[8] == bb[8] == bc[8] and ba[9] == bb[9] == bc[9]
        errs.append(((ic - ib).abs().max() / ib.abs().max()).item())
        redo.append(len(recompute_rows(bb[7].tolist(), store.reach)))

    def timed(fn, idx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(idx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for i in range(a.warmup):
        for fn in (host, resident, cached):
            fn(batches[i % len(batches)])
    ta, tb, tc = [], [], []
    for i in range(a.triples):
        idx = batches[i % len(batches)]
        ta.append(timed(host, idx))
        tb.append(timed(resident, idx))
        tc.append(timed(cached, idx))

    # the collates alone (no intensity), the same way
    pa, pb = [], []
    for i in range(a.triples):
        idx = batches[i % len(batches)]
        pa.append(timed(lambda ix: collate([items[j] for j in ix]), idx))
        pb.append(timed(store.collate, idx))

    # the kernel alone, between device events, cache gather included
    rows, Tp, Tm = store._sorted(batches[0])
    desc = store.table_d.index_select(1, torch.from_numpy(rows).to(dev))
    E = store.cache.shape[1]
    o = store._outputs(B, Tp, Tm, E, None)
    kt = []
    for i in range(a.warmup + a.triples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.store_collate(store.buffer, store.ibuffer, desc, store.cache, B, Tp, Tm, n_mels, E,
                          o[0], o[5], o[1], o[2], o[3], o[4], o[7], o[6], o[8])
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            kt.append(e0.elapsed_time(e1) * 1e3)
    valid = int(o[6].sum())
    res = {"metric": "FastSpeech2 batch assembly + intensity input, ms per batch (host clock "
                     "around a synchronised call; items in host memory)",
           "a_host_ms": spread(ta), "b_store_ms": spread(tb), "c_cached_ms": spread(tc),
           "ratio_b_over_a": spread([y / x for x, y in zip(ta, tb)]),
           "ratio_c_over_b": spread([y / x for x, y in zip(tb, tc)]),
           "ratio_c_over_a": spread([y / x for x, y in zip(ta, tc)]),
           "collate_only_host_ms": spread(pa), "collate_only_store_ms": spread(pb),
           "ratio_collate_store_over_host": spread([y / x for x, y in zip(pa, pb)]),
           "tuples_a_b_bit_identical": True,
           "intensity_c_vs_b_rel_max": max(errs), "intensity_c_vs_b_rel_by_batch": errs,
           "rows_recomputed_by_batch": redo, "rows_recomputed_mean": statistics.mean(redo),
           "reach_R": store.reach, "cache_fill_ms": cache_ms,
           "kernel_us": spread(kt),
           "kernel_batch": {"B": B, "Tp": Tp, "Tm": Tm, "n_mels": n_mels, "E": E,
                            "valid_frames": valid,
                            "bytes_moved": 4 * (n_mels + 2) * (valid + 2 * B * Tm)},
           "triples": a.triples, "B": B, "utterances": len(items), "dtype": a.dtype,
           "store_bytes": store.nbytes, "cache_bytes": 4 * store.cache.numel(),
           "batches_in_cycle": len(batches),
           "note": "synthetic items; the kernel's time between device events includes the "
                   "launch; not measured: .npz reads, DataLoader workers, more than one GPU"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
