"""CPU: the rank-model data path without a GPU.

* tests/rank_collate_restatement.py reproduces the reference ``collate_fn``'s own output on the
  fixture's raw items, exactly (rank_ref.npz ``bank.raw_*`` -> ``bank.b{k}.*``), which is what
  lets test_gpu_rank_collate.py use it for shapes the fixture lacks;
* ``FineGrainedDataset`` reads the reference's files and ``{split}.txt`` and refuses pickles;
* ``fs2_rank_collate`` refuses bad arguments before any launch;
* the header, the ctypes table and the library agree on the new symbol;
* the module refuses a non-HIP device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import rank_collate_restatement as RC


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "rank_ref.npz"))


def test_restatement_reproduces_reference_collate_on_fixture(z):
    items = RC.fixture_items(z)
    assert len(items) == 25 and int(z["bank.n_batches"]) == 4
    seen_T, directions = [], set()
    for k in range(4):
        batch = items[8 * k:8 * k + 8]
        got = RC.collate_restatement(batch)
        for key in ("emo_X", "neu_X", "speakers", "emotions", "length"):
            ref = z[f"bank.b{k}.{key}"]
            assert got[key].dtype == ref.dtype and got[key].shape == ref.shape, (k, key)
            assert np.array_equal(got[key], ref), (k, key)
        seen_T.append(got["emo_X"].shape[1])
        assert got["emo_X"].shape[1] > got["length"].max()      # max_T exceeds every length
        for it in batch:
            d = it["emo_X"].shape[1] - it["neu_X"].shape[1]
            directions.add(int(np.sign(d)))
    assert seen_T == [30, 30, 28, 27]
    assert directions >= {-1, 1}                                 # truncation in both directions
    assert z["bank.b3.length"].tolist() == [19] and z["bank.b3.emo_X"].shape == (1, 27, 16)


# ------------------------------------------------------------------ dataset loader
SPEAKERS = ["spk_a", "spk_b"]
EMOTIONS = ["neutral", "amused", "angry"]
LINES = [("spk_a", "amused", "0", "1"), ("spk_b", "angry", "0", "2"), ("spk_a", "angry", "3", "1"),
         ("spk_b", "amused", "1", "2"), ("spk_a", "amused", "2", "0")]


def _write_tiny(root, n_mels=4):
    rng = np.random.default_rng(3)
    arrays = {}

    def put(spk, name):
        X = rng.standard_normal((n_mels + 2, int(rng.integers(3, 12)))).astype(np.float32)
        os.makedirs(os.path.join(root, spk), exist_ok=True)
        RC.write_utterance(os.path.join(root, spk, name + ".npz"), X)
        arrays[spk, name] = X

    for spk in SPEAKERS:
        for n in range(3):
            put(spk, f"neutral_{n}")
    for spk, emo, e, _ in LINES:
        put(spk, f"{emo}_{e}")
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join("|".join(l) for l in LINES) + "\n")
    return arrays


def test_dataset_reads_reference_files(tmp_path):
    from fastspeech2.rank_dataset import FineGrainedDataset
    arrays = _write_tiny(str(tmp_path))
    ds = FineGrainedDataset(str(tmp_path), SPEAKERS, EMOTIONS, split="train")
    assert len(ds) == 5
    for i, (spk, emo, e, n) in enumerate(LINES):
        it = ds[i]
        assert set(it) == {"emo_X", "neu_X", "speaker", "emotion"}
        for key, want in (("emo_X", arrays[spk, f"{emo}_{e}"]),
                          ("neu_X", arrays[spk, f"neutral_{n}"])):
            assert isinstance(it[key], np.ndarray) and it[key].dtype == np.float32
            assert it[key].shape == want.shape and np.array_equal(it[key], want), (i, key)
        assert it["speaker"] == SPEAKERS.index(spk) and it["emotion"] == EMOTIONS.index(emo)
    a, b = ds[0], ds[2]                          # lines 0 and 2 share spk_a/neutral_1
    assert a["neu_X"] is b["neu_X"] and a["emo_X"] is not b["emo_X"]


_TRIPPED = []


def _trip():
    _TRIPPED.append(1)
    return 0


class _Trip:
    def __reduce__(self):
        return (_trip, ())


def test_dataset_refuses_object_arrays_without_unpickling(tmp_path):
    from fastspeech2.rank_dataset import FineGrainedDataset
    _write_tiny(str(tmp_path))
    bad = np.empty(1, dtype=object)
    bad[0] = _Trip()
    path = os.path.join(str(tmp_path), "spk_a", "amused_0.npz")
    np.savez(path, mel=bad, pitch=np.zeros(3, np.float32), energy=np.zeros(3, np.float32))
    ds = FineGrainedDataset(str(tmp_path), SPEAKERS, EMOTIONS)
    del _TRIPPED[:]
    with pytest.raises(ValueError, match="allow_pickle"):
        ds[0]
    assert not _TRIPPED                          # nothing was unpickled
    with np.load(path, allow_pickle=True) as f:  # the file does hold a live pickle
        f["mel"]
    assert _TRIPPED


# ------------------------------------------------------------------ C ABI
def test_rank_collate_host_validation():
    """Every call here is refused or empty: one that passed the checks would launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    names = ("store", "emo_off", "emo_len", "neu_off", "neu_len", "emo_X", "neu_X", "length")
    good = dict({n: p for n in names}, B=2, T=5, C=16)

    def call(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_rank_collate(a["store"], a["emo_off"], a["emo_len"], a["neu_off"],
                                    a["neu_len"], a["B"], a["T"], a["C"], a["emo_X"], a["neu_X"],
                                    a["length"], None)

    for n in names:
        assert call(**{n: None}) == -1, n
    assert call(C=2) == -1 and call(C=131) == -1
    assert call(B=-1) == -1 and call(T=-1) == -1
    assert call(B=0) == 0 and call(T=0) == 0


def test_rank_collate_symbol_declared_bound_and_exported():
    from fastspeech2 import _native as N, ops
    src = open(os.path.join(ROOT, "include", "fs2_hip.h")).read()
    m = re.search(r"int\s+fs2_rank_collate\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, "include/fs2_hip.h does not declare fs2_rank_collate"
    assert "rank_model/dataset.py:71-115" in src
    n_args = m.group(1).count(",") + 1
    res, args = N.SIGNATURES["fs2_rank_collate"]
    assert res is ctypes.c_int and len(args) == n_args == 12
    assert [a is ctypes.c_int for a in args] == [False] * 5 + [True] * 3 + [False] * 4
    assert hasattr(N.load(), "fs2_rank_collate") and callable(ops.rank_collate)


def test_public_names_and_device_refusal():
    import fastspeech2
    from fastspeech2 import rank_dataset as RD
    for name in ("FineGrainedDataset", "RankGpuCollate", "RankDeviceStore"):
        assert getattr(fastspeech2, name) is getattr(RD, name)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RD.RankGpuCollate(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        RD.RankDeviceStore(None, device="cpu")
