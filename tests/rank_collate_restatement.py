"""Test helper: a numpy restatement of the rank model's pair collate, written from the
description of the algorithm (rank_model/dataset.py:71-115), and the slicing of the raw items
out of tests/golden/rank_ref.npz.

test_rank_collate_host.py pins this restatement to the reference collate's own output (the
``bank.b{k}.*`` batches of the fixture); test_gpu_rank_collate.py uses it as the reference for
the shapes the fixture lacks.
"""
import numpy as np


def collate_restatement(items, T=None):
    """items: dicts with ``emo_X``, ``neu_X`` float32 (C, T_i) and int ``speaker``, ``emotion``.

    Per item the pair is cut to the shorter of its two arrays; the batch is zero-padded to ``T``
    frames, by default the longest array of the batch BEFORE the cut (so T may exceed every
    ``length``); the result is frame-major (B, T, C).  A given ``T`` below a pair's cut clamps
    it (``fs2_rank_collate``'s rule; the reference never passes one)."""
    B = len(items)
    C = items[0]["emo_X"].shape[0]
    if T is None:
        T = max(max(it["emo_X"].shape[1], it["neu_X"].shape[1]) for it in items)
    out = {"emo_X": np.zeros((B, T, C), dtype=np.float32),
           "neu_X": np.zeros((B, T, C), dtype=np.float32),
           "speakers": np.array([it["speaker"] for it in items], dtype=np.int64).reshape(B),
           "emotions": np.array([it["emotion"] for it in items], dtype=np.int64).reshape(B),
           "length": np.zeros(B, dtype=np.int64)}
    for b, it in enumerate(items):
        n = min(it["emo_X"].shape[1], it["neu_X"].shape[1], T)
        out["length"][b] = n
        for key in ("emo_X", "neu_X"):
            out[key][b, :n] = np.asarray(it[key], dtype=np.float32)[:, :n].T
    return out


def fixture_items(z):
    """The 25 raw items of rank_ref.npz as the dataset returned them: ``bank.raw_emo`` /
    ``bank.raw_neu`` hold the (C, T_i) arrays side by side, cut here at the cumulative lengths."""
    eo = np.concatenate([[0], np.cumsum(z["bank.raw_emo_len"])])
    no = np.concatenate([[0], np.cumsum(z["bank.raw_neu_len"])])
    emo, neu = z["bank.raw_emo"], z["bank.raw_neu"]
    return [{"emo_X": np.ascontiguousarray(emo[:, eo[i]:eo[i + 1]]),
             "neu_X": np.ascontiguousarray(neu[:, no[i]:no[i + 1]]),
             "speaker": int(z["bank.raw_speaker"][i]), "emotion": int(z["bank.raw_emotion"][i])}
            for i in range(len(z["bank.raw_emo_len"]))]


def random_items(C, emo_lens, neu_lens, seed=0):
    """Random pairs of the given lengths; speaker / emotion ids count up."""
    rng = np.random.default_rng(seed)
    return [{"emo_X": rng.standard_normal((C, le)).astype(np.float32),
             "neu_X": rng.standard_normal((C, ln)).astype(np.float32),
             "speaker": i % 3, "emotion": (2 * i + 1) % 5}
            for i, (le, ln) in enumerate(zip(emo_lens, neu_lens))]


def write_utterance(path, X):
    """One preprocessed .npz with the keys of make_golden_rank.py::_write_utterance, holding
    X = (n_mels + 2, T) split back into mel / pitch / energy."""
    T = X.shape[1]
    np.savez(path, mel=X[:-2], pitch=X[-2], energy=X[-1], durations=np.array([T]),
             phones=np.array(["a"]), transcript=np.array("a"), audio_path=np.array("a.wav"),
             textgrid_path=np.array("a.TextGrid"))
