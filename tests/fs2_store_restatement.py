"""Test helper for the FastSpeech2 device store (fastspeech2/device_store.py).

* ``pack`` / ``gather``: a numpy restatement of the store, written from its description: the
  items packed as the store packs them (per utterance the (n_mels + 2, T) block
  cat(mel, pitch, energy) in one float32 array, phoneme ids then durations in one int64 array,
  a (7, n) descriptor table) and a batch gathered back out of the packed arrays.
  test_fs2_store_host.py pins it to ``oracle.collate_oracle.collate_np`` and to
  tests/golden/collate_ref.npz; test_gpu_fs2_store.py uses it as a second reference.
* ``random_items`` / ``write_dataset``: hand-made item dicts and the same items as the
  reference's preprocessed files.
* ``intensity_case``: the fixed small extractor config, weights and six utterances shared by
  the CPU R-frame-rule tests and the GPU cache test.
"""
import os

import numpy as np
import torch

NAMES = ["phoneme", "speakers", "input_lengths", "mel", "pitch", "energy", "duration",
         "output_lengths", "labels", "wavs", "rank_X", "emotions"]


def pack(items):
    """(fbuf float32, ibuf int64, table (7, n) int64) with rows float offset, frames,
    int offset, phonemes, speaker, emotion, cache offset (-1: no cache)."""
    fl, il, table = [], [], np.zeros((7, len(items)), dtype=np.int64)
    fo = io = 0
    for u, it in enumerate(items):
        mel = np.asarray(it["mel"], dtype=np.float32)
        X = np.concatenate([mel, np.asarray(it["pitch"], dtype=np.float32)[None],
                            np.asarray(it["energy"], dtype=np.float32)[None]], axis=0)
        ph = np.asarray(it["phoneme"], dtype=np.int64)
        du = np.asarray(it["duration"], dtype=np.int64)
        table[:, u] = (fo, mel.shape[1], io, ph.size, int(it["speaker"]), int(it["emotion"]), -1)
        fl.append(X.reshape(-1))
        il += [ph, du]
        fo += X.size
        io += 2 * ph.size
    return np.concatenate(fl), np.concatenate(il), table


def gather(fbuf, ibuf, table, indices, texts, paths, n_mels):
    """The collate's 12 outputs (``NAMES``) for the batch ``indices``, read from the packed
    arrays alone."""
    idx = np.asarray(list(indices), dtype=np.int64)
    lens, order = torch.sort(torch.LongTensor(table[3, idx].tolist()), dim=0, descending=True)
    rows = idx[order.numpy()]
    B, Tp, Tm, C = len(rows), int(lens[0]), int(table[1, idx].max()), n_mels + 2
    out = {"phoneme": np.zeros((B, Tp), np.int64), "duration": np.zeros((B, Tp), np.int64),
           "rank_X": np.zeros((B, C, Tm), np.float32)}
    for b, u in enumerate(rows):
        fo, T, io, n = table[:4, u]
        out["phoneme"][b, :n] = ibuf[io:io + n]
        out["duration"][b, :n] = ibuf[io + n:io + 2 * n]
        out["rank_X"][b, :, :T] = fbuf[fo:fo + C * T].reshape(C, T)
    out["mel"] = np.ascontiguousarray(out["rank_X"][:, :n_mels].transpose(0, 2, 1))
    out["pitch"] = np.ascontiguousarray(out["rank_X"][:, n_mels])
    out["energy"] = np.ascontiguousarray(out["rank_X"][:, n_mels + 1])
    out["input_lengths"] = table[3, rows].copy()
    out["output_lengths"] = table[1, rows].copy()
    out["speakers"] = table[4, rows].copy()
    out["emotions"] = table[5, rows].copy()
    out["labels"] = [texts[u] for u in rows]
    out["wavs"] = [paths[u] for u in rows]
    return out


def split_durations(frames, n, rng):
    """n durations >= 1 summing to ``frames`` (needs n <= frames)."""
    cuts = np.sort(rng.choice(np.arange(1, frames), size=n - 1, replace=False)) if n > 1 else []
    return np.diff(np.concatenate([[0], cuts, [frames]])).astype(np.int64)


def random_items(n_mels, frames, phonemes, seed=0):
    """Item dicts as ``FastSpeech2Dataset`` returns them.  Durations sum to the frame count
    where the utterance has at least as many frames as phonemes (random otherwise)."""
    rng = np.random.default_rng(seed)
    items = []
    for i, (T, n) in enumerate(zip(frames, phonemes)):
        dur = split_durations(T, n, rng) if n <= T else rng.integers(1, 10, n)
        items.append({"mel": torch.from_numpy(rng.standard_normal((n_mels, T)).astype(np.float32)),
                      "pitch": torch.from_numpy(rng.standard_normal(T).astype(np.float32)),
                      "energy": torch.from_numpy(rng.standard_normal(T).astype(np.float32)),
                      "duration": torch.from_numpy(np.asarray(dur, dtype=np.int64)),
                      "phoneme": torch.from_numpy(rng.integers(1, 89, n).astype(np.int64)),
                      "speaker": torch.tensor(i % 3), "emotion": torch.tensor((2 * i + 1) % 5),
                      "text": f"text {i}", "audio_path": f"utt_{i}.wav"})
    return items


SPEAKERS = ["spk_a", "spk_b", "spk_c", "spk_d"]
EMOTIONS = ["Neutral", "Angry", "Happy", "Sad", "Surprise"]


def write_dataset(root, items, valid_tokens, mode="train"):
    """The items as preprocessed ``.npz`` files plus ``fs2_{mode}.txt``; returns the constructor
    arguments of ``FastSpeech2Dataset`` (root, noise_symbol, speakers, emotions)."""
    paths = []
    for i, it in enumerate(items):
        path = os.path.join(root, f"utt_{i}.npz")
        np.savez(path, mel=it["mel"].numpy(), pitch=it["pitch"].numpy(),
                 energy=it["energy"].numpy(), durations=it["duration"].numpy(),
                 phones=np.array([valid_tokens[int(p)] for p in it["phoneme"]]),
                 speaker=np.array(SPEAKERS[int(it["speaker"])]),
                 emotion=np.array(EMOTIONS[int(it["emotion"])]),
                 transcript=np.array(it["text"]), audio_path=np.array(it["audio_path"]))
        paths.append(path)
    with open(os.path.join(root, f"fs2_{mode}.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    return root, " [noise] ", SPEAKERS, EMOTIONS


# ------------------------------------------------------------------ the intensity case
# tests/golden/intensity_ref.npz's config: 2 layers, k = 9 (R = 16), hidden 32 = 4 * 8, 2 heads
EXT_KW = dict(n_mels=14, n_heads=2, n_emotions=5, n_encoder_layers=2, hidden_dim=32,
              kernel_size=9, dropout=0.1)
REACH = 16
CASE_FRAMES = [120, 119, 105, 104, 61, 60]       # pads 0, 1, 15, 16, 59, 60 at T_m = 120
CASE_PHONEMES = [30, 29, 27, 26, 16, 15]         # strictly descending: batch row i = item i
CASE_RECOMPUTED = [0, 1, 2]
CASE_SEED = 2                                    # chosen for the sensitivity condition, see
#                                                  test_fs2_store_host.py::test_r_frame_rule
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}    # tests/test_gpu_intensity.py's, same oracle


def intensity_case():
    """(state dict, items): seeded extractor weights (the module's own initialisation) and the
    six utterances of ``CASE_FRAMES``, durations summing to the frame counts."""
    from fastspeech2.intensity import IntensityExtractor
    torch.manual_seed(CASE_SEED)
    sd = {k: v.clone() for k, v in IntensityExtractor(**EXT_KW).state_dict().items()}
    return sd, random_items(EXT_KW["n_mels"], CASE_FRAMES, CASE_PHONEMES, seed=CASE_SEED)


def padded_batch(items, T):
    """rank_X (B, C, T) zero padded, lengths, emotions, durations (B, Tp), phon_len: the items
    as one batch in the given order."""
    B, C = len(items), items[0]["mel"].shape[0] + 2
    Tp = max(len(it["phoneme"]) for it in items)
    x = torch.zeros(B, C, T)
    dur = torch.zeros(B, Tp, dtype=torch.int64)
    for b, it in enumerate(items):
        n = it["mel"].shape[1]
        x[b, :, :n] = torch.cat([it["mel"], it["pitch"][None], it["energy"][None]], 0)
        dur[b, :len(it["duration"])] = it["duration"]
    return (x, torch.tensor([it["mel"].shape[1] for it in items]),
            torch.tensor([int(it["emotion"]) for it in items]), dur,
            torch.tensor([len(it["phoneme"]) for it in items]))


def oracle_rep(sd, items, T):
    """The oracle's in-batch intensity representation of ``items`` padded to T frames:
    ``extractor_forward`` then ``phoneme_average_np``; (B, Tp, E) float32 numpy."""
    from oracle.intensity_oracle import extractor_forward, phoneme_average_np
    x, lengths, emo, dur, pl = padded_batch(items, T)
    I = extractor_forward(sd, x, lengths, emo, EXT_KW["n_heads"], EXT_KW["n_encoder_layers"],
                          layout="BCT")
    return phoneme_average_np(I.numpy(), dur.numpy(), pl.numpy())
