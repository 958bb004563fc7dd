"""Generates tests/golden/rank_ref.npz from the REFERENCE itself (run in the dev container, where
/root/reference exists; the GPU box never runs this).

    python tests/golden/make_golden_rank.py

Everything is the reference's own code, imported, on seeded weights and inputs:
* ``RankModel`` (rank_model/model.py) and ``RankLoss`` (rank_model/loss.py) need only torch;
* ``FineGrainedDataset`` / ``collate_fn`` (rank_model/dataset.py) and ``bucketize(config)``
  (rank_model/inference.py) run unmodified on CPU over a synthetic preprocessed dataset written
  to a temporary directory (matplotlib on the Agg backend).

One small config for both cases (that of make_golden_intensity.py): n_mels=14 (C=16), 2 heads,
5 emotions, 2 layers, hidden 32, kernel 9; one ``RankModel`` state dict, stored as ``sd.*``
(without the layers that equal layer 0: tests/rank_restatement.py::load_golden puts them back).

Eval case (``eval.*``): B=4, T=40, lengths [40, 31, 17, 1], zero-padded inputs, lambdas =
linspace(0, 1, B) in both rows and targets (emotions, zeros) as train.py::validate_one_epoch
uses; the model's 8-tuple and RankLoss(0.1, 1.0)'s three values.

Bank case (``bank.*``): 2 speakers, 5 emotions, bucket_size 3, 25 lines of 9-30 frames in
shuffled order; no line carries the emotion 'neutral' (two empty groups) and one group has a
single utterance.  Stored: the raw items as the dataset returns them (``bank.raw_*``, the
(C, T_i) arrays side by side), the batches of the reference's loader (batch_size=8, unshuffled)
with the model's I, h, r for each (lambdas = ones; h and r depend on the batch's padded length),
and the bank that the reference's ``bucketize`` wrote.

The script asserts that within every group two scores are at least 1e-2 * max|r| apart, 100x
the fp32 tolerance of the GPU tests, so that rounding cannot reorder the sort; a seed that
misses it is skipped for the next one.
"""
import os
import sys
import tempfile

os.environ["MPLBACKEND"] = "Agg"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/emo_rank_tts"

CFG = dict(n_mels=14, n_heads=2, n_emotions=5, n_encoder_layers=2, hidden_dim=32, kernel_size=9,
           dropout=0.1)
SPEAKERS = ["spk_a", "spk_b"]
EMOTIONS = ["neutral", "amused", "angry", "disgusted", "sleepy"]
BUCKET = 3
# utterances per (speaker, emotion); 'neutral' has none, (spk_a, disgusted) has one
COUNTS = {("spk_a", "amused"): 4, ("spk_a", "angry"): 3, ("spk_a", "disgusted"): 1,
          ("spk_a", "sleepy"): 4, ("spk_b", "amused"): 3, ("spk_b", "angry"): 4,
          ("spk_b", "disgusted"): 3, ("spk_b", "sleepy"): 3}
N_NEUTRAL = 5   # neutral recordings per speaker, shared among that speaker's lines


def _write_utterance(path, rng, T):
    n_mels = CFG["n_mels"]
    np.savez(path, mel=rng.standard_normal((n_mels, T)).astype(np.float32),
             pitch=rng.standard_normal(T).astype(np.float32),
             energy=rng.standard_normal(T).astype(np.float32),
             durations=np.array([T]), phones=np.array(["a"]), transcript=np.array("a"),
             audio_path=np.array("a.wav"), textgrid_path=np.array("a.TextGrid"))


def _write_dataset(root, rng):
    lines = []
    for spk in SPEAKERS:
        os.makedirs(os.path.join(root, spk))
        for n in range(N_NEUTRAL):
            _write_utterance(os.path.join(root, spk, f"neutral_{n}.npz"), rng,
                             int(rng.integers(9, 31)))
    for (spk, emo), count in COUNTS.items():
        for n in range(count):
            _write_utterance(os.path.join(root, spk, f"{emo}_{n}.npz"), rng,
                             int(rng.integers(9, 31)))
            lines.append(f"{spk}|{emo}|{n}|{int(rng.integers(0, N_NEUTRAL))}")
    lines = [lines[i] for i in rng.permutation(len(lines))]
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def _bank_case(model, seed, ref):
    """Returns the dict of bank.* arrays, or None when two scores of a group are too close."""
    rng = np.random.default_rng(seed)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        pre, exp = os.path.join(tmp, "preprocessed"), os.path.join(tmp, "experiments")
        os.makedirs(pre)
        _write_dataset(pre, rng)
        ds = ref["FineGrainedDataset"](pre, SPEAKERS, EMOTIONS, split="train")
        items = [ds[i] for i in range(len(ds))]
        out["bank.raw_emo"] = np.concatenate([it["emo_X"] for it in items], axis=1)
        out["bank.raw_neu"] = np.concatenate([it["neu_X"] for it in items], axis=1)
        out["bank.raw_emo_len"] = np.array([it["emo_X"].shape[1] for it in items])
        out["bank.raw_neu_len"] = np.array([it["neu_X"].shape[1] for it in items])
        out["bank.raw_speaker"] = np.array([it["speaker"] for it in items])
        out["bank.raw_emotion"] = np.array([it["emotion"] for it in items])
        loader = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False,
                                             collate_fn=ref["collate_fn"], num_workers=0)
        scores, groups = [], []
        for k, batch in enumerate(loader):
            B = batch["emo_X"].size(0)
            with torch.no_grad():
                _, _, I, _, h, _, r, _ = model(batch["emo_X"], batch["neu_X"], batch["emotions"],
                                               batch["length"], torch.ones(2, B))
            for key in ("emo_X", "neu_X", "speakers", "emotions", "length"):
                out[f"bank.b{k}.{key}"] = batch[key].numpy()
            out[f"bank.b{k}.I"], out[f"bank.b{k}.h"], out[f"bank.b{k}.r"] = \
                I.numpy(), h.numpy(), r.numpy()
            scores.append(r.numpy())
            groups.append((batch["speakers"] * len(EMOTIONS) + batch["emotions"]).numpy())
        out["bank.n_batches"] = np.array(len(scores))
        scores, groups = np.concatenate(scores), np.concatenate(groups)
        margin = 1e-2 * np.abs(scores).max()
        for g in np.unique(groups):
            s = np.sort(scores[groups == g])
            if len(s) > 1 and np.diff(s).min() < margin:
                return None
        # the reference's own bucketize on the same files and weights
        exp_dir = os.path.join(exp, "rank_model", "golden")
        os.makedirs(exp_dir)
        torch.save(model.state_dict(), os.path.join(exp_dir, "best_model.pth"))
        config = {"path": {"experiment_path": exp, "preprocessed_path": pre},
                  "inference": {"exp_name": "golden", "bucket_size": BUCKET},
                  "preprocessing": {"speakers": SPEAKERS, "emotions": EMOTIONS},
                  "audio": {"n_mels": CFG["n_mels"]},
                  "model": {k: CFG[k] for k in ("n_heads", "n_encoder_layers", "hidden_dim",
                                                "kernel_size", "dropout")}}
        ref["bucketize"](config)
        out["bank.bank"] = np.load(os.path.join(exp_dir, "intensity.npy"))
    assert out["bank.bank"].shape == (len(SPEAKERS), len(EMOTIONS), BUCKET, len(EMOTIONS))
    assert not out["bank.bank"][:, 0].any(), "no line is 'neutral': those groups stay zero"
    return out


def _eval_case(model, ref, seed):
    g = torch.Generator().manual_seed(seed)
    B, T, C = 4, 40, CFG["n_mels"] + 2
    length = torch.tensor([40, 31, 17, 1])
    emo_X, neu_X = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    for b in range(B):
        emo_X[b, int(length[b]):] = 0.0                 # collate zero padding
        neu_X[b, int(length[b]):] = 0.0
    emotions = torch.tensor([3, 1, 4, 2])
    lambdas = torch.linspace(0, 1, steps=B).unsqueeze(0).repeat(2, 1)   # validate_one_epoch
    with torch.no_grad():
        pred = model(emo_X, neu_X, emotions, length, lambdas=lambdas)
        losses = ref["RankLoss"](0.1, 1.0)(pred, (emotions, torch.zeros_like(emotions)))
    out = {"eval.emo_X": emo_X, "eval.neu_X": neu_X, "eval.emotions": emotions,
           "eval.length": length, "eval.lambdas": lambdas,
           "eval.losses": torch.stack(list(losses))}
    for name, t in zip(("lam_i", "lam_j", "Ii", "Ij", "hi", "hj", "ri", "rj"), pred):
        out["eval." + name] = t
    return {k: v.numpy() for k, v in out.items()}


def main():
    sys.path[:0] = [REF, os.path.join(REF, "rank_model")]
    from rank_model.model import RankModel
    from rank_model.loss import RankLoss
    from rank_model.dataset import FineGrainedDataset, collate_fn
    from rank_model.inference import bucketize
    ref = dict(RankLoss=RankLoss, FineGrainedDataset=FineGrainedDataset, collate_fn=collate_fn,
               bucketize=bucketize)
    for seed in range(17, 117):
        torch.manual_seed(seed)
        model = RankModel(**CFG).eval().requires_grad_(False)
        arrays = _bank_case(model, seed, ref)
        if arrays is not None:
            break
        print(f"seed {seed}: two scores of a group closer than the margin, next seed")
    else:
        raise SystemExit("no seed met the score margin")
    arrays.update(_eval_case(model, ref, seed))
    # nn.TransformerEncoder deep-copies ONE initialised layer, so the layers are identical:
    # layer 0 is stored, and a later layer only where it differs (rank_restatement.load_golden
    # fills the others in from layer 0)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    first = "intensity_extractor.fft_block.layers.0."
    for k in list(sd):
        head, _, tail = k.partition(".fft_block.layers.")
        if tail and not tail.startswith("0.") and \
                np.array_equal(sd[k], sd[first + tail.split(".", 1)[1]]):
            del sd[k]
    arrays.update({"sd." + k: v for k, v in sd.items()})
    np.savez_compressed(os.path.join(HERE, "rank_ref.npz"), seed=np.array(seed),
                        cfg_keys=np.array(list(CFG)),
                        cfg_vals=np.array([float(v) for v in CFG.values()]),
                        speakers=np.array(SPEAKERS), emotions=np.array(EMOTIONS),
                        bucket_size=np.array(BUCKET), **arrays)
    print("wrote rank_ref.npz: seed", seed, "bank", arrays["bank.bank"].shape,
          "losses", arrays["eval.losses"])


if __name__ == "__main__":
    main()
