"""Generates tests/golden/rank_train_ref.npz from the REFERENCE itself (run in the dev container,
where /root/reference exists; the GPU box never runs this).

    python tests/golden/make_golden_rank_train.py

The reference's ``RankModel`` (rank_model/model.py) and ``RankLoss`` (rank_model/loss.py),
imported unmodified, run ONE training step's forward and backward (rank_model/train.py:28-42
without the optimiser) on the CPU in fp32:

* config: that of rank_ref.npz with ``dropout = 0.0``, ``model.train()`` -- the training-mode
  code path with every dropout the identity, so the result does not depend on torch's RNG;
* weights: rank_ref.npz's state dict (not stored again);
* inputs: B=4, T=40, lengths (40, 33, 1, 17), zero-padded, emotions (3, 1, 3, 2) -- two
  sequences share emotion 3, emotions 0 and 4 are unused -- given lambdas, alpha 0.1, beta 1.0,
  targets (emotions, zeros) as train.py:32.

Stored: the inputs (``in.*``), the 8-tuple (``out.*``), the three losses and the gradient of
every parameter (``grad.<state-dict key>``).  The script asserts that every parameter has a
non-zero gradient, that the unused emotions' embedding rows are exact zeros, and prints the
distance of the fp32 gradients from a float64 run of the same module (per tensor, max-norm
relative): the reference's own fp32 noise, which bounds what a parity tolerance can mean.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/emo_rank_tts"
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]       # rank_restatement, and the oracle it imports

NAMES = ("lam_i", "lam_j", "Ii", "Ij", "hi", "hj", "ri", "rj")
ALPHA, BETA = 0.1, 1.0


def _step(model, RankLoss, inp, dtype):
    model = model.to(dtype).train()
    model.zero_grad()
    emo_X, neu_X, lambdas = (inp[k].to(dtype) for k in ("emo_X", "neu_X", "lambdas"))
    pred = model(emo_X, neu_X, inp["emotions"], inp["length"], lambdas=lambdas)
    losses = RankLoss(ALPHA, BETA)(pred, (inp["emotions"], torch.zeros_like(inp["emotions"])))
    losses[0].backward()
    return pred, losses, {k: p.grad.clone() for k, p in model.named_parameters()}


def main():
    import rank_restatement as R
    sys.path[:0] = [REF, os.path.join(REF, "rank_model")]
    from rank_model.model import RankModel
    from rank_model.loss import RankLoss
    _, kw, sd = R.load_golden(HERE)
    kw = dict(kw, dropout=0.0)
    model = RankModel(**kw)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(29)
    B, T, C = 4, 40, kw["n_mels"] + 2
    length = torch.tensor([40, 33, 1, 17])
    emo_X, neu_X = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    for b in range(B):
        emo_X[b, int(length[b]):] = 0.0                 # collate zero padding
        neu_X[b, int(length[b]):] = 0.0
    inp = dict(emo_X=emo_X, neu_X=neu_X, emotions=torch.tensor([3, 1, 3, 2]), length=length,
               lambdas=torch.rand(2, B, generator=g))
    pred, losses, grads = _step(model, RankLoss, inp, torch.float32)
    for k, v in grads.items():
        assert v.abs().max() > 0, f"{k}: zero gradient"
    ge = grads["intensity_extractor.emotion_embedding.weight"]
    assert not ge[0].any() and not ge[4].any() and ge[3].any() and ge[1].any() and ge[2].any()
    _, _, g64 = _step(model, RankLoss, inp, torch.float64)
    worst = max(((grads[k].double() - g64[k]).abs().max() / g64[k].abs().max()).item()
                for k in grads)
    model.float()
    print(f"fp32 gradients vs the reference's float64 run: worst rel {worst:.2e}")
    out = {"in." + k: v.numpy() for k, v in inp.items()}
    out.update({"out." + n: t.detach().numpy() for n, t in zip(NAMES, pred)})
    out["losses"] = torch.stack([l.detach() for l in losses]).numpy()
    out.update({"grad." + k: v.numpy() for k, v in grads.items()})
    path = os.path.join(HERE, "rank_train_ref.npz")
    np.savez_compressed(path, alpha=np.array(ALPHA), beta=np.array(BETA),
                        fp32_noise=np.array(worst), **out)
    print("wrote rank_train_ref.npz:", os.path.getsize(path), "bytes, losses", out["losses"])


if __name__ == "__main__":
    main()
