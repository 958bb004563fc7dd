"""Rank-model eval forward at the reference size (parameter.yaml model.rank_model: 6 layers,
hidden 384, 2 heads, k=9; B=8, T=600, bf16) on 1 MI355X, random-init weights:

  one_pass    ``RankModel.forward``: fs2_rank_mixup_input, ONE extractor pass over the 2B mixed
              sequences, fs2_rank_pool;
  two_passes  what the code before this path could do: the two mixes, the pooling and the
              projector in torch around two ``IntensityExtractor`` calls of B sequences.

The two are timed as interleaved pairs (A B A B ...), each call ended by a device synchronise;
reported are the medians, the median of the per-pair ratios and its range.  The outputs of the
two arms are compared first.

    python tools/rank_eval_bench.py [--pairs 30] [--warmup 5] [--batch 8] [--frames 600]
Prints one JSON line (and writes it to --out when given).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from fastspeech2 import load_config
    from fastspeech2.intensity import RankModel
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    rc = load_config()["model"]["rank_model"]
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    m = RankModel(80, rc["n_heads"], 5, rc["n_encoder_layers"], rc["hidden_dim"],
                  rc["kernel_size"], rc["dropout"], act_dtype=dt).cuda().eval()
    B, T = a.batch, a.frames
    g = torch.Generator().manual_seed(1)
    length = torch.randint(T // 2, T + 1, (B,), generator=g)
    length[0] = T
    emo_X, neu_X = torch.randn(B, T, 82, generator=g), torch.randn(B, T, 82, generator=g)
    for b in range(B):
        emo_X[b, int(length[b]):] = 0.0
        neu_X[b, int(length[b]):] = 0.0
    emo_X, neu_X, length = emo_X.cuda(), neu_X.cuda(), length.cuda()
    emotions = torch.randint(0, 5, (B,), generator=g).cuda()
    lambdas = torch.rand(2, B, generator=g).cuda()

    def one_pass():
        return m(emo_X, neu_X, emotions, length, lambdas)

    @torch.no_grad()
    def two_passes():
        ext = m.intensity_extractor
        lam_i, lam_j = lambdas[0].reshape(B, 1, 1), lambdas[1].reshape(B, 1, 1)
        Ii = ext(lam_i * emo_X + (1 - lam_i) * neu_X, length, emotions)
        Ij = ext(lam_j * emo_X + (1 - lam_j) * neu_X, length, emotions)
        hi = Ii.sum(dim=1) / length.unsqueeze(1).float()
        hj = Ij.sum(dim=1) / length.unsqueeze(1).float()
        return lam_i, lam_j, Ii, Ij, hi, hj, m.projector(hi).squeeze(-1), \
            m.projector(hj).squeeze(-1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pa, pb = one_pass(), two_passes()
    torch.cuda.synchronize()
    diff = {n: ((x - y).abs().max() / y.abs().max()).item()
            for n, x, y in zip(("Ii", "Ij", "hi", "hj", "ri", "rj"), pa[2:], pb[2:])}
    ta, tb = [], []
    for _ in range(a.pairs):
        ta.append(timed(one_pass))
        tb.append(timed(two_passes))
    ratios = [x / y for x, y in zip(ta, tb)]
    res = {"metric": "rank-model eval forward, ms per call (host clock around a synchronised call)",
           "one_pass_ms_median": statistics.median(ta), "two_passes_ms_median": statistics.median(tb),
           "one_pass_ms_min": min(ta), "two_passes_ms_min": min(tb),
           "ratio_one_over_two_median": statistics.median(ratios),
           "ratio_min": min(ratios), "ratio_max": max(ratios), "pairs": a.pairs,
           "B": B, "T": T, "dtype": a.dtype, "layers": rc["n_encoder_layers"],
           "hidden": rc["hidden_dim"], "max_rel_diff_between_arms": diff,
           "note": "random-init weights; two_passes mixes, pools and projects in torch"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
