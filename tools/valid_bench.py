"""One validation batch at the benchmark's size (B=32, bf16, reference configuration, the
synthetic batch of bench.py), two ways:

  (a) what a user could do before ``eval_step``: ``model.eval()``, ``torch.no_grad()``,
      ``Loss()(model(...))`` -- the loss goes through fs2_loss_fwd_bwd, gradients and all;
  (b) ``FusedTrainer.eval_step`` -- the forward-only fs2_loss_fwd, no host sync.

Interleaved (a), (b) pairs after a warm-up, each arm ended by a device synchronise and timed on
the host; per arm the median and the range in ms and ``torch.cuda.max_memory_allocated`` of one
call (peak reset before it).  Then the two loss entries alone on the batch's predictions, between
device events.  Prints one JSON line; ``--out`` also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))
import torch  # noqa: E402


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fastspeech2 import _native, load_config
    from fastspeech2.loss import Loss, fused_loss
    from fastspeech2.model import FastSpeech2
    from fastspeech2.synthetic import as_tuple, make_batch
    from fastspeech2.train import FusedTrainer
    _native.load()
    cfg = load_config()
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    model = FastSpeech2(**cfg["model"]["fastspeech2"], n_speakers=4, act_dtype=dt).cuda().eval()
    crit = Loss(**cfg["loss"])
    trainer = FusedTrainer(model, loss_weights=crit.weights, lr=cfg["train"]["learning_rate"])
    bt, inten = as_tuple(make_batch(B=args.batch, seed=0, device="cuda"))
    (phoneme, spk, phon_len, mel_tgt, pitch_tgt, energy_tgt, dur_tgt, mel_len) = bt
    Tm, Tp = mel_tgt.shape[1], phoneme.shape[1]
    targets = (mel_tgt, dur_tgt, pitch_tgt, energy_tgt, mel_len, phon_len)

    def arm_a():
        with torch.no_grad():
            pred = model(phoneme, spk, dur_tgt, pitch_tgt, energy_tgt, intensity=inten)
            return crit(pred, targets, 0)["total_loss"]

    def arm_b():
        return trainer.eval_step(bt, inten, mel_len_max=Tm)[0]

    def timed(fn):
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return {"max_memory_allocated": torch.cuda.max_memory_allocated(),
                "resident_before": base}

    for _ in range(args.warmup):
        timed(arm_a)
        timed(arm_b)
    ta, tb = [], []
    for _ in range(args.pairs):
        ms, va = timed(arm_a)
        ta.append(ms)
        ms, vb = timed(arm_b)
        tb.append(ms)
    res = {"tool": "valid_bench", "device": torch.cuda.get_device_name(0), "batch": args.batch,
           "dtype": args.dtype, "t_mel": Tm, "t_phon": Tp, "pairs": args.pairs,
           "warmup": args.warmup,
           "loss_module_no_grad": dict(_stats(ta), **peak(arm_a), total_loss=float(va)),
           "eval_step": dict(_stats(tb), **peak(arm_b), total_loss=float(vb))}

    # the two loss entries alone, on this batch's eval-mode predictions
    with torch.no_grad():
        out, _ = trainer.eng.forward(phoneme, spk, dur_tgt, pitch_tgt, energy_tgt, intensity=inten,
                                     training=False, seed=0, mel_len_max=Tm)
    mel, post, pd, pp, avg_p, pe, avg_e, _ = out
    largs = (mel, post, pd, pp.view(pd.shape), pe.view(pd.shape), mel_tgt, dur_tgt,
             avg_p.view(pd.shape), avg_e.view(pd.shape), mel_len, phon_len, crit.weights)
    for key, need in (("fs2_loss_fwd_bwd", True), ("fs2_loss_fwd", False)):
        for _ in range(3):
            fused_loss(*largs, need_grads=need)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.loss_reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fused_loss(*largs, need_grads=need)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        res[key] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us),
                    "reps": args.loss_reps,
                    "note": "one fused_loss call between device events, its allocations included"}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
