"""Log-mel front end at the reference size (rank_model parameter.yaml ``audio:``: 16 kHz, n_fft
1024, hop 256, 80 mels) on 1 MI355X: B = 32 seeded synthetic utterances of 8 to 16 s (noise plus
a tone), already in host memory as fp32 tensors:

  a  torch   what a user could do before, on the same device: per utterance upload,
             ``torch.stft`` + ``abs`` + matmul with the same filterbank + ``norm`` +
             ``clamp`` / ``log`` + the min-max of the energy;
  b  fused   ``MelFrontEnd.__call__`` on the list: one upload, one fs2_melspec and one
             fs2_energy_minmax launch.

Timed as interleaved pairs (a b a b ...) after warm-up, each arm ended by a device
synchronise.  Reported: medians and ranges of both arms and of the per-pair ratio b / a, the
two kernels' own time between device events (tables and waveforms resident), and the largest
difference between the arms' log mels and energies.  If ``torch.stft`` raises on the device its
message is recorded and arm a becomes the CPU computation on 16 threads plus the upload of its
results.  Not measured: other n_fft, utterances shorter than a second, the device store fed
from the front end, reading and resampling the audio files.

    python tools/melspec_bench.py [--pairs 30] [--warmup 5] [--batch 32] [--out FILE]
Prints one JSON line (and writes it to --out, default profiles/melspec_bench.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd"))

import numpy as np
import torch

AUDIO = dict(sampling_rate=16000, hop_length=256, win_length=1024, n_fft=1024, n_mels=80,
             f_min=0.0, f_max=8000.0)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def make_waves(B, seed=0):
    r = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        n = int(r.integers(8 * 16000, 16 * 16000 + 1))
        t = np.arange(n) / 16000.0
        y = 0.1 * r.uniform(-1, 1, n) + 0.05 * np.sin(2 * np.pi * float(r.uniform(100, 3000)) * t)
        out.append(torch.from_numpy(y.astype(np.float32)))
    return out


class TorchArm:
    """arm a: the torch route, per utterance"""

    def __init__(self, fb, device):
        self.device = device
        self.fb = fb.to(device)
        self.win = torch.hann_window(AUDIO["win_length"], periodic=True, device=device)

    def one(self, y):
        X = torch.stft(y, AUDIO["n_fft"], AUDIO["hop_length"], AUDIO["win_length"], self.win,
                       center=True, pad_mode="reflect", normalized=False, onesided=True,
                       return_complex=True).abs()
        mel = torch.matmul(X.transpose(-1, -2), self.fb).transpose(-1, -2)
        e = torch.norm(mel, dim=0)
        e = (e - e.min()) / (e.max() - e.min())
        return torch.log(torch.clamp(mel, min=1e-5)), e

    def __call__(self, waves, out_device):
        res = [self.one(y.to(self.device)) for y in waves]
        return [(m.to(out_device), e.to(out_device)) for m, e in res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melspec_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("melspec_bench needs a GPU: a CPU timing says nothing about it")
    from fastspeech2 import _native, ops
    from fastspeech2.audio import MelFrontEnd, mel_filterbank
    _native.load()
    dev = torch.device("cuda", 0)
    waves = make_waves(args.batch)
    fe = MelFrontEnd(**AUDIO, device=dev)
    fb = torch.from_numpy(mel_filterbank(513, 0.0, 8000.0, 80, 16000).astype(np.float32))

    res = {"metric": "waveform -> log mel + normalised energy, ms per batch of B utterances "
                     "(host clock around a call ended by a device synchronise; waveforms in "
                     "host memory)"}
    arm_a, a_where = TorchArm(fb, dev), "device"
    try:
        arm_a(waves[:1], dev)
        torch.cuda.synchronize()
    except Exception as exc:                     # noqa: BLE001 -- recorded, not hidden
        res["torch_stft_on_device_error"] = f"{type(exc).__name__}: {exc}"[:400]
        torch.set_num_threads(16)
        arm_a, a_where = TorchArm(fb, torch.device("cpu")), "cpu, 16 threads, + upload"
    res["arm_a_runs_on"] = a_where

    def run_a():
        out = arm_a(waves, dev)
        torch.cuda.synchronize()
        return out

    def run_b():
        out = fe(waves, layout="bct")
        torch.cuda.synchronize()
        return out

    # the arms agree
    ra, (mel, energy, mel_len) = run_a(), run_b()
    dm = de = 0.0
    for i, (m, e) in enumerate(ra):
        T = int(mel_len[i])
        assert m.shape == (80, T)
        dm = max(dm, float((mel[i, :, :T] - m).abs().max()))
        de = max(de, float((energy[i, :T] - e).abs().max()))
    res["max_abs_diff_log_mel"], res["max_abs_diff_energy"] = dm, de

    for _ in range(args.warmup):
        run_a()
        run_b()
    ta, tb = [], []
    for _ in range(args.pairs):
        t0 = time.perf_counter()
        run_a()
        t1 = time.perf_counter()
        run_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    res["a_torch_ms"], res["b_fused_ms"] = spread(ta), spread(tb)
    res["ratio_b_over_a"] = spread([b / a for a, b in zip(ta, tb)])

    # the kernels' own time: everything resident, device events around each launch
    packed, offsets, lens = fe._pack(waves, None)
    B, T = len(lens), max(1 + n // 256 for n in lens)
    mel = torch.empty(B, 80, T, device=dev)
    energy = torch.empty(B, T, device=dev)
    mel_len = torch.empty(B, dtype=torch.int64, device=dev)
    km, ke = [], []
    for it in range(args.warmup + args.pairs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        ops.melspec(packed, offsets, B, fe.window, fe.twiddle, fe.bands, fe.band_w, 1024, 1024,
                    256, 80, T, True, True, mel, energy, mel_len)
        ev[1].record()
        ops.energy_minmax(energy, mel_len, B, T, energy)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            km.append(ev[0].elapsed_time(ev[1]) * 1e3)
            ke.append(ev[1].elapsed_time(ev[2]) * 1e3)
    frames = sum(1 + n // 256 for n in lens)
    res["melspec_kernel_us"], res["energy_minmax_kernel_us"] = spread(km), spread(ke)
    res["batch"] = {"B": B, "T_max": T, "frames": frames, "samples": int(sum(lens)),
                    "bytes_in": 4 * int(sum(lens)), "bytes_out": 4 * B * T * 81}
    res["pairs"], res["warmup"] = args.pairs, args.warmup
    res["note"] = ("synthetic utterances of 8-16 s; the kernels' times between device events "
                   "include the launch; not measured: other n_fft, utterances under a second, "
                   "the device store fed from the front end, audio file reading")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
