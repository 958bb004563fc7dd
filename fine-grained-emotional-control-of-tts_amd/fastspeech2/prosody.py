"""Prosody feature stage on the GPU: F0 and energy tracks -> finished items and ``stats.json``.

Reference: the second half of ``emo_rank_tts/rank_model/preprocess.py::feature_extraction``
(:104-168) with ``_average_by_duration`` (:16-23), ``remove_outliers`` (:27-31) and
``normalize_field`` (:35-46), for a whole corpus slice at once:

1. ``D = sum(durations)``; pitch, mel and energy are cut to their first D frames (:104,117-118);
2. pitch: ``scipy.interpolate.interp1d(voiced ids, voiced values, fill_value=(first, last),
   bounds_error=False)`` over all frames, float64 (:106-112);
3. with ``pitch_averaging`` / ``energy_averaging`` the track is averaged per phoneme into a
   float32 array and repeated over the phoneme's frames (:120-126);
4. the values inside ``[q1 - 1.5 iqr, q3 + 1.5 iqr]`` (``np.percentile(x, [25, 75])``) of every
   utterance of a (speaker, emotion) group feed one ``StandardScaler.partial_fit`` (:128-131);
5. every track becomes ``(x - mean) / scale`` in float64; the group's min and max of that, with
   mean and scale, are ``stats.json`` (:153-168).

The kernels are csrc/prosody.hip (``fs2_prosody_track`` / ``_stats`` / ``_normalize`` /
``_minmax``): four launches per field whatever the lengths, no atomics, the same bits on every
run.  ``ProsodyStage`` makes one upload, the eight launches, and one read-back of the groups'
statistics and the utterances' status words.  ``extract_features`` runs ``MelFrontEnd`` and
``ProsodyStage`` and returns a ``FeatureSet``, whose items are ``FastSpeech2Dataset``'s, so
``FS2DeviceStore(feature_set)`` works as it stands, and whose ``write`` leaves the reference's
``.npz`` files and ``stats.json``.

Deviations from the reference, all documented in DESIGN.md section 7:

* un-averaged pitch is float64 in the reference's ``.npz`` and rounded to float32 when the
  dataset loads it; here it is rounded once at the same point of the arithmetic (after the
  division), so the loaded values are the same float32 rounding of the same float64 quotient;
* the energy's phoneme mean is accumulated in float64 and rounded once to float32, where numpy's
  float32 ``mean`` accumulates in float32 (a few float32 roundings, bounded in
  tests/prosody_restatement.py);
* voiced frames keep their F0 exactly, where interp1d recomputes them from the two-point
  formula (a few float64 roundings);
* an utterance whose energy holds a NaN (a one-frame utterance: min-max of one value is 0 / 0),
  or whose pitch has no voiced frame inside D, is rejected; the reference crashes on either;
* utterances longer than 4096 frames (65 s at hop 256 / 16 kHz) are refused.

MFA alignment, pyworld F0, librosa loading and G2P stay offline CPU work: their results are the
inputs here.
"""

import collections
import json
import os

import numpy as np
import torch

from . import ops
from .audio import MelFrontEnd, n_frames
from .dataset import phoneme2sequence

__all__ = ["ProsodyStage", "ProsodyResult", "extract_features", "FeatureSet"]

HOST_SKIPPED = 8      # status bit: np.count_nonzero(pitch) <= 1 (preprocess.py:101), host side

ProsodyResult = collections.namedtuple(
    "ProsodyResult", "pitch energy order offsets lengths stats rejected status")
ProsodyResult.__doc__ = """pitch, energy: packed float32 device tensors; slot k holds utterance
``order[k]`` at ``[offsets[k], offsets[k + 1])`` (utterances ordered by group; those skipped on
the host have no slot).  lengths: D per utterance (B).  stats: {group: {"pitch": [min, max,
mean, std], "energy": [...]}} for the groups with an accepted utterance.  rejected: the sorted
indices of the utterances left out.  status: (B) int, FS2_PROSODY_* bits of either field |
HOST_SKIPPED."""


def check_alignment(f0s, energy_lengths, durations):
    """D per utterance after the host refusals: a negative duration, D == 0, D larger than the
    F0 or the energy track (the reference's ``assert``, :133), D > 4096."""
    D = np.zeros(len(durations), np.int64)
    for i, d in enumerate(durations):
        d = np.asarray(d, np.int64).reshape(-1)
        if d.size and d.min() < 0:
            raise ValueError(f"utterance {i}: negative duration {int(d.min())}")
        D[i] = int(d.sum())
        if D[i] == 0:
            raise ValueError(f"utterance {i}: the durations sum to 0 frames")
        if D[i] > ops.PROSODY_MAX_D:
            raise ValueError(f"utterance {i}: {D[i]} frames, more than the supported "
                             f"{ops.PROSODY_MAX_D}")
        if D[i] > len(f0s[i]) or D[i] > energy_lengths[i]:
            raise ValueError(f"utterance {i}: the durations sum to {D[i]} frames, the F0 track "
                             f"has {len(f0s[i])} and the energy {energy_lengths[i]}")
    return D


class ProsodyStage:
    """``ProsodyStage(pitch_averaging, energy_averaging, device=...)``: the two switches of the
    reference yaml's ``preprocessing:`` block."""

    def __init__(self, pitch_averaging, energy_averaging, device="cuda"):
        self.pitch_averaging, self.energy_averaging = bool(pitch_averaging), bool(energy_averaging)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    @torch.no_grad()
    def __call__(self, f0s, energies, durations, groups, energy_lengths=None):
        """f0s: B host float64 arrays as pyworld returns them (0 = unvoiced), of any lengths.
        energies: a device (B, T_max) float32 tensor with ``energy_lengths`` (host integers), or
        a list of 1-D arrays / tensors.  durations: B integer sequences.  groups: B hashable
        ids, in any order.  Returns a ``ProsodyResult``."""
        B = len(f0s)
        f0s = [np.asarray(f, np.float64).reshape(-1) for f in f0s]
        padded = torch.is_tensor(energies) and energies.dim() == 2
        if padded:
            if energy_lengths is None:
                raise ValueError("a (B, T_max) energy tensor goes with energy_lengths")
            if energies.device != self.device or energies.dtype != torch.float32 \
                    or not energies.is_contiguous():
                raise ValueError(f"the energy tensor must be contiguous float32 on {self.device}")
            e_len = [min(int(n), energies.shape[1]) for n in energy_lengths]
        else:
            if energy_lengths is not None:
                raise ValueError("energy_lengths go with a (B, T_max) tensor, not with a list")
            energies = [torch.as_tensor(e).reshape(-1) for e in energies]
            e_len = [int(e.numel()) for e in energies]
        if not (len(e_len) == len(durations) == len(groups) == B):
            raise ValueError("f0s, energies, durations and groups must have one entry per "
                             "utterance")
        durs = [np.asarray(d, np.int64).reshape(-1) for d in durations]
        D = check_alignment(f0s, e_len, durs)
        if self.device.type != "cuda":
            raise RuntimeError("ProsodyStage runs only on the HIP device (libfs2_hip.so); there "
                               "is no CPU path")

        status = np.zeros(B, np.int64)
        for i, f in enumerate(f0s):                      # preprocess.py:101, on the whole track
            if np.count_nonzero(f) <= 1:
                status[i] = HOST_SKIPPED
        gid = {}
        for g in groups:
            gid.setdefault(g, len(gid))
        keep = [i for i in range(B) if not status[i]]
        order = np.asarray(sorted(keep, key=lambda i: gid[groups[i]]), np.int64)   # stable
        n = order.size
        names = []
        for i in order:
            if not names or names[-1] != groups[i]:
                names.append(groups[i])
        G = len(names)
        if n == 0:
            empty = torch.empty(0, dtype=torch.float32, device=self.device)
            return ProsodyResult(empty, empty.clone(), order, np.zeros(1, np.int64), D, {},
                                 sorted(range(B)), status)

        cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
        Dn = D[order]
        trk_off = cum(Dn)
        total = int(trk_off[-1])
        dur_off = cum([durs[i].size for i in order])
        group_off = cum(np.bincount([names.index(groups[i]) for i in order], minlength=G))
        f0_start, f0_len = trk_off[:-1], Dn               # only the first D values are uploaded
        if padded:
            e_start, e_n = order * energies.shape[1], Dn
        else:
            e_start, e_n = trk_off[:-1], Dn
        ints = np.concatenate([f0_start, f0_len, e_start, e_n, dur_off, trk_off, group_off]
                              + [durs[i] for i in order]).astype(np.int64)
        f0 = np.concatenate([f0s[i][:D[i]] for i in order])
        host_e = not padded and not all(e.device == self.device for e in energies)
        nb_i, nb_f = ints.nbytes, f0.nbytes
        host = torch.empty(nb_i + nb_f + (4 * total if host_e else 0), dtype=torch.uint8)
        host[:nb_i] = torch.from_numpy(ints).view(torch.uint8)
        host[nb_i:nb_i + nb_f] = torch.from_numpy(f0).view(torch.uint8)
        if host_e:
            torch.cat([energies[i][:D[i]].detach().cpu().float() for i in order],
                      out=host[nb_i + nb_f:].view(torch.float32))
        dev = host.to(self.device)                        # the one upload
        ints_d = dev[:nb_i].view(torch.int64)
        cuts = np.cumsum([n, n, n, n, n + 1, n + 1, G + 1])
        f0_start_d, f0_len_d, e_start_d, e_len_d, dur_off_d, trk_off_d, group_off_d = \
            [ints_d[a:b] for a, b in zip(np.concatenate([[0], cuts[:-1]]), cuts)]
        dur_d = ints_d[cuts[-1]:]
        f0_d = dev[nb_i:nb_i + nb_f].view(torch.float64)
        if padded:
            e_d = energies
        elif host_e:
            e_d = dev[nb_i + nb_f:].view(torch.float32)
        else:
            e_d = torch.cat([energies[i][:D[i]].float() for i in order])

        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=self.device)
        track, ustat, umm = f64(2, total), f64(2, n, 5), f64(2, n, 2)
        res = f64(8 * G + n)                              # gstat (2, G, 4), then status (2, n) int32
        gstat = res[:8 * G].view(2, G, 4)
        st = res[8 * G:].view(torch.int32).view(2, n)
        z = torch.empty(2, total, dtype=torch.float32, device=self.device)
        D_max = int(Dn.max())
        with torch.cuda.device(self.device):
            ops.prosody_track(f0_d, f0_start_d, f0_len_d, dur_d, dur_off_d, trk_off_d, n, D_max,
                              True, self.pitch_averaging, track[0], ustat[0], st[0])
            ops.prosody_track(e_d, e_start_d, e_len_d, dur_d, dur_off_d, trk_off_d, n, D_max,
                              False, self.energy_averaging, track[1], ustat[1], st[1])
            for k in (0, 1):
                ops.prosody_stats(ustat[k], st[k], st[1 - k], group_off_d, G, gstat[k])
            for k in (0, 1):
                ops.prosody_normalize(track[k], trk_off_d, st[k], st[1 - k], group_off_d, n, G,
                                      D_max, gstat[k], z[k], umm[k])
            for k in (0, 1):
                ops.prosody_minmax(umm[k], st[k], st[1 - k], group_off_d, G, gstat[k])
            back = res.cpu()                              # the one read-back
        gs = back[:8 * G].view(2, G, 4).numpy()
        sn = back[8 * G:].view(torch.int32).view(2, n).numpy()
        status[order] = sn[0] | sn[1]
        stats = {}
        for g, name in enumerate(names):
            if (status[order[group_off[g]:group_off[g + 1]]] == 0).any():
                stats[name] = {"pitch": [float(v) for v in gs[0, g]],
                               "energy": [float(v) for v in gs[1, g]]}
        rejected = [i for i in range(B) if status[i]]
        return ProsodyResult(z[0], z[1], order, trk_off, D, stats, rejected, status)


def build_feature_set(mels, pitches, energies, durations, phones, meta, stats, rejected=(),
                      speakers=None, emotions=None, noise_symbol=""):
    """A ``FeatureSet`` from finished per-utterance arrays (entries of rejected utterances are
    not looked at).  meta: one dict per utterance with ``speaker``, ``emotion``, ``audio_id``,
    ``audio_path``, ``transcript`` and optionally ``textgrid_path``.  stats: {(speaker, emotion):
    {"pitch": [...], "energy": [...]}}.  speakers / emotions: the name lists the items' integer
    ids index (the reference yaml's ``preprocessing:`` lists); by default the names in order of
    first appearance."""
    rejected = sorted(int(i) for i in rejected)
    out = set(rejected)
    first = lambda key: list(dict.fromkeys(m[key] for m in meta))
    speakers = list(speakers) if speakers is not None else first("speaker")
    emotions = list(emotions) if emotions is not None else first("emotion")
    items, records = [], []
    for i, m in enumerate(meta):
        if i in out:
            continue
        dur = torch.as_tensor(np.asarray(durations[i], np.int64).reshape(-1))
        Dn = int(dur.sum())
        mel = torch.as_tensor(mels[i], dtype=torch.float32)[:, :Dn].contiguous().cpu()
        pitch = torch.as_tensor(pitches[i], dtype=torch.float32).reshape(-1).cpu()
        energy = torch.as_tensor(energies[i], dtype=torch.float32).reshape(-1).cpu()
        ph = [str(p) for p in phones[i]]
        if not (mel.shape[1] == pitch.numel() == energy.numel() == Dn) or len(ph) != dur.numel():
            raise ValueError(f"utterance {i}: mel {tuple(mel.shape)}, pitch {pitch.numel()}, "
                             f"energy {energy.numel()} against {Dn} frames; {len(ph)} phonemes "
                             f"against {dur.numel()} durations")
        items.append({
            "mel": mel, "pitch": pitch, "energy": energy, "duration": dur,
            "phoneme": torch.LongTensor(phoneme2sequence(ph)),
            "speaker": torch.tensor(speakers.index(m["speaker"]), dtype=torch.long),
            "emotion": torch.tensor(emotions.index(m["emotion"]), dtype=torch.long),
            "text": str(m["transcript"]).replace(noise_symbol.strip(), "").strip(),
            "audio_path": str(m["audio_path"]),
        })
        records.append(dict(m, phones=ph))
    nested = {}
    for (spk, emo), s in stats.items():
        nested.setdefault(spk, {})[emo] = {"pitch": list(s["pitch"]), "energy": list(s["energy"])}
    return FeatureSet(items, records, nested, rejected)


class FeatureSet:
    """The finished items of one ``extract_features`` call: ``len``, ``[i]`` (the item dict of
    ``FastSpeech2Dataset.__getitem__``, CPU tensors), ``.stats`` (the nested dict of
    ``stats.json``), ``.rejected`` (indices into the call's inputs) and ``.write``."""

    def __init__(self, items, records, stats, rejected):
        self.items, self.records, self.stats, self.rejected = items, records, stats, rejected

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def write(self, preprocessed_path):
        """One ``{speaker}/{emotion}_{audio_id}.npz`` per item with the reference's keys
        (preprocess.py:134-151; pitch and energy already float32), and ``stats.json`` merged
        into an existing one per speaker and emotion (:162-168).  Returns the paths written."""
        paths = []
        for it, r in zip(self.items, self.records):
            os.makedirs(os.path.join(preprocessed_path, r["speaker"]), exist_ok=True)
            path = os.path.join(preprocessed_path, r["speaker"],
                                f"{r['emotion']}_{r['audio_id']}.npz")
            np.savez(path, phones=np.asarray(r["phones"], dtype=np.str_), emotion=r["emotion"],
                     speaker=r["speaker"], audio_id=str(r["audio_id"]),
                     audio_path=str(r["audio_path"]), transcript=str(r["transcript"]),
                     textgrid_path=str(r.get("textgrid_path", "")), mel=it["mel"].numpy(),
                     pitch=it["pitch"].numpy(), energy=it["energy"].numpy(),
                     durations=it["duration"].numpy())
            paths.append(path)
        stats_file = os.path.join(preprocessed_path, "stats.json")
        stats = {}
        if os.path.exists(stats_file):
            with open(stats_file) as f:
                stats = json.load(f)
        for spk, emos in self.stats.items():
            for emo, s in emos.items():
                stats.setdefault(spk, {})[emo] = s
        os.makedirs(preprocessed_path, exist_ok=True)
        with open(stats_file, "w") as f:
            f.write(json.dumps(stats, indent=4))
        return paths


def extract_features(wavs, f0s, durations, phones, meta, audio_cfg, pitch_averaging,
                     energy_averaging, device="cuda", speakers=None, emotions=None,
                     noise_symbol=""):
    """wavs: the trimmed waveforms (list of 1-D float arrays / tensors); f0s, durations: as
    ``ProsodyStage`` takes them; phones: the phoneme strings per utterance; meta: as
    ``build_feature_set`` takes it, the group of an utterance being (speaker, emotion);
    audio_cfg: the reference yaml's ``audio:`` block.  Returns a ``FeatureSet``."""
    fe = MelFrontEnd(**audio_cfg, device=device)
    wavs = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in wavs]
    mel, energy, _ = fe(wavs, layout="bct")
    lens = [n_frames(int(w.numel()), fe.hop_length) for w in wavs]
    groups = [(m["speaker"], m["emotion"]) for m in meta]
    res = ProsodyStage(pitch_averaging, energy_averaging, device=fe.device)(
        f0s, energy, durations, groups, energy_lengths=lens)
    mel_h, pitch_h, energy_h = mel.cpu(), res.pitch.cpu(), res.energy.cpu()
    B = len(wavs)
    pitches, energies = [None] * B, [None] * B
    for k, i in enumerate(res.order):
        pitches[i] = pitch_h[res.offsets[k]:res.offsets[k + 1]]
        energies[i] = energy_h[res.offsets[k]:res.offsets[k + 1]]
    return build_feature_set(mel_h, pitches, energies, durations, phones, meta, res.stats,
                             res.rejected, speakers, emotions, noise_symbol)
