"""GPU: the FastSpeech2 device store (``fs2_store_collate`` in csrc/collate.hip,
``fastspeech2.device_store``, ``fastspeech2.train.train_one_epoch``).

The collate is byte movement: ``store.collate`` is compared bit for bit (``torch.equal``) with
``GpuCollate`` on the same items and with tests/fs2_store_restatement.py (pinned to the
reference collate's output in test_fs2_store_host.py).  Every ``out=`` tensor lies inside a
NaN-prefilled (int64: sentinel-prefilled) allocation whose odd guard regions must be untouched.

The cached intensity is compared with the oracle's in-batch value (``extractor_forward`` on the
padded batch, then ``phoneme_average_np``) at test_gpu_intensity.py's tolerances against the
same oracle, 1e-3 relative in fp32 and 3e-2 in bf16; test_fs2_store_host.py::test_r_frame_rule
shows that serving the longest row from the cache would miss both by more than 3x.
"""
import os

import numpy as np
import pytest
import torch

import fs2_store_restatement as S

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -(2 ** 62)
GUARD = 257            # guard floats on each side (odd on purpose)
IGUARD = 7


class Guarded:
    """The eight (with E: nine) ``out=`` tensors, each in the middle of a prefilled allocation."""

    def __init__(self, cuda, B, Tp, Tm, NM, E=0):
        spec = [((B, Tp), 1), ((B,), 1), ((B, Tm, NM), 0), ((B, Tm), 0), ((B, Tm), 0),
                ((B, Tp), 1), ((B,), 1), ((B, NM + 2, Tm), 0)] + ([((B, Tp, E), 0)] if E else [])
        self.flat, self.out = [], []
        for shape, is_int in spec:
            n, g = int(np.prod(shape)), IGUARD if is_int else GUARD
            f = torch.full((g + n + g,), SENTINEL if is_int else NAN,
                           dtype=torch.int64 if is_int else torch.float32, device=cuda)
            self.flat.append((f, g, n, is_int))
            self.out.append(f[g:g + n].view(shape))

    def check(self):
        for f, g, n, is_int in self.flat:
            for part in (f[:g], f[g + n:]):
                assert bool((part == SENTINEL).all() if is_int else torch.isnan(part).all())
            assert not bool(torch.isnan(f[g:g + n]).any()) if not is_int \
                else not bool((f[g:g + n] == SENTINEL).any())


def _same_as_numpy(got, want):
    for k, g in zip(S.NAMES, got):
        if k in ("labels", "wavs"):
            assert isinstance(g, list) and g == [str(s) for s in want[k]], k
            continue
        w = torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.device.type == "cuda" and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), k
        assert g.is_contiguous(), k
        assert torch.equal(g.cpu(), w), k


def _same_as_tuple(got, other):
    for k, g, o in zip(S.NAMES, got, other):
        if k in ("labels", "wavs"):
            assert g == o, k
            continue
        assert g.dtype == o.dtype and g.shape == o.shape and g.device == o.device, k
        assert g.is_contiguous() == o.is_contiguous() is True, k
        assert torch.equal(g, o), k


def _check_store(cuda, store, items, indices):
    """store.collate(indices) into guarded outputs and into its own, against ``GpuCollate`` on
    the items and the restatement."""
    from fastspeech2.dataset import GpuCollate
    NM = items[0]["mel"].shape[0]
    fbuf, ibuf, table = S.pack(items)
    want = S.gather(fbuf, ibuf, table, indices, [it["text"] for it in items],
                    [it["audio_path"] for it in items], NM)
    B, Tp = want["phoneme"].shape
    Tm = want["pitch"].shape[1]
    g = Guarded(cuda, B, Tp, Tm, NM)
    got = store.collate(indices, out=g.out)
    torch.cuda.synchronize()
    g.check()
    assert got[0] is g.out[0] and got[10] is g.out[7] and len(got) == 12
    _same_as_numpy(got, want)
    other = GpuCollate(cuda)([items[i] for i in indices])
    _same_as_tuple(got, other)
    _same_as_tuple(store.collate(indices), other)          # outputs it allocates itself
    return got


# ------------------------------------------------------------------ 1: golden, from files
def test_golden_items_from_files(cuda, golden_dir, tmp_path):
    from fastspeech2.dataset import FastSpeech2Dataset, VALID_TOKENS
    from fastspeech2.device_store import FS2DeviceStore
    from oracle.collate_oracle import items_from_golden
    z = np.load(os.path.join(golden_dir, "collate_ref.npz"))
    raw = items_from_golden(z)
    ds = FastSpeech2Dataset(*S.write_dataset(str(tmp_path), raw, VALID_TOKENS))
    items = [ds[i] for i in range(len(ds))]
    store = FS2DeviceStore(ds, device=cuda)
    assert len(store) == len(raw) == 6 and store.n_mels == 80
    assert store.nbytes == 4 * store.buffer.numel() + 8 * store.ibuffer.numel()
    assert store.buffer.numel() == sum(82 * it["mel"].shape[1] for it in raw)
    assert store.table.shape == (7, 6) and torch.equal(store.table_d.cpu(),
                                                       torch.from_numpy(store.table))
    with pytest.raises(ValueError, match="max_bytes"):
        FS2DeviceStore(ds, device=cuda, max_bytes=store.nbytes - 1)
    assert FS2DeviceStore(ds, device=cuda, max_bytes=store.nbytes).nbytes == store.nbytes
    got = _check_store(cuda, store, items, list(range(6)))
    # speaker / emotion names map back to the fixture's ids, texts lose nothing: the reference's
    # own collate output
    for k, g in zip(S.NAMES, got):
        if k in ("labels", "wavs"):
            assert g == [str(s) for s in z["out_" + k].tolist()], k
        elif k not in ("speakers", "emotions"):
            assert np.array_equal(g.cpu().numpy(), z["out_" + k]), k
    _check_store(cuda, store, items, [4, 1, 1, 3])


# ------------------------------------------------------------------ 2: tile edges
FRAMES = (1, 63, 64, 65, 129)
PHONEMES = (2, 7, 1, 7, 2)                  # ties in phoneme length, counts {1, 2, 7}


@pytest.mark.parametrize("n_mels", [80, 3])
def test_tile_edges_ties_and_repeats(cuda, n_mels):
    from fastspeech2.device_store import FS2DeviceStore
    items = S.random_items(n_mels, FRAMES, PHONEMES, seed=n_mels)
    store = FS2DeviceStore(items, device=cuda)              # any sequence of item dicts
    offs = store.table[0]
    if n_mels == 3:
        assert (offs % 4 != 0).any()                        # unaligned bases
    for idx in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2], [4], [0], [3, 3, 0, 3, 1], [1, 3]):
        got = _check_store(cuda, store, items, idx)
        assert got[3].shape[1] == max(FRAMES[i] for i in idx)
    with pytest.raises(IndexError):
        store.collate([0, 5])
    with pytest.raises(IndexError):
        store.collate([-1])
    with pytest.raises(ValueError, match="empty"):
        store.collate([])
    with pytest.raises(ValueError, match="out"):
        store.collate([0, 1], out=Guarded(cuda, 2, 7, 64, n_mels).out)   # Tm is 63


def test_direct_call_on_a_shifted_store(cuda):
    """``ops.store_collate`` on a hand-packed store one float off its allocation, descriptors
    gathered on the host, a cache for rows 0 and 2 only."""
    from fastspeech2 import ops
    NM, E = 5, 3
    items = S.random_items(NM, (65, 7, 129, 64), (4, 2, 9, 5), seed=11)
    fbuf, ibuf, table = S.pack(items)
    rng = np.random.default_rng(1)
    cache = rng.standard_normal(1 + 4 * E + 9 * E).astype(np.float32)
    table[6] = (1, -1, 1 + 4 * E, -1)
    rows = [2, 3, 0, 1]                                     # batch-row order, as collate sorts
    want = S.gather(fbuf, ibuf, table, rows, [""] * 4, [""] * 4, NM)
    flat = torch.full((1 + fbuf.size + 1,), NAN, device=cuda)
    fstore = flat[1:1 + fbuf.size]
    fstore.copy_(torch.from_numpy(fbuf))
    assert fstore.data_ptr() % 16 == 4
    desc = torch.from_numpy(np.ascontiguousarray(table[:, rows])).to(cuda)
    B, Tp, Tm = 4, 9, 129
    g = Guarded(cuda, B, Tp, Tm, NM, E)
    o = g.out
    ops.store_collate(fstore, torch.from_numpy(ibuf).to(cuda), desc,
                      torch.from_numpy(cache).to(cuda), B, Tp, Tm, NM, E, o[0], o[5], o[1], o[2],
                      o[3], o[4], o[7], o[6], o[8])
    torch.cuda.synchronize()
    g.check()
    for k, i in (("phoneme", 0), ("input_lengths", 1), ("mel", 2), ("pitch", 3), ("energy", 4),
                 ("duration", 5), ("output_lengths", 6), ("rank_X", 7)):
        assert torch.equal(o[i].cpu(), torch.from_numpy(want[k])), k
    inten = np.zeros((B, Tp, E), np.float32)
    inten[0, :9] = cache[1 + 4 * E:].reshape(9, E)
    inten[2, :4] = cache[1:1 + 4 * E].reshape(4, E)
    assert torch.equal(o[8].cpu(), torch.from_numpy(inten))
    # a Tm beyond every utterance: zero padded (what cache_intensity asks for)
    g = Guarded(cuda, B, Tp, Tm + 16, NM)
    o = g.out
    ops.store_collate(fstore, torch.from_numpy(ibuf).to(cuda), desc, None, B, Tp, Tm + 16, NM, 0,
                      o[0], o[5], o[1], o[2], o[3], o[4], o[7], o[6], None)
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(o[7][:, :, :Tm].cpu(), torch.from_numpy(want["rank_X"]))
    assert not o[7][:, :, Tm:].any() and not o[2][:, Tm:].any()


# ------------------------------------------------------------------ 3: the cached intensity
def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-12)).item()


@pytest.fixture(scope="module")
def case():
    sd, items = S.intensity_case()
    # computed once, shared by both dtypes, never written to
    return sd, items, torch.from_numpy(S.oracle_rep(sd, items, max(S.CASE_FRAMES)))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cached_intensity_equals_in_batch_oracle(cuda, case, parity_log, dt):
    from fastspeech2.device_store import FS2DeviceStore, recompute_rows
    from fastspeech2.intensity import IntensityExtractor, get_intensity_representation
    sd, items, ref = case
    tol = S.TOL[dt]
    ext = IntensityExtractor(**S.EXT_KW, act_dtype=dt)
    ext.load_state_dict(sd)
    ext = ext.to(cuda)
    store = FS2DeviceStore(items, device=cuda)
    with pytest.raises(RuntimeError, match="cache_intensity"):
        store.collate(range(6), intensity=True, extractor=ext)
    store.cache_intensity(ext, batch_size=4)
    assert store.reach == S.REACH and store.cache.shape == (sum(S.CASE_PHONEMES), 5)
    assert store.table[6].tolist() == (5 * (np.cumsum(S.CASE_PHONEMES)
                                            - S.CASE_PHONEMES)).tolist()
    seen = []
    real = ext.forward
    ext.forward = lambda x, *a, **k: (seen.append(tuple(x.shape)), real(x, *a, **k))[1]
    idx = [3, 0, 5, 1, 4, 2]                                # the collate sorts it back
    g = Guarded(cuda, 6, 30, 120, 14, 5)
    batch, inten = store.collate(idx, out=g.out, intensity=True, extractor=ext)
    torch.cuda.synchronize()
    g.check()
    assert seen == [(3, 16, 120)]                           # exactly recompute_rows' three
    assert recompute_rows(batch[7].tolist(), S.REACH) == S.CASE_RECOMPUTED
    assert inten is g.out[8] and inten.dtype == torch.float32 and inten.shape == (6, 30, 5)
    _same_as_tuple(batch, store.collate(idx))
    err = rel(inten, ref)
    rows = [rel(inten[r], ref[r]) for r in range(6)]
    parity_log[f"fs2_store.cached_intensity.{g_name(dt)}"] = {"rel": err, "tol": tol,
                                                              "rel_by_row": rows}
    print(f"cached intensity {g_name(dt)}: rel {err:.3e}, by row {rows}")
    assert err < tol
    for r, n in enumerate(S.CASE_PHONEMES):
        assert not inten[r, n:].any()                       # exact zeros past phon_len
    # the unchanged in-batch path on the store's tuple
    del seen[:]
    full = get_intensity_representation(ext, batch)
    assert seen == [(6, 16, 120)]
    e_full = rel(full, ref)
    parity_log[f"fs2_store.in_batch_intensity.{g_name(dt)}"] = {"rel": e_full, "tol": tol}
    assert e_full < tol
    # a batch without its longest rows: other rows become the recomputed ones
    del seen[:]
    _, part = store.collate([3, 4, 5], intensity=True, extractor=ext)
    assert seen == [(1, 16, 104)]
    ref3 = S.oracle_rep(sd, items[3:], 104)
    assert rel(part, ref3) < tol
    # stale cache: a parameter changed in place
    ext.forward = real
    with torch.no_grad():
        ext.classifier.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="cache_intensity"):
        store.collate(idx, intensity=True, extractor=ext)
    store.collate(idx)                                      # the plain collate does not care
    store.cache_intensity(ext)
    store.collate(idx, intensity=True, extractor=ext)


def g_name(dt):
    return "fp32" if dt == torch.float32 else "bf16"


# ------------------------------------------------------------------ 4: an epoch
def test_train_one_epoch_equals_steps_by_hand(cuda, cfg_all):
    """Three steps of batch 2 over six utterances, 2+2 layers: the epoch's mean loss vector is
    the bits of ``trainer.step`` called by hand on ``store.collate`` outputs from the same
    initial weights and seeds, and so are the weights afterwards.

    The utterances have at most 32 frames on purpose.  The train step is run-to-run
    reproducible only then: the fused loss adds one partial per 16-frame tile into two float
    atomics per utterance (csrc/loss.hip, the SSIM normalisation sums), and a sum of up to two
    terms does not depend on their order, while one of three does (two runs of the
    step differ at rounding level).  With utterances of 36 to 90 frames the two runs of this
    test did differ, in the last digit of the mean loss.  Weight gradients here are unsplit."""
    from fastspeech2.device_store import FS2DeviceStore
    from fastspeech2.intensity import IntensityExtractor
    from fastspeech2.model import FastSpeech2
    from fastspeech2.train import FusedTrainer, train_one_epoch
    phon = [9, 12, 6, 11, 8, 10]
    frames = [27, 32, 13, 31, 20, 29]
    items = S.random_items(80, frames, phon, seed=3)
    store = FS2DeviceStore(items, device=cuda)
    torch.manual_seed(4)
    ext = IntensityExtractor(80, 2, 5, 2, 32, 9, 0.1).to(cuda)
    store.cache_intensity(ext)
    kw = dict(cfg_all["model"]["fastspeech2"], enc_num_layers=2, dec_num_layers=2)

    def trainer():
        torch.manual_seed(0)
        m = FastSpeech2(**kw, n_speakers=4).to(cuda).train()
        return m, FusedTrainer(m, lr=1e-4, graph=False)

    m1, t1 = trainer()
    mean = train_one_epoch(t1, store, 2, ext, shuffle=False)
    m2, t2 = trainer()
    by_hand = []
    for idx in ([0, 1], [2, 3], [4, 5]):
        batch, inten = store.collate(idx, intensity=True, extractor=ext)
        by_hand.append(t2.step(batch, inten, mel_len_max=batch[3].shape[1]).clone())
    assert t1.seed == t2.seed == 3
    assert mean.device.type == "cpu" and mean.shape == by_hand[0].shape
    assert torch.isfinite(mean).all()
    want = ((by_hand[0] + by_hand[1] + by_hand[2]) / 3).cpu()
    assert torch.equal(mean, want)
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1, p2), n
    # shuffled, with the in-batch extractor: the same batches in another order, finite
    m3, t3 = trainer()
    other = train_one_epoch(t3, store, 2, ext, shuffle=True,
                            generator=torch.Generator().manual_seed(1), cached=False)
    assert torch.isfinite(other).all() and t3.seed == 3
