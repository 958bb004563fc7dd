"""GPU: the rank-model data path (``fs2_rank_collate`` in csrc/collate.hip,
``fastspeech2.rank_dataset``) against the reference collate's own output
(tests/golden/rank_ref.npz ``bank.b{k}.*``) and, for the shapes the fixture lacks, against
tests/rank_collate_restatement.py (pinned to that output in test_rank_collate_host.py).

The collate is byte movement, so every comparison is bit-exact (``torch.equal``).  Every case
writes into NaN-prefilled outputs (int64: a sentinel) that sit inside larger prefilled
allocations, whose guard regions must be untouched afterwards.  The two model tests at the end
go from files to a prototype bank (fp32 bank tolerance 1e-4) and to
a training step whose losses and gradients must be the bits of the step on the fixture's tensors.
"""
import os

import numpy as np
import pytest
import torch

import rank_collate_restatement as RC
import rank_restatement as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -(2 ** 62)
GUARD = 257            # guard floats on each side (odd on purpose)
KEYS = ("emo_X", "neu_X", "speakers", "emotions", "length")


class Guarded:
    """Output tensors in the middle of prefilled allocations, ``shift`` floats off the
    allocation's alignment."""

    def __init__(self, cuda, B, T, C, shift=0):
        n = B * T * C
        lo = GUARD + shift
        self.flat = [torch.full((lo + n + GUARD,), NAN, device=cuda) for _ in range(2)]
        self.lflat = torch.full((8 + B + 8,), SENTINEL, dtype=torch.int64, device=cuda)
        self.lo, self.n, self.B = lo, n, B
        self.emo_X, self.neu_X = (f[lo:lo + n].view(B, T, C) for f in self.flat)
        self.length = self.lflat[8:8 + B]
        self.out = (self.emo_X, self.neu_X, self.length)

    def check(self):
        for f in self.flat:
            assert torch.isnan(f[:self.lo]).all() and torch.isnan(f[self.lo + self.n:]).all()
        assert bool((self.lflat[:8] == SENTINEL).all())
        assert bool((self.lflat[8 + self.B:] == SENTINEL).all())


def _equal(got, want, keys=KEYS):
    """got: the device dict; want: numpy arrays (restatement or fixture)."""
    for k in keys:
        w = torch.from_numpy(np.ascontiguousarray(want[k]))
        g = got[k]
        assert g.device.type == "cuda" and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), k
        assert g.dtype == (torch.float32 if k.endswith("_X") else torch.int64), k
        assert torch.equal(g.cpu(), w), k


def _collate_guarded(cuda, items, shift=0):
    from fastspeech2.rank_dataset import RankGpuCollate
    want = RC.collate_restatement(items)
    B, T, C = want["emo_X"].shape
    g = Guarded(cuda, B, T, C, shift)
    got = RankGpuCollate(cuda)(items, out=g.out)
    assert got["emo_X"] is g.emo_X and got["length"] is g.length
    g.check()
    _equal(got, want)
    return got, want


def _direct(cuda, items, T, pad_to=1, shift=0):
    """``ops.rank_collate`` on a store packed by hand: every array's base rounded up to
    ``pad_to`` floats, the store and the outputs ``shift`` floats into their allocations."""
    from fastspeech2 import ops
    B, C = len(items), items[0]["emo_X"].shape[0]
    chunks, desc, total = [], np.zeros((4, B), dtype=np.int64), 0
    for b, it in enumerate(items):
        for k, key in enumerate(("emo_X", "neu_X")):
            x = it[key]
            pad = -total % pad_to
            chunks.append(np.full(pad, np.nan, dtype=np.float32))
            total += pad
            desc[2 * k, b], desc[2 * k + 1, b] = total, x.shape[1]
            chunks.append(np.ascontiguousarray(x).reshape(-1))
            total += x.size
    flat = torch.full((shift + total + 1,), NAN, device=cuda)
    store = flat[shift:shift + total]
    store.copy_(torch.from_numpy(np.concatenate(chunks)))
    desc_d = torch.from_numpy(desc).to(cuda)
    g = Guarded(cuda, B, T, C, shift)
    ops.rank_collate(store, desc_d[0], desc_d[1], desc_d[2], desc_d[3], B, T, C, *g.out)
    torch.cuda.synchronize()
    g.check()
    return {"emo_X": g.emo_X, "neu_X": g.neu_X, "length": g.length}, desc


@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


# ------------------------------------------------------------------ 1
def test_fixture_batches_match_reference_collate(cuda, golden):
    from fastspeech2.rank_dataset import RankGpuCollate
    z = golden[0]
    items = RC.fixture_items(z)
    for k in range(int(z["bank.n_batches"])):
        batch = items[8 * k:8 * k + 8]
        got, _ = _collate_guarded(cuda, batch)
        ref = {key: z[f"bank.b{k}.{key}"] for key in KEYS}
        _equal(got, ref)
        _equal(RankGpuCollate(cuda)(batch), ref)          # outputs it allocates itself
    assert got["emo_X"].shape == (1, 27, 16) and got["length"].tolist() == [19]


# ------------------------------------------------------------------ 2
def test_tile_edges_and_degenerate_items(cuda):
    items = RC.random_items(82, (65, 1, 64), (63, 130, 64), seed=2)
    got, want = _collate_guarded(cuda, items)
    assert got["emo_X"].shape == (3, 130, 82)             # three 64-frame tiles
    assert want["length"].tolist() == [63, 1, 64] and got["length"].tolist() == [63, 1, 64]


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("C", [3, 130])
def test_channel_bounds(cuda, C):
    items = RC.random_items(C, (5, 70), (70, 5), seed=C)
    got, want = _collate_guarded(cuda, items)
    assert got["emo_X"].shape == (2, 70, C) and want["length"].tolist() == [5, 5]


# ------------------------------------------------------------------ 4
def test_unaligned_bases_equal_the_aligned_run(cuda):
    C = 5
    items = RC.random_items(C, (7, 65, 3, 129), (9, 1, 67, 131), seed=4)
    assert all((C * it[k].shape[1]) % 2 == 1 for it in items for k in ("emo_X", "neu_X"))
    T = 131
    want = RC.collate_restatement(items)
    aligned, desc_a = _direct(cuda, items, T, pad_to=4, shift=0)
    odd, desc_o = _direct(cuda, items, T, pad_to=1, shift=1)
    assert not (desc_a[[0, 2]] % 4).any() and (desc_o[[0, 2]] % 4).any()
    assert aligned["emo_X"].data_ptr() % 16 != odd["emo_X"].data_ptr() % 16
    for k in ("emo_X", "neu_X", "length"):
        assert torch.equal(aligned[k], odd[k]), k
    _equal(odd, want, keys=("emo_X", "neu_X", "length"))


# ------------------------------------------------------------------ 5
def test_rows_sharing_one_neutral_item(cuda, monkeypatch):
    from fastspeech2 import rank_dataset as RD
    items = RC.random_items(16, (20, 70, 40, 33), (40, 40, 40, 12), seed=5)
    shared = items[0]["neu_X"]
    for it in items[:3]:
        it["neu_X"] = shared                               # 20 < 40, 70 > 40, 40 == 40
    seen = []
    real = RD.ops.rank_collate
    monkeypatch.setattr(RD.ops, "rank_collate",
                        lambda store, *a: (seen.append(store.numel()), real(store, *a))[1])
    got, want = _collate_guarded(cuda, items)
    assert want["length"].tolist() == [20, 40, 40, 12]
    distinct = [it["emo_X"] for it in items] + [shared, items[3]["neu_X"]]
    assert seen == [sum(x.size for x in distinct)]         # the shared array is packed once
    for b in range(3):
        n = int(want["length"][b])
        assert torch.equal(got["neu_X"][b, :n].cpu(), torch.from_numpy(shared[:, :n].T.copy()))


# ------------------------------------------------------------------ 6
def test_zero_and_clamped_lengths(cuda):
    items = RC.random_items(16, (0, 9, 70), (12, 0, 66), seed=6)
    got, want = _collate_guarded(cuda, items)
    assert want["length"].tolist() == [0, 0, 66]
    assert not got["emo_X"][:2].any() and not got["neu_X"][:2].any()
    # every item empty: T = 0, nothing to launch, length still defined
    got, want = _collate_guarded(cuda, RC.random_items(16, (0, 0), (0, 0)))
    assert got["emo_X"].shape == (2, 0, 16) and got["length"].tolist() == [0, 0]
    # T passed smaller than the lengths: length = T, nothing written past T (the guards)
    items = RC.random_items(16, (10, 70, 3), (12, 66, 80), seed=7)
    for T in (6, 64, 65):
        res, _ = _direct(cuda, items, T)
        want = RC.collate_restatement(items, T=T)
        assert want["length"].tolist() == [min(10, T), min(66, T), 3]
        _equal(res, want, keys=("emo_X", "neu_X", "length"))
    # a negative length on the device counts as 0
    from fastspeech2 import ops
    store = torch.randn(16 * 8, device=cuda)
    off = torch.zeros(2, dtype=torch.int64, device=cuda)
    el = torch.tensor([-3, 8], device=cuda)
    nl = torch.tensor([8, 8], device=cuda)
    g = Guarded(cuda, 2, 8, 16)
    ops.rank_collate(store, off, el, off, nl, 2, 8, 16, *g.out)
    g.check()
    assert g.length.tolist() == [0, 8] and not g.emo_X[0].any() and not g.neu_X[0].any()
    assert torch.equal(g.emo_X[1], store.view(16, 8).t()) and torch.equal(g.emo_X[1], g.neu_X[1])


# ------------------------------------------------------------------ 7-9: from files
@pytest.fixture(scope="module")
def files_case(golden, tmp_path_factory):
    """The fixture's raw arrays as a preprocessed dataset on disk: one file per distinct array,
    lines of a speaker sharing its neutral files.  Returns (dataset, floats in distinct files)."""
    from fastspeech2.rank_dataset import FineGrainedDataset
    z = golden[0]
    root = str(tmp_path_factory.mktemp("rank_preprocessed"))
    speakers, emotions = z["speakers"].tolist(), z["emotions"].tolist()
    items = RC.fixture_items(z)
    for spk in speakers:
        os.makedirs(os.path.join(root, spk))
    neutral, lines, floats = {}, [], 0
    for i, it in enumerate(items):
        spk, emo = speakers[it["speaker"]], emotions[it["emotion"]]
        RC.write_utterance(os.path.join(root, spk, f"{emo}_{i}.npz"), it["emo_X"])
        floats += it["emo_X"].size
        key = (spk, it["neu_X"].tobytes())
        if key not in neutral:
            neutral[key] = sum(1 for k in neutral if k[0] == spk)
            RC.write_utterance(os.path.join(root, spk, f"neutral_{neutral[key]}.npz"),
                               it["neu_X"])
            floats += it["neu_X"].size
        lines.append(f"{spk}|{emo}|{i}|{neutral[key]}")
    assert len(neutral) < len(items)                        # lines do share neutral files
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return FineGrainedDataset(root, speakers, emotions, split="train"), floats, len(neutral)


@pytest.fixture(scope="module")
def store(cuda, files_case):
    from fastspeech2.rank_dataset import RankDeviceStore
    return RankDeviceStore(files_case[0], device=cuda)


def test_store_collate_equals_gpu_collate(cuda, golden, files_case, store):
    from fastspeech2.rank_dataset import RankDeviceStore, RankGpuCollate
    ds, floats, n_neutral = files_case
    z = golden[0]
    assert len(store) == len(ds) == 25
    assert store.n_files == 25 + n_neutral
    assert store.nbytes == 4 * floats == 4 * store.buffer.numel()   # distinct files, not lines
    assert 4 * floats < 4 * int(z["bank.raw_emo"].size + z["bank.raw_neu"].size)
    with pytest.raises(ValueError, match="max_bytes"):
        RankDeviceStore(ds, device=cuda, max_bytes=store.nbytes - 1)
    assert RankDeviceStore(ds, device=cuda, max_bytes=store.nbytes).nbytes == store.nbytes
    collate = RankGpuCollate(cuda)
    for idx in (list(range(8)), list(range(24, 15, -1)), [3, 3, 17, 3, 0], [24]):
        items = [ds[i] for i in idx]
        want = RC.collate_restatement(items)
        B, T, C = want["emo_X"].shape
        g = Guarded(cuda, B, T, C)
        got = store.collate(idx, out=g.out)
        g.check()
        _equal(got, want)
        other = collate(items)
        for k in KEYS:
            assert torch.equal(got[k], other[k]), (idx, k)
    # the loader's order: the fixture's four batches
    batches = list(store.batches(8))
    assert len(batches) == 4 and len(list(store.batches(8, drop_last=True))) == 3
    for k, b in enumerate(batches):
        _equal(b, {key: z[f"bank.b{k}.{key}"] for key in KEYS})
    gen = torch.Generator().manual_seed(0)
    perm = torch.randperm(25, generator=torch.Generator().manual_seed(0)).tolist()
    shuffled = list(store.batches(8, shuffle=True, generator=gen))
    for k, b in enumerate(shuffled):
        _equal(b, RC.collate_restatement([ds[i] for i in perm[8 * k:8 * k + 8]]))


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-12)).item()


def test_files_to_bank_fp32(cuda, golden, store):
    from fastspeech2.intensity import RankModel
    from fastspeech2.rank import bucketize
    z, kw, sd = golden
    m = RankModel(**kw, act_dtype=torch.float32)
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    for k, b in enumerate(store.batches(8)):
        B, T, C = b["emo_X"].shape
        g = Guarded(cuda, B, T, C)
        again = store.collate(range(8 * k, 8 * k + B), out=g.out)
        g.check()
        for key in KEYS:
            assert torch.equal(again[key], b[key]), (k, key)
        _, _, I, _, h, _, r, _ = m(b["emo_X"], b["neu_X"], b["emotions"], b["length"],
                                   torch.ones(2, B, device=cuda))
        for name, got in (("I", I), ("h", h), ("r", r)):
            e = rel(got, z[f"bank.b{k}.{name}"])
            print(f"files to bank: batch {k} {name} rel {e:.3e}")
            assert e < 1e-4, (k, name, e)
    n_spk, n_emo, K = len(z["speakers"]), len(z["emotions"]), int(z["bucket_size"])
    bank = bucketize(m, store.batches(8), n_spk, n_emo, K)
    ref = z["bank.bank"]
    assert bank.dtype == np.float32 and bank.shape == ref.shape
    e = rel(bank, ref)
    print(f"files to bank: bank rel {e:.3e}")
    assert e < 1e-4


def test_files_to_training_step_bits(cuda, golden, store):
    """One ``rank_train_step`` (fp32, dropout 0.1, fixed seed and lambdas) on
    ``store.collate(range(8))`` and on the fixture's ``bank.b0.*`` uploaded with torch: the
    engine has no atomics and the inputs are the same bits, so losses and gradients are too."""
    from fastspeech2.rank_train import RankTrainLoss, TrainableRankModel, rank_train_step
    z, kw, sd = golden
    lambdas = torch.rand(2, 8, generator=torch.Generator().manual_seed(9)).to(cuda)
    g = Guarded(cuda, *z["bank.b0.emo_X"].shape)
    from_store = dict(store.collate(range(8)), lambdas=lambdas)
    guarded = store.collate(range(8), out=g.out)
    g.check()
    for k in KEYS:
        assert torch.equal(guarded[k], from_store[k]), k
    from_fixture = {k: torch.from_numpy(z[f"bank.b0.{k}"]).contiguous().to(cuda) for k in KEYS}
    from_fixture["lambdas"] = lambdas
    runs = []
    for batch in (from_store, from_fixture):
        m = TrainableRankModel(**dict(kw, dropout=0.1), act_dtype=torch.float32)
        m.load_state_dict(sd)
        m = m.to(cuda).train()
        m._step_seed = 4321
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        losses = rank_train_step(m, RankTrainLoss(0.1, 1.0), opt, batch)
        assert m.last_dropout[0] == (4321 * 1103515245 + 12345) & 0x7fffffff
        runs.append((losses, {k: p.grad.clone() for k, p in m.named_parameters()}))
    (la, ga), (lb, gb) = runs
    for a, b in zip(la, lb):
        assert torch.isfinite(a) and torch.equal(a, b)
    assert set(ga) == set(gb) and len(ga) > 10
    for k in ga:
        assert torch.isfinite(ga[k]).all(), k
        assert torch.equal(ga[k], gb[k]), k
    assert ga["projector.weight"].any() and ga["intensity_extractor.input_proj.weight"].any()
