"""CPU: the FastSpeech2 device store without a GPU.

* tests/fs2_store_restatement.py (pack the items as the store does, gather a batch back) equals
  ``oracle.collate_oracle.collate_np`` and the reference collate's own output
  (tests/golden/collate_ref.npz), which is what lets test_gpu_fs2_store.py use it;
* ``recompute_rows`` and ``epoch_order`` are pure host functions;
* the R-frame rule the intensity cache rests on, shown with the CPU oracle on the small config
  both cache tests use (``fs2_store_restatement.intensity_case``);
* ``fs2_store_collate`` refuses bad arguments before any launch; the header, the ctypes table
  and the library agree on the symbol; the store refuses a non-HIP device.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import fs2_store_restatement as S
from fastspeech2 import device_store as DS


def _same(got, want):
    for k in S.NAMES:
        if k in ("labels", "wavs"):
            assert list(got[k]) == [str(s) for s in want[k]], k
        else:
            w = np.asarray(want[k])
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
            assert np.array_equal(got[k], w), k


# ------------------------------------------------------------------ the restatement
def _restate(items, indices):
    fbuf, ibuf, table = S.pack(items)
    return S.gather(fbuf, ibuf, table, indices, [it["text"] for it in items],
                    [it["audio_path"] for it in items], items[0]["mel"].shape[0])


def test_restatement_equals_reference_collate_on_golden(golden_dir):
    from oracle.collate_oracle import collate_np, items_from_golden
    z = np.load(os.path.join(golden_dir, "collate_ref.npz"))
    items = items_from_golden(z)
    # the restatement's table rows are the store's
    assert (DS.F_OFF, DS.FRAMES, DS.I_OFF, DS.PHONEMES, DS.SPEAKER, DS.EMOTION, DS.C_OFF) \
        == tuple(range(7)) and S.pack(items)[2].shape == (7, len(items))
    got = _restate(items, range(len(items)))
    _same(got, {k: (z["out_" + k].tolist() if k in ("labels", "wavs") else z["out_" + k])
                for k in S.NAMES})
    _same(got, collate_np(items))
    assert len(set(z["out_input_lengths"].tolist())) < len(items)       # ties in phoneme length


@pytest.mark.parametrize("indices", [[0, 1, 2, 3, 4], [4, 2, 2, 0], [3]])
def test_restatement_equals_oracle_on_tile_edges(indices):
    from oracle.collate_oracle import collate_np
    items = S.random_items(3, (1, 63, 64, 65, 129), (2, 7, 1, 7, 2), seed=1)
    fbuf, _, table = S.pack(items)
    assert (table[0] % 4 != 0).any() and fbuf.size == 5 * sum((1, 63, 64, 65, 129))
    _same(_restate(items, indices), collate_np([items[i] for i in indices]))


# ------------------------------------------------------------------ recompute_rows
def test_recompute_rows():
    from fastspeech2.device_store import recompute_rows
    assert recompute_rows(S.CASE_FRAMES, S.REACH) == S.CASE_RECOMPUTED == [0, 1, 2]
    pads = [120 - f for f in S.CASE_FRAMES]
    assert pads[:4] == [0, 1, 15, 16]                  # pad exactly R is served from the cache
    assert recompute_rows([60, 120, 104, 105], 16) == [1, 3]            # any row order
    assert recompute_rows(S.CASE_FRAMES, 0) == []      # no convolution reach: all cached
    assert recompute_rows([77, 77, 77], 16) == [0, 1, 2]
    assert recompute_rows([77, 77, 77], 1) == [0, 1, 2]
    assert recompute_rows([5], 16) == [0]
    assert recompute_rows(np.array(S.CASE_FRAMES), 17) == [0, 1, 2, 3]


def test_extractor_reach():
    from fastspeech2.device_store import extractor_reach
    from fastspeech2.intensity import IntensityExtractor
    assert extractor_reach(IntensityExtractor(**S.EXT_KW)) == S.REACH
    assert extractor_reach(IntensityExtractor(80, 2, 5, 6, 16, 9, 0.1)) == 48
    assert extractor_reach(IntensityExtractor(80, 2, 5, 3, 16, 1, 0.1)) == 0


# ------------------------------------------------------------------ epoch_order
def test_epoch_order_sequential():
    from fastspeech2.device_store import epoch_order
    got = epoch_order(10, 4)
    assert [b.tolist() for b in got] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert [b.tolist() for b in epoch_order(10, 4, drop_last=True)] == [[0, 1, 2, 3],
                                                                        [4, 5, 6, 7]]
    assert epoch_order(0, 4) == [] and epoch_order(3, 4, drop_last=True) == []
    with pytest.raises(ValueError):
        epoch_order(10, 0)
    with pytest.raises(ValueError):
        epoch_order(10, 4, rank=2, world_size=2)


def test_epoch_order_shuffle_is_one_randperm():
    from fastspeech2.device_store import epoch_order
    perm = torch.randperm(23, generator=torch.Generator().manual_seed(7)).tolist()
    a = epoch_order(23, 5, shuffle=True, generator=torch.Generator().manual_seed(7))
    b = epoch_order(23, 5, shuffle=True, generator=torch.Generator().manual_seed(7))
    assert [x.tolist() for x in a] == [x.tolist() for x in b]
    assert [i for x in a for i in x.tolist()] == perm
    c = epoch_order(23, 5, shuffle=True, generator=torch.Generator().manual_seed(8))
    assert [x.tolist() for x in a] != [x.tolist() for x in c]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_order_ranks(world, drop_last):
    from fastspeech2.device_store import epoch_order
    n, bs = 23, 3
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist()
    shares = [epoch_order(n, bs, shuffle=True, generator=torch.Generator().manual_seed(5),
                          drop_last=drop_last, rank=r, world_size=world) for r in range(world)]
    assert len({len(s) for s in shares}) == 1                       # as many batches per rank
    for k in range(len(shares[0])):
        assert len({len(s[k]) for s in shares}) == 1                # of the same sizes
    sets = [set(i for b in s for i in b.tolist()) for s in shares]
    flat = [i for s in shares for b in s for i in b.tolist()]
    assert len(flat) == len(set(flat)) and len({len(s) for s in sets}) == 1     # disjoint, equal
    per = n // world
    kept = per // bs * bs if drop_last else per
    assert len(sets[0]) == kept
    for r, s in enumerate(shares):                                  # every world-th entry
        assert [i for b in s for i in b.tolist()] == perm[:per * world][r::world][:kept]
    if not drop_last:
        assert set(flat) == set(perm[:per * world])                 # all but the cut tail


# ------------------------------------------------------------------ the R-frame rule
@pytest.fixture(scope="module")
def case():
    return S.intensity_case()


def _rel(a, b, top):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / top)


def test_r_frame_rule(case):
    """The oracle extractor on the case's config (2 layers, k = 9: R = 16), values after
    ``phoneme_average_np``, errors relative to the in-batch result's largest magnitude (the
    GPU test's measure).

    fp32 rounding here is 2e-6: the same arithmetic at another padded length runs through
    differently blocked BLAS / softmax reductions (observed 1e-7 to 2.4e-7).  The sensitivity
    condition holds for both of the GPU test's tolerances with this seed: the longest row's
    pad-0 and pad->=R values differ by 0.14 > 3 * 3e-2 (bf16) > 3 * 1e-3 (fp32)."""
    sd, items = case
    Tm = max(S.CASE_FRAMES)
    ref = S.oracle_rep(sd, items, Tm)                       # the reference loop's in-batch value
    top = np.abs(ref).max()
    eps = 2e-6
    for r, it in enumerate(items):
        n, T = S.CASE_PHONEMES[r], S.CASE_FRAMES[r]
        at_R = S.oracle_rep(sd, [it], T + S.REACH)[0]
        far = S.oracle_rep(sd, [it], T + S.REACH + 40)[0]
        assert _rel(at_R, far, top) < eps, r               # the dependence saturates at R
        alone = S.oracle_rep(sd, [it], Tm)[0]               # rows do not see each other
        assert _rel(ref[r, :n], alone, top) < eps, r
        assert not ref[r, n:].any()
        # exactly the rows with at least R padded frames have the cached (pad >= R) value
        cached_ok = _rel(ref[r, :n], at_R, top) < eps
        assert cached_ok == (r not in S.CASE_RECOMPUTED), r
    # another batch around the same row: same value
    other = S.oracle_rep(sd, [items[3], items[0], items[5]], Tm)
    assert _rel(other[1], ref[0], top) < eps
    # the sensitivity condition of the GPU cache test
    pad0 = S.oracle_rep(sd, [items[0]], Tm)[0]
    padR = S.oracle_rep(sd, [items[0]], Tm + S.REACH)[0]
    sens = _rel(pad0, padR, top)
    print(f"pad 0 against pad R on the longest row: {sens:.3e}")
    assert sens > 3 * S.TOL[torch.bfloat16] > 3 * S.TOL[torch.float32]
    # one padded frame short of R is still another value, if only in the last digits
    assert np.abs(S.oracle_rep(sd, [items[2]], S.CASE_FRAMES[2] + S.REACH - 1)[0]
                  - S.oracle_rep(sd, [items[2]], S.CASE_FRAMES[2] + S.REACH)[0]).max() > 0


# ------------------------------------------------------------------ C ABI
def test_store_collate_host_validation():
    """Every call here is refused or empty: one that passed the checks would launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    ptrs = ("fstore", "istore", "desc", "cache", "phoneme", "duration", "in_len", "mel", "pitch",
            "energy", "rank_x", "out_len", "intensity")
    good = dict({n: p for n in ptrs}, B=2, Tp=3, Tm=5, n_mels=16, E=5)

    def call(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_store_collate(a["fstore"], a["istore"], a["desc"], a["cache"], a["B"],
                                     a["Tp"], a["Tm"], a["n_mels"], a["E"], a["phoneme"],
                                     a["duration"], a["in_len"], a["mel"], a["pitch"],
                                     a["energy"], a["rank_x"], a["out_len"], a["intensity"], None)

    for n in ptrs:
        if n != "cache":                               # no cache: a plain collate, it would launch
            assert call(**{n: None}) == -1, n
    assert call(n_mels=0) == -1 and call(n_mels=129) == -1
    assert call(B=-1) == -1 and call(Tp=-1) == -1 and call(Tm=-1) == -1
    assert call(B=65536) == -1 and call(E=0) == -1
    assert call(B=0) == 0 and call(Tm=0) == 0          # nothing to write: no launch


def test_store_collate_symbol_declared_bound_and_exported():
    from fastspeech2 import _native as N, ops
    src = open(os.path.join(ROOT, "include", "fs2_hip.h")).read()
    m = re.search(r"int\s+fs2_store_collate\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, "include/fs2_hip.h does not declare fs2_store_collate"
    n_args = m.group(1).count(",") + 1
    res, args = N.SIGNATURES["fs2_store_collate"]
    assert res is ctypes.c_int and len(args) == n_args == 19
    assert [a is ctypes.c_int for a in args] == [False] * 4 + [True] * 5 + [False] * 10
    assert hasattr(N.load(), "fs2_store_collate") and callable(ops.store_collate)


def test_public_names_and_device_refusal():
    import fastspeech2
    from fastspeech2 import device_store as DS
    from fastspeech2.train import train_one_epoch
    assert fastspeech2.FS2DeviceStore is DS.FS2DeviceStore and callable(train_one_epoch)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DS.FS2DeviceStore(None, device="cpu")
