"""The engine's conv / linear lowering, pinned without a GPU: the launch trace of the tree
(tests/lowering_trace.py) against the one recorded from the commit named in
tests/golden/engine_lowering.json, every traced fs2_gemm call through fs2_gemm_plan, and the
pure functions of fastspeech2/lowering.py on their own."""
import json
import os

import pytest

import lowering_trace
from conftest import GOLDEN
from fastspeech2 import lowering


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "engine_lowering.json")) as f:
        fx = json.load(f)
    assert fx["recorded_from"] and fx["cases"] and "plan_exceptions" in fx
    return fx


@pytest.fixture(scope="module")
def traced():
    gemms = {}
    cases = lowering_trace.trace(gemms)
    return json.loads(json.dumps(cases)), gemms


def test_trace_matches_recorded(recorded, traced):
    """every case launches, allocates and refuses what the recorded commit did, in order"""
    cases, _ = traced
    want = recorded["cases"]
    assert len(want) > 450 and sorted(cases) == sorted(want)
    diff = [k for k in want if cases[k] != want[k]]
    assert not diff, "\n".join(f"{k}\n  now      {cases[k]}\n  recorded {want[k]}" for k in diff[:5])
    # the recorded cases do reach every path and both refusals
    text = json.dumps(want)
    for needle in ("conv=(6, ", "conv=(4, ", "conv=(3, ", "conv=(1, ", "a_kw=9", "c_row=(977, -8)",
                   "accumulate=0)", "torch.add_", "k_eff=offs", "ValueError: ", "RuntimeError: "):
        assert needle in text, needle


def test_weight_images_match_recorded(recorded, traced):
    """the w_okc bits _weight_specs stores answer, for every weight of the default config under
    each setting of the two switches, what the recorded commit's _pad_dgrad, _tap_inner and
    _tap_inner_fwd answered"""
    import torch
    n = 0
    for adt, d in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        for sw in ((0, 0), (1, 0), (0, 1), (1, 1)):
            want = dict(recorded["cases"][f"images {d} sw{sw}"])
            with lowering_trace.switches(*sw):
                s = lowering_trace.make_stub(adt)
            assert want.pop("weights") == len(s._okc) == len(s._wspecs)
            for name, okc in s._okc.items():
                bits = "".join("01"[bool(okc & b)] for b in
                               (lowering.W_REV, lowering.W_TAP_INNER, lowering.W_TAP_INNER_FWD))
                assert bits == want.get(name, "000"), (name, d, sw)
                assert okc & 1 == int(s._wspecs[name][2] > 1)
                n += bits != "000"
    assert n == 12 * 4          # bf16 only: the 12 FFN conv1 weights under each setting


def test_traced_gemms_plan(recorded, traced):
    """fs2_gemm_plan accepts every traced gemm call and keeps the slice count of every call
    into split-K slices (no memset launch, eff_split's promise) -- but for the calls it
    refused or re-split at the recorded commit, which are listed there: T = P (reflect padding
    needs P < T), an odd row pitch in bf16 (the case that closes the K-major gate), the tap-inner
    forward past the 4-wave kernel's offsets (experiment switch), and concat_proj's forced 2
    slices over a single K-tile"""
    from fastspeech2 import _native
    _native.load()
    _, gemms = traced
    assert sum(map(len, gemms.values())) > 400
    assert sorted(lowering_trace.split_mismatches(gemms)) == recorded["plan_exceptions"]


def test_eff_split_leaves_no_slice_empty():
    for bk in (32, 64):
        for nkt in range(1, 4097):          # every K <= 4096 bk, by its K-tile count
            for K in (nkt * bk, nkt * bk - bk + 1):
                for ns in range(1, 33):
                    s = lowering.eff_split(K, ns, bk)
                    per = -(-nkt // s)                 # K-tiles per slice, as fs2_gemm rounds
                    assert 1 <= s <= ns and per * (s - 1) < nkt, (K, ns, bk, s)


def test_fp32_takes_no_slices():
    for args in ((31520, 384, 13824), (6656, 384, 13824), (31392, 512, 2560)):
        assert lowering.dgrad_split(*args, lowering.N.F32) == 1
        assert lowering.dgrad_split(*args, lowering.N.BF16) >= 1
    assert lowering.dgrad_split(6656, 384, 13824, lowering.N.BF16) == 3
    for args in ((384, 384, 384, 6400), (384, 1536, 1536, 6400), (512, 400, 400, 31264)):
        assert lowering.wgrad_slices(*args, lowering.N.F32) == 1
        assert lowering.wgrad_slices(*args, lowering.N.BF16) > 1


def test_rank_slices_values():
    """about one (128 x 128 tile, slice) unit per CU, >= 4 K-tiles a slice, as fs2_gemm rounds"""
    bf16, f32 = lowering.N.BF16, lowering.N.F32
    assert lowering.rank_slices(384, 384, 6400, bf16) == 25      # 9 tiles: 28 asked, 100 / 4 K-tiles
    assert lowering.rank_slices(384, 1536, 6400, bf16) == 7      # 36 tiles: 256 // 36
    assert lowering.rank_slices(80, 384, 31264, bf16) == 82      # 85 asked: 489 K-tiles in sixes
    assert lowering.rank_slices(1152, 384, 640, f32) == 5        # 20 K-tiles of 32, four each
    assert lowering.rank_slices(512, 2560, 8, bf16) == 1         # less than one K-tile


def test_ps_plain_ok_flips_at_int32_max():
    """each operand alone: accepted up to 2^31 - 2 bytes, refused from 2^31 - 1 on"""
    lim = 2 ** 31 - 1
    one = [1, 1, 1, 1, 1, 1]
    for k, unit in ((0, 2), (2, 2), (4, 1), (4, 2), (4, 4)):      # A, B (2 bytes), the output
        for field in (k, k + 1):                                    # rows, then the pitch
            a = list(one)
            a[field] = (lim - 1) // unit
            assert lowering.ps_plain_ok(*a, unit if k == 4 else 2), (k, unit, field)
            a[field] = -(-lim // unit)          # the first size of >= 2^31 - 1 bytes
            assert not lowering.ps_plain_ok(*a, unit if k == 4 else 2), (k, unit, field)
    assert lowering.ps_plain_ok(1, 1, 1, 1, lim - 1, 1, 1)          # 2^31 - 2 bytes
    assert not lowering.ps_plain_ok(1, 1, 1, 1, lim, 1, 1)          # exactly 2^31 - 1


def test_engine_reexports_are_lowerings():
    """one definition: the names the engine, ops and the rank trainer use are lowering's"""
    from fastspeech2 import engine, ops, rank_train
    for name in ("BK", "dgrad_split", "eff_split", "ps_plain_ok", "wgrad_slices", "round_up"):
        assert getattr(engine, name) is getattr(lowering, name)
    assert ops.EPC is lowering.EPC and ops.round_up is lowering.round_up
    assert rank_train.rank_slices is lowering.rank_slices
