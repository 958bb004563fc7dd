"""CPU: host logic of the product package and the C ABI (no kernel launches).

* libfs2_hip.so loads and exports every function include/fs2_hip.h declares;
* host-side argument validation of fs2_gemm (returns before any launch);
* the drop-in module's constructor, parameter count and state_dict keys equal the oracle's
  (SB naming) and identical init under the same seed;
* synthetic batches have the reference collate's layout (dataset.py:62-133);
* algorithmic FLOP count matches SURVEY.md section 8d;
* data-parallel gradient bucketing is contiguous and complete.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _header_functions():
    src = open(os.path.join(ROOT, "include", "fs2_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fs2_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from fastspeech2 import _native
    lib = _native.load()
    declared = _header_functions()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), name
    assert set(declared) == set(_native.SIGNATURES), "ctypes table out of sync with the header"
    assert lib.fs2_version().startswith(b"fs2_hip")


def test_library_built_from_this_tree_and_stale_build_refused(monkeypatch):
    """fs2_source_hash (Makefile buildinfo) equals the hash of the tree's csrc + header, and
    a library whose hash differs from the tree's is refused at load (no stale build runs)."""
    from fastspeech2 import _native
    lib = _native.load()
    tree = _native.source_hash()
    assert tree is not None and len(tree) == 16
    assert lib.fs2_source_hash().decode() == tree
    monkeypatch.setattr(_native, "source_hash", lambda: "0" * 16)
    with pytest.raises(_native.NativeLibraryError, match="other sources"):
        _native.load(_native.LIB_PATH)


def test_source_hash_follows_every_csrc_header(tmp_path, monkeypatch):
    """source_hash() covers every header of csrc/, not one known by name: a change to any of them
    changes the hash, so a library built before the change is refused as stale."""
    import shutil
    from fastspeech2 import _native
    csrc = shutil.copytree(_native._CSRC, tmp_path / "csrc",
                           ignore=shutil.ignore_patterns("build*"))
    inc = shutil.copytree(os.path.dirname(_native._HEADER), tmp_path / "include")
    monkeypatch.setattr(_native, "_CSRC", str(csrc))
    monkeypatch.setattr(_native, "_HEADER", str(inc / "fs2_hip.h"))
    headers = sorted(csrc.glob("*.h"))
    assert {"fs2_common.h", "fs2_launch.h", "fs2_cdna.h"} <= {h.name for h in headers}
    seen = {_native.source_hash()}
    for h in headers:
        with open(h, "a") as fh:
            fh.write(" ")
        now = _native.source_hash()
        assert now not in seen, h.name
        seen.add(now)


def test_gemm_host_validation_rejects_bad_args():
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    d = N.GemmDesc(M=16, N=16, K=12, dtype=N.BF16, A=p16, lda=16, a_kmajor=1, B=p16, ldb=16,
                   b_kmajor=1, C=p16, ldc=16)
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # K not a multiple of 8 (bf16)
    d.K, d.lda = 16, 12
    assert lib.fs2_gemm(ctypes.byref(d), None) == -2          # pitch not 16-byte aligned
    d.lda, d.conv_mode, d.conv_t, d.conv_kw, d.conv_c = 16, 1, 3, 9, 16
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # reflect pad 4 >= T=3
    d.conv_mode = 0
    d.A = p16 + 2
    assert lib.fs2_gemm(ctypes.byref(d), None) == -2          # misaligned pointer
    d.A = p16
    d.split_k, d.c_fp32 = 2, 0
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # split-K needs an fp32 output
    d.split_k = 1
    # tap-inner K order (a_kw): K must equal a_kw * lda with lda % 64 == 0, K-major, no conv
    d.M, d.N, d.K, d.lda, d.ldb, d.a_kw = 16, 16, 9 * 48, 48, 9 * 48, 9
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # lda 48 % 64 != 0
    d.K, d.lda, d.ldb, d.a_kw = 9 * 64, 64, 9 * 64, 8
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # K != a_kw * lda
    d.a_kw, d.conv_mode, d.conv_t, d.conv_kw, d.conv_c = 9, 1, 16, 9, 64
    assert lib.fs2_gemm(ctypes.byref(d), None) == -1          # no implicit conv with a_kw
    d.conv_mode, d.a_kw = 0, 0
    assert lib.fs2_loss_fwd_bwd(None, None) == -1


def _gemm_plan_cases():
    """(descriptor on a 16-byte-aligned host buffer, recorded answer) for every case of
    tests/golden/gemm_plans.json (sweep) and gemm_plan_sites.npz (call sites), the dispatcher's
    decisions recorded from commit 10745b4"""
    import json
    import numpy as np
    from fastspeech2 import _native as N
    golden = os.path.join(ROOT, "tests", "golden")
    fx = json.load(open(os.path.join(golden, "gemm_plans.json")))
    assert fx["recorded_from"] == "10745b4"
    fields = dict(N.GemmDesc._fields_)
    assert fx["desc_fields"] == list(fields)
    sites = np.load(os.path.join(golden, "gemm_plan_sites.npz"))
    rows = list(zip(sites["desc"].tolist(), sites["ans"].tolist()))
    for sp, *ans in fx["sweep"]:
        r = list(fx["desc_defaults"])
        for i, v in zip(sp[::2], sp[1::2]):
            r[i] = v
        rows.append((r, ans))
    buf = (ctypes.c_char * 64)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    cases = []
    for r, (rc, k, *rest) in rows:
        d = N.GemmDesc()
        for (name, ty), v in zip(d._fields_, r):
            if ty is not ctypes.c_void_p:
                setattr(d, name, v)
            elif v >= 0:                            # -1 = NULL: absent
                setattr(d, name, base + v)
        cases.append((d, (rc, fx["kernels"][k] if k >= 0 else "", *rest)))
    return buf, cases


def test_gemm_plan_matches_recorded():
    """fs2_gemm_plan returns, for every recorded descriptor, the code, kernel, grid, block and
    rewritten tiling / split fields the dispatcher of commit 10745b4 chose (recorded at its
    launch points): the bench step's and the GPU suite's call sites, a sample of a 50 000
    descriptor sweep with every reachable instantiation and error return, and pairs on either
    side of the thresholds"""
    from fastspeech2 import _native as N
    lib = N.load()
    buf, cases = _gemm_plan_cases()
    assert len(cases) > 2500 and len({a[1] for _, a in cases}) >= 48
    for d, want in cases:
        i = N.GemmPlanInfo()
        rc = lib.fs2_gemm_plan(ctypes.byref(d), ctypes.byref(i))
        got = (rc, i.kernel.decode(), *i.grid, i.block, i.tiles_m, i.tiles_n, i.split_k,
               i.k_per_split, i.vec_ok, i.accumulate)
        assert got == want, {n: getattr(d, n) for n, _ in d._fields_ if getattr(d, n)}


def test_gemm_plan_agrees_with_gemm_on_errors():
    """fs2_gemm and fs2_gemm_plan return the same code for every recorded descriptor that was
    refused (fs2_gemm returns before any launch there)"""
    from fastspeech2 import _native as N
    lib = N.load()
    buf, cases = _gemm_plan_cases()
    bad = [(d, a[0]) for d, a in cases if a[0] != 0]
    assert {rc for _, rc in bad} == {-1, -2} and len(bad) > 50
    for d, rc in bad:
        assert lib.fs2_gemm(ctypes.byref(d), None) == rc
        assert lib.fs2_gemm_plan(ctypes.byref(d), ctypes.byref(N.GemmPlanInfo())) == rc


def test_gemm_plan_is_pure():
    """planning twice gives identical output and leaves the descriptor untouched"""
    from fastspeech2 import _native as N
    lib = N.load()
    buf, cases = _gemm_plan_cases()
    for d, _ in cases[::7]:
        before = bytes(d)
        a, b = N.GemmPlanInfo(), N.GemmPlanInfo()
        ctypes.memset(ctypes.byref(b), 0xff, ctypes.sizeof(b))      # every byte of the output is written
        assert lib.fs2_gemm_plan(ctypes.byref(d), ctypes.byref(a)) == \
            lib.fs2_gemm_plan(ctypes.byref(d), ctypes.byref(b))
        assert bytes(a) == bytes(b) and bytes(d) == before
    assert lib.fs2_gemm_plan(ctypes.byref(cases[0][0]), None) == -1


def test_attention_host_validation_rejects_bad_args():
    """fs2_attn_fwd / fs2_attn_bwd / fs2_softmax_fwd / fs2_softmax_bwd return before any launch
    on bad arguments.  Every call here must be refused: one that passed the checks would launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    good = dict(qkv=p16, ldq=3 * 2 * 64, key_pad=p16, B=2, H=2, T=16, dh=64, out=p16, ldo=128,
                dout=p16, lddo=128, lse=p16, dqkv=p16, lddq=3 * 2 * 64, ws=p16, dtype=N.BF16)

    def fwd(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_attn_fwd(a["qkv"], a["ldq"], a["key_pad"], 1, a["B"], a["H"], a["T"],
                                a["dh"], 0.125, 0.1, 1, 2, a["out"], a["ldo"], a["lse"],
                                a["dtype"], None)

    def bwd(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_attn_bwd(a["qkv"], a["ldq"], a["key_pad"], 1, a["out"], a["ldo"], a["dout"],
                                a["lddo"], a["lse"], a["B"], a["H"], a["T"], a["dh"], 0.125, 0.1,
                                1, 2, a["dqkv"], a["lddq"], a["ws"], a["dtype"], None)

    for call in (fwd, bwd):
        assert call(dtype=N.F32) == -1                        # bf16 only
        assert call(T=0) == -1 and call(T=2049) == -1         # 1 <= T <= 2048
        assert call(B=0) == -1
        assert call(dh=96) == -1                              # head sizes 64 / 128 / 192 / 256
        for name in ("key_pad", "out", "lse"):
            assert call(**{name: None}) == -1, name
        assert call(qkv=p16 + 2) == -2                        # misaligned pointer
        assert call(ldq=3 * 2 * 64 + 4) == -2                 # pitch not 16-byte aligned
        assert call(ldq=3 * 2 * 64 - 8) == -2                 # pitch below q | k | v
    assert bwd(ws=None) == -1
    for name in ("out", "dout", "dqkv"):
        assert bwd(**{name: p16 + 2}) == -2, name
    for name in ("ldo", "lddo", "lddq"):
        assert bwd(**{name: good[name] + 4}) == -2, name

    for dh in (64, 128, 192, 256):
        assert lib.fs2_attn_supported(2048, dh, N.BF16) == 1
    assert lib.fs2_attn_supported(2049, 64, N.BF16) == 0
    assert lib.fs2_attn_supported(2048, 96, N.BF16) == 0
    assert lib.fs2_attn_supported(2048, 64, N.F32) == 0

    def sm_fwd(B=3, Tk=16, ldt=16, dtype=N.F32):
        return lib.fs2_softmax_fwd(p16, p16, 1, B, 2, 16, Tk, ldt, 0.5, 0.1, 1, 2, p16, p16,
                                   dtype, None)

    def sm_bwd(B=3, Tk=16, ldt=16, dtype=N.F32):
        return lib.fs2_softmax_bwd(p16, p16, B, 2, 16, Tk, ldt, 0.5, 0.1, 1, 2, p16, dtype, None)

    for call in (sm_fwd, sm_bwd):
        assert call(Tk=17) == -1                              # ldt < Tk
        assert call(dtype=7) == -1                            # unknown dtype
        assert call(B=0) == 0                                 # an empty batch is a no-op


def test_layernorm_host_validation_rejects_bad_args():
    """fs2_ln_fwd / fs2_ln_bwd / fs2_sum_slices return FS2_EINVAL before any launch on bad
    arguments, and 0 for an empty problem.  Every other call here must be refused: one that
    passed the checks would launch."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    good = dict(x=p16, y=p16, gamma=p16, beta=p16, mean=p16, rstd=p16, dy=p16, s=p16, ds=p16,
                dgamma=None, dbeta=None, dcol=None, ws=None, img=None, img_t=0, img_p=0,
                M=16, D=64, dtype=N.BF16)

    def fwd(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_ln_fwd(a["x"], a["D"], None, 0, 0.0, 0, None, a["gamma"], a["beta"], 1e-5,
                              0, 0.1, 3, None, None, 0, a["y"], a["D"], a["mean"], a["rstd"],
                              a["M"], a["D"], a["dtype"], 1, a["img"], a["img_t"], a["img_p"], None)

    def bwd(**bad):
        a = dict(good, **bad)
        assert bad, "a call without a fault would launch"
        return lib.fs2_ln_bwd(a["dy"], a["D"], a["s"], a["D"], a["mean"], a["rstd"], a["gamma"],
                              a["beta"], 0, 0.1, 3, None, 0, a["ds"], a["D"], None, 0.0, 0,
                              a["dgamma"], a["dbeta"], a["dcol"], a["M"], a["D"], a["dtype"], 1,
                              a["ws"], None)

    for call in (fwd, bwd):
        assert call(D=0) == -1 and call(D=1025) == -1         # 1 <= D <= 1024
        assert call(dtype=7) == -1                            # fp32 and bf16 only
        assert call(M=0) == 0 and call(M=-3) == 0             # an empty problem is a no-op
        assert call(M=0, D=0, gamma=None, mean=None) == 0     # ... whatever else is passed
        for name in ("gamma", "mean"):
            assert call(**{name: None}) == -1, name
    for name in ("x", "y"):
        assert fwd(**{name: None}) == -1, name
    assert bwd(ds=None) == -1
    assert bwd(dgamma=p16, ws=p16) == -1                      # dgamma without dbeta
    assert bwd(dbeta=p16, ws=p16) == -1
    assert bwd(dgamma=p16, dbeta=p16) == -1                   # sums without a workspace
    assert bwd(dcol=p16) == -1
    # the padded image of y: bf16 only, whole utterances, pad below the length, 8-column chunks
    assert fwd(img=p16, img_t=8, img_p=2, dtype=N.F32) == -1
    assert fwd(img=p16, img_t=5, img_p=2) == -1               # M % img_t != 0
    assert fwd(img=p16, img_t=8, img_p=8) == -1               # img_p >= img_t
    assert fwd(img=p16, img_t=8, img_p=2, D=60) == -1         # D % 8 != 0

    def slices(ws=p16, nslices=2, stride=64, n=64, out=p16):
        return lib.fs2_sum_slices(ws, nslices, stride, n, out, 1, None)

    assert slices(n=62) == -1 and slices(stride=66) == -1     # n, stride multiples of 4
    assert slices(nslices=0) == -1
    assert slices(ws=p16 + 4) == -1 and slices(out=p16 + 8) == -1   # 16-byte aligned pointers
    assert slices(ws=None) == -1 and slices(out=None) == -1
    assert slices(n=0) == 0


def test_every_entry_point_refuses_an_unknown_dtype():
    """Every entry point that takes a dtype, called with dtype = 2 (neither FS2_F32 = 0 nor
    FS2_BF16 = 1) and otherwise valid arguments -- non-zero sizes, non-null 16-byte aligned
    addresses that are never followed -- returns FS2_EINVAL before any launch; the dtype arms of
    a launcher are written once, so this is the arm neither activation mode reaches.
    fs2_attn_supported is a predicate and answers 0."""
    from fastspeech2 import _native as N
    lib = N.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    BAD = 2
    assert BAD not in (N.F32, N.BF16)
    calls = {
        "fs2_conv_fold": (p, 1, 0, 2, 16, 1, 64, p, 64, p, 64, p, p, BAD, None),
        "fs2_pad_transpose": (p, 64, 2, 16, 64, 1, 1, p, 128, 128, None, None, BAD, None),
        "fs2_pad_transpose_bounded": (p, 64, 2, 16, 64, 1, 1, p, 128, 128, None, None, p, 1, BAD,
                                      None),
        "fs2_pad_rows": (p, 64, 2, 16, 64, 1, 1, 0, p, 64, BAD, None),
        "fs2_colsum": (p, 64, 16, 64, BAD, p, 0, p, None),
        "fs2_ln_fwd": (p, 64, None, 0, 0.0, 0, None, p, p, 1e-5, 0, 0.1, 3, None, None, 0, p, 64,
                       p, p, 16, 64, BAD, 1, None, 0, 0, None),
        "fs2_ln_bwd": (p, 64, p, 64, p, p, p, p, 0, 0.1, 3, None, 0, p, 64, None, 0.0, 0, None,
                       None, None, 16, 64, BAD, 1, None, None),
        "fs2_softmax_fwd": (p, p, 1, 2, 2, 16, 16, 16, 0.5, 0.1, 1, 2, p, p, BAD, None),
        "fs2_softmax_bwd": (p, p, 2, 2, 16, 16, 16, 0.5, 0.1, 1, 2, p, BAD, None),
        "fs2_attn_fwd": (p, 384, p, 1, 2, 2, 16, 64, 0.125, 0.1, 1, 2, p, 128, p, BAD, None),
        "fs2_attn_bwd": (p, 384, p, 1, p, 128, p, 128, p, 2, 2, 16, 64, 0.125, 0.1, 1, 2, p, 384,
                         p, BAD, None),
        "fs2_attn_bwd_bounded": (p, 384, p, 1, p, 128, p, 128, p, 2, 2, 16, 64, 0.125, 0.1, 1, 2,
                                 p, 384, p, p, BAD, None),
        "fs2_embed_fwd": (p, p, p, 0, 2, 16, 64, p, p, BAD, None),
        "fs2_embed_bwd": (p, p, p, 32, 64, 8, p, p, BAD, None),
        "fs2_concat_fwd": (p, p, p, p, 2, 16, 64, 4, p, 136, BAD, None),
        "fs2_concat_bwd_spk": (p, 136, p, 2, 16, 64, 4, p, BAD, p, None),
        "fs2_mask_rows": (p, 64, p, 16, 64, BAD, None),
        "fs2_add3_mask_rows": (p, p, p, 64, p, 16, 64, BAD, None),
        "fs2_rowdot_fwd": (p, 64, p, p, 1.0, 16, 64, p, BAD, None),
        "fs2_rowdot_bwd": (p, p, 64, p, 1.0, 16, 64, p, p, p, BAD, p, None),
        "fs2_embed1d_fwd": (p, p, p, p, 2, 16, 64, 3, p, BAD, None),
        "fs2_embed1d_bwd": (p, p, 2, 16, 64, 3, p, p, BAD, p, None),
        "fs2_lr_gather": (p, p, p, 2, 8, 16, 64, p, p, BAD, None),
        "fs2_lr_scatter": (p, p, p, 2, 8, 16, 64, p, BAD, None),
        "fs2_weight_prep": (p, 16, 16, 3, 0, p, 48, p, 48, BAD, None),
        "fs2_weight_prep_batched": (p, 1, 1, BAD, None),
        "fs2_adamw_prep": (p, 1, 1, p, 1, 1, p, p, p, p, 1.0, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8,
                           1.0, BAD, None),
        "fs2_intensity_input": (p, 1, 2, 16, 80, p, 96, BAD, None),
        "fs2_intensity_head": (p, 64, p, p, p, p, p, 2, 16, 64, 4, p, BAD, None),
        "fs2_rank_mixup_input": (p, p, p, 2, 16, 80, p, 96, BAD, None),
        "fs2_gelu_dropout_fwd": (p, 64, 0, p, 64, p, 64, 16, 64, 0.1, 1, 2, BAD, None),
        "fs2_gelu_dropout_bwd": (p, 64, p, 64, p, 64, 16, 64, 0.1, 1, 2, BAD, None),
        "fs2_intensity_head_bwd": (p, p, 64, p, p, 4, p, p, 2, 16, 64, 4, p, 64, p, p, p, p, BAD,
                                   None),
        "fs2_vocoder_input": (p, 2, 80, 16, 3, p, 96, BAD, None),
        "fs2_leaky_relu": (p, p, 64, 0.1, BAD, None),
        "fs2_mean3_leaky_relu": (p, p, p, p, 64, 0.1, BAD, None),
        "fs2_fill": (p, 64, 0.0, BAD, None),
        "fs2_add": (p, p, 64, 1.0, BAD, None),
    }
    for name, args in calls.items():
        assert len(args) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name)(*args) == -1, name
    for src, dst in ((BAD, N.F32), (N.BF16, BAD), (BAD, BAD)):
        assert lib.fs2_cast(p, src, p, dst, 64, None) == -1, (src, dst)
    assert lib.fs2_attn_supported(16, 64, BAD) == 0
    # the descriptors' dtype: the GEMM's checks take every dtype but bf16 for fp32 and its planner
    # refuses it; the loss refuses it after its pointer checks
    g = N.GemmDesc(M=16, N=16, K=16, dtype=BAD, A=p, lda=16, a_kmajor=1, B=p, ldb=16, b_kmajor=1,
                   C=p, ldc=16)
    assert lib.fs2_gemm(ctypes.byref(g), None) == -1
    assert lib.fs2_gemm_plan(ctypes.byref(g), ctypes.byref(N.GemmPlanInfo())) == -1
    ld = N.LossDesc(B=2, Tm=16, Tp=8, NM=80, dtype=BAD,
                    **{f: p for f, t in N.LossDesc._fields_ if t is ctypes.c_void_p})
    assert lib.fs2_loss_fwd_bwd(ctypes.byref(ld), None) == -1
    # every prototype with a dtype parameter is covered above
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fs2_hip.h")).read(),
                 flags=re.S)
    takes = {n for n, a in re.findall(r"\b(fs2_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
             if re.search(r"\bint (src_)?dtype\b", a)}
    assert takes == set(calls) | {"fs2_cast", "fs2_attn_supported"}


def test_ctypes_argument_counts_match_header():
    """every prototype in include/fs2_hip.h has as many parameters as its ctypes signature in
    fastspeech2/_native.py (a parameter added on one side only shifts every later argument)"""
    from fastspeech2 import _native
    src = open(os.path.join(ROOT, "include", "fs2_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in re.findall(r"\b(fs2_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = args.strip()
        n = 0 if args in ("", "void") else args.count(",") + 1
        assert n == len(_native.SIGNATURES[name][1]), name


def _tiny_cfg():
    return dict(enc_num_layers=2, enc_num_head=2, enc_d_model=32, enc_ffn_dim=64, enc_k_dim=32,
                enc_v_dim=32, enc_dropout=0.1, dec_num_layers=2, dec_num_head=2, dec_d_model=32,
                dec_ffn_dim=64, dec_k_dim=32, dec_v_dim=32, dec_dropout=0.1,
                normalize_before=False, ffn_type="1dcnn", ffn_cnn_kernel_size_list=[9, 1],
                n_char=20, n_mels=16, postnet_embedding_dim=32, postnet_kernel_size=5,
                postnet_n_convolutions=5, postnet_dropout=0.5, padding_idx=0,
                dur_pred_kernel_size=3, pitch_pred_kernel_size=3, energy_pred_kernel_size=3,
                variance_predictor_dropout=0.5)


def test_dropin_module_matches_oracle_keys_and_init(cfg_all):
    from fastspeech2.model import FastSpeech2
    from oracle.fs2_oracle import FastSpeech2Oracle
    kw = cfg_all["model"]["fastspeech2"]
    torch.manual_seed(0)
    o = FastSpeech2Oracle(**kw, n_speakers=4)
    torch.manual_seed(0)
    m = FastSpeech2(**kw, n_speakers=4)
    so, sm = o.state_dict(), m.state_dict()
    assert list(so) == list(sm)
    for k in so:
        assert so[k].shape == sm[k].shape and torch.equal(so[k], sm[k]), k
    assert sum(p.numel() for p in m.parameters()) == 85_295_299
    # reference checkpoints interchange
    m.load_state_dict(o.state_dict())


def test_backward_groups_contiguous_and_complete():
    """Flat layout = backward-completion order; group ranges tile the buffer."""
    from fastspeech2.model import FastSpeech2, _group_key, group_tag
    m = FastSpeech2(**_tiny_cfg(), n_speakers=4)
    names = [n for n, _ in m.named_parameters()]
    keys = sorted({_group_key(n, 2, 2) for n in names})
    tags = [group_tag(k) for k in keys]
    # a group may hold several sort keys (the variance group orders the duration / pitch
    # conv1 weights and biases first, adjacent): consecutive keys share its tag
    tags = [t for i, t in enumerate(tags) if i == 0 or t != tags[i - 1]]
    assert tags == ["postnet", "linear", "decoder.layers.1", "decoder.layers.0", "variance",
                    "conditioning", "encoder.layers.1", "encoder.layers.0", "prenet"]


def test_grad_bucketer_partition():
    from fastspeech2.train import GradBucketer
    flat = torch.zeros(1000)
    ranges = [("a", 0, 100), ("b", 100, 400), ("c", 400, 420), ("d", 420, 1000)]
    bk = GradBucketer(flat, ranges, bucket_bytes=300 * 4)
    assert bk.buckets == [(0, 400, "b"), (400, 1000, "d")]
    cover = sorted((s, e) for s, e, _ in bk.buckets)
    assert cover[0][0] == 0 and cover[-1][1] == 1000
    assert all(cover[i][1] == cover[i + 1][0] for i in range(len(cover) - 1))


def test_synthetic_batch_layout():
    from fastspeech2.synthetic import make_batch
    b = make_batch(B=8, seed=3)
    pl = b["phon_len"]
    assert torch.all(pl[:-1] >= pl[1:])                       # collate sorts descending
    assert torch.equal(b["duration"].sum(1), b["mel_len"])    # durations sum to mel length
    assert int(b["mel_len"].max()) == b["mel"].shape[1] <= 1000
    for i in range(8):
        L, P = int(b["mel_len"][i]), int(pl[i])
        assert torch.all(b["phoneme"][i, :P] > 0) and torch.all(b["phoneme"][i, P:] == 0)
        assert torch.all(b["mel"][i, L:] == 0) and torch.all(b["pitch"][i, L:] == 0)
        assert torch.all(b["intensity"][i, P:] == 0)
    mx = make_batch(B=4, max_shape=True)
    assert mx["mel"].shape[1] == 1000 and mx["phoneme"].shape[1] == 200


def test_flop_count_matches_survey(cfg_all):
    from fastspeech2.model import FastSpeech2
    from fastspeech2.flops import forward_flops
    m = FastSpeech2(**cfg_all["model"]["fastspeech2"], n_speakers=4)
    f = forward_flops(m.cfg, 1, 200, 1000)
    assert abs(f / 1e9 - 112.9) < 0.5     # 112.9 GFLOP per utterance forward


def test_get_intensity_rep_prototype_lookup():
    """fastspeech2/inference.py:12-21 as called at :76 (integer emo_id): the prototype bank
    lookup expanded over the phonemes for EVERY emotion id, neutral (id 0) included -- the
    reference's `emotion == 'neutral'` string test never matches an int.  Only the string
    'neutral' (that dead branch) gives zeros, with n_emotions (=5) channels instead of 256."""
    import numpy as np
    from fastspeech2.inference import get_intensity_rep
    bank = np.random.default_rng(0).standard_normal((4, 5, 3, 5)).astype(np.float32)
    n = get_intensity_rep(1, 0, 2, 7, bank)
    assert n.shape == (1, 7, 5)
    assert torch.equal(n[0, 3], torch.from_numpy(bank[1, 0, 2]))
    z = get_intensity_rep(1, "neutral", 2, 7, bank)
    assert z.shape == (1, 7, 5) and torch.all(z == 0)
    r = get_intensity_rep(2, 3, 1, 7, bank)
    assert r.shape == (1, 7, 5)
    assert torch.equal(r[0, 4], torch.from_numpy(bank[2, 3, 1]))


@pytest.mark.parametrize("u", [8, 2])
def test_vocoder_polyphase_transposed_conv(u):
    """fastspeech2.vocoder.polyphase_weights: ConvTranspose1d(k=2u, stride u, padding u/2) ==
    a 3-tap zero-padded conv whose u output phases are stacked along the channel axis (the
    form the GEMM runs, conv_mode 5)."""
    import torch.nn.functional as F
    from fastspeech2.vocoder import polyphase_weights
    torch.manual_seed(u)
    C, O, L = 6, 5, 9
    W, b, x = torch.randn(C, O, 2 * u), torch.randn(O), torch.randn(2, C, L)
    ref = F.conv_transpose1d(x, W, b, stride=u, padding=u // 2)
    W3 = polyphase_weights(W, u).reshape(u * O, 3, C).permute(0, 2, 1)
    y = F.conv1d(x, W3, b.repeat(u), padding=1)
    y = y.reshape(2, u, O, L).permute(0, 2, 3, 1).reshape(2, O, L * u)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)


def _hazard_checker():
    import importlib.util
    p = os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd", "csrc", "check_hazards.py")
    spec = importlib.util.spec_from_file_location("check_hazards", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mfma_hazard_checker_flags_early_reads():
    """check_hazards (run by build()): an accumulator read 3 wait states after the asm MFMA that
    writes it is flagged, one behind an s_nop 15 / s_nop 3 drain is not, and an accumulate chain
    on the same range needs no wait states."""
    hz = _hazard_checker()
    head = "0000000000001000 <_ZN12gemm_w4b_kernelILb0ELi8EEEv>:\n"
    mfma = "  v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]\n"
    early = head + mfma + mfma + "  v_add_u32_e32 v9, 1, v9\n  s_nop 1\n  v_accvgpr_read_b32 v10, a2\n"
    late = head + mfma + "  s_nop 15\n  s_nop 3\n  v_accvgpr_read_b32 v10, a2\n"
    f = hz.check(early, hz.MIN_WAIT)
    assert len(f) == 1 and f[0][1] == 3 and "a2" in f[0][3]
    assert hz.check(late, hz.MIN_WAIT) == []


def test_built_objects_have_no_mfma_hazards():
    """the gfx950 code of the built library objects passes the hazard check (skipped before a
    build: the objects are not in the repository)"""
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd", "csrc",
                                         "build", "*.o")))
    if not objs:
        pytest.skip("library not built")
    hz = _hazard_checker()
    assert hz.main(objs) == 0


def test_fused_adamw_state_remaps_moments_by_name():
    """FusedAdamW.state_dict records the flat layout (name, offset, numel); a state saved under
    another parameter order (e.g. before the predictor conv1 pair moved to the front of the
    variance group) loads with every parameter's moments at its current offset, and a state whose
    names differ is refused instead of loading the moments onto the wrong parameters"""
    from fastspeech2.optim import FusedAdamW

    class _Packed:   # the flat-buffer view of a model (FastSpeech2 packs only on a HIP device)
        _layout = [(f"p{i}", 16 * i * (i + 1) // 2, 16 * (i + 1), None, None) for i in range(6)]
        _flat = torch.zeros(16 * 21)

        def _ensure_packed(self):
            pass

    m = _Packed()
    opt = FusedAdamW(m)
    lay = opt._layout_record()
    # an "old" layout: the first two parameters swapped in the flat buffer
    (n0, o0, k0), (n1, o1, k1) = lay[0], lay[1]
    old_lay = [(n1, o0, k1), (n0, o0 + k1, k0)] + [tuple(x) for x in lay[2:]]
    old_avg = torch.zeros_like(opt.exp_avg)
    old_sq = torch.zeros_like(opt.exp_avg_sq)
    want_avg = torch.zeros_like(opt.exp_avg)
    for i, (n, o, k) in enumerate(old_lay):
        old_avg[o:o + k] = float(i + 1)
        old_sq[o:o + k] = float(-(i + 1))
    cur = {n: (o, k) for n, o, k in lay}
    for i, (n, o, k) in enumerate(old_lay):
        co, _ = cur[n]
        want_avg[co:co + k] = float(i + 1)
    opt.load_state_dict({"step": 7, "exp_avg": old_avg, "exp_avg_sq": old_sq, "layout": old_lay})
    assert opt.step_count == 7
    assert torch.equal(opt.exp_avg, want_avg) and torch.equal(opt.exp_avg_sq, -want_avg)
    # same layout: a plain copy; round trip through state_dict
    sd = opt.state_dict()
    opt2 = FusedAdamW(m)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.exp_avg, opt.exp_avg)
    bad = dict(sd, layout=[("nope", o, k) for _, o, k in sd["layout"]])
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)
