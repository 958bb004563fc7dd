"""GPU parity of the attention kernels (csrc/flash.hip, csrc/attention.hip) against torch in
float64, at the launch variants, tile edges, mask shapes and row pitches the other files leave out.

Fused kernels (fs2_attn_fwd / fs2_attn_bwd, bf16).  Reference: float64 torch on the same bf16
input values, masks as ``test_fused_attention_vs_torch`` builds them, the dropout keep mask from
``_attn_keep_np``.  Metrics: the global ``rel`` (max error / max reference) and a per-(b, h) slab
version (max error in the slab / max(slab reference max, 0.1 * global reference max): slabs whose
rows have one valid key have an exactly zero dQ / dK reference).  Bounds on both: 2e-2 for ``out``,
3e-2 for dQ / dK / dV.  A float64 emulation that rounds the unnormalised P, dS and the outputs to
bf16 gives a slab error of 2.7e-3 .. 5.4e-3 (T = 17 .. 300, dh = 64 .. 256, dropout and hole
masks), so the bounds leave at least 3.7x over rounding alone.  ``lse * ln 2`` is compared with the
float64 logsumexp of the masked, scaled scores on every query row, absolute bound 5e-4: an error
d in lse is a relative error d in every probability the backward recomputes, and 5e-4 is a quarter
of the bf16 half-ulp 2^-9 those probabilities are rounded to anyway.  Every case pre-fills out,
lse, dqkv and the workspace with NaN, asserts finite results, and asserts that a second backward
call is bit-identical.  Every input set leaves each (b, h) a valid key (asserted on the reference
mask): fully masked rows are outside the fused kernels' contract.

Which case launches which instantiation (launch_fwd / launch_bwd, non-experiments build;
"small" = ceil(T/128)*B*H < 256, asserted per group):

  group B (small, B=3 H=2)         dh  64: attn_fwd<64,2,4>   attn_bwd_dq<64,2,4>   attn_bwd_dkv<64,4>
                                   dh 128: attn_fwd<128,2,4>  attn_bwd_dq<128,1,4>  attn_bwd_dkv<128,4>
                                   dh 192: attn_fwd<192,1,4>  attn_bwd_dq<192,1,4>  attn_bwd_dkv<192,4>
                                   dh 256: attn_fwd<256,1,4>  attn_bwd_dq<256,1,4>  attn_bwd_dkv<256,4>
  group A (large, B=32 H=4)  dh  64 T=129: attn_fwd<64,2,8>   attn_bwd_dq<64,2,8>   attn_bwd_dkv<64,8>
                             dh 128 T=129: attn_fwd<128,2,8>  attn_bwd_dq<128,1,8>  attn_bwd_dkv<128,8>
                             dh 192 T=257: attn_fwd<192,2,16> attn_bwd_dq<192,1,8>  attn_bwd_dkv<192,8>
                             dh 256 T=129: attn_fwd<256,1,8>  attn_bwd_dq<256,1,8>  attn_bwd_dkv<256,8>
  groups C, D, E run the dh = 64 / 192 small-block kernels (C3's B=32 repeat: the dh = 64 large ones).

Single-valid-key slabs and T = 1 are what found a fault: the backward took D = rowsum(dO * O)
from the bf16 O the forward stored.  With one valid key P = 1, so dS = dP - D was not zero but dO
dotted with the rounding of O (O = v / (1 - p) is no bf16 value under dropout; 2^-9 relative), times
a probability of 1: the dQ / dK slab figure of the four large-block cases was 3.2e-2 .. 4.1e-2 /
4.3e-2 .. 5.0e-2 against 3e-2 (6.9e-3 / 5.8e-3 over the slabs with more valid keys) and
max|dQ|, max|dK| at T = 1, dh = 64 were 1.24e-3 / 1.06e-3 of max|dV| against 1e-3; a float64
backward in which only O is rounded reproduced both.  The dQ kernel now takes D from the
unrounded probabilities where one key tile holds every valid key of the (b, h) (flash.hip), which
covers every case where a single key can carry the whole row at no cost; rows with more key tiles
keep D from the bf16 O, where the term is P_k times as large (all such cases here: below 7e-3).
``_slab_multikey`` (the slab figure over the slabs with more than one valid key) is logged beside
the asserted ones.

Materialised path (fs2_softmax_fwd / fs2_softmax_bwd, fp32 and bf16, both mask modes): P, the
dropped Pd and dS against float64, the zero pattern of Pd against the numpy keep mask exactly,
the padding columns [T, ldt) exactly zero, a fully masked row NaN as documented; and the fused
``out`` against Pd @ V of the materialised path under one seed and salt (the two paths draw the
same dropout mask).
"""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_ops import _attn_keep_np, rel

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD, TOL_LSE = 2e-2, 3e-2, 5e-4
SENTINEL = 3.0
NAN = float("nan")


@functools.lru_cache(maxsize=4)
def _keep(seed, salt, nrows, T, p):
    """numpy keep mask (nrows, T) of the attention dropout, shared by the cases of one grid"""
    k = _attn_keep_np(seed, salt, np.arange(nrows)[:, None], np.arange(T)[None, :], p)
    return torch.from_numpy(k)


def _prefix_pad(lens, T):
    pad = torch.zeros(len(lens), T, dtype=torch.bool)
    for b, L in enumerate(lens):
        assert 1 <= L <= T
        pad[b, L:] = True
    return pad


def _holes(pad):
    """masks that are no prefixes (key 150 stays valid everywhere): utterance 0 has its whole
    first K/V tile and six keys of the second masked, utterance 1 a whole interior tile,
    utterance 2 scattered single keys below its length"""
    assert pad.shape[1] >= 200 and not pad[:, 150].any()
    pad[0, 0:70] = True
    pad[1, 64:128] = True
    pad[2, [3, 17, 62, 63, 64, 100, 129, 151]] = True
    return pad


def _union_mask(pad, H, mask_mode):
    """(B, H, 1, T) bool: mask_mode 1 is the head-major tiling rule, 0 plain key padding"""
    B, T = pad.shape
    own = pad.repeat_interleave(H, 0)
    if mask_mode:
        b2 = [(b * H + h) % B for b in range(B) for h in range(H)]
        own = own | pad[b2]
    return own.view(B, H, 1, T)


def _slab_errs(got, ref, multi=None):
    """got (B*T, H*dh) kernel rows, ref (B, H, T, dh) float64 -> (global rel, worst slab rel);
    with ``multi`` (B, H) bool also the worst slab rel over those slabs only (0 if none)"""
    B, H, T, dh = ref.shape
    err = (got.double().view(B, T, H, dh).permute(0, 2, 1, 3) - ref).abs()
    gmax = ref.abs().max()
    slab = err.amax((2, 3)) / torch.maximum(ref.abs().amax((2, 3)), 0.1 * gmax)
    if multi is None:
        return (err.max() / gmax).item(), slab.max().item()
    return (err.max() / gmax).item(), slab.max().item(), (slab * multi).max().item()


def _log_max(parity_log, key, figs):
    old = parity_log.setdefault(key, {})
    for k, v in figs.items():
        old[k] = max(old.get(k, 0.0), v)


def _small_blocks(B, H, T):
    return -(-T // 128) * B * H < 256


def _ref64(qkv, dout, pad, B, H, T, dh, p_drop, mask_mode, seed, salt):
    """float64 attention on the given (bf16) values qkv [B*T][3D], dout [B*T][D], pad (B, T) on
    the device: (o, lse, q, k, v, mask), o and the leaves q, k, v (B, H, T, dh) with .grad set"""
    x = qkv.double().view(B, T, 3, H, dh)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3).clone().requires_grad_(True) for i in range(3))
    mask = _union_mask(pad, H, mask_mode)
    assert bool((~mask).any(-1).all()), "every (b, h) needs a valid key"
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh))
    sm = s.masked_fill(mask, float("-inf"))
    lse_ref = torch.logsumexp(sm.detach(), -1)
    P = torch.softmax(sm, -1)
    if p_drop > 0:
        keep = _keep(seed, salt, B * H * T, T, p_drop).view(B, H, T, T).to(qkv.device)
        P = P * keep / (1 - p_drop)
    o = P @ v
    o.backward(dout.double().view(B, T, H, dh).permute(0, 2, 1, 3))
    return o.detach(), lse_ref, q, k, v, mask


def _run_fused(cuda, parity_log, key, B, H, T, dh, p_drop, pad, mask_mode=1, ramp_k=False,
               gaps=(0, 0, 0, 0), seed=77, salt=5):
    """one fused forward + two backward calls against float64; returns (figures, float64 out)"""
    from fastspeech2 import ops
    assert B * H * T * T <= 128 * 257 * 257
    D = H * dh
    ldq, ldo, lddo, lddq = 3 * D + gaps[0], D + gaps[1], D + gaps[2], 3 * D + gaps[3]
    bf = torch.bfloat16
    torch.manual_seed(1000 * dh + 10 * T + B + H)
    vals = (torch.randn(B * T, 3 * D, device=cuda) * 0.5).to(bf)
    if ramp_k:   # the row maximum rises along the keys: the online-softmax rescale runs per tile
        ramp = torch.linspace(0.5, 6, T, device=cuda).repeat(B)[:, None]
        vals[:, D:2 * D] = (vals[:, D:2 * D].float() * ramp).to(bf)
    qkv = torch.full((B * T, ldq), NAN, device=cuda, dtype=bf)
    qkv[:, :3 * D] = vals
    dout = torch.full((B * T, lddo), NAN, device=cuda, dtype=bf)
    dout[:, :D] = torch.randn(B * T, D, device=cuda).to(bf)
    pad = pad.to(cuda)
    kp = pad.to(torch.uint8).contiguous()
    scale = 1.0 / math.sqrt(dh)

    o, lse_ref, q, k, v, mask = _ref64(qkv[:, :3 * D], dout[:, :D], pad, B, H, T, dh, p_drop,
                                       mask_mode, seed, salt)

    out = torch.full((B * T, ldo), NAN, device=cuda, dtype=bf)
    out[:, D:] = SENTINEL
    lse = torch.full((B * H, T), NAN, device=cuda)
    ops.attn_fwd(qkv, ldq, kp, B, H, T, dh, scale, p_drop, seed, salt, out, ldo, lse, dt=1,
                 mask_mode=mask_mode)
    assert bool(torch.isfinite(out[:, :D]).all()) and bool(torch.isfinite(lse).all())
    assert bool((out[:, D:] == SENTINEL).all()), "forward wrote into the pitch gap of out"
    out[:, D:] = NAN   # out is an input of the backward: its gap is never read

    def backward():
        dqkv = torch.full((B * T, lddq), NAN, device=cuda, dtype=bf)
        dqkv[:, 3 * D:] = SENTINEL
        ws = torch.full((int(ops.attn_ws(B, H, T)),), NAN, device=cuda)
        ops.attn_bwd(qkv, ldq, kp, out, ldo, dout, lddo, lse, B, H, T, dh, scale, p_drop, seed,
                     salt, dqkv, lddq, dt=1, ws=ws, mask_mode=mask_mode)
        return dqkv

    dqkv = backward()
    assert bool(torch.isfinite(dqkv[:, :3 * D]).all())
    assert bool((dqkv[:, 3 * D:] == SENTINEL).all()), "backward wrote into the pitch gap of dqkv"
    assert torch.equal(dqkv, backward()), "the backward is not repeatable"

    figs = {"lse": (lse.double().view(B, H, T) * math.log(2.0) - lse_ref).abs().max().item()}
    figs["out"], figs["out_slab"] = _slab_errs(out[:, :D], o)
    grads = {"dq": q.grad, "dk": k.grad, "dv": v.grad}
    multi = (~mask).sum(-1).view(B, H) > 1   # slabs with more than one valid key
    for i, (name, g) in enumerate(grads.items()):
        got = dqkv[:, i * D:(i + 1) * D]
        if T == 1 and name != "dv":
            # one key: P = 1 and the dQ / dK reference is exactly zero -- an absolute bound
            # against the size of dV
            assert float(g.abs().max()) == 0.0
            figs[name + "_abs_over_dv"] = (got.double().abs().max() / v.grad.abs().max()).item()
        else:
            figs[name], figs[name + "_slab"], figs[name + "_slab_multikey"] = _slab_errs(got, g, multi)
    print(key, (B, H, T, dh, p_drop, mask_mode), figs)
    _log_max(parity_log, key, figs)
    assert figs["lse"] <= TOL_LSE, figs
    assert figs["out"] < TOL_OUT and figs["out_slab"] < TOL_OUT, figs
    for name in grads:
        if name in figs:
            assert figs[name] < TOL_GRAD and figs[name + "_slab_multikey"] < TOL_GRAD, figs
    # the two checks that single-valid-key slabs decide (see the module docstring)
    for name in grads:
        if name in figs:
            assert figs[name + "_slab"] < TOL_GRAD, figs
        else:
            assert figs[name + "_abs_over_dv"] <= 1e-3, figs
    return figs, o


# ------------------------------------------------------------------ A: the large-block variants
def _lens_large(B, T):
    """one utterance at T, the rest spread down to 1, the tile-edge lengths among them"""
    fixed = [T, 128, 65, 64, 16, 1]
    n = B - len(fixed)
    spread = [2 + (i * (T - 4)) // (n - 1) for i in range(n)]
    return sorted(fixed + spread, reverse=True)


@pytest.mark.parametrize("dh,T", [(64, 129), (128, 129), (192, 257), (256, 129)])
def test_fused_attention_large_blocks(cuda, parity_log, dh, T):
    """128-row blocks (dh = 192 forward: 256-row) at every head size: a last block of one query /
    one key; most (b, h) have their last key block fully masked (the dK/dV kernel's skip path)
    and the ones tiled onto the one-key utterance have a single valid key."""
    B, H = 32, 4
    assert -(-T // 128) * B * H >= 256, "must not slip to the small-block kernels"
    lens = _lens_large(B, T)
    assert len(lens) == B and max(lens) == T and {1, 16, 64, 65, 128} <= set(lens)
    _run_fused(cuda, parity_log, "attn_large_blocks", B, H, T, dh, 0.1, _prefix_pad(lens, T))


# ------------------------------------------------------------------ B: tile edges, small blocks
_EDGES = ([(64, T, 0.1) for T in (1, 16, 17, 63, 64, 65, 127, 128, 129)] +
          [(dh, T, 0.1) for dh in (128, 192, 256) for T in (1, 17, 65, 129)] +
          [(192, 17, 0.0), (192, 129, 0.0)])


@pytest.mark.parametrize("dh,T,p_drop", _EDGES)
def test_fused_attention_tile_edges(cuda, parity_log, dh, T, p_drop):
    """T on and next to a 16-query group, a 64-key K/V tile and a 64-row block; T = 1;
    utterances shorter than one tile."""
    B, H = 3, 2
    assert _small_blocks(B, H, T)
    lens = [T, max(1, T - 5), max(1, T // 2)]
    _run_fused(cuda, parity_log, "attn_tile_edges", B, H, T, dh, p_drop, _prefix_pad(lens, T))


def test_fused_attention_tmax(cuda, parity_log):
    """T = 2048: the key-valid bytes fill their LDS array"""
    B, H, T = 1, 2, 2048
    assert _small_blocks(B, H, T)
    _run_fused(cuda, parity_log, "attn_tmax", B, H, T, 64, 0.1, _prefix_pad([T], T))


# ------------------------------------------------------------------ C: mask shapes
@pytest.mark.parametrize("dh", [192, 64])
def test_fused_attention_plain_key_padding(cuda, parity_log, dh):
    """mask_mode 0, forward and backward, at lengths where the tiling rule masks more: a kernel
    that ignores the flag is off by more than the bound"""
    B, H, T = 3, 2, 200
    assert _small_blocks(B, H, T)
    pad = _prefix_pad([200, 150, 90], T)
    assert not torch.equal(_union_mask(pad, H, 0), _union_mask(pad, H, 1))
    _, o0 = _run_fused(cuda, parity_log, "attn_mask_mode0", B, H, T, dh, 0.1, pad, mask_mode=0)
    _, o1 = _run_fused(cuda, parity_log, "attn_mask_mode1", B, H, T, dh, 0.1, pad, mask_mode=1)
    assert ((o0 - o1).abs().max() / o0.abs().max()).item() > 10 * TOL_OUT


@pytest.mark.parametrize("dh", [192, 64])
@pytest.mark.parametrize("B,H", [(3, 1), (1, 2), (3, 4), (4, 3), (5, 2)])
def test_fused_attention_tiling_rule(cuda, parity_log, B, H, dh):
    """(b*H + h) % B at other (B, H) than (3, 2), ascending lengths: a short utterance's padding
    lands on a longer one"""
    T = 200
    assert _small_blocks(B, H, T)
    lens = [T * (b + 1) // B for b in range(B)]
    _run_fused(cuda, parity_log, "attn_tiling_rule", B, H, T, dh, 0.1, _prefix_pad(lens, T))


@pytest.mark.parametrize("B,H,dh", [(3, 2, 192), (3, 2, 64), (32, 4, 64)])
@pytest.mark.parametrize("mask_mode", [0, 1])
def test_fused_attention_hole_masks(cuda, parity_log, B, H, dh, mask_mode):
    """masks that are no prefixes: fully masked leading tiles (the forward's running maximum
    stays -inf), a masked interior tile, scattered keys; B = 32 repeats it on the large blocks"""
    T = 200
    assert _small_blocks(B, H, T) == (B == 3)
    lens = [200, 180, 170] if B == 3 else [200 - (i * 49) // (B - 1) for i in range(B)]
    # key 150 is valid everywhere, utterance 2's holes lie below its length
    assert min(lens) >= 151 and lens[2] > 151
    _run_fused(cuda, parity_log, "attn_hole_masks", B, H, T, dh, 0.1,
               _holes(_prefix_pad(lens, T)), mask_mode=mask_mode)


# ------------------------------------------------------------------ D: row pitches
def test_fused_attention_row_pitches(cuda, parity_log):
    """ldq = 3D + 8, ldo = D + 8, lddo = D + 16, lddq = 3D + 24: NaN in the gap columns of every
    input, sentinels (checked in _run_fused) in the gap columns of out and dqkv"""
    B, H, T, dh = 3, 2, 150, 192
    _run_fused(cuda, parity_log, "attn_row_pitches", B, H, T, dh, 0.1,
               _prefix_pad([150, 113, 60], T), gaps=(8, 8, 16, 24))


# ------------------------------------------------------------------ E: rising row maximum
@pytest.mark.parametrize("dh,T", [(64, 129), (192, 300)])
def test_fused_attention_rising_row_max(cuda, parity_log, dh, T):
    """K rows scaled by linspace(0.5, 6, T) along the key index: the row maximum rises in every
    key tile, so the forward rescales its accumulator every tile and lse spans the whole range"""
    B, H = 3, 2
    lens = [T, T - 5, T // 2]
    _run_fused(cuda, parity_log, "attn_rising_row_max", B, H, T, dh, 0.1, _prefix_pad(lens, T),
               ramp_k=True)


# ------------------------------------------------------------------ F: materialised softmax
_SM_SHAPES = ([(3, H, T, False) for H in (2, 1) for T in (1, 37, 63, 64, 65, 130)] +
              [(3, 2, 200, True)])


@pytest.mark.parametrize("dt,code,tol", [(torch.float32, 0, 1e-5), (torch.bfloat16, 1, 2e-2)])
@pytest.mark.parametrize("mask_mode", [0, 1])
@pytest.mark.parametrize("B,H,T,holes", _SM_SHAPES)
def test_softmax_fwd_bwd_vs_float64(cuda, parity_log, B, H, T, holes, mask_mode, dt, code, tol):
    """fs2_softmax_fwd (P, and Pd at p = 0.1) and fs2_softmax_bwd (p = 0 and 0.1, fed the
    reference P rounded to the dtype) against float64; (Pd != 0) equals the numpy keep mask
    exactly; the padding columns [T, ldt) of P, Pd and dS come out exactly zero from NaN"""
    from fastspeech2 import ops
    ldt = ops.round_up(T, 8) + 8
    scale, p, seed, salt = 0.5, 0.1, 1234, 9
    torch.manual_seed(100 * T + 10 * H + mask_mode)
    lens = [200, 180, 170] if holes else [T, max(1, T - 5), max(1, T // 2)]
    pad = _prefix_pad(lens, T)
    if holes:
        pad = _holes(pad)
    pad = pad.to(cuda)
    kp = pad.to(torch.uint8).contiguous()
    mask = _union_mask(pad, H, mask_mode).view(B * H, 1, T)
    assert bool((~mask).any(-1).all())
    n = B * H * T

    def padded(x, dtype):
        buf = torch.full((B * H, T, ldt), NAN, device=cuda, dtype=dtype)
        if x is not None:
            buf[..., :T] = x.to(dtype)
        return buf

    S = padded(torch.randn(B * H, T, T, device=cuda) * 2, torch.float32)
    P, Pd = padded(None, dt), padded(None, dt)
    ops.softmax_fwd(S, kp, B, H, T, T, ldt, scale, p, seed, salt, P, Pd, dt=code,
                    mask_mode=mask_mode)
    assert bool((P[..., T:] == 0).all()) and bool((Pd[..., T:] == 0).all())
    Pref = torch.softmax((S[..., :T].double() * scale).masked_fill(mask, float("-inf")), -1)
    keep = _keep(seed, salt, n, T, p).view(B * H, T, T).to(cuda)
    figs = {"P": rel(P[..., :T], Pref), "Pd": rel(Pd[..., :T], Pref * keep / (1 - p))}
    live = ~mask.expand(-1, T, -1) & (P[..., :T] != 0)
    assert bool(live.any())
    assert torch.equal((Pd[..., :T] != 0)[live], keep[live])

    Pin = padded(Pref, dt)
    dPd = padded(torch.randn(B * H, T, T, device=cuda), torch.float32)
    Pq, g = Pin[..., :T].double(), dPd[..., :T].double()
    for pb in (0.0, p):
        dS = padded(None, dt)
        ops.softmax_bwd(dPd, Pin, B, H, T, T, ldt, scale, pb, seed, salt, dS, dt=code)
        assert bool((dS[..., T:] == 0).all())
        dP = g * keep / (1 - pb) if pb > 0 else g
        ref = scale * Pq * (dP - (Pq * dP).sum(-1, keepdim=True))
        figs["dS_p%g" % pb] = rel(dS[..., :T], ref)
    print("softmax", (B, H, T, holes, mask_mode, code), figs)
    _log_max(parity_log, "softmax_vs_float64_" + ("fp32" if code == 0 else "bf16"), figs)
    assert max(figs.values()) < tol, figs


def test_softmax_fully_masked_row_is_nan(cuda):
    """one row with every key masked (fp32): NaN in that row, as attention.hip documents and
    torch's softmax gives; every other row unaffected"""
    from fastspeech2 import ops
    B, H, Tq, Tk = 3, 1, 1, 37
    ldt = ops.round_up(Tk, 8) + 8
    torch.manual_seed(3)
    S = torch.randn(B * H, Tq, ldt, device=cuda)
    pad = torch.zeros(B, Tk, dtype=torch.bool, device=cuda)
    pad[0, 30:] = True
    pad[1, :] = True
    P = torch.full((B * H, Tq, ldt), 7.0, device=cuda)
    ops.softmax_fwd(S, pad.to(torch.uint8).contiguous(), B, H, Tq, Tk, ldt, 0.5, 0.0, 0, 1, P,
                    None, dt=0, mask_mode=0)
    ref = torch.softmax((S[..., :Tk].double() * 0.5).masked_fill(pad[:, None, :], float("-inf")), -1)
    assert bool(torch.isnan(ref[1]).all()) and bool(torch.isnan(P[1, :, :Tk]).all())
    assert bool((P[..., Tk:] == 0).all())
    assert rel(P[[0, 2], :, :Tk], ref[[0, 2]]) < 1e-5


# ------------------------------------------------------------------ G: the two paths agree
def test_fused_and_materialised_paths_agree(cuda, parity_log):
    """attention.hip: "the same draw as flash.hip" -- S = Q K^T by torch in fp32 through
    fs2_softmax_fwd (bf16, p = 0.1), Pd @ V against the fused out under the same seed and salt,
    and Pd's zero pattern against the numpy mask the fused reference uses"""
    from fastspeech2 import ops
    B, H, dh, T, p = 3, 2, 64, 130, 0.1
    D = H * dh
    seed, salt = 77, 5
    bf = torch.bfloat16
    torch.manual_seed(130)
    qkv = (torch.randn(B * T, 3 * D, device=cuda) * 0.5).to(bf)
    pad = _prefix_pad([130, 125, 65], T).to(cuda)
    kp = pad.to(torch.uint8).contiguous()
    scale = 1.0 / math.sqrt(dh)
    out = torch.full((B * T, D), NAN, device=cuda, dtype=bf)
    lse = torch.full((B * H, T), NAN, device=cuda)
    ops.attn_fwd(qkv, 3 * D, kp, B, H, T, dh, scale, p, seed, salt, out, D, lse, dt=1)

    x = qkv.float().view(B, T, 3, H, dh)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3).reshape(B * H, T, dh) for i in range(3))
    ldt = ops.round_up(T, 8)
    S = torch.zeros(B * H, T, ldt, device=cuda)
    S[..., :T] = q @ k.transpose(-1, -2)
    P = torch.full((B * H, T, ldt), NAN, device=cuda, dtype=bf)
    Pd = torch.full((B * H, T, ldt), NAN, device=cuda, dtype=bf)
    ops.softmax_fwd(S, kp, B, H, T, T, ldt, scale, p, seed, salt, P, Pd, dt=1)
    o2 = (Pd[..., :T].float() @ v).view(B, H, T, dh).permute(0, 2, 1, 3).reshape(B * T, D)
    keep = _keep(seed, salt, B * H * T, T, p).view(B * H, T, T).to(cuda)
    live = ~_union_mask(pad, H, 1).view(B * H, 1, T).expand(-1, T, -1) & (P[..., :T] != 0)
    assert torch.equal((Pd[..., :T] != 0)[live], keep[live])
    err = rel(out, o2)
    print("fused vs materialised", err)
    _log_max(parity_log, "attn_fused_vs_materialised", {"out": err})
    assert err < 2e-2


# ------------------------------------------------------------------ H: the engines' attention block
@pytest.mark.parametrize("mask_mode", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_block_both_paths_vs_float64(cuda, parity_log, p, mask_mode):
    """fastspeech2.attention (what every engine calls): forward and backward once on the fused
    path and once with it forced off, every buffer they are handed NaN-filled; out and dQKV on
    the rows of non-padded queries against float64, the materialised Pd's zero pattern against
    the numpy keep mask.  T = 130 crosses the 64- and 128-row tile edges and ldt = 136 != T."""
    from fastspeech2.attention import attention_bwd, attention_fwd, use_flash
    B, H, dh, T = 3, 2, 64, 130
    D = H * dh
    seed, salt = 77, 5
    bf = torch.bfloat16
    torch.manual_seed(130)
    qkv = (torch.randn(B * T, 3 * D, device=cuda) * 0.5).to(bf)
    dout = torch.randn(B * T, D, device=cuda).to(bf)
    pad = _prefix_pad([130, 125, 65], T).to(cuda)
    kp = pad.to(torch.uint8).contiguous()
    o, _, q, k, v, mask = _ref64(qkv, dout, pad, B, H, T, dh, p, mask_mode, seed, salt)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, D)
    want = {"out": rows(o), "dq": rows(q.grad), "dk": rows(k.grad), "dv": rows(v.grad)}
    live_q = ~pad.view(B * T)
    assert use_flash(T, dh, 1)
    empty = lambda *shape: torch.full(shape, NAN, device=cuda, dtype=bf)
    kw = dict(dt=1, dev=cuda, mask_mode=mask_mode, p_drop=p, seed=seed, salt=salt, empty=empty)
    for flash in (None, False):
        out, dqkv = empty(B * T, D), empty(B * T, 3 * D)
        saved = attention_fwd(qkv, kp, B, H, T, D, out, flash=flash, **kw)
        assert ("lse" in saved) == (flash is None)
        attention_bwd(qkv, kp, out, dout, saved, B, H, T, D, dqkv,
                      ws=lambda n: torch.full((int(n),), NAN, device=cuda), **kw)
        got = {"out": out, "dq": dqkv[:, :D], "dk": dqkv[:, D:2 * D], "dv": dqkv[:, 2 * D:]}
        figs = {n: rel(got[n][live_q], want[n][live_q]) for n in got}
        name = "attn_block_" + ("fused" if flash is None else "materialised")
        print(name, (p, mask_mode), figs)
        _log_max(parity_log, name, figs)
        assert figs["out"] < TOL_OUT, figs
        assert all(figs[n] < TOL_GRAD for n in ("dq", "dk", "dv")), figs   # a NaN fails
        if flash is None:
            continue
        Pm, Pd, ldt = saved["Pm"], saved["Pd"], saved["ldt"]
        assert ldt == 136 and Pm.shape == (B * H, T, ldt)
        if p == 0:
            assert Pd is Pm
            continue
        keep = _keep(seed, salt, B * H * T, T, p).view(B * H, T, T).to(cuda)
        live = ~mask.view(B * H, 1, T).expand(-1, T, -1) & (Pm[..., :T] != 0)
        assert bool(live.any())
        assert torch.equal((Pd[..., :T] != 0)[live], keep[live])
