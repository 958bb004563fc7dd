"""The host side of one multi-head self-attention block, forward and backward, for every engine
(``engine.FS2Engine``, ``intensity.ExtractorEngine``, ``rank_train.RankTrainEngine``).

From ``QKV [M][3D]`` (M = B*T token rows; Q, K, V in column blocks of D = H*dh) either the fused
kernels (``fs2_attn_fwd`` / ``fs2_attn_bwd``: no (B*H, T, T) tensor, ``lse`` kept) or the
materialised path: S = Q K^T, ``fs2_softmax_fwd`` into the probabilities Pm and their dropped
copy Pd, Pd V; backwards dPd, dV, ``fs2_softmax_bwd``, dQ, dK.  The callers differ in
``mask_mode`` (1: FastSpeech2's head-major tiling rule, 0: plain key padding), the dropout triple
and where memory comes from: ``empty(*shape)`` allocates in the activation dtype, ``ws(n)`` hands
out n fp32 words of scratch.  Nothing here waits for the device (the FastSpeech2 step is captured).
"""

import contextlib
import math

import torch

from . import _native as N
from . import ops
from .ops import round_up


def use_flash(T, dh, dt):
    """fused attention kernels on the bf16 path (fp32 parity mode keeps the materialised
    softmax)."""
    return dt == N.BF16 and ops.attn_supported(T, dh, dt)


def attention_fwd(QKV, key_pad, B, H, T, D, out, *, dt, dev, mask_mode, p_drop, seed, salt, empty,
                  flash=None, timed=contextlib.nullcontext()):
    """out [M][D] = attention over QKV [M][3D].  Returns what ``attention_bwd`` needs:
    ``{"lse"}`` from the fused path, ``{"Pm", "Pd", "ldt"}`` from the materialised one (Pd is Pm
    at p_drop = 0).  ``flash``: None decides by ``use_flash``, as every engine does; the tests
    alone pass True / False, to put both paths on one shape.  ``timed``: a context manager entered
    around exactly the fused kernel's launch (a caller's timer)."""
    dh = D // H
    scale = 1.0 / math.sqrt(dh)
    if use_flash(T, dh, dt) if flash is None else flash:
        lse = torch.empty(B * H, T, dtype=torch.float32, device=dev)
        with timed:
            ops.attn_fwd(QKV, 3 * D, key_pad, B, H, T, dh, scale, p_drop, seed, salt, out, D, lse,
                         dt=dt, mask_mode=mask_mode)
        return {"lse": lse}
    ldt = round_up(T, 8)
    S = torch.empty(B * H, T, ldt, dtype=torch.float32, device=dev)
    ops.gemm(T, T, dh, QKV, 3 * D, QKV[:, D:], 3 * D, S, ldt, dt=dt, c_fp32=1,
             batch=B * H, batch_div=H,
             strides=(T * 3 * D, dh, T * 3 * D, dh, H * T * ldt, T * ldt, 0, 0))
    Pm = empty(B * H, T, ldt)
    Pd = empty(B * H, T, ldt) if p_drop > 0 else Pm
    ops.softmax_fwd(S, key_pad, B, H, T, T, ldt, scale, p_drop, seed, salt, Pm,
                    Pd if p_drop > 0 else None, dt=dt, mask_mode=mask_mode)
    del S
    ops.gemm(T, dh, ldt, Pd, ldt, QKV[:, 2 * D:], 3 * D, out, D, dt=dt, b_kmajor=0,
             kvalid=T, batch=B * H, batch_div=H,
             strides=(H * T * ldt, T * ldt, T * 3 * D, dh, T * D, dh, 0, 0))
    return {"Pm": Pm, "Pd": Pd, "ldt": ldt}


def attention_bwd(QKV, key_pad, out, dout, saved, B, H, T, D, dQKV, *, dt, dev, mask_mode, p_drop,
                  seed, salt, empty, ws, q_bound=None, timed=contextlib.nullcontext()):
    """dQKV [M][3D] from dout [M][D], the forward's ``out`` and what it returned (``saved``).
    ``q_bound`` (int32 [B], see ``ops.attn_bwd``) reaches the fused kernel only; ``timed`` as in
    ``attention_fwd``."""
    dh = D // H
    scale = 1.0 / math.sqrt(dh)
    if "lse" in saved:     # fused attention backward (dQ, dK, dV in one pass each)
        with timed:
            ops.attn_bwd(QKV, 3 * D, key_pad, out, D, dout, D, saved["lse"], B, H, T, dh, scale,
                         p_drop, seed, salt, dQKV, 3 * D, dt=dt, ws=ws(ops.attn_ws(B, H, T)),
                         mask_mode=mask_mode, q_bound=q_bound)
        return
    # ---- attention backward over the materialised probabilities
    ldt, Pm, Pd = saved["ldt"], saved["Pm"], saved["Pd"]
    sPT = (H * T * ldt, T * ldt)
    dPd = torch.empty(B * H, T, ldt, dtype=torch.float32, device=dev)
    ops.gemm(T, T, dh, dout, D, QKV[:, 2 * D:], 3 * D, dPd, ldt, dt=dt, c_fp32=1,
             batch=B * H, batch_div=H, strides=(T * D, dh, T * 3 * D, dh, *sPT, 0, 0))
    ops.gemm(ldt, dh, ldt, Pd, ldt, dout, D, dQKV[:, 2 * D:], 3 * D, dt=dt, a_kmajor=0,
             b_kmajor=0, kvalid=T, mvalid=T, batch=B * H, batch_div=H,
             strides=(*sPT, T * D, dh, T * 3 * D, dh, 0, 0))                   # dV = Pd^T dO
    dS = empty(B * H, T, ldt)
    ops.softmax_bwd(dPd, Pm, B, H, T, T, ldt, scale, p_drop, seed, salt, dS, dt=dt)
    del dPd
    ops.gemm(T, dh, ldt, dS, ldt, QKV[:, D:], 3 * D, dQKV, 3 * D, dt=dt, b_kmajor=0,
             kvalid=T, batch=B * H, batch_div=H,
             strides=(*sPT, T * 3 * D, dh, T * 3 * D, dh, 0, 0))               # dQ = dS K
    ops.gemm(ldt, dh, ldt, dS, ldt, QKV, 3 * D, dQKV[:, D:], 3 * D, dt=dt, a_kmajor=0,
             b_kmajor=0, kvalid=T, mvalid=T, batch=B * H, batch_div=H,
             strides=(*sPT, T * 3 * D, dh, T * 3 * D, dh, 0, 0))               # dK = dS^T Q
