"""Float64 reference, derived error bound and case tables for the vocoder's conv GEMMs.

The HiFi-GAN generator (fastspeech2/vocoder.py) is the only caller of three GEMM features:
dilated reflect convs (conv_mode 1 with ``conv_dil`` 3 and 5), the zero-padded 3-tap polyphase
form of ConvTranspose1d (conv_mode 5, N = u * C_out) and the epilogue activations 3 (leaky ReLU
0.1) and 4 (tanh, with the N = 1 fp32 output of conv_post).  This module holds what
tests/test_vocoder_conv_host.py (CPU) and tests/test_gpu_vocoder_conv.py (GPU) share; it has no
tests of its own and touches no kernel.

* ``conv_rows``: the source row of every (output row, tap), written from the definition.
* ``conv_ref``: gather with that index, multiply in float64 (torch indexing + matmul on
  whatever device the operands live on).
* the per-element bound of a kernel that multiplies the SAME rounded operands and accumulates
  in fp32::

      bound = K * 2^-23 * S + out_round * |ref| + act_term

  S is the same conv applied to |X|, |W|, |bias|, plus |residual|.  Products of two bf16 values
  are exact in fp32 (8 + 8 significand bits), and a product of two fp32 values carries one
  rounding of 2^-24; K - 1 fp32 additions in any order, each faithful or truncating (at most
  2^-23 relative to a partial sum that |.|-sums bound by S), stay under K * 2^-23 * S.
  ``out_round`` is 2^-8 for a bf16 output (half an ulp of 8 significand bits, relative to the
  value) and 2^-24 for an fp32 output.  Identity and leaky ReLU are 1-Lipschitz and add
  nothing.  tanh is 1-Lipschitz too, so the pre-activation error passes through unamplified,
  but the device ``tanhf`` has an error of its own: ``act_term``.  The documents
  installed with ROCm state no ulp bound for ``tanhf``, so ``tanh_act_term`` MEASURES it on the
  reference side: ``torch.tanh`` in fp32, on the device of the operands, against float64 over
  the case's own pre-activation values, and takes twice the measured maximum (the kernel is
  not involved).  The figure is case dependent; on the CPU it is about 1.2e-7 (two ulps of a
  value below 1), on an MI355X 1.2e-7 to 1.8e-7; the GPU tests record theirs in
  ``parity_log``.  No constant is tuned.
* ``check``: every element against its bound; the failure names the worst element.
* ``generator_layers``: the generator's GEMM calls in the order VocoderEngine.forward issues
  them, derived from the hyper-parameters alone.
* ``GPU_CASES``: the op-level cases of tests/test_gpu_vocoder_conv.py with the kernel each one
  must take; the host test pins those kernels and checks that every vocoder layer's
  (kernel, operand path, epilogue) combination is among them.
"""
import ctypes
import math

import torch
import torch.nn.functional as F

LRELU = 0.1
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 3, 4

BF16_K128 = "gemm_kernel<bf16, true, true, true, true>"
F32_K128 = "gemm_kernel<float, true, true, false, false>"
BIG_C1 = "gemm_big_kernel<true, true, 1, 0>"
BIG_C5 = "gemm_big_kernel<true, true, 5, 0>"
BIG_GEN = "gemm_big_kernel<true, true, -1, -1>"
G256_GEN = "gemm256_kernel<true, true, -1, -1>"
G256R_C5 = "gemm256r_kernel<5, false, 64>"

_BUF = (ctypes.c_char * 64)()
ADDR = (ctypes.addressof(_BUF) + 15) // 16 * 16    # stands for every tensor of a planned gemm


def conv_rows(B, T, k, dil, mode, device="cpu"):
    """(rows, valid), both [B*T][k]: output row b*T + t reads, at tap j, step
    t + (j - (k-1)//2) * dil of utterance b.  mode 1 reflects a step outside [0, T) without
    repeating the edge (-i -> i, T-1+i -> T-1-i); mode 5 reads zero there (valid False, the
    index clamped so that it can still be gathered).  No read leaves its utterance."""
    assert mode in (1, 5)
    P = (k - 1) // 2
    t = torch.arange(T, device=device)[:, None]
    j = torch.arange(k, device=device)[None, :]
    s = t + (j - P) * dil
    if mode == 1:
        assert P * dil < T, "a reflect pad must be shorter than the utterance"
        s = torch.where(s < 0, -s, s)
        s = torch.where(s > T - 1, 2 * (T - 1) - s, s)
        valid = torch.ones_like(s, dtype=torch.bool)
    else:
        valid = (s >= 0) & (s < T)
        s = s.clamp(0, T - 1)
    assert int(s.min()) >= 0 and int(s.max()) <= T - 1
    rows = (torch.arange(B, device=device)[:, None, None] * T + s[None]).reshape(B * T, k)
    return rows, valid[None].expand(B, T, k).reshape(B * T, k)


def _apply(X, W, bias, rows, valid):
    """sum_j X[rows[:, j]] W[:, j, :]^T + bias in float64 (one tap's gather at a time)"""
    O, k, C = W.shape
    out = torch.zeros(X.shape[0], O, dtype=torch.float64, device=X.device)
    for j in range(k):
        out += (X[rows[:, j]] * valid[:, j, None]) @ W[:, j, :].t()
    return out if bias is None else out + bias[None, :]


def conv_ref(X, W, bias, residual, act, *, B, T, dil, mode, c_fp32=False, act_term=0.0,
             slope=LRELU, rows=None):
    """Reference and bound of one conv GEMM.  X [B*T][C] and residual [B*T][O] hold the values
    the kernel reads (already rounded to the activation dtype, whose type they keep), W is
    [O][k][C] likewise, bias [O] fp32.  Returns a dict: ``pre`` (float64, before the
    activation), ``ref`` (float64: act(pre) + residual), ``S`` and ``bound`` (module
    docstring; ``act_term`` None: measured by tanh_act_term).  ``rows`` replaces conv_rows'
    (rows, valid) and ``slope`` the leaky ReLU's: the host test plants its mistakes through
    them."""
    O, k, C = W.shape
    assert X.shape == (B * T, C)
    out_bf16 = X.dtype == torch.bfloat16 and not c_fp32
    rows, valid = conv_rows(B, T, k, dil, mode, X.device) if rows is None else rows
    X64, W64 = X.double(), W.double()
    b64 = None if bias is None else bias.double()
    pre = _apply(X64, W64, b64, rows, valid)
    S = _apply(X64.abs(), W64.abs(), None if b64 is None else b64.abs(), rows, valid)
    if act == ACT_LRELU:
        ref = torch.where(pre >= 0, pre, slope * pre)
    elif act == ACT_TANH:
        ref = torch.tanh(pre)
    else:
        assert act == ACT_NONE
        ref = pre
    if act_term is None:      # measured over this case's own pre-activation values
        act_term = tanh_act_term(pre) if act == ACT_TANH else 0.0
    if residual is not None:
        ref = ref + residual.double()
        S = S + residual.double().abs()
    out_round = 2.0 ** -8 if out_bf16 else 2.0 ** -24
    bound = (k * C) * 2.0 ** -23 * S + out_round * ref.abs() + act_term
    return dict(pre=pre, ref=ref, S=S, bound=bound, act_term=act_term)


def tanh_act_term(pre):
    """twice the largest error of fp32 torch.tanh against float64 over ``pre`` (float64), on
    pre's device: the stand-in for the device tanhf's undocumented error (module docstring)"""
    return 2.0 * float((torch.tanh(pre.float()).double() - torch.tanh(pre)).abs().max())


def upsample_ref(X, Wt, bias, B, L, u):
    """F.conv_transpose1d(stride u, padding u/2) in float64 on the un-prepared weight
    Wt (C, O, 2u), from rows X [B*L][C]; returned as rows [B*L*u][O]"""
    C, O, _ = Wt.shape
    x = X.double().view(B, L, C).transpose(1, 2)
    y = F.conv_transpose1d(x, Wt.double(), None if bias is None else bias.double(), stride=u,
                           padding=u // 2)
    assert y.shape == (B, O, L * u)
    return y.transpose(1, 2).reshape(B * L * u, O)


def check(got, ref, bound, T, what=""):
    """Every element of ``got`` against ``ref`` within ``bound`` (same shapes, rows of
    utterances of T steps).  Returns the largest err/bound; fails on any element beyond its
    bound (or not finite), naming the worst one."""
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    bad = ~(err <= bound)                 # a NaN is bad
    if bool(bad.any()):
        score = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
        score = torch.where(bad, score, torch.zeros_like(score))
        flat = int(score.flatten().argmax())
        m, n = divmod(flat, got.shape[1])
        b, t = divmod(m, T)
        bad_rows = bad.any(dim=1)
        per_t = bad_rows.view(-1, T).any(dim=0).nonzero().flatten().tolist()
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound in "
            f"{int(bad_rows.sum())} of {got.shape[0]} rows; worst at utterance {b}, step {t} "
            f"({t} after the first, {T - 1 - t} before the last of {T}), column {n}: got "
            f"{float(got[m, n]):.9g}, reference {float(ref[m, n]):.9g}, err/bound "
            f"{float(ratio[m, n]):.4g} (bound {float(bound[m, n]):.4g}); steps with a bad row: "
            f"{per_t[:12]}{' ...' if len(per_t) > 12 else ''}")
    return float(ratio.max())


# ---- the generator's GEMM calls -------------------------------------------------------------

def generator_layers(B, T0, hparams=None):
    """The GEMM calls of one VocoderEngine.forward on a (B, n_mels, T0) mel, in order, from
    the hyper-parameters alone.  One dict per call: name, M, N, K, C, k, mode, T, dil, act,
    residual, c_fp32, ldo."""
    if hparams is None:
        from fastspeech2.vocoder import HPARAMS as hparams
    hp = hparams
    out = []

    def add(name, L, C, O, k, mode=1, dil=1, act=ACT_NONE, residual=False, c_fp32=0):
        out.append(dict(name=name, M=B * L, N=O, K=k * C, C=C, k=k, mode=mode, T=L, dil=dil,
                        act=act, residual=residual, c_fp32=c_fp32, ldo=O))

    L = T0 + 2 * hp["inference_padding"]
    ch = hp["upsample_initial_channel"]
    add("conv_pre", L, hp["in_channels"], ch, 7, act=ACT_LRELU)
    nk = len(hp["resblock_kernel_sizes"])
    for i, (u, ku) in enumerate(zip(hp["upsample_factors"], hp["upsample_kernel_sizes"])):
        assert ku == 2 * u
        add(f"ups.{i}", L, ch, u * (ch // 2), 3, mode=5)
        L, ch = L * u, ch // 2
        for j, (kr, dils) in enumerate(zip(hp["resblock_kernel_sizes"],
                                           hp["resblock_dilation_sizes"])):
            for n, d in enumerate(dils):
                add(f"resblocks.{i * nk + j}.convs1.{n}", L, ch, ch, kr, dil=d, act=ACT_LRELU)
                add(f"resblocks.{i * nk + j}.convs2.{n}", L, ch, ch, kr, residual=True)
    add("conv_post", L, ch, 1, 7, act=ACT_TANH, c_fp32=1)
    return out


def gemm_call(c, dt, A=ADDR, Wf=ADDR, out=ADDR, bias=ADDR, residual=ADDR):
    """(args, kwargs) of the ops.gemm call of a layer / case dict ``c`` in dtype code ``dt``,
    as VocoderEngine._conv issues it; every tensor defaults to a stand-in address (enough for
    ops.gemm_plan).  ``lda`` / ``ldr`` default to C rounded to the 16-byte granule / N."""
    epc = 8 if dt == 1 else 4
    lda = c.get("lda") or (c["C"] + epc - 1) // epc * epc
    args = (c["M"], c["N"], c["K"], A, lda, Wf, c["K"], out, c["ldo"])
    kw = dict(dt=dt, conv=(c["mode"], c["T"], c["k"], c["C"]), conv_dil=c["dil"], bias=bias,
              relu=c["act"], residual=residual if c["residual"] else None,
              ldr=c["N"] if c["residual"] else 0, c_fp32=c["c_fp32"])
    return args, kw


def path_key(kernel, c):
    """what distinguishes the code a conv GEMM runs: kernel, conv mode, tap-uniform K-tiles
    (C % 64 == 0), dilated, activation, residual operand, fp32 output"""
    return (kernel, c["mode"], c["C"] % 64 == 0, c["dil"] > 1, c["act"], bool(c["residual"]),
            int(c["c_fp32"]))


# ---- the GPU cases ----------------------------------------------------------------------------

def _case(kernel, dt, C, N, k, mode, B, T=77, dil=1, act=ACT_NONE, residual=False, c_fp32=0,
          lda=None, ldo=None, u=None):
    name = (f"{'bf16' if dt == 1 else 'fp32'}-C{C}-N{N}-k{k}-m{mode}-B{B}-T{T}-d{dil}-a{act}"
            f"{'-res' if residual else ''}{'-f32out' if c_fp32 else ''}"
            f"{f'-lda{lda}' if lda else ''}{f'-ldo{ldo}' if ldo else ''}")
    return dict(name=name, kernel=kernel, dt=dt, C=C, N=N, k=k, K=k * C, mode=mode, B=B, T=T,
                M=B * T, dil=dil, act=act, residual=residual, c_fp32=c_fp32, lda=lda,
                ldo=ldo or N, u=u)


def _small(kernel, dt):
    """the 128 x 128 kernel's cases (B = 3), the same in bf16 and fp32"""
    cs = [_case(kernel, dt, 32, 32, 11, 1, 3, T=26, dil=5, act=ACT_LRELU, lda=40, ldo=40),
          _case(kernel, dt, 32, 32, 3, 1, 3, T=26, act=ACT_LRELU),
          _case(kernel, dt, 32, 32, 3, 1, 3, T=26, residual=True, ldo=40)]
    cs += [_case(kernel, dt, 256, 256, k, 1, 3, T=40, dil=d, act=ACT_LRELU)
           for k in (3, 7, 11) for d in (1, 3, 5)]
    cs += [_case(kernel, dt, 256, 256, 7, 1, 3, T=40, residual=True, lda=264, ldo=264),
           # conv_post: N = 1, fp32 output, ldc = 1, tanh
           _case(kernel, dt, 32, 1, 7, 1, 3, T=50, act=ACT_TANH, c_fp32=1),
           _case(kernel, dt, 32, 1, 7, 1, 300, T=77, act=ACT_TANH, c_fp32=1, lda=40),
           # ups.0 at a small batch
           _case(kernel, dt, 512, 2048, 3, 5, 3, T=30, u=8, ldo=2056)]
    return cs


GPU_CASES = _small(BF16_K128, 1) + [
    # resblocks at the workload's batch, C % 64 == 0: taps aligned to the 64-wide K-tiles
    _case(BIG_C1, 1, 64, 64, 11, 1, 200, dil=5, act=ACT_LRELU),
    _case(BIG_C1, 1, 64, 64, 3, 1, 200, dil=3, residual=True, ldo=72),
    _case(BIG_C1, 1, 64, 64, 7, 1, 200, act=ACT_LRELU, lda=72),
    _case(BIG_C1, 1, 64, 64, 3, 1, 200, residual=True),
    _case(BIG_C1, 1, 256, 256, 7, 1, 97, dil=3, act=ACT_LRELU),          # two column tiles
    # ups.2 / ups.3 (u = 2): the bias repeats per phase
    _case(BIG_C5, 1, 128, 128, 3, 5, 197, u=2, ldo=136),
    _case(BIG_C5, 1, 64, 64, 3, 5, 197, u=2, lda=72),
    _case(BIG_C5, 1, 512, 2048, 3, 5, 59, u=8),                          # 16 column tiles
    # C = 32: taps inside a K-tile, the run-time generic operand path
    _case(BIG_GEN, 1, 32, 32, 11, 1, 197, dil=5, act=ACT_LRELU, lda=40),  # K = 352: partial tile
    _case(BIG_GEN, 1, 32, 32, 3, 1, 197, residual=True, ldo=40),          # K = 96
    _case(BIG_GEN, 1, 32, 32, 7, 1, 197, act=ACT_LRELU),
    # conv_pre: K = 560, taps of 80 straddle the 64-wide K-tiles
    _case(G256_GEN, 1, 80, 512, 7, 1, 247, act=ACT_LRELU, ldo=520),
    _case(G256_GEN, 1, 80, 512, 7, 1, 247, act=ACT_LRELU, lda=88),
    # ups.0 / ups.1 (u = 8)
    _case(G256R_C5, 1, 512, 2048, 3, 5, 60, u=8),
    _case(G256R_C5, 1, 256, 1024, 3, 5, 124, u=8, lda=264, ldo=1032),
] + _small(F32_K128, 0)
