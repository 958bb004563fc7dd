"""GPU: per-element parity of the vocoder's conv GEMMs on every kernel they reach.

Each case is ONE launch of fs2_gemm as VocoderEngine._conv issues it (dilated reflect conv,
conv_mode 1 with conv_dil; the 3-tap zero-padded polyphase ConvTranspose1d, conv_mode 5; the
epilogue activations 3 leaky ReLU and 4 tanh; the resblock residual) against the float64
gather + matmul of tests/vocoder_conv_reference.py over the same rounded operands.  EVERY
element is held to the derived bound K 2^-23 S + out_round |ref| + act_term of that module (no
tuned constant; the tanh term is measured on the reference side and recorded in parity_log).
The kernel is asserted before it is launched; pad columns of X hold NaN and must not be read;
pad columns of the output and one spare utterance of rows behind it hold a sentinel that must
be bit-identical afterwards; a mode 5 output is also compared, as the upsampled sequence
[B*L*u][C_out], with F.conv_transpose1d in float64 on the un-prepared weights
(polyphase_weights, weight_prep and the GEMM together).

Kernels, the generator layers they stand for (which layer takes which kernel follows the
batch: tests/test_vocoder_conv_host.py checks the coverage at B = 1, 2 and the 256-sentence
workload), and the largest err/bound measured on an MI355X:

  kernel                                       layers                                  err/bound
  gemm_kernel<bf16, true, true, true, true>    every layer at small batches; conv_post   0.97
  gemm_big_kernel<true, true, 1, 0>            resblocks, C = 256 / 128 / 64             0.98
  gemm_big_kernel<true, true, 5, 0>            ups.2, ups.3 (ups.0 at mid batches)       0.98
  gemm_big_kernel<true, true, -1, -1>          resblocks, C = 32                         0.99
  gemm256_kernel<true, true, -1, -1>           conv_pre (C = 80)                         0.93
  gemm256r_kernel<5, false, 64>                ups.0, ups.1                              0.89
  gemm_kernel<float, true, true, false, false> every layer of an fp32 generator          0.022

The bf16 figures are the output rounding meeting its half ulp (a value just above a power of
two); the accumulation term stays far from its bound, as the fp32 row shows.  The measured
tanh term (twice fp32 torch.tanh's error on the device) was 1.2e-7 to 1.8e-7; the conv_post
cases came to 0.004 of their bound at most.

``test_layer_table_matches_engine`` keeps generator_layers (the table the host coverage test
reads) equal to what VocoderEngine.forward really launches.
"""
import zlib

import pytest
import torch

import vocoder_conv_reference as R
from vocoder_conv_reference import GPU_CASES

pytestmark = pytest.mark.gpu

SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}


def gemm_on(kernel, *args, **kw):
    """ops.gemm(*args, **kw), after asserting that the dispatcher takes ``kernel`` for exactly
    these arguments (ops.gemm_plan: a host call, no GPU work)."""
    from fastspeech2 import ops
    assert ops.gemm_plan(*args, **kw).kernel == kernel
    ops.gemm(*args, **kw)


def run_case(c, dev):
    """one case: operands, one launch, sentinels, reference, check.  Returns the largest
    err/bound and the tanh term (0 without tanh)."""
    from fastspeech2 import ops
    from fastspeech2.vocoder import polyphase_weights
    dt = torch.bfloat16 if c["dt"] == 1 else torch.float32
    B, T, C, N, k, M, K, u = (c[x] for x in ("B", "T", "C", "N", "k", "M", "K", "u"))
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(c["name"].encode()))

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=dev)

    lda = c["lda"] or C
    Xbuf = torch.full((M, lda), float("nan"), dtype=dt, device=dev)
    Xbuf[:, :C] = randn(M, C).to(dt)
    X = Xbuf[:, :C].contiguous()
    Wf = torch.empty(N, K, dtype=dt, device=dev)
    if c["mode"] == 5:           # ConvTranspose1d (C, O, 2u) -> its 3-tap polyphase form
        O = N // u
        Wt = (randn(C, O, 2 * u) / K ** 0.5).to(dt).float()
        W3 = polyphase_weights(Wt, u)
        ops.weight_prep(W3, N, C, 3, Wf, K, None, 0, dt=c["dt"], w_okc=1)
        Wref = W3.view(N, 3, C).to(dt)
        bias_o = 0.1 * randn(O)
        bias = bias_o.repeat(u).contiguous()
    else:                        # Conv1d (O, C, k) -> [O][k][C]
        Wc = (randn(N, C, k) / K ** 0.5).to(dt).float().contiguous()
        ops.weight_prep(Wc, N, C, k, Wf, K, None, 0, dt=c["dt"], w_okc=0)
        Wref = Wc.permute(0, 2, 1).to(dt)
        bias = 0.1 * randn(N)
    res = randn(M, N).to(dt) if c["residual"] else None
    odt = torch.float32 if c["c_fp32"] else dt
    ldo = c["ldo"]
    ity, pat = SENTINEL[odt]
    out = torch.empty((B + 1) * T, ldo, dtype=odt, device=dev)      # one spare utterance
    out.view(ity).fill_(pat)
    args, kw = R.gemm_call(dict(c, lda=lda), c["dt"], A=Xbuf, Wf=Wf, out=out, bias=bias,
                           residual=res)
    gemm_on(c["kernel"], *args, **kw)
    torch.cuda.synchronize()
    bits = out.view(ity)
    assert bool((bits[M:] == pat).all()), "rows behind M were written"
    assert bool((bits[:M, N:] == pat).all()), "pad columns of the output were written"
    got = out[:M, :N].contiguous()
    r = R.conv_ref(X, Wref, bias, res, c["act"], B=B, T=T, dil=c["dil"], mode=c["mode"],
                   c_fp32=bool(c["c_fp32"]), act_term=None)
    worst = R.check(got, r["ref"], r["bound"], T, c["name"])
    if c["mode"] == 5:
        up = R.upsample_ref(X, Wt, bias_o, B, T, u)
        worst = max(worst, R.check(got.view(M * u, O), up, r["bound"].view(M * u, O), T * u,
                                   c["name"] + " as conv_transpose1d"))
    return worst, r["act_term"]


@pytest.mark.parametrize("case", GPU_CASES, ids=[c["name"] for c in GPU_CASES])
def test_conv_gemm_per_element(cuda, case, parity_log):
    worst, term = run_case(case, cuda)
    print(f"{case['kernel']} {case['name']}: err/bound max {worst:.4f}, tanh term {term:.3g}")
    rec = parity_log.setdefault("vocoder_conv " + case["kernel"],
                                {"err_over_bound_max": 0.0, "cases": 0, "tanh_act_term_max": 0.0})
    rec["err_over_bound_max"] = max(rec["err_over_bound_max"], worst)
    rec["tanh_act_term_max"] = max(rec["tanh_act_term_max"], term)
    rec["cases"] += 1
    assert worst <= 1.0


def test_layer_table_matches_engine(cuda, monkeypatch):
    """generator_layers(2, 23) is, call for call, what one decode_batch launches"""
    from fastspeech2 import vocoder
    calls = []
    real = vocoder.ops.gemm

    def rec(M, N, K, A, lda, Bm, ldb, C, ldc, **kw):
        calls.append((M, N, K, tuple(kw["conv"]), kw.get("conv_dil", 1), kw.get("relu", 0),
                      kw.get("residual") is not None, kw.get("c_fp32", 0), ldc))
        return real(M, N, K, A, lda, Bm, ldb, C, ldc, **kw)

    torch.manual_seed(0)
    gen = vocoder.HifiganGenerator(act_dtype=torch.bfloat16).to(cuda)
    mel = torch.randn(2, 80, 23, device=cuda)
    monkeypatch.setattr(vocoder.ops, "gemm", rec)
    wav = gen.decode_batch(mel)
    torch.cuda.synchronize()
    assert wav.shape == (2, 1, 256 * 33)
    want = [(l["M"], l["N"], l["K"], (l["mode"], l["T"], l["k"], l["C"]), l["dil"], l["act"],
             l["residual"], l["c_fp32"], l["ldo"]) for l in R.generator_layers(2, 23)]
    assert calls == want
