"""CPU: the reference, the bound and the case tables of the vocoder conv GEMM parity tests
(tests/vocoder_conv_reference.py) are themselves checked here, without a GPU:

* the float64 reference equals torch's own dilated reflect conv and ConvTranspose1d;
* the derived bound lets an honest fp32 evaluation through and stops five planted index /
  epilogue mistakes (planted in reference-side copies, never in product code);
* every GPU case takes the kernel it was written for (fs2_gemm_plan, host only);
* every (kernel, operand path, epilogue) combination a generator layer takes -- at the small
  test shapes and at the 256-sentence workload -- is among the GPU cases, so a dispatcher
  change that moves a vocoder layer onto an untested kernel fails here;
* fs2_gemm_plan refuses a reflect pad as long as the utterance and a tap width that is no
  multiple of the 16-byte granule.
"""
import pytest
import torch
import torch.nn.functional as F

import vocoder_conv_reference as R
from vocoder_conv_reference import ACT_LRELU, ACT_NONE, ACT_TANH, GPU_CASES


def _rand(*shape, seed, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _torch_conv(X, W_okc, bias, B, T, dil, dtype):
    """F.conv1d over the dilation-aware reflect pad, rows [B*T][C] -> rows [B*T][O]"""
    O, k, C = W_okc.shape
    pad = dil * (k - 1) // 2
    x = X.to(dtype).view(B, T, C).transpose(1, 2)
    y = F.conv1d(F.pad(x, (pad, pad), mode="reflect"), W_okc.to(dtype).permute(0, 2, 1),
                 bias.to(dtype), dilation=dil)
    return y.transpose(1, 2).reshape(B * T, O)


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_reference_is_torch_reflect_conv(k, d):
    B, C, O = 2, 8, 5
    P = (k - 1) // 2
    for T in (d * P + 1, d * P + 2, 2 * d * P + 3):      # the smallest legal length first
        X, W, bias = _rand(B * T, C, seed=T), _rand(O, k, C, seed=k), _rand(O, seed=d)
        r = R.conv_ref(X, W, bias, None, ACT_NONE, B=B, T=T, dil=d, mode=1)
        want = _torch_conv(X, W, bias, B, T, d, torch.float64)
        assert (r["pre"] - want).abs().max() <= 1e-12 * want.abs().max()
        assert r["ref"] is r["pre"]
        rows, valid = R.conv_rows(B, T, k, d, 1)
        assert bool(valid.all()) and rows.shape == (B * T, k)
        assert bool((rows // T == torch.arange(B * T)[:, None] // T).all())   # own utterance only


@pytest.mark.parametrize("u", [2, 8])
@pytest.mark.parametrize("B", [2, 3])
def test_mode5_polyphase_is_conv_transpose(u, B):
    from fastspeech2.vocoder import polyphase_weights
    L, C, O = 7, 6, 5
    X = _rand(B * L, C, seed=u, dtype=torch.float32)
    Wt = _rand(C, O, 2 * u, seed=B, dtype=torch.float32)
    bias = _rand(O, seed=3, dtype=torch.float32)
    W3 = polyphase_weights(Wt, u).view(u * O, 3, C)
    r = R.conv_ref(X, W3, bias.repeat(u), None, ACT_NONE, B=B, T=L, dil=1, mode=5)
    want = R.upsample_ref(X, Wt, bias, B, L, u)
    # the GEMM output [B*L][u*O] is the upsampled sequence [B*L*u][O] in place
    assert (r["pre"].view(B * L * u, O) - want).abs().max() <= 1e-12 * want.abs().max()
    rows, valid = R.conv_rows(B, L, 3, 1, 5)
    assert int((~valid).sum()) == 2 * B                  # one zero tap at each utterance edge


# ---- the bound: sufficient and discriminating -----------------------------------------------

B3 = 3
# (C, O, k, d, T, act, residual): shapes of the GPU cases' small end
CONV_SHAPES = [(32, 32, 11, 5, 26, ACT_LRELU, False), (256, 256, 7, 3, 40, ACT_LRELU, False),
               (80, 64, 7, 1, 30, ACT_LRELU, False), (32, 32, 3, 1, 26, ACT_NONE, True)]


def _operands(C, O, k, T, seed, residual=False, B=B3):
    bf = torch.bfloat16
    X = _rand(B * T, C, seed=seed, dtype=torch.float32).to(bf)
    W = (_rand(O, k, C, seed=seed + 1, dtype=torch.float32) / (k * C) ** 0.5).to(bf)
    bias = 0.1 * _rand(O, seed=seed + 2, dtype=torch.float32)
    res = _rand(B * T, O, seed=seed + 3, dtype=torch.float32).to(bf) if residual else None
    return X, W, bias, res


@pytest.mark.parametrize("C,O,k,d,T,act,residual", CONV_SHAPES)
def test_fp32_evaluation_passes_the_bound(C, O, k, d, T, act, residual):
    X, W, bias, res = _operands(C, O, k, T, 10, residual)
    r = R.conv_ref(X, W, bias, res, act, B=B3, T=T, dil=d, mode=1)
    y = _torch_conv(X, W, bias, B3, T, d, torch.float32)
    if act == ACT_LRELU:
        y = F.leaky_relu(y, 0.1)
    if residual:
        y = y + res.float()
    worst = R.check(y.to(torch.bfloat16), r["ref"], r["bound"], T, "fp32 conv1d")
    assert 0 < worst <= 1


def test_fp32_upsample_passes_the_bound():
    from fastspeech2.vocoder import polyphase_weights
    bf = torch.bfloat16
    C, O, u, L = 512, 16, 8, 30
    X = _rand(B3 * L, C, seed=20, dtype=torch.float32).to(bf)
    Wt = (_rand(C, O, 2 * u, seed=21, dtype=torch.float32) / (3 * C) ** 0.5).to(bf).float()
    bias = 0.1 * _rand(O, seed=22, dtype=torch.float32)
    W3 = polyphase_weights(Wt, u).view(u * O, 3, C).to(bf)
    assert bool((W3.float() == polyphase_weights(Wt, u).view(u * O, 3, C)).all())
    r = R.conv_ref(X, W3, bias.repeat(u), None, ACT_NONE, B=B3, T=L, dil=1, mode=5)
    y = F.conv_transpose1d(X.float().view(B3, L, C).transpose(1, 2), Wt, bias, stride=u,
                           padding=u // 2).transpose(1, 2).reshape(B3 * L, u * O)
    assert 0 < R.check(y.to(bf), r["ref"], r["bound"], L, "fp32 conv_transpose1d") <= 1


def test_fp32_tanh_passes_the_bound():
    C, k, T = 32, 7, 50
    X, W, bias, _ = _operands(C, 1, k, T, 30)
    pre = R.conv_ref(X, W, bias, None, ACT_NONE, B=B3, T=T, dil=1, mode=1)["pre"]
    term = R.tanh_act_term(pre)
    assert 0 < term < 2.0 ** -21       # a few ulps of a value below 1, not a tuned allowance
    r = R.conv_ref(X, W, bias, None, ACT_TANH, B=B3, T=T, dil=1, mode=1, c_fp32=True,
                   act_term=term)
    y = torch.tanh(_torch_conv(X, W, bias, B3, T, 1, torch.float32))
    assert 0 < R.check(y, r["ref"], r["bound"], T, "fp32 tanh") <= 1


def _edge_repeat_rows(B, T, k, d):
    """MISTAKE: a reflect that repeats the edge sample (-i -> i-1, T-1+i -> T-i)"""
    P = (k - 1) // 2
    s = torch.arange(T)[:, None] + (torch.arange(k)[None, :] - P) * d
    s = torch.where(s < 0, -s - 1, s)
    s = torch.where(s > T - 1, 2 * T - 1 - s, s)
    rows = (torch.arange(B)[:, None, None] * T + s[None]).reshape(B * T, k)
    return rows, torch.ones_like(rows, dtype=torch.bool)


def _tap0_undilated_rows(B, T, k, d):
    """MISTAKE: the dilation dropped on tap 0"""
    P = (k - 1) // 2
    dj = torch.full((k,), d)
    dj[0] = 1
    s = torch.arange(T)[:, None] + (torch.arange(k)[None, :] - P) * dj[None, :]
    s = torch.where(s < 0, -s, s)
    s = torch.where(s > T - 1, 2 * (T - 1) - s, s)
    rows = (torch.arange(B)[:, None, None] * T + s[None]).reshape(B * T, k)
    return rows, torch.ones_like(rows, dtype=torch.bool)


def _neighbour_rows(B, T, k):
    """MISTAKE: the zero pad of mode 5 reads the neighbouring utterance's row"""
    P = (k - 1) // 2
    m = torch.arange(B * T)[:, None] + (torch.arange(k)[None, :] - P)
    valid = (m >= 0) & (m < B * T)
    return m.clamp(0, B * T - 1), valid


def _expect_caught(wrong, r, T, edge_steps=None):
    """check() refuses ``wrong`` (a float64 evaluation of a mistaken operator: no rounding
    noise at all) and reports the rows the mistake moves"""
    with pytest.raises(AssertionError, match="beyond the bound") as e:
        R.check(wrong, r["ref"], r["bound"], T, "planted")
    bad_t = ((wrong - r["ref"]).abs() > r["bound"]).any(dim=1).view(-1, T).any(dim=0)
    if edge_steps is not None:            # only edge rows move, and the message says which
        assert set(bad_t.nonzero().flatten().tolist()) <= set(edge_steps)
        assert "before the last" in str(e.value) and "utterance" in str(e.value)
    # far above the bound, not a near miss
    assert float(((wrong - r["ref"]).abs() / r["bound"]).max()) > 10


@pytest.mark.parametrize("C,O,k,d,T,act,residual", CONV_SHAPES[:2])
def test_planted_reflect_and_dilation_mistakes_fail(C, O, k, d, T, act, residual):
    X, W, bias, res = _operands(C, O, k, T, 40, residual)
    kw = dict(B=B3, T=T, dil=d, mode=1)
    r = R.conv_ref(X, W, bias, res, act, **kw)
    P = (k - 1) // 2
    edge = [t for t in range(T) if t < P * d or t > T - 1 - P * d]
    wrong = R.conv_ref(X, W, bias, res, act, rows=_edge_repeat_rows(B3, T, k, d), **kw)["ref"]
    _expect_caught(wrong, r, T, edge)
    wrong = R.conv_ref(X, W, bias, res, act, rows=_tap0_undilated_rows(B3, T, k, d), **kw)["ref"]
    _expect_caught(wrong, r, T)           # tap 0 moves in every row
    wrong = R.conv_ref(X, W, bias, res, act, slope=0.01, **kw)["ref"]
    _expect_caught(wrong, r, T)


def test_planted_zero_pad_and_phase_bias_mistakes_fail():
    from fastspeech2.vocoder import polyphase_weights
    bf = torch.bfloat16
    C, O, u, L = 64, 32, 2, 30
    X = _rand(B3 * L, C, seed=50, dtype=torch.float32).to(bf)
    Wt = (_rand(C, O, 2 * u, seed=51, dtype=torch.float32) / (3 * C) ** 0.5).to(bf).float()
    bias = 0.1 * _rand(O, seed=52, dtype=torch.float32)
    W3 = polyphase_weights(Wt, u).view(u * O, 3, C).to(bf)
    kw = dict(B=B3, T=L, dil=1, mode=5)
    r = R.conv_ref(X, W3, bias.repeat(u), None, ACT_NONE, **kw)
    wrong = R.conv_ref(X, W3, bias.repeat(u), None, ACT_NONE, rows=_neighbour_rows(B3, L, 3),
                       **kw)["ref"]
    # only the rows on an utterance boundary inside the batch move
    assert bool((wrong.view(B3, L, -1)[:, 1:-1] == r["ref"].view(B3, L, -1)[:, 1:-1]).all())
    _expect_caught(wrong, r, L, [0, L - 1])
    # MISTAKE: the per-phase bias rotated by one column, (r, o) reads bias[o - 1]
    wrong = R.conv_ref(X, W3, bias.repeat(u).roll(1), None, ACT_NONE, **kw)["ref"]
    _expect_caught(wrong, r, L)


# ---- kernels and coverage ---------------------------------------------------------------------

def _kernel(c, dt):
    from fastspeech2 import ops
    args, kw = R.gemm_call(c, dt)
    return ops.gemm_plan(*args, **kw).kernel


@pytest.mark.parametrize("case", GPU_CASES, ids=[c["name"] for c in GPU_CASES])
def test_gpu_case_takes_its_kernel(case):
    assert _kernel(case, case["dt"]) == case["kernel"]


def test_gpu_cases_cover_every_generator_layer():
    covered = {R.path_key(c["kernel"], c) for c in GPU_CASES if c["dt"] == 1}
    kernels = set()
    for B, T0 in ((1, 60), (2, 23), (256, 340)):
        layers = R.generator_layers(B, T0)
        assert len(layers) == 1 + 4 * (1 + 18) + 1
        for l in layers:
            key = R.path_key(_kernel(l, 1), l)
            kernels.add(key[0])
            assert key in covered, (B, T0, l["name"], key)
    # the workload reaches the large-tile kernels the op-level cases were written for
    assert kernels == {R.BF16_K128, R.BIG_C1, R.BIG_C5, R.BIG_GEN, R.G256_GEN, R.G256R_C5}
    # at least one case per kernel writes into a padded output, and pad columns of X are there
    for kern in {c["kernel"] for c in GPU_CASES}:
        assert any(c["ldo"] > c["N"] for c in GPU_CASES if c["kernel"] == kern), kern
        assert any(c["lda"] for c in GPU_CASES if c["kernel"] == kern), kern


def test_gemm_plan_refusals():
    from fastspeech2 import ops

    def plan(C, k, d, T, mode=1, B=2, lda=None):
        c = dict(M=B * T, N=32, K=k * C, C=C, k=k, mode=mode, T=T, dil=d, act=ACT_LRELU,
                 residual=False, c_fp32=0, ldo=32, lda=lda)
        args, kw = R.gemm_call(c, 1)
        return ops.gemm_plan(*args, **kw)

    einval = r"fs2_gemm_plan returned -1$"
    assert plan(32, 11, 5, 26).kernel == R.BF16_K128      # pad 25 < T = 26: the smallest legal
    with pytest.raises(RuntimeError, match=einval):      # conv_p * conv_dil >= conv_t
        plan(32, 11, 5, 25)
    assert plan(32, 11, 5, 25, mode=5).kernel             # a zero pad has no such limit
    assert plan(40, 3, 1, 26).kernel == R.BF16_K128
    with pytest.raises(RuntimeError, match=einval):      # C = 36: no whole 16-byte granules
        plan(36, 3, 1, 26, lda=40)
    with pytest.raises(RuntimeError, match=einval):      # the same with K = 144 a multiple of 8
        plan(36, 4, 1, 26, lda=40)
