"""CPU checks around the fused loss: the float64-capable restatement is the oracle in float32,
the workspace size is what carve() lays out, the host refuses what the SSIM tiles cannot hold,
and the anti-correlated input really drives the SSIM loss into its clamp."""
import ctypes

import pytest
import torch

import loss_restatement as LR


@pytest.mark.parametrize("name", ["weights", "short_mel"])
def test_restatement_is_the_oracle_in_float32(name):
    """Same ops in the same order, so all seven values and all five gradients are equal bit for
    bit, with unequal weights (a weight on the wrong term would show)."""
    inp = LR.make_inputs(name)
    vals, grads = LR.run_restatement(inp, LR.W_MIXED, torch.float32)
    ovals, ograds = LR.run_oracle(inp, LR.W_MIXED)
    assert vals == ovals
    for k, g, o in zip(LR.GRAD_KEYS, grads, ograds):
        assert g.dtype == torch.float32 and torch.equal(g, o), k
        assert bool(g.abs().max() > 0), k


def test_restatement_runs_in_float64():
    inp = LR.make_inputs("weights")
    vals, grads = LR.run_restatement(inp, LR.W_MIXED, torch.float64)
    ovals, _ = LR.run_oracle(inp, LR.W_MIXED)
    assert all(g.dtype == torch.float64 for g in grads)
    for v, o in zip(vals, ovals):
        assert abs(v - o) <= 1e-5 * max(1.0, abs(v))


@pytest.mark.parametrize("B,Tm,NM", LR.case_shapes() + [(300, 60, 80), (32, 1000, 80)])
def test_workspace_size_is_the_carve(B, Tm, NM):
    """fs2_loss_workspace_floats is the sum of carve()'s regions plus one 16-byte unit for its
    alignment step, and the carve ends inside it for every phase of the workspace start."""
    from fastspeech2 import _native as N
    got = N.load().fs2_loss_workspace_floats(B, Tm, NM)
    assert got == LR.workspace_floats(B, Tm, NM)
    for phase in range(4):
        assert LR.carve_extent(B, Tm, NM, phase) <= got
    assert got - LR.carve_extent(B, Tm, NM, 0) <= 4


def test_loss_host_refusals():
    """The shape checks come before the pointer checks: no pointer is needed to be refused."""
    from fastspeech2 import _native as N
    f = N.load().fs2_loss_fwd_bwd

    def call(B, Tm, NM):
        d = N.LossDesc()
        d.B, d.Tm, d.Tp, d.NM, d.dtype = B, Tm, 8, NM, N.F32
        return f(ctypes.byref(d), None)

    assert call(2, 10, 80) == -1      # Tm < 11: the SSIM window does not fit
    assert call(2, 27, 10) == -1      # NM < 11
    assert call(2, 27, 97) == -1      # NM > 96: the SSIM LDS tiles
    assert call(0, 27, 80) == 0       # empty batch
    assert call(2, 27, 80) == -1      # a valid shape reaches the (null) pointer check
    assert f(None, None) == -1


@pytest.mark.parametrize("name", ["anti", "anti_small"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_anticorrelated_input_clamps_the_ssim_loss(name, dtype):
    """mel_out = -target: the mean SSIM is negative, 1 - SSIM exceeds 1 and is replaced by the
    constant 1.0, so the SSIM term carries no gradient: with SSIM-only weights every gradient is
    zero, and the value is exactly the weight."""
    inp = LR.make_inputs(name)
    w = (0.7, 0.0, 0.0, 0.0, 0.0, 0.0)
    vals, grads = LR.run_restatement(inp, w, dtype)
    assert vals[1] == float(torch.tensor(1.0) * 0.7)
    assert vals[0] == vals[1]
    for g in grads:
        assert not g.any()
    # and the unclamped value is well away from the clamp, so fp32 kernels agree on the branch
    from oracle.fs2_oracle import SSIMLoss, ssim
    s = SSIMLoss()
    x, y = inp["mel"].to(dtype), inp["tgt"].to(dtype)
    mask = s.sequence_mask(inp["mel_len"], y.size(1)).unsqueeze(2)
    raw = 1.0 - ssim((s.sample_wise_min_max(y, mask) * mask).unsqueeze(1),
                     (s.sample_wise_min_max(x, mask) * mask).unsqueeze(1))
    assert float(raw) > 1.05
