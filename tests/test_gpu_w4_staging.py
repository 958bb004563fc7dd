"""GPU: operand staging of the 4-wave GEMM (gemm_w4b_kernel: 1 KiB pieces of 8 rows x 128 B
into the swizzled two-slot LDS image, stages past K, rows past M / N, the tap-inner A offsets)
at the smallest shapes the dispatcher sends there: 32 and 34 K-stages on all four
instantiations, ragged row and column tiles, overlapping-row A in both K orders, both c_row
remaps, determinism.

Every case asserts through fs2_gemm_plan that the call takes the named instantiation.
Reference: fp32 matmul of the same bf16 values, rel 1e-2 (max |C - ref| / max |ref|, the bound
tests/test_gpu_ops.py::test_gemm_four_wave uses).  Outputs are NaN-filled (rows and columns the
call must not write stay NaN) and every operand is followed directly by a NaN guard, so a read
past an extent that reaches a stored output shows up as a non-finite result.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096   # guard elements after an operand's last valid one
bf = torch.bfloat16


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-12)).item()


def guarded(vals):
    """A flat copy of ``vals`` followed directly by GUARD NaNs; returns the view of the copy."""
    buf = torch.full((vals.numel() + GUARD,), float("nan"), device=vals.device, dtype=vals.dtype)
    buf[:vals.numel()] = vals.reshape(-1)
    return buf[:vals.numel()].view(vals.shape)


def kname(c32, nf):
    return f"gemm_w4b_kernel<{'true' if c32 else 'false'}, {nf}>"


def gemm_on(kernel, *args, **kw):
    from fastspeech2 import ops
    assert ops.gemm_plan(*args, **kw).kernel == kernel
    ops.gemm(*args, **kw)


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """(A, W, bias, ref) of a plain K-major GEMM, made once per shape and left unchanged"""
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    A = guarded(torch.randn(M, K, device="cuda", generator=g).to(bf))
    W = guarded((torch.randn(N, K, device="cuda", generator=g) * 0.05).to(bf))
    bias = guarded(torch.randn(N, device="cuda", generator=g))
    return A, W, bias, A.float() @ W.float().t() + bias


def check_plain(M, N, K, c32, nf, crow=None, twice=False):
    """One plain call into a NaN-filled output with a pitch of N + 8 and spare rows: written
    rows finite and within 1e-2, everything else still NaN."""
    A, W, bias, ref = operands(M, N, K)
    odt = torch.float32 if c32 else bf
    m = torch.arange(M, device="cuda")
    if crow is None:
        rows, keep, nrows = m, torch.ones(M, dtype=torch.bool, device="cuda"), M
    elif crow[1] > 0:      # gaps of crow[1] rows inserted every crow[0] rows
        rows, keep = m + (m // crow[0]) * crow[1], torch.ones(M, dtype=torch.bool, device="cuda")
        nrows = M + (M // crow[0] + 1) * crow[1]
    else:                  # the last -crow[1] rows of every crow[0] - crow[1] dropped
        L = crow[0] - crow[1]
        rows, keep = (m // L) * crow[0] + m % L, (m % L) < crow[0]
        nrows = (M // L + 1) * crow[0]
    ldc = N + 8
    outs = []
    for _ in range(2 if twice else 1):
        C = torch.full((nrows + 3, ldc), float("nan"), device="cuda", dtype=odt)
        gemm_on(kname(c32, nf), M, N, K, A, K, W, K, C, ldc, dt=1, c_fp32=c32, bias=bias,
                **({"c_row": crow} if crow else {}))
        outs.append(C)
    torch.cuda.synchronize()
    C = outs[0]
    written = torch.zeros(nrows + 3, dtype=torch.bool, device="cuda")
    written[rows[keep]] = True
    assert torch.isfinite(C[written][:, :N].float()).all()
    assert torch.isnan(C[~written].float()).all()       # rows past M, gap rows
    assert torch.isnan(C[:, N:].float()).all()          # columns past N
    assert rel(C[rows[keep]][:, :N], ref[keep]) < 1e-2
    if twice:
        iv = torch.int32 if c32 else torch.int16
        assert torch.equal(outs[0].view(iv), outs[1].view(iv))


@pytest.mark.parametrize("c32", [0, 1])
@pytest.mark.parametrize("N,nf", [(3456, 6), (5504, 8)])
@pytest.mark.parametrize("K", [2048, 2176])
def test_w4_smallest(cuda, K, N, nf, c32):
    """M = 2304 (9 row tiles): N = 3456 gives 162 tiles of 256 x 192, N = 5504 gives 198 of
    256 x 256 (261 of the narrower tile would need a second round); K = 2048 is 32 stages,
    K = 2176 an odd number of 128-multiples (34 stages); bf16 and fp32 outputs."""
    check_plain(2304, N, K, c32, nf)


@pytest.mark.parametrize("M", [2304 + 1, 2304 + 7, 2304 + 249])
def test_w4_ragged_rows(cuda, M):
    """A last row tile with one live row, a piece whose 8 rows straddle M, and 249 live rows;
    rows past M stay NaN."""
    check_plain(M, 3456, 2048, 0, 6)


@pytest.mark.parametrize("N,nf,c32", [(776, 8, 0), (520, 6, 1)])
def test_w4_ragged_columns(cuda, N, nf, c32):
    """A partial column tile on each width: N = 776 = 3 x 256 + 8 and N = 520 = 2 x 192 + 136,
    with a partial last row tile (M = 13817, 54 row tiles: 216 / 162 tiles); columns past N
    stay NaN."""
    check_plain(13817, N, 2048, c32, nf)


@pytest.mark.parametrize("crow", [(300, 8), (200, -8)])
def test_w4_c_row_remaps(cuda, crow):
    """Both c_row remaps: gaps inserted every 300 rows; the last 8 of every 208 rows dropped.
    Skipped rows stay NaN.  The same call twice gives identical bits."""
    check_plain(2304 + 249, 3456, 2048, 1, 6, crow=crow, twice=True)


@pytest.mark.parametrize("a_kw", [0, 9])
def test_w4_overlapping_rows(cuda, a_kw):
    """Overlapping-row A as in the padded-domain convs: lda = C < K = 9 C, so row m of A is
    image rows m .. m + 8 and the operand's extent ends (M - 1) lda + K elements in, inside
    the reach of the last tile's rows past M; the NaN guard starts right there.  Natural K
    order on the plain dispatch (M = 2311: a partial last tile) and the tap-inner order (a_kw:
    64-channel chunks outer, taps inner) at B = 3, T = 37, which selects the 4-wave kernel at
    any size; there the pad rows are dropped (c_row = (T, -2P)) and stay NaN."""
    from fastspeech2 import ops
    KW, P = 9, 4
    if a_kw:
        Bn, T, C, O = 3, 37, 128, 384
        M, crow = Bn * (T + 2 * P), (T, -2 * P)
    else:
        C, O = 256, 3456
        M, crow = 2304 + 7, None
    K = KW * C
    g = torch.Generator(device="cuda").manual_seed(a_kw + 5)
    img = guarded((torch.randn(M - 1 + KW, C, device="cuda", generator=g) * 0.5).to(bf))
    W = guarded((torch.randn(O, K, device="cuda", generator=g) * 0.05).to(bf))
    Ar = img.float().as_strided((M, K), (C, 1))          # row m = image rows m .. m + 8
    ref = Ar @ W.float().t()
    Wk = W
    if a_kw:
        Wk = guarded(W.view(O, KW, C // 64, 64).permute(0, 2, 1, 3).reshape(O, K).contiguous())
        L = T + 2 * P
        m = torch.arange(M, device="cuda")
        keep = (m % L) < T
        nrows = Bn * T
    else:
        keep = torch.ones(M, dtype=torch.bool, device="cuda")
        nrows = M
    Cout = torch.full((nrows + 3, O), float("nan"), device="cuda")
    gemm_on(kname(1, 6), M, O, K, img, C, Wk, K, Cout, O, dt=1, c_fp32=1, a_kw=a_kw,
            **({"c_row": crow} if crow else {}))
    torch.cuda.synchronize()
    assert torch.isfinite(Cout[:nrows]).all()
    assert torch.isnan(Cout[nrows:]).all()
    assert rel(Cout[:nrows], ref[keep]) < 1e-2
