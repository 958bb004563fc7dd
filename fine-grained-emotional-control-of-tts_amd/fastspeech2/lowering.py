"""How a conv or linear site of the train step becomes fs2_gemm launches: pure decisions.

Ints in, ints or a small named tuple out; no torch, no tensors.  The engine asks (fwd_padded,
dgrad_split, dgrad_refusal, wgrad_plan), allocates what the answer names and issues the
launches; w_okc says which weight images a weight gets, once, when the engine lists its
weights.  What each plan makes the engine launch is pinned on the CPU by
tests/test_lowering_host.py against tests/golden/engine_lowering.json.
"""

import collections

from . import _native as N

EPC = {N.F32: 4, N.BF16: 8}   # elements per 16-byte chunk (GEMM K / pitch granularity)
BK = {N.F32: 32, N.BF16: 64}


def round_up(x, m):
    return (x + m - 1) // m * m


def dgrad_split(Mp, C, K, dt, n_cu=256, max_split=8):
    """K split for the shift-conv data gradient, chosen for wave quantisation over the 256 CUs
    (one 256x128 tile per CU at a time): the decoder's 372 tiles fill 1.45 rounds (73 %), two
    slices fill 2.9 (97 %); the encoder's 78 tiles fill 30 %, three slices 91 %.  Slices are
    fp32 planes summed by fs2_conv_fold, so a split must gain > 5 % occupancy to pay for its
    extra plane."""
    if dt != 1:
        return 1
    if K >= 2048 and C >= 128 and C % 4 == 0:
        # the persistent 256 x 192 / 256 x 256 kernel (gemm_ps_kernel) takes an unsplit data
        # gradient when its tiles fill most of one round (the decoder: 124 x 2 = 248 tiles)
        w = 192 if C % 256 and -(-C // 192) * 192 < -(-C // 256) * 256 else 256
        if -(-Mp // 256) * -(-C // w) >= 200:
            return 1
    tiles = -(-Mp // 256) * -(-C // 128)

    def eff(s):
        return tiles * s / (n_cu * -(-(tiles * s) // n_cu))

    best, best_eff = 1, eff(1)
    for s in range(2, max(1, min(max_split, (K // 64) // 8)) + 1):
        if eff(s) > best_eff + 0.05:
            best, best_eff = s, eff(s)
    return best


# large weight gradients (the FFN conv1 weights, 5.3 M floats) as split-K planes + fixed-order
# sum instead of split-K fp32 atomics: decoder 428 -> 420 us, encoder 128 -> 119 us, and the
# result no longer depends on atomic ordering.  (tile, slice) units they aim for:
_SLICE_TARGET = 240
# CU budget of the small weight gradients' split-K on the side stream: sliced ones fill
# _WG_SLICE_CU CUs, the atomic ones _WG_ATOMIC_UNITS (tile, split) units
_WG_SLICE_CU = 256
_WG_ATOMIC_UNITS = 512
# decoder FFN conv1 data gradient in the tap-inner K order (w_okc bit 2): off -- 11 %
# faster standalone and 190 instead of 995 MB read, but the step measured 0.03-0.08 ms slower
# with it in three same-box A/Bs (17.18 vs 17.13 ms on the final tree); the FFN conv1 forward in
# that order (w_okc bit 3): off -- 316-318 vs 314 us for the decoder's in the step,
# step 17.42 vs 17.37 ms (experiments library, 2 x 2 interleaved)
_TAP_INNER = N.exp_int("FS2_TAP_INNER", 0)
_TAP_INNER_FWD = N.exp_int("FS2_TAP_INNER_FWD", 0)


def ps_plain_ok(M, lda, N, ldb, out_rows, ldc, out_bytes):
    """fs2_gemm can take a padded-domain GEMM (c_row output remap) only on its persistent
    kernel, with every operand within the kernel's 32-bit buffer offsets -- otherwise the engine
    keeps the implicit-conv path instead of handing fs2_gemm a call it refuses."""
    lim = 0x7fffffff
    return M * lda * 2 < lim and N * ldb * 2 < lim and out_rows * ldc * out_bytes < lim


def eff_split(K, ns, bk):
    """the split-K slice count fs2_gemm actually uses for ``ns`` requested slices of K (it
    rounds the K-tiles per slice up, which can leave trailing slices empty -- those it zeroes
    with a memset so a consumer summing all ``ns`` stays right).  Requesting this count instead
    skips the memset launch."""
    if ns <= 1:
        return 1
    nkt = -(-K // bk)
    return -(-nkt // -(-nkt // ns))


def wgrad_slices(O, Ncols, ldc, K, dt, n_cu=256):
    """Split-K slice count for a weight gradient with a small output: enough 256x128 tiles x
    slices to fill the 256 CUs once, each slice >= 8 K-tiles; slices are fp32 planes summed in
    a fixed order instead of tens of fp32 atomics landing on every output element.  Applied
    where it measured faster (bench.py --detail): outputs of
    >= 256 rows and <= 256 K elements (out-projection 62 -> 55 us, PostNet conv_pre 73 -> 57 us),
    or <= 600 K elements over encoder-length K (conv2 58 -> 42 us, out-projection 47 -> 31 us).
    1 = the atomic split-K path (decoder conv2 91 vs 144 us, PostNet 150 vs 231 us)."""
    if dt != 1 or ldc % 8 or Ncols != ldc or O < 256:
        return 1
    n = O * ldc
    if not (n <= (1 << 18) or (n <= 600_000 and K <= 8192)):
        return 1
    tiles = -(-O // 256) * -(-Ncols // 128)
    ns = min(-(-n_cu // tiles), max(1, (K // 64) // 8))
    return ns if ns >= 2 else 1


def rank_slices(O, ncols, K, dt):
    """the rank trainer's split-K slice count of a weight gradient: about one (tile, slice)
    unit per CU, at least four K-tiles per slice"""
    bk = BK[dt]
    tiles = -(-O // 128) * -(-ncols // 128)
    return eff_split(K, max(1, min(256 // tiles, (K // bk) // 4)), bk)


def km_ok(O, C, KW, dt, T, n_cols, lddy=0, ldx=0):
    """conv weight gradients that take the K-major path (conv_mode 6): the FFN conv1
    (k = 9) and PostNet (k = 5) weights.  tools/km_wgrad_bench.py, B = 32, GEMM + slice sum
    + both transposes vs the MN-major implicit-conv GEMM: decoder conv1 464 -> 372 us,
    encoder conv1 115 -> 110, PostNet 218 / 237 / 221 -> 125 / 98 / 75; the k = 3
    predictor convs lose (58 -> 67: the transposes cost more than the GEMM saves)."""
    return (dt == 1 and KW >= 5 and n_cols is None and C % 8 == 0 and O % 8 == 0 and
            (KW - 1) // 2 < T and lddy % 8 == 0 and ldx % 8 == 0)


W_REV, W_TAP_INNER, W_TAP_INNER_FWD = 2, 4, 8     # w_okc bits beside bit 0 (a conv weight)


def w_okc(name, O, C, KW, dt):
    """fs2_weight_prep's w_okc of one GEMM weight: bit 0 a conv weight ([O][KW][C] in the flat
    buffer, model._kw_major), and which of the FFN conv1 images it gets:

    W_REV: the data-gradient image with its taps reversed, for FFN conv1 data gradients over a
    zero-padded token-major dY image (bf16): the producing conv2 data gradient writes dY into
    the image (fs2_gemm c_row_t), and with the taps reversed the shift conv is a plain K-major
    GEMM whose A rows overlap, A(m, k) = image[m * O + k] (tools/dgrad_probe.py, B = 32:
    decoder 417 -> 339 us, encoder 83 -> 76) -- no per-K-tile tap offsets or row bounds in the
    loader.
    W_TAP_INNER: that image's columns in tap-inner 64-channel chunks (fs2_gemm_desc.a_kw), the
    decoder's only: consecutive 64-deep K-stages read image rows one tap apart, so the 96 MB
    image is fetched about once instead of once per tap (profiles/r05e_dgrad_traffic.json).
    Always the 4-wave kernel, unsplit; the encoder's (M = 6656) keeps its split-K path.
    W_TAP_INNER_FWD: the forward image in that order, both stacks.  Needs the padded path on
    every batch (fwd_padded's conditions other than P < T, which reflect padding requires)."""
    ffn1 = dt == 1 and ".pos_ffn.0." in name and KW > 1
    rev = ffn1 and km_ok(O, C, KW, dt, KW, None)
    ti = bool(_TAP_INNER) and rev and name.startswith("decoder.") and \
        O % 64 == 0 and (KW * O) % 128 == 0
    tif = bool(_TAP_INNER_FWD) and ffn1 and C % 64 == 0 and (KW * C) % 128 == 0 and \
        (KW * C) % EPC[dt] == 0
    return int(KW > 1) | (W_REV if rev else 0) | (W_TAP_INNER if ti else 0) | \
        (W_TAP_INNER_FWD if tif else 0)


# path "km" (ns = S, K = Kp) | "cols" | "slices" | "atomic"; accumulate: of the slice sum, or None
WgradPlan = collections.namedtuple("WgradPlan", "path K ns ldc stride ws_floats accumulate")


def fwd_padded(O, C, KW, dt, M, T, okc):
    """The FFN conv1 forward over a reflect-padded token-major X image (fs2_pad_rows + a plain
    GEMM whose A rows overlap, 2P dropped rows per utterance): tools/fwd_probe.py, B = 32:
    decoder 374 -> 305 us, encoder 100 -> 89 standalone (the implicit conv's per-K-tile reflect
    rows and tap offsets are gone from the loader).  Both stacks: over the image the decoder's
    conv1 is a plain GEMM for the 4-wave kernel (gemm_w4b_kernel), step 17.54 -> 17.35 ms on one
    box (tools/step_ab.sh, 3 rounds); on the 8-wave implicit conv it had measured no faster."""
    P = (KW - 1) // 2
    if okc & W_TAP_INNER_FWD:   # the 4-wave kernel: 32-bit offsets to 2.8 M rows
        return P < T
    return (dt == 1 and KW > 1 and C % 64 == 0 and P < T and (KW * C) % EPC[dt] == 0 and
            ps_plain_ok((M // T) * (T + 2 * P), C, O, KW * C, M, O, 2))


def dgrad_refusal(O, C, KW, B, T):
    """why a batch cannot take the data gradient over the padded dY image (W_REV): past the
    persistent kernel's 32-bit offsets -- the image (Mp + 2P rows of O), the weight image, the
    fp32 padded-domain output, and conv2's data gradient written into the image"""
    P = (KW - 1) // 2
    Mp = B * (T + 2 * P)
    fits = ps_plain_ok(Mp + 2 * P, O, C, KW * O, Mp, C, 4) and \
        ps_plain_ok(B * T, O, O, O, Mp + 2 * P, O, 2)
    return None if fits else (f"batch of {B} x {T} tokens exceeds the 32-bit offsets of the "
                              "padded conv data gradient; split the batch")


def wgrad_plan(O, C, KW, dt, M, T, lddy, ldx, n_cols, ctas):
    """Weight gradient of one site."""
    if km_ok(O, C, KW, dt, T, n_cols, lddy, ldx):
        # one (split, tile) unit per CU; >= 16 K-tiles per unit, <= 25 fp32 slices to sum
        Bt = (M // T) * (T + 2 * ((KW - 1) // 2))
        ncol = KW * C
        tiles = -(-O // 256) * -(-ncol // 256)
        cus = ctas if 0 < ctas < 256 else 256
        S = max(1, min(cus // tiles, -(-Bt // 64) // 16, 25))
        return WgradPlan("km", round_up(Bt, 64 * S), S, ncol, O * ncol, S * O * ncol, 1)
    K = round_up(M, EPC[dt])
    if n_cols is not None and n_cols != KW * C and KW == 1 and n_cols % 8 == 0 and dt == 1:
        # padded X columns (concat_proj: 2D + 5 -> 776): split-K slices over the padded width,
        # then the valid columns added into the gradient -- the unpadded GEMM's odd row
        # pitch forced the scalar atomic epilogue (92 -> ~35 us, tools/wgrad1x1_bench.py)
        ns = max(eff_split(K, wgrad_slices(O, n_cols, n_cols, K, dt), BK[dt]), 2)
        return WgradPlan("cols", K, ns, n_cols, O * n_cols, (ns + 1) * O * n_cols, 0)
    Ncols = n_cols or KW * C
    ldc = C * KW
    ns = wgrad_slices(O, Ncols, ldc, K, dt, _WG_SLICE_CU)
    if ns == 1 and dt == 1 and Ncols == ldc and O * ldc > 600_000:
        tiles = -(-O // 256) * -(-Ncols // 256)
        ns = max(1, min(-(-_SLICE_TARGET // tiles), (K // 64) // 8))
    ns = eff_split(K, ns, BK[dt])
    if ns > 1:
        # small outputs: split-K slices into fp32 planes, summed in a fixed order -- instead
        # of tens of fp32 atomics landing on every output element
        return WgradPlan("slices", K, ns, ldc, O * ldc, ns * O * ldc, 1)
    tiles = -(-O // 128) * -(-Ncols // 128)
    split = max(1, min(-(-_WG_ATOMIC_UNITS // tiles), K // (BK[dt] * 4))) if tiles < 256 else 1
    return WgradPlan("atomic", K, split, ldc, 0, 0, None)
