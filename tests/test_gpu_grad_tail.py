"""Backward pass over a padded batch: the kernels that skip gradient rows known to be exact zeros.

The decoder's incoming gradient is exactly 0.0 on every padded frame, and only a k > 1 conv's
data gradient moves gradient between rows, so in every decoder layer the gradient rows
t >= grad_end[b] = min(T, mel_len[b] + halo) are exact zeros (engine.FS2Engine.__init__).  The
fused attention backward takes that bound (fs2_attn_bwd_bounded) and skips the query tiles past it.

Attention (ops level, the bound handed in directly): dO random with rows >= bound[b] exactly zero.
  1. the bounded call returns a dQ | dK | dV torch.equal to the unbounded call's;
  2. a second bounded call whose dO holds NaN in rows >= round_up(bound[b], 128), on a NaN-filled
     workspace, returns the same finite tensor: the tiles are not read at all.
  Shapes, one per launch path: B = 32, T = 400 (128-row blocks: ceil(T / 128) * B * H >= 256) and
  B = 4, T = 200 (64-row blocks); dh = 192 (dQ kernel QG = 1) and dh = 64 (QG = 2); bounds on
  multiples of 64 and of 128, one row either side of each, below 64, and len + halo >= T.

Premise: one train step of the default-dims model with the skipping off and check_grad_tail on:
every site that would receive the bound sees an exactly zero tail.

K-major weight gradient (ops level): fs2_pad_transpose_bounded -> fs2_gemm conv_mode 6 with k_eff
-> fs2_sum_slices against the float64 conv weight gradient, at the tolerances of the existing
conv_mode 6 test; the compacted images against their torch construction, exactly; without split-K
the bounded gradient equals the unbounded one bit for bit.

Whole model: the same step with the skipping on and off; the gradients must agree within twice the
spread of two skip-off steps (max over the parameters of max|a - b| / max|b|).  At B = 4 that
spread is about 1e-7 (the few split-K atomics of so small a batch hardly reorder anything), which
is why the images drop whole K-tiles only (fs2_km_width): dropping every column past the bound
moved the utterances against the K-tile and MFMA boundaries, regrouped the fp32 sums and differed
by 4.9e-7.  With whole tiles an S = 1 weight gradient is bit-identical, like the attention part.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HALO = 8
NAN = float("nan")


def _round_up(x, m):
    return -(-x // m) * m


def _lens_for_bounds(bounds, T):
    """lengths whose bound min(T, len + HALO) is the wanted one (len = T - 3 for a bound of T:
    len + halo > T, nothing skipped)"""
    lens = []
    for e in bounds:
        L = T - 3 if e >= T else e - HALO
        assert 1 <= L <= T and min(T, L + HALO) == min(e, T), (e, L)
        lens.append(L)
    return lens


# B = 32, T = 400: every multiple of 64 below T with its neighbours (128, 256, 384 are the
# multiples of 128), one bound below 64, the smallest possible (len 1), and two at T
BOUNDS_LARGE = [400, 400, 9, 20, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320,
                321, 383, 384, 385, 399, 100, 150, 200, 250, 300, 350, 70, 130, 260]
# B = 4, T = 200: three sets covering 64, 128, 192 with their neighbours, below 64, and T
BOUNDS_SMALL = [[200, 128, 64, 20], [129, 127, 65, 63], [200, 193, 192, 191]]


def _attn_case(cuda, B, H, T, dh, p_drop, bounds, seed=31, salt=3):
    from fastspeech2 import ops
    assert len(bounds) == B
    D = H * dh
    bf = torch.bfloat16
    lens = _lens_for_bounds(bounds, T)
    torch.manual_seed(100 * dh + T + B)
    qkv = (torch.randn(B * T, 3 * D, device=cuda) * 0.5).to(bf)
    t = torch.arange(T, device=cuda)
    lens_t = torch.tensor(lens, device=cuda)
    bound = torch.clamp(lens_t + HALO, max=T).to(torch.int32)
    assert bound.tolist() == [min(e, T) for e in bounds]
    kp = (t[None, :] >= lens_t[:, None]).to(torch.uint8).contiguous().view(B * T)
    scale = 1.0 / math.sqrt(dh)
    out = torch.empty(B * T, D, device=cuda, dtype=bf)
    lse = torch.empty(B * H, T, device=cuda)
    ops.attn_fwd(qkv, 3 * D, kp, B, H, T, dh, scale, p_drop, seed, salt, out, D, lse, dt=1,
                 mask_mode=1)
    tail = (t[None, :] >= bound[:, None]).view(B * T)
    dout = torch.randn(B * T, D, device=cuda).to(bf)
    dout[tail] = 0
    r128 = torch.tensor([_round_up(min(e, T), 128) for e in bounds], device=cuda)
    dout_nan = dout.clone()
    dout_nan[(t[None, :] >= r128[:, None]).view(B * T)] = NAN

    def bwd(do, q_bound):
        dqkv = torch.full((B * T, 3 * D), NAN, device=cuda, dtype=bf)
        ws = torch.full((int(ops.attn_ws(B, H, T)),), NAN, device=cuda)
        ops.attn_bwd(qkv, 3 * D, kp, out, D, do, D, lse, B, H, T, dh, scale, p_drop, seed, salt,
                     dqkv, 3 * D, dt=1, ws=ws, mask_mode=1, q_bound=q_bound)
        return dqkv

    ref = bwd(dout, None)
    assert bool(torch.isfinite(ref).all())
    assert bool((ref[:, :D][tail] == 0).all()), "dQ of a zero dO row is zero"
    assert float(ref.float().abs().max()) > 0
    got = bwd(dout, bound)
    assert torch.equal(got, ref), "bounded backward differs from the unbounded one"
    got_nan = bwd(dout_nan, bound)
    assert bool(torch.isfinite(got_nan).all()), "a query tile past the bound was read"
    assert torch.equal(got_nan, ref)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("dh", [192, 64])
def test_attn_bwd_bounded_large_blocks(cuda, dh, p_drop):
    """128-row dQ blocks (attn_bwd_dq<192,1,8> / <64,2,8>) and attn_bwd_dkv<dh,8>"""
    B, H, T = 32, 2, 400
    assert -(-T // 128) * B * H >= 256
    _attn_case(cuda, B, H, T, dh, p_drop, BOUNDS_LARGE)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("dh", [192, 64])
@pytest.mark.parametrize("bounds", BOUNDS_SMALL, ids=["tiles", "offby1", "last"])
def test_attn_bwd_bounded_small_blocks(cuda, dh, p_drop, bounds):
    """64-row blocks (attn_bwd_dq<192,1,4> / <64,2,4>) and attn_bwd_dkv<dh,4>"""
    B, H, T = 4, 2, 200
    assert -(-T // 128) * B * H < 256
    _attn_case(cuda, B, H, T, dh, p_drop, bounds)


def test_attn_bwd_bounded_refuses_null_bound(cuda):
    """the C entry point itself returns FS2_EINVAL before any launch when the bound is missing"""
    from fastspeech2 import _native
    lib = _native.load()
    x = torch.zeros(64, 3 * 64, device=cuda, dtype=torch.bfloat16)
    o = torch.zeros(64, 64, device=cuda, dtype=torch.bfloat16)
    f = torch.zeros(4 * 64, device=cuda)
    kp = torch.zeros(64, device=cuda, dtype=torch.uint8)
    rc = lib.fs2_attn_bwd_bounded(x.data_ptr(), 192, kp.data_ptr(), 1, o.data_ptr(), 64,
                                  o.data_ptr(), 64, f.data_ptr(), 1, 1, 64, 64, 0.125, 0.0, 1, 1,
                                  x.data_ptr(), 192, f.data_ptr(), None, 1, None)
    assert rc != 0


# ------------------------------------------------- K-major weight gradient at the ops level
TOL_WGRAD, TOL_BIAS = 1e-3, 1e-5   # test_gpu_ops.test_wgrad_kmajor_padded_images (conv_mode 6)
O_W, C_W = 256, 64
# (B, T, S, bounds): S = 1 and S = 2 (passed explicitly); the last set has every bound at T
WGRAD_SHAPES = {"s1": (4, 200, 1, [200, 128, 65, 20]),
                "s2": (8, 264, 2, [264, 256, 255, 129, 128, 64, 63, 30]),
                "full": (4, 200, 1, [200, 200, 200, 200])}


def _rel64(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def _km_nk(k_eff, K, S):
    nk_host = K // 64 // S
    per = -(-(-(-k_eff // 64)) // S)
    return min(nk_host, max(2, per))


def _km_widths(bounds, T, P):
    """columns per utterance of the compacted images: T + 2P less the whole 64-column tiles of the
    uncompacted image inside [b (T + 2P) + bound + 2P, (b + 1)(T + 2P))"""
    Tp = T + 2 * P
    return [Tp - 64 * max(0, (b + 1) * Tp // 64 - -(-(b * Tp + min(T, e) + 2 * P) // 64))
            for b, e in enumerate(bounds)]


def _reflect(i, T):
    i = torch.where(i < 0, -i, i)
    return torch.where(i >= T, 2 * (T - 1) - i, i)


@pytest.fixture(scope="module")
def wgrad_data(cuda):
    """per (shape, KW): inputs, the float64 reference and the unbounded chain's results"""
    cache = {}

    def get(name, KW):
        from fastspeech2 import ops
        key = (name, KW)
        if key in cache:
            return cache[key]
        B, T, S, bounds = WGRAD_SHAPES[name]
        P = (KW - 1) // 2
        bf = torch.bfloat16
        torch.manual_seed(B * T + KW)
        X = torch.randn(B, T, C_W, device=cuda).to(bf)
        G = torch.randn(B, T, O_W, device=cuda).to(bf)
        bound = torch.tensor(bounds, device=cuda, dtype=torch.int32)
        t = torch.arange(T, device=cuda)
        G[t[None, :] >= bound[:, None]] = 0
        cols = [X[:, _reflect(t + j - P, T), :].double() for j in range(KW)]
        ref = G.double().reshape(B * T, O_W).t() @ torch.cat(cols, dim=2).reshape(B * T, KW * C_W)
        bias_ref = G.double().sum((0, 1))
        Kp = ops.round_up(B * (T + 2 * P), 64 * S)
        d = dict(B=B, T=T, S=S, KW=KW, P=P, X=X, G=G, bound=bound, bounds=bounds, ref=ref,
                 bias_ref=bias_ref, Kp=Kp)
        d["plain"] = _km_chain(cuda, d, None)
        cache[key] = d
        return d

    return get


def _images(cuda, d):
    """NaN-filled images between zeroed 64-element guards: whatever a kernel leaves unwritten and
    then reads shows up as NaN"""
    out = []
    for rows in (O_W, C_W):
        buf = torch.zeros(rows * d["Kp"] + 128, device=cuda, dtype=torch.bfloat16)
        buf[64:64 + rows * d["Kp"]] = NAN
        out.append(buf[64:64 + rows * d["Kp"]])
    return out


def _km_chain(cuda, d, bound, dy_img=False):
    """pad_transpose x 2 -> gemm conv_mode 6 -> sum_slices; returns (grad, bias, dYT, XT, k_eff)"""
    from fastspeech2 import ops
    B, T, S, KW, P, Kp = d["B"], d["T"], d["S"], d["KW"], d["P"], d["Kp"]
    dYT, XT = _images(cuda, d)
    bias = torch.zeros(O_W, device=cuda)
    pws = torch.full((int(ops.pad_transpose_ws(Kp, O_W)),), NAN, device=cuda)
    keff, bk = None, {}
    if bound is not None:   # the engine's construction (engine._km_offs)
        offs = ops.km_offsets(bound, T, P)
        assert bool((offs[B + 1:] == 2 ** 31 - 1).all()) and offs.numel() >= B + 17
        keff, bk = offs[B:B + 1], dict(offs=offs, ksplit=S)
    if dy_img:   # the zero-padded token-major dY image, T + 2P rows per utterance
        img = torch.zeros(B, T + 2 * P, O_W, device=cuda, dtype=torch.bfloat16)
        img[:, P:P + T] = d["G"]
        ops.pad_transpose(img, O_W, B, T + 2 * P, O_W, 0, 0, dYT, Kp, Kp, dt=1, colsum=bias,
                          ws=pws, **bk)
    else:
        ops.pad_transpose(d["G"], O_W, B, T, O_W, P, 0, dYT, Kp, Kp, dt=1, colsum=bias, ws=pws,
                          **bk)
    ops.pad_transpose(d["X"], C_W, B, T, C_W, P, 1, XT, Kp, Kp, dt=1, **bk)
    stride = O_W * KW * C_W
    ws = torch.full((S * stride,), NAN, device=cuda)
    ops.gemm(O_W, KW * C_W, Kp, dYT, Kp, XT, Kp, ws, KW * C_W, dt=1, conv=(6, T, KW, C_W),
             c_fp32=1, split_k=S, split_stride=stride if S > 1 else 0, k_eff=keff)
    grad = torch.zeros(O_W, KW * C_W, device=cuda)
    ops.sum_slices(ws, S, stride, stride, grad, accumulate=1)
    torch.cuda.synchronize()
    return grad, bias, dYT.view(O_W, Kp), XT.view(C_W, Kp), -1 if keff is None else int(keff)


@pytest.mark.parametrize("KW", [9, 5])
@pytest.mark.parametrize("name", ["s1", "s2"])
def test_wgrad_kmajor_compacted(cuda, wgrad_data, name, KW):
    """bounded chain against the float64 conv weight gradient of the same bf16 inputs, at the
    tolerances of the existing conv_mode 6 test (the unbounded chain is held to them too); the
    compacted images against their torch construction, exactly, with the columns past the
    zero-filled end untouched; both dY routes give the same image"""
    d = wgrad_data(name, KW)
    B, T, S, P, Kp = d["B"], d["T"], d["S"], d["P"], d["Kp"]
    grad0, bias0 = d["plain"][:2]
    e0, eb0 = _rel64(grad0, d["ref"]), _rel64(bias0, d["bias_ref"])
    grad, bias, dYT, XT, keff = _km_chain(cuda, d, d["bound"])
    e1, eb1 = _rel64(grad, d["ref"]), _rel64(bias, d["bias_ref"])
    print(name, KW, "unbounded", e0, eb0, "bounded", e1, eb1)
    assert bool(torch.isfinite(grad0).all()) and e0 < TOL_WGRAD and eb0 < TOL_BIAS
    assert bool(torch.isfinite(grad).all()) and e1 < TOL_WGRAD and eb1 < TOL_BIAS
    # the images
    widths = _km_widths(d["bounds"], T, P)
    assert all(min(T, e) + 2 * P <= w <= T + 2 * P for e, w in zip(d["bounds"], widths))
    assert keff == sum(widths) and keff <= B * (T + 2 * P) - 3 * 64
    if S == 1:   # whole K-tiles dropped, nothing regrouped
        assert torch.equal(grad, grad0) and torch.equal(bias, bias0)
    kz = min(Kp, S * _km_nk(keff, Kp, S) * 64 + 64)
    assert kz < Kp - 64, "the shape must leave whole blocks unwritten"
    xi = torch.zeros(C_W, kz, device=cuda, dtype=torch.bfloat16)
    yi = torch.zeros(O_W, kz, device=cuda, dtype=torch.bfloat16)
    off = 0
    for b, w in enumerate(widths):   # dY rows from the bound to w - 2P are zeros in G itself
        e = w - 2 * P
        i = torch.arange(-P, e + P, device=cuda)
        xi[:, off:off + w] = d["X"][b, _reflect(i, T), :].t()
        yi[:, off + P:off + P + e] = d["G"][b, :e, :].t()
        off += w
    assert torch.equal(XT[:, :kz], xi)
    assert torch.equal(dYT[:, :kz], yi)
    for im in (XT, dYT):   # untouched, but for the last 64 columns (read by the next row's taps)
        assert bool(torch.isnan(im[:, kz:Kp - 64]).all()) and bool((im[:, Kp - 64:] == 0).all())
    # the route through the zero-padded token-major dY image
    grad2, bias2, dYT2, _, keff2 = _km_chain(cuda, d, d["bound"], dy_img=True)
    assert keff2 == keff and torch.equal(dYT2[:, :kz], yi)
    assert torch.equal(grad2, grad) and torch.equal(bias2, bias)


@pytest.mark.parametrize("KW", [9, 5])
def test_wgrad_kmajor_full_bounds_change_nothing(cuda, wgrad_data, KW):
    """every bound at T: nothing is compacted and the result is the unbounded one, bit for bit"""
    d = wgrad_data("full", KW)
    grad0, bias0, dYT0, XT0, _ = d["plain"]
    grad, bias, dYT, XT, keff = _km_chain(cuda, d, d["bound"])
    assert keff == d["B"] * (d["T"] + 2 * d["P"])
    assert torch.equal(dYT, dYT0) and torch.equal(XT, XT0)
    assert torch.equal(grad, grad0) and torch.equal(bias, bias0)
    assert _rel64(grad, d["ref"]) < TOL_WGRAD and _rel64(bias, d["bias_ref"]) < TOL_BIAS


@pytest.mark.parametrize("B", [1, 32, 64, 70])
def test_grad_tail_bounds_kernel_matches_torch(cuda, B):
    """fs2_grad_tail_bounds (the engine's bounds and column offsets, one launch) against the
    torch construction ops.km_offsets, exactly: one utterance, a full wave, more than one wave"""
    from fastspeech2 import ops
    T, halo, P = 300, 24, 4
    g = torch.Generator().manual_seed(B)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    end, offs = ops.grad_tail_bounds(lens.to(cuda), T, halo, P)
    want = torch.clamp(lens + halo, max=T).to(torch.int32).to(cuda)
    assert torch.equal(end, want)
    assert torch.equal(offs, ops.km_offsets(want, T, P))
    assert offs[1:B + 1].diff(prepend=offs[:1]).tolist() == _km_widths(want.tolist(), T, P)


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def small_step(cuda, cfg_all):
    """default-dims bf16 model, B = 4, uneven mel lengths up to about 300; step(skip, check) runs
    one forward + loss + backward with dropout on (same seed: same masks) and returns the flat
    gradient"""
    from fastspeech2.model import FastSpeech2
    from fastspeech2.train import FusedTrainer
    from fastspeech2.synthetic import make_batch, as_tuple
    torch.manual_seed(0)
    m = FastSpeech2(**cfg_all["model"]["fastspeech2"], n_speakers=4,
                    act_dtype=torch.bfloat16).cuda().train()
    tr = FusedTrainer(m, lr=1e-4, graph=False)
    b = make_batch(B=4, tp_min=20, tp_max=60, t_mel_cap=300, seed=13, device="cuda")
    lens = b["mel_len"].tolist()
    Tm = max(lens)
    assert 200 <= Tm <= 300 and min(lens) + 64 < Tm, lens
    bt, inten = as_tuple(b)
    eng = m.engine()

    def step(skip, check=False):
        eng.skip_grad_tail, eng.check_grad_tail = skip, check
        eng.grad_tail_checked = []
        try:
            tr.forward_backward(bt, inten, seed=5)
            torch.cuda.synchronize()
        finally:
            eng.skip_grad_tail, eng.check_grad_tail = True, False
        return m._gflat.clone()

    return m, eng, step, lens


def test_grad_tail_premise_every_bounded_site_is_zero(small_step, cfg_all):
    """skipping off, check_grad_tail on: the engine asserts at every site that would receive the
    bound that its dO rows >= grad_end[b] are exactly zero; every decoder layer reports, and the
    tails are not empty"""
    m, eng, step, lens = small_step
    assert eng.skip_grad_tail, "skipping is on by default"
    c = cfg_all["model"]["fastspeech2"]
    k0, k1 = c["ffn_cnn_kernel_size_list"]
    assert eng._dec_halo() == c["dec_num_layers"] * ((k0 - 1) // 2 + (k1 - 1) // 2)
    step(skip=False, check=True)
    sites = dict(eng.grad_tail_checked)
    assert len(eng.grad_tail_checked) == len(sites)
    want = {f"decoder.layers.{i}.attn_bwd" for i in range(c["dec_num_layers"])}
    want |= {f"decoder.layers.{i}.pos_ffn.0.conv.weight" for i in range(c["dec_num_layers"])}
    post = {"postnet.conv_pre.conv.weight", "postnet.conv_post.conv.weight"}
    post |= {f"postnet.convs_intermedite.{i}.conv.weight"
             for i in range(c["postnet_n_convolutions"] - 2)}
    assert set(sites) == want | post, sites
    assert eng._postnet_halo() == c["postnet_n_convolutions"] * ((c["postnet_kernel_size"] - 1) // 2)
    Tm = max(lens)
    for halo, names in ((eng._dec_halo(), want), (eng._postnet_halo(), post)):
        rows = sum(Tm - min(Tm, L + halo) for L in lens)
        assert rows > 0 and all(sites[n] == rows for n in names), (sites, rows)


def test_grad_tail_step_matches_unskipped_step(small_step, parity_log):
    """gradients of the step with the skipping on against the step with it off, within twice
    the spread of two skip-off steps (max over the parameters of max|a - b| / max|b|)."""
    m, eng, step, lens = small_step

    def spread(a, b):
        worst = (0.0, "")
        for name, s, e in _ranges(m):
            ref = b[s:e].abs().max().item()
            if ref > 0:
                worst = max(worst, ((a[s:e] - b[s:e]).abs().max().item() / ref, name))
        return worst

    off1, off2, on = step(False), step(False), step(True)
    assert bool(torch.isfinite(on).all()) and float(on.abs().max()) > 0
    noise, noise_at = spread(off2, off1)
    got, got_at = max(spread(on, off1), spread(on, off2))
    print("grad_tail step: skip-off spread", noise, noise_at, "skip-on vs skip-off", got, got_at)
    parity_log["grad_tail_step"] = {"skip_off_spread": noise, "skip_on_vs_off": got}
    assert got <= 2 * noise, (got, got_at, noise, noise_at)


def _ranges(m):
    """(name, start, end) of every parameter's slice of the flat gradient"""
    out = []
    for name, g in m._grad_views.items():
        s = (g.data_ptr() - m._gflat.data_ptr()) // m._gflat.element_size()
        out.append((name, s, s + g.numel()))
    return out
