"""Rank-model training on the MI355X kernels: the train-mode forward of ``RankModel`` with its
four dropout sites per layer, the backward, and the differentiable ranking loss.

Reference (emo_rank_tts/rank_model/):
* ``train.py:19-43``   -- ``train_one_epoch``'s step: forward, ``RankLoss``, ``loss.backward()``,
  ``optim.step()`` (``rank_train_step`` here);
* ``model.py:8-50``    -- ``ConvTransformerEncoderLayer`` in training mode: dropout on the
  attention probabilities (``nn.MultiheadAttention(dropout=...)``), on the attention output
  before the residual (:36), after the GELU (:43) and on the conv2 output (:45);
* ``model.py:138-166`` -- ``RankModel.forward``; ``loss.py:36-55`` -- ``RankLoss``.

``TrainableRankModel`` is a ``RankModel`` (same parameters and ``state_dict`` keys) whose
training forward is one ``torch.autograd.Function`` over libfs2_hip.so: its inputs are the
parameters, its outputs ``Ii, Ij, hi, hj, ri, rj``, so ``loss.backward()``, ``.grad``
accumulation, ``zero_grad()`` and any torch optimiser work as usual.  There is no CPU path.

``RankTrainEngine`` is the training counterpart of ``intensity.ExtractorEngine``: one stream,
activations in the model's ``act_dtype`` (fp32 for parity, bf16), parameters, gradients and
LayerNorm statistics in fp32.  The backward mirrors ``engine.FS2Engine._fft_bwd``.  Padded frames
are not skipped: the k = 9 convs read live frames from rows ``t >= length``, so gradients flow
through them.  Every reduction has a fixed order (split-K slices summed by ``fs2_sum_slices``, no
atomics), so a step repeated from the same seed gives the same bits.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import ops
from .attention import attention_bwd, attention_fwd, use_flash
from .lowering import rank_slices
from .intensity import RankModel, stage_mixup
from .ops import round_up


class RankTrainEngine:
    """Train-mode forward and backward of the extractor over the 2B mixed sequences."""

    def __init__(self, ext):
        N.load()
        self.x = ext
        self.adt = ext.act_dtype
        self.dt = N.dtype_code(self.adt)
        self.epc = ops.EPC[self.dt]
        self.dev = ext.input_proj.weight.device
        D, KW = ext.hidden, ext.kernel
        if KW % 2 != 1:
            raise ValueError("kernel_size must be odd (padding=k//2 keeps the length only then)")
        if D % 8 or D % ext.n_heads:
            raise ValueError("hidden_dim must be a multiple of 8 and of n_heads")
        self.specs = {"input_proj.weight": (D, ext.n_mels + 2, 1)}
        for i in range(ext.n_layers):
            p = f"fft_block.layers.{i}."
            self.specs[p + "self_attn.in_proj_weight"] = (3 * D, D, 1)
            self.specs[p + "self_attn.out_proj.weight"] = (D, D, 1)
            self.specs[p + "conv1.weight"] = (4 * D, D, KW)
            self.specs[p + "conv2.weight"] = (D, 4 * D, KW)
        self.names = [n for n, _ in ext.named_parameters()]
        self.wf, self.wb, self.p = {}, {}, {}
        self._ver = None
        self.last = None          # (seed, [per-layer salts]) of the last training forward

    # ------------------------------------------------------------------ weight images
    def prepare(self):
        """fp32 torch-layout weights (O, C, KW) -> Wf[O][KW*C] for the forward and
        Wb[C][KW*O] (taps reversed) for the data gradients, in the activation dtype; rebuilt when
        a parameter's ``_version`` changes (an optimiser step, ``load_state_dict``)."""
        params = dict(self.x.named_parameters())
        ver = tuple(p._version for p in params.values())
        if self._ver == ver:
            return
        for name, (O, C, KW) in self.specs.items():
            ldf, ldb = round_up(KW * C, self.epc), round_up(KW * O, self.epc)
            if name not in self.wf:
                self.wf[name] = torch.empty(O, ldf, dtype=self.adt, device=self.dev)
                # the input projection has no data gradient
                self.wb[name] = None if name == "input_proj.weight" else \
                    torch.empty(C, ldb, dtype=self.adt, device=self.dev)
            W = params[name].detach().float().contiguous()
            ops.weight_prep(W, O, C, KW, self.wf[name], ldf, self.wb[name], ldb, dt=self.dt,
                            w_okc=2 if KW > 1 else 0)
        self.p = {n: t.detach().float().contiguous() for n, t in params.items()}
        self._ver = ver

    def empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.adt, device=self.dev)

    def _ws(self, n):
        return torch.empty(max(int(n), 4), dtype=torch.float32, device=self.dev)

    def use_flash(self, T, dh):
        return use_flash(T, dh, self.dt)

    # ------------------------------------------------------------------ GEMM forms
    def _fwd(self, X, ldx, M, T, wname, out, ldo, conv=False, **epi):
        O, C, KW = self.specs[wname]
        Wf = self.wf[wname]
        K = Wf.shape[1]
        ops.gemm(M, O, K, X, ldx, Wf, K, out, ldo, dt=self.dt,
                 conv=(5, T, KW, C) if conv else None, **epi)

    def _dgrad(self, dY, lddy, M, T, wname, out, ldo, **epi):
        """dX = dY W as a K-major GEMM on Wb; a conv's is the zero-padded conv of dY with the
        tap-reversed Wb (conv_mode 5, conv_c = O)."""
        O, C, KW = self.specs[wname]
        Wb = self.wb[wname]
        K = Wb.shape[1]
        ops.gemm(M, C, K, dY, lddy, Wb, K, out, ldo, dt=self.dt,
                 conv=(5, T, KW, O) if KW > 1 else None, **epi)

    def _wgrad(self, dY, lddy, X, ldx, rows, O, ncols, out, conv=None):
        """out[O][ncols] (fp32, overwritten) = dY^T X over ``rows`` token rows, both operands
        MN-major; ``conv`` = (3, rows per utterance, KW, C): X taken tap by tap (a conv weight
        gradient over zero-padded images, columns n = (tap, channel)).  Split-K slices summed in
        a fixed order."""
        K = round_up(rows, self.epc)
        ns = rank_slices(O, ncols, K, self.dt)
        kw = dict(dt=self.dt, a_kmajor=0, b_kmajor=0, conv=conv, c_fp32=1, kvalid=rows)
        if ns > 1:
            stride = O * ncols
            ws = self._ws(ns * stride)
            ops.gemm(O, ncols, K, dY, lddy, X, ldx, ws, ncols, split_k=ns, split_stride=stride,
                     **kw)
            ops.sum_slices(ws, ns, stride, stride, out, accumulate=0)
        else:
            ops.gemm(O, ncols, K, dY, lddy, X, ldx, out, ncols, **kw)

    def _conv_wgrad(self, dY, X, B, T, wname, out):
        """Conv weight gradient over zero-padded token-major images of T + 2P rows per utterance
        (conv_mode 3 with conv_t = T + 2P): dY's pad rows are zero, so every row the loader
        reflects multiplies a zero.  ``out`` (O, C, KW) fp32, torch's layout."""
        O, C, KW = self.specs[wname]
        P = (KW - 1) // 2
        Tp = T + 2 * P
        dYp = F.pad(dY.view(B, T, O), (0, 0, P, P)).view(B * Tp, O)
        Xp = F.pad(X.view(B, T, C), (0, 0, P, P)).view(B * Tp, C)
        g = torch.empty(O, KW, C, dtype=torch.float32, device=self.dev)
        self._wgrad(dYp, O, Xp, C, B * Tp, O, KW * C, g, conv=(3, Tp, KW, C))
        out.copy_(g.permute(0, 2, 1))

    def _colsum(self, X, ldx, M, n, out):
        ops.colsum(X, ldx, M, n, out, dt=self.dt, ws=self._ws(ops.colsum_ws(M, n)), accumulate=0)

    def _ln_fwd(self, x, r, gamma, beta, M, D, p_drop, seed, salt):
        """y = LN(s), s = x + drop(r), with s kept for the backward: (y, s, mean, rstd).
        fs2_ln_fwd with ``s_out`` normalises the STORED s, which in bf16 is s rounded.  The
        evaluation forward normalises the unrounded sum, so in bf16 y, mean and rstd come from a
        call without ``s_out`` -- the training forward at p = 0 is then the evaluation forward,
        value for value -- and a second call only writes s (the same mask: same seed and salt)."""
        f32 = lambda: torch.empty(M, dtype=torch.float32, device=self.dev)
        y, s, mean, rstd = self.empty(M, D), self.empty(M, D), f32(), f32()
        kw = dict(dt=self.dt, seed=seed, r=r, ldr=D, p_r=p_drop, salt_r=salt)
        if self.dt == N.F32:
            ops.ln_fwd(x, D, gamma, beta, 1e-5, y, D, mean, rstd, M, D, s_out=s, **kw)
        else:
            ops.ln_fwd(x, D, gamma, beta, 1e-5, y, D, mean, rstd, M, D, **kw)
            ops.ln_fwd(x, D, gamma, beta, 1e-5, self.empty(M, D), D, f32(), f32(), M, D, s_out=s,
                       **kw)
        return y, s, mean, rstd

    # ------------------------------------------------------------------ forward
    def forward(self, X0, B, T, length, emotions, p_drop, seed):
        """Training forward from the staged rows X0 [B*T][ldx]: returns (I (B,T,E) fp32, ctx)."""
        ext = self.x
        self.prepare()
        D, H, E = ext.hidden, ext.n_heads, ext.n_emotions
        M = B * T
        P = self.p
        p_drop = float(p_drop)
        key_pad = torch.empty(M, dtype=torch.uint8, device=self.dev)
        ops.keypad_from_lengths(length, B, T, key_pad)                  # model.py:84-93
        X = self.empty(M, D)
        self._fwd(X0, X0.shape[1], M, T, "input_proj.weight", X, D, bias=P["input_proj.bias"])
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        layers, salts, n_salt = [], [], 0
        for i in range(ext.n_layers):
            p = f"fft_block.layers.{i}."
            s_att, s_r1, s_gelu, s_r2 = n_salt + 1, n_salt + 2, n_salt + 3, n_salt + 4
            n_salt += 4
            c = {"X": X}
            QKV = self.empty(M, 3 * D)
            self._fwd(X, D, M, T, p + "self_attn.in_proj_weight", QKV, 3 * D,
                      bias=P[p + "self_attn.in_proj_bias"])
            Att = self.empty(M, D)
            c.update(attention_fwd(QKV, key_pad, B, H, T, D, Att, dt=self.dt, dev=self.dev,
                                   mask_mode=0, p_drop=p_drop, seed=seed, salt=s_att,
                                   empty=self.empty))
            Ao = self.empty(M, D)
            self._fwd(Att, D, M, T, p + "self_attn.out_proj.weight", Ao, D,
                      bias=P[p + "self_attn.out_proj.bias"])
            X1, s1, mean1, rstd1 = self._ln_fwd(X, Ao, P[p + "norm1.weight"], P[p + "norm1.bias"],
                                                M, D, p_drop, seed, s_r1)   # model.py:36-37
            del Ao
            # conv1's output in fp32, so that GELU sees the unrounded value as the evaluation
            # path's fused epilogue does (bf16: the same Hc at p = 0); the backward keeps Z in
            # the activation dtype
            Z32 = f32(M, 4 * D)
            self._fwd(X1, D, M, T, p + "conv1.weight", Z32, 4 * D, conv=True,
                      bias=P[p + "conv1.bias"], c_fp32=1)                    # :41
            Z = Z32 if self.dt == N.F32 else self.empty(M, 4 * D)
            Hc = self.empty(M, 4 * D)
            ops.gelu_dropout_fwd(Z32, 4 * D, Hc, 4 * D, M, 4 * D, p_drop, seed, s_gelu,
                                 dt=self.dt, z_fp32=1, Zact=None if Z is Z32 else Z,
                                 ldza=4 * D)                                 # :42-43
            del Z32
            Y = self.empty(M, D)
            self._fwd(Hc, 4 * D, M, T, p + "conv2.weight", Y, D, conv=True,
                      bias=P[p + "conv2.bias"])                              # :44
            X2, s2, mean2, rstd2 = self._ln_fwd(X1, Y, P[p + "norm2.weight"], P[p + "norm2.bias"],
                                                M, D, p_drop, seed, s_r2)   # :45-49
            del Y
            c.update(QKV=QKV, Att=Att, X1=X1, s1=s1, mean1=mean1, rstd1=rstd1, Z=Z, Hc=Hc, s2=s2,
                     mean2=mean2, rstd2=rstd2, s_att=s_att, s_r1=s_r1, s_gelu=s_gelu, s_r2=s_r2)
            layers.append(c)
            salts.append({"attn": s_att, "res1": s_r1, "gelu": s_gelu, "res2": s_r2})
            X = X2
        I = f32(B, T, E)
        ops.intensity_head(X, D, P["emotion_embedding.weight"], emotions, length,
                           P["classifier.weight"], P["classifier.bias"], B, T, D, E, I,
                           dt=self.dt)                                      # :103-107
        self.last = (seed, salts)
        ctx = dict(X0=X0, B=B, T=T, length=length, emotions=emotions, key_pad=key_pad,
                   layers=layers, Hf=X, p=p_drop, seed=seed, P=P, ver=self._ver)
        return I, ctx

    # ------------------------------------------------------------------ backward
    def backward(self, ctx, gI):
        """gI (B, T, E) fp32, the gradient of the extractor's output.  Returns {parameter name:
        fp32 gradient in the parameter's shape} for every extractor parameter."""
        ext = self.x
        D, H, E, KW = ext.hidden, ext.n_heads, ext.n_emotions, ext.kernel
        B, T, p_drop, seed, P = ctx["B"], ctx["T"], ctx["p"], ctx["seed"], ctx["P"]
        # the weight images (and, in fp32, P itself) are the current parameters': a backward
        # after a parameter changed would mix them with the forward's activations
        if ctx["ver"] != tuple(q._version for q in ext.parameters()) or ctx["ver"] != self._ver:
            raise RuntimeError("a parameter of the extractor was modified between the training "
                               "forward and its backward; run the forward again")
        M = B * T
        n_emo = P["emotion_embedding.weight"].shape[0]
        G = {n: torch.zeros_like(t) for n, t in P.items()}
        dX = self.empty(M, D)
        ops.intensity_head_bwd(gI, ctx["Hf"], D, P["emotion_embedding.weight"], ctx["emotions"],
                               n_emo, ctx["length"], P["classifier.weight"], B, T, D, E, dX, D,
                               G["classifier.weight"], G["classifier.bias"],
                               G["emotion_embedding.weight"], dt=self.dt,
                               ws=self._ws(ops.intensity_head_bwd_ws(B, T, D, E)))
        for i in reversed(range(ext.n_layers)):
            p = f"fft_block.layers.{i}."
            c = ctx["layers"][i]
            ds2, dY = self.empty(M, D), self.empty(M, D)
            ops.ln_bwd(dX, D, c["s2"], D, c["mean2"], c["rstd2"], P[p + "norm2.weight"],
                       P[p + "norm2.bias"], ds2, D, M, D, dt=self.dt,
                       ws=self._ws(ops.ln_ws(M, D)), seed=seed, dr=dY, p_r=p_drop,
                       salt_r=c["s_r2"], dgamma=G[p + "norm2.weight"], dbeta=G[p + "norm2.bias"],
                       dcol=G[p + "conv2.bias"])
            self._conv_wgrad(dY, c["Hc"], B, T, p + "conv2.weight", G[p + "conv2.weight"])
            dZ = self.empty(M, 4 * D)
            self._dgrad(dY, D, M, T, p + "conv2.weight", dZ, 4 * D)
            ops.gelu_dropout_bwd(dZ, 4 * D, c["Z"], 4 * D, dZ, 4 * D, M, 4 * D, p_drop, seed,
                                 c["s_gelu"], dt=self.dt)
            self._conv_wgrad(dZ, c["X1"], B, T, p + "conv1.weight", G[p + "conv1.weight"])
            self._colsum(dZ, 4 * D, M, 4 * D, G[p + "conv1.bias"])
            dX1 = self.empty(M, D)
            self._dgrad(dZ, 4 * D, M, T, p + "conv1.weight", dX1, D, residual=ds2, ldr=D)
            del dY, dZ, ds2
            ds1, dAo = self.empty(M, D), self.empty(M, D)
            ops.ln_bwd(dX1, D, c["s1"], D, c["mean1"], c["rstd1"], P[p + "norm1.weight"],
                       P[p + "norm1.bias"], ds1, D, M, D, dt=self.dt,
                       ws=self._ws(ops.ln_ws(M, D)), seed=seed, dr=dAo, p_r=p_drop,
                       salt_r=c["s_r1"], dgamma=G[p + "norm1.weight"], dbeta=G[p + "norm1.bias"],
                       dcol=G[p + "self_attn.out_proj.bias"])
            del dX1
            wo = p + "self_attn.out_proj.weight"
            self._wgrad(dAo, D, c["Att"], D, M, D, D, G[wo])
            dAtt = self.empty(M, D)
            self._dgrad(dAo, D, M, T, wo, dAtt, D)
            del dAo
            QKV = c["QKV"]
            dQKV = self.empty(M, 3 * D)
            attention_bwd(c["QKV"], ctx["key_pad"], c["Att"], dAtt, c, B, H, T, D, dQKV,
                          dt=self.dt, dev=self.dev, mask_mode=0, p_drop=p_drop, seed=seed,
                          salt=c["s_att"], empty=self.empty, ws=self._ws)
            del dAtt
            wi = p + "self_attn.in_proj_weight"
            self._wgrad(dQKV, 3 * D, c["X"], D, M, 3 * D, D, G[wi])
            self._colsum(dQKV, 3 * D, M, 3 * D, G[p + "self_attn.in_proj_bias"])
            dX = self.empty(M, D)
            self._dgrad(dQKV, 3 * D, M, T, wi, dX, D, residual=ds1, ldr=D)
            del dQKV, ds1
        # the input projection: a weight gradient from the staged rows (K padded to the vector
        # width, the pad columns are zeros), no data gradient
        X0 = ctx["X0"]
        ldx = X0.shape[1]
        C = ext.n_mels + 2
        g = torch.empty(D, ldx, dtype=torch.float32, device=self.dev)
        self._wgrad(dX, D, X0, ldx, M, D, ldx, g)
        G["input_proj.weight"].copy_(g[:, :C])
        self._colsum(dX, D, M, D, G["input_proj.bias"])
        return G


class _RankTrainFunction(torch.autograd.Function):
    """(parameters) -> (Ii, Ij, hi, hj, ri, rj) of rank_model/model.py:148-166 in training mode."""

    @staticmethod
    def forward(ctx, model, seed, emo_X, neu_X, emotions, length, lambdas, *params):
        ext = model.intensity_extractor
        eng = model.train_engine()
        B, T, _ = emo_X.shape
        E = model.n_emotions
        X0, B2, _ = stage_mixup(ext.n_mels + 2, eng.dev, eng.adt, emo_X, neu_X, lambdas)
        len2, emo2 = length.repeat(2).contiguous(), emotions.repeat(2).contiguous()
        I, ectx = eng.forward(X0, B2, T, len2, emo2, ext.fft_block.layers[0].dropout.p, seed)
        h = torch.empty(B2, E, dtype=torch.float32, device=eng.dev)
        r = torch.empty(B2, dtype=torch.float32, device=eng.dev)
        Wp = model.projector.weight.detach().float().reshape(-1).contiguous()
        ops.rank_pool(I, len2, Wp, B2, T, E, h, r)                           # :160-164
        ctx.set_materialize_grads(False)
        ctx.model, ctx.eng, ctx.ectx, ctx.h, ctx.Wp, ctx.len2 = model, eng, ectx, h, Wp, len2
        return I[:B], I[B:], h[:B], h[B:], r[:B], r[B:]

    @staticmethod
    def backward(ctx, gIi, gIj, ghi, ghj, gri, grj):
        eng, ectx = ctx.eng, ctx.ectx
        B2, T = ectx["B"], ectx["T"]
        B = B2 // 2
        E = ctx.model.n_emotions
        dev = eng.dev

        def pair(a, b, *shape):
            if a is None and b is None:
                return None
            z = lambda t: torch.zeros(B, *shape, dtype=torch.float32, device=dev) if t is None \
                else t.to(torch.float32)
            return torch.cat([z(a), z(b)]).contiguous()

        gI = pair(gIi, gIj, T, E)
        gh = pair(ghi, ghj, E)
        gr = pair(gri, grj)
        if gh is None:
            gh = torch.zeros(B2, E, dtype=torch.float32, device=dev)
        if gr is None:
            gr = torch.zeros(B2, dtype=torch.float32, device=dev)
        dI = torch.empty(B2, T, E, dtype=torch.float32, device=dev)
        dWp = torch.empty(E, dtype=torch.float32, device=dev)
        ops.rank_pool_bwd(gI, gh, gr, ctx.h, ctx.Wp, ctx.len2, B2, T, E, dI, dWp)
        G = eng.backward(ectx, dI)
        grads = [G[n] for n in eng.names]
        grads.append(dWp.reshape(1, E))
        return (None,) * 7 + tuple(grads)


class TrainableRankModel(RankModel):
    """``RankModel`` whose training forward runs (rank_model/model.py:138-166 under
    ``model.train()``).  Same constructor, parameters and ``state_dict`` keys; in eval mode the
    parent's forward, unchanged.

    In training mode ``forward`` returns the reference's 8-tuple ``(lam_i, lam_j, Ii, Ij, hi,
    hj, ri, rj)``; ``Ii .. rj`` carry an autograd graph back to the parameters.  Dropout masks
    come from a per-step seed (drawn as ``FastSpeech2.forward`` draws its own, or ``seed=``) and
    one salt per dropout site; ``last_dropout`` holds ``(seed, salts)`` of the last step."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._train_engine = None
        self._step_seed = 1234

    def train_engine(self):
        if self._train_engine is None:
            self._train_engine = RankTrainEngine(self.intensity_extractor)
        return self._train_engine

    def _apply(self, fn, *args, **kwargs):
        self._train_engine = None     # device / dtype moves invalidate the weight images
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        r = super().load_state_dict(*args, **kwargs)
        self._train_engine = None
        return r

    @property
    def last_dropout(self):
        return None if self._train_engine is None else self._train_engine.last

    def forward(self, emo_X, neu_X, emotions, length, lambdas=None, seed=None):
        if not self.training:
            return super().forward(emo_X, neu_X, emotions, length, lambdas)
        if emo_X.device.type != "cuda" or neu_X.device.type != "cuda":
            raise RuntimeError("TrainableRankModel runs only on the HIP device (libfs2_hip.so); "
                               "there is no CPU path")
        B, T, _ = emo_X.shape
        eng = self.train_engine()
        dev = eng.dev
        if lambdas is None:
            lambdas = torch.distributions.Beta(1.0, 1.0).sample((2, B))       # model.py:144-146
        lambdas = lambdas.detach().to(device=dev, dtype=torch.float32)
        length = length.to(device=dev, dtype=torch.int64)
        emotions = emotions.to(device=dev, dtype=torch.int64)
        if length.shape != (B,) or emotions.shape != (B,):
            raise RuntimeError(f"length and emotions must be ({B},)")
        if seed is None:
            self._step_seed = (self._step_seed * 1103515245 + 12345) & 0x7fffffff
            seed = self._step_seed
        params = [p for _, p in self.intensity_extractor.named_parameters()]
        params.append(self.projector.weight)
        Ii, Ij, hi, hj, ri, rj = _RankTrainFunction.apply(self, int(seed), emo_X, neu_X, emotions,
                                                          length, lambdas, *params)
        lam_i = lambdas[0].unsqueeze(1).unsqueeze(1)
        lam_j = lambdas[1].unsqueeze(1).unsqueeze(1)
        return lam_i, lam_j, Ii, Ij, hi, hj, ri, rj


class _RankLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hi, hj, ri, rj, lam_i, lam_j, y_emo, y_neu, alpha, beta):
        B, E = hi.shape
        dev = hi.device
        f = lambda t, *shape: t.detach().to(device=dev, dtype=torch.float32).reshape(*shape) \
            .contiguous()
        y = lambda t: t.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
        out = torch.zeros(3, dtype=torch.float32, device=dev)
        dhi, dhj = torch.zeros(B, E, device=dev), torch.zeros(B, E, device=dev)
        dri, drj = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
        ops.rank_loss_fwd_bwd(f(lam_i, B), f(lam_j, B), f(hi, B, E), f(hj, B, E), f(ri, B),
                              f(rj, B), y(y_emo), y(y_neu), B, E, alpha, beta, out, dhi, dhj, dri,
                              drj)
        ctx.grads = (dhi, dhj, dri.reshape(ri.shape), drj.reshape(rj.shape))
        mix, rank = out[1], out[2]
        ctx.mark_non_differentiable(mix, rank)
        return out[0], mix, rank

    @staticmethod
    def backward(ctx, g, _gm, _gr):
        return tuple(g * t for t in ctx.grads) + (None,) * 6


class RankTrainLoss(nn.Module):
    """rank_model/loss.py:9-55 with gradients: ``forward(predictions, targets)`` returns
    ``(loss, L_mixup, L_rank)`` as 0-d fp32 tensors on the device (``fs2_rank_loss_fwd_bwd``);
    ``loss`` is differentiable with respect to ``hi, hj, ri, rj``, the two parts are values."""

    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha = alpha
        self.beta = beta

    def forward(self, predictions, targets):
        y_emo, y_neu = targets
        lam_i, lam_j, _, _, hi, hj, ri, rj = predictions
        if hi.device.type != "cuda":
            raise RuntimeError("RankTrainLoss runs only on the HIP device (libfs2_hip.so); there "
                               "is no CPU path")
        N.load()
        return _RankLossFunction.apply(hi, hj, ri, rj, lam_i, lam_j, y_emo, y_neu,
                                       float(self.alpha), float(self.beta))


def rank_train_step(model, criterion, optim, batch):
    """The body of rank_model/train.py:28-43 for one batch: ``batch`` is the rank collate's dict
    (``emo_X``, ``neu_X`` (B, T, n_mels+2), ``emotions``, ``length``; optionally ``lambdas``
    (2, B) instead of the Beta(1, 1) draw), as ``fastspeech2.rank_dataset`` makes it.  Returns ``(loss, L_mixup, L_rank)`` as detached 0-d
    device tensors: nothing here waits for the device, the caller's ``.item()`` does."""
    dev = next(model.parameters()).device
    emo_X, neu_X = batch["emo_X"].to(dev), batch["neu_X"].to(dev)
    emotions, length = batch["emotions"].to(dev), batch["length"].to(dev)
    targets = (emotions, torch.zeros_like(emotions))                        # train.py:32
    predictions = model(emo_X, neu_X, emotions, length, lambdas=batch.get("lambdas"))
    loss, L_mixup, L_rank = criterion(predictions, targets)
    optim.zero_grad()
    loss.backward()
    optim.step()
    return loss.detach(), L_mixup.detach(), L_rank.detach()
