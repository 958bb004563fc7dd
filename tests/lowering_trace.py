"""CPU launch trace of the engine's conv / linear lowering (no GPU, no library).

``trace()`` drives FS2Engine's own ``_fwd``, ``_dgrad_impl`` and ``_wgrad_impl`` as unbound
functions on a stub engine whose tensors live on the ``meta`` device, with the engine module's
``ops`` replaced by a recorder.  A case's record is the list of everything the call would have
enqueued or allocated, in order:

    "ws(15925248)"                    a workspace request
    "km_image(dy, 1536, 31680)"       a K-major image request
    "gemm(1536, 3456, 31680, km.dy, 31680, km.x, 31680, ws2, 3456; dt=1 conv=(6, 977, 9, 384) ...)"
    "torch.empty[1, 31520, 384]f32"   a torch op that is not a view (allocations, add_, ...)

or the refusal the call raised.  A tensor is written as its role (the arguments of the call
under trace, ws1, ws2, ... and km.dy / km.x as requested, new0, ... as allocated), a view of
one as role[shape]+storage offset; scalars and tuples verbatim; keyword arguments in the order of the
real op's signature, those at their default left out.  tests/golden/make_golden_lowering.py
records the trace of a commit, tests/test_lowering_host.py compares the tree against it.
"""
import contextlib
import ctypes
import dataclasses
import inspect
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import PKG  # noqa: F401  (puts the package on sys.path)
from fastspeech2 import _native as N
from fastspeech2 import engine as E
from fastspeech2 import load_config, ops as real_ops
from fastspeech2.model import FS2Config

LIM = 0x7fffffff
BATCHES = [(32, 977), (32, 200), (32, 640), (1, 640), (4, 77), (3, 130), (2, 50), (1, 5)]
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.uint8: "u8"}
_BUF = (ctypes.c_char * 64)()
ADDR = (ctypes.addressof(_BUF) + 15) // 16 * 16    # stands for every tensor of a re-planned gemm
_VIEWS = {"view", "_unsafe_view", "slice", "select", "as_strided", "permute", "transpose", "t",
          "reshape", "detach", "alias", "expand", "unsqueeze", "squeeze"}


def _same(v, default):
    return not isinstance(v, torch.Tensor) and v == default


class _Rec:
    """one case's record; names tensors by role"""

    def __init__(self):
        self.out = []
        self.roles = {}
        self.keep = []      # named tensors stay alive, so no id is reused within a case
        self.quiet = 0

    def name(self, t, role):
        self.roles[id(t)] = role
        self.keep.append(t)
        return t

    def new(self, role, *shape, dtype):
        self.quiet += 1
        try:
            return self.name(torch.empty(*shape, dtype=dtype, device="meta"), role)
        finally:
            self.quiet -= 1

    def fmt(self, v):
        if isinstance(v, torch.Tensor):
            base = v._base if v._base is not None else v
            role = self.roles.get(id(v)) or self.roles.get(id(base))
            if role is None:          # allocated by the code under trace: numbered as first seen
                role = f"new{sum(r.startswith('new') for r in self.roles.values())}"
                self.name(base, role)
            if v._base is None or self.roles.get(id(v)):
                return role       # a whole buffer: its size stands where it was made or asked for
            return f"{role}{list(v.shape)}+{v.storage_offset()}"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.fmt(x) for x in v) + ")"
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}={self.fmt(x)}" for k, x in v.items()) + "}"
        return repr(v)

    def call(self, fn, args, kw):
        real = getattr(real_ops, fn, None)
        if real is not None:      # keyword arguments in the signature's order, defaults dropped
            par = inspect.signature(real).parameters
            kw = {k: kw[k] for k in par if k in kw and not _same(kw[k], par[k].default)}
        s = ", ".join(self.fmt(a) for a in args)
        if kw:
            s += "; " + " ".join(f"{k}={self.fmt(v)}" for k, v in kw.items())
        self.out.append(f"{fn}({s})")
        if fn == "gemm":
            addr = lambda v: ADDR if isinstance(v, torch.Tensor) else v  # noqa: E731
            self.gemms.append(([addr(a) for a in args], {k: addr(v) for k, v in kw.items()}))


class _Ops:
    """stands in for fastspeech2.ops inside the engine module: records every call"""
    round_up = staticmethod(real_ops.round_up)
    pad_transpose_ws = staticmethod(real_ops.pad_transpose_ws)
    EPC = real_ops.EPC

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, fn):
        return lambda *a, **kw: self._rec.call(fn, a, kw)


class _TorchOps(TorchDispatchMode):
    """records the torch ops of the code under trace that are not views"""

    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__
        if not self.rec.quiet and name not in _VIEWS and isinstance(out, torch.Tensor):
            self.rec.out.append(f"torch.{name}{list(out.shape)}{_DT[out.dtype]}")
        return out


class _Stub:
    """what the lowering methods read of an engine; every other attribute (the predicate
    methods, _dtag, PRED1, ...) is FS2Engine's own, bound to the stub"""
    timer = None
    dev = "meta"

    def __getattr__(self, name):
        f = getattr(E.FS2Engine, name)
        return f.__get__(self) if callable(f) else f

    def ws(self, n):
        self.rec.out.append(f"ws({int(n)})")
        return self.rec.new(f"ws{sum(o.startswith('ws(') for o in self.rec.out)}", int(n),
                            dtype=torch.float32)

    # the engine's own two ask torch.cuda whether a capture is running, which raises without a GPU
    def _km_image(self, key, C, ld):
        self.rec.out.append(f"km_image({key}, {C}, {ld})")
        return self.rec.new(f"km.{key}", C * ld, dtype=torch.bfloat16)

    def _km_offs(self, grad_end, P):
        self.rec.out.append(f"km_offs({self.rec.fmt(grad_end)}, {P})")
        B = grad_end.numel()
        return self.rec.new("offs", real_ops.round_up(B + 1, 16) + 16, dtype=torch.int32)


def _switch_modules():
    """the module(s) that define the tap-inner switches"""
    try:
        from fastspeech2 import lowering
    except ImportError:
        lowering = None
    return [m for m in (lowering, E) if m is not None and hasattr(m, "_TAP_INNER")]


@contextlib.contextmanager
def switches(tap_inner, tap_inner_fwd):
    mods = _switch_modules()
    old = [(m, m._TAP_INNER, m._TAP_INNER_FWD) for m in mods]
    for m in mods:
        m._TAP_INNER, m._TAP_INNER_FWD = tap_inner, tap_inner_fwd
    try:
        yield
    finally:
        for m, a, b in old:
            m._TAP_INNER, m._TAP_INNER_FWD = a, b


def make_stub(adt):
    """stub engine of the default config in activation dtype ``adt``, built by the engine's own
    _weight_specs and _fuse_pred_conv1 (over a layout in which the two predictor conv1 weights
    and biases are adjacent, as model._group_key lays them out) under the current switches"""
    kw = load_config()["model"]["fastspeech2"]
    s = _Stub()
    s.cfg = FS2Config(**{f.name: kw.get(f.name, 4) for f in dataclasses.fields(FS2Config)})
    s.adt, s.dt = adt, N.dtype_code(adt)
    s.epc = real_ops.EPC[s.dt]
    s.rec = rec = _Rec()
    s._wspecs = E.FS2Engine._weight_specs(s)
    s.params, s.grads = {}, {}
    for n, (O, C, KW) in s._wspecs.items():
        g = rec.new("dW", O, KW, C, dtype=torch.float32)
        s.grads[n] = rec.name(g.permute(0, 2, 1) if KW > 1 else g.view(O, C), "dW")
    wd, wp = "durPred.conv1.conv.weight", "pitchPred.conv1.conv.weight"
    bd, bp = "durPred.conv1.conv.bias", "pitchPred.conv1.conv.bias"
    O, C, KW = s._wspecs[wd]
    nw = O * C * KW
    s.m = type("M", (), {})()
    s.m._layout = [(wd, 0, nw, None, None), (wp, nw, nw, None, None),
                   (bd, 2 * nw, O, None, None), (bp, 2 * nw + O, O, None, None)]
    s.m._flat = rec.new("flat", 2 * nw + 2 * O, dtype=torch.float32)
    s.m._gflat = rec.new("dW", 2 * nw + 2 * O, dtype=torch.float32)
    s._fuse_pred_conv1()
    for n, (O, C, KW) in s._wspecs.items():
        if n.endswith(".conv.weight"):
            b = n.replace("weight", "bias")
            s.grads[b] = rec.new("db", O, dtype=torch.float32)
    s.w = {}
    for n, (O, C, KW) in s._wspecs.items():
        s.w[n] = (rec.new("Wf", O, real_ops.round_up(KW * C, s.epc), dtype=adt),
                  rec.new("Wb", C, KW * O, dtype=adt))
    s.base_roles, s.base_keep = dict(rec.roles), list(rec.keep)
    return s


def site_names(s):
    """one weight per distinct (O, C, KW) and kind: layer 0 of each stack, the predictors'
    unfused convs of one predictor, everything else"""
    out = []
    for n in s._wspecs:
        if ".layers." in n and ".layers.0." not in n:
            continue
        if n.startswith("decoder.") and ".pos_ffn.0." not in n:
            continue        # as the encoder's; only the FFN conv1's lowering reads the stack
        if n.startswith(("durPred.", "pitchPred.", "energyPred.conv2")) or \
                n.startswith("postnet.convs_intermedite.") and ".0." not in n:
            continue        # as energyPred.conv1 / postnet.convs_intermedite.0
        out.append(n)
    return out


def ask(s, question, n, *batch):
    """one of the questions the callers of the three methods ask -- pad_dgrad, tap_inner,
    tap_inner_fwd (of a weight), pad_fwd (of M, T), pad_dgrad_fits (of B, T): answered by the
    engine method of that name where the engine has one, else by fastspeech2.lowering"""
    if hasattr(E.FS2Engine, "_" + question):
        return bool(getattr(s, "_" + question)(n, *batch))
    from fastspeech2 import lowering as L
    if question == "pad_fwd":
        return bool(L.fwd_padded(*s._wspecs[n], s.dt, *batch, s._okc[n]))
    if question == "pad_dgrad_fits":
        return L.dgrad_refusal(*s._wspecs[n], *batch) is None
    return bool(s._okc[n] & {"pad_dgrad": L.W_REV, "tap_inner": L.W_TAP_INNER,
                             "tap_inner_fwd": L.W_TAP_INNER_FWD}[question])


def images(s):
    """the weight-image predicates for every weight of the stub under the current switches:
    {weight: "pad_dgrad tap_inner tap_inner_fwd" as 0/1} of those with any set, and how many
    weights were asked"""
    bits = {n: "".join("01"[ask(s, q, n)] for q in ("pad_dgrad", "tap_inner", "tap_inner_fwd"))
            for n in s._wspecs}
    return {"weights": len(bits), **{n: b for n, b in bits.items() if b != "000"}}


def run(s, fn, *args, **kw):
    """one case: the record of FS2Engine.<fn>(stub, ...) or its refusal"""
    rec = s.rec
    rec.out, rec.gemms = [], []
    old = E.ops
    E.ops = _Ops(rec)
    try:
        with _TorchOps(rec):
            ret = getattr(E.FS2Engine, fn)(s, *args, **kw)
        if ret is not None:
            rec.out.append(f"return {ret!r}")
    except (ValueError, RuntimeError) as e:
        rec.out.append(f"{type(e).__name__}: {e}")
    finally:
        E.ops = old
        rec.roles, rec.keep = dict(s.base_roles), list(s.base_keep)   # the case's own are done
    return rec.out


def _edge(per_b, extra=0):
    """largest B with B * per_b + extra < 2^31 - 1"""
    return (LIM - 1 - extra) // per_b


def short(n):
    """a weight's name in the case ids"""
    for a, b in (("encoder.layers.0.", "enc."), ("decoder.layers.0.", "dec."), (".conv.weight", ""),
                 (".w.weight", ""), (".weight", ""), ("_weight", ""), ("self_att.att.", "")):
        n = n.replace(a, b)
    return n


def cases(adt, sw, gemms):
    """{case id: record} of every case in activation dtype ``adt`` under switches ``sw``;
    ``gemms[case id]``: the (args, kwargs) of its gemm calls, ADDR for every tensor"""
    out = {}

    def do(key, fn, *a, head=(), **kw):
        out[key] = list(head) + run(s, fn, *a, **kw)
        gemms[key] = s.rec.gemms

    with switches(*sw):
        s = make_stub(adt)
        d = _DT[adt] + ("" if sw == (0, 0) else " tap-inner")
        bf16 = s.dt == N.BF16
        t = lambda role, *shape, dtype=adt: s.rec.new(role, *shape, dtype=dtype)  # noqa: E731
        out[f"images {_DT[adt]} sw{sw}"] = images(s)
        for n in site_names(s):
            O, C, KW = s._wspecs[n]
            P = (KW - 1) // 2
            ffn1 = ".pos_ffn.0." in n
            if sw != (0, 0) and not ffn1:
                continue        # the switches reach the FFN conv1 only
            # every batch shape in bf16 with the switches off and for every weight gradient; a
            # large, a small and a tiny one otherwise (fp32: the large and the tiny one); for a
            # conv the reflect-pad limit T = P, P + 1
            few = [BATCHES[0], BATCHES[4], BATCHES[7]] if bf16 else [BATCHES[0], BATCHES[7]]
            edge = [(2, P), (2, P + 1)] if KW > 1 else []
            bts = (BATCHES if bf16 and sw == (0, 0) else few) + edge
            fwd_b, dg_b = [], []
            if ffn1 and bf16 and n.startswith("decoder."):
                T = 1000    # either side of each ps_plain_ok limit
                fwd_b = [(b + i, T) for b in (_edge((T + 2 * P) * C * 2), _edge(T * O * 2))
                         for i in (0, 1)]
                dg_b = [(b + i, T) for b in (_edge((T + 2 * P) * O * 2, 4 * P * O),
                                             _edge((T + 2 * P) * C * 4), _edge(T * O * 2))
                        for i in (0, 1)]
            for B, T in (bts if ffn1 else few + edge) + fwd_b:   # only the FFN conv1's reads B, T
                M = B * T
                ldx = real_ops.round_up(C, s.epc)
                # as _fft_fwd, the one caller that asks _pad_fwd: the FFN conv1's reflect-padded
                # image where it says so, else X itself
                pad = ffn1 and ask(s, "pad_fwd", n, M, T)
                X = (t("img", B * (T + 2 * P) + 2 * P, C),) if pad else t("X", M, ldx)
                do(f"fwd {short(n)} {d} B{B} T{T}", "_fwd", X, ldx, M, T, n, t("out", M, O), O,
                   head=[f"pad_fwd={pad}"] * ffn1, bias=t("bias", O, dtype=torch.float32), relu=1)
            for B, T in (bts if KW > 1 else few) + dg_b:          # a 1x1's reads neither
                M = B * T
                key = f"dgrad {short(n)} {d} B{B} T{T}"
                n_out = 2 * s.cfg.enc_d_model if n.startswith("concat_proj") else None
                ldo = n_out or C
                # as _fft_bwd: the zero-padded dY image where _pad_dgrad takes it (a batch past
                # _pad_dgrad_fits is refused there, before any launch), else dY itself
                dY, head = t("dY", M, O), []
                if ffn1 and ask(s, "pad_dgrad", n):
                    head = [f"pad_dgrad_fits={ask(s, 'pad_dgrad_fits', n, B, T)}"]
                    if "False" in head[0]:
                        out[key] = head
                        continue
                    dY = (t("img", B * (T + 2 * P) + 2 * P, O),)
                do(key, "_dgrad_impl", dY, O, M, T, n, t("out", M, ldo), ldo, n_out, head=head,
                   residual=t("res", M, ldo), ldr=ldo)
            if sw != (0, 0):
                continue        # the weight gradient reads neither switch
            for B, T in BATCHES + edge:
                M = B * T
                n_cols = real_ops.round_up(C, 8) if n.startswith("concat_proj") else None
                # a second pair of row pitches, of whole 16-byte chunks (in fp32 that is no
                # multiple of 8), and for the convs of the K-major path in bf16 a third, odd
                # pair, which closes that path's gate (fs2_gemm refuses such a pitch in bf16:
                # these calls are among the fixture's plan_exceptions)
                lds = [(O, n_cols or C), (O + s.epc, (n_cols or C) + s.epc), (O + 1, C + 1)]
                # (pitches, dy_img, grad_end, ctas): all 16 forms at the bench shape of the
                # decoder's FFN conv1, three at every site's bench shape and at the small shapes
                # of the convs the K-major path takes, else the plain one
                forms = [(lds[0], 0, 0, 0)]
                if (B, T) == bts[0] and ffn1 and bf16 and n.startswith("decoder."):
                    forms = [(ld, im, ge, ct) for ld in lds[:2] for im in (0, 1) for ge in (0, 1)
                             for ct in (0, 208)]
                elif (B, T) == bts[0] or KW >= 5 and bf16 and (B, T) in ((4, 77), (2, P + 1)):
                    forms += [(lds[1], 0, 0, 208), (lds[0], 1, 1, 208)]
                if KW >= 5 and bf16 and (B, T) in (bts[0], (4, 77), (2, P + 1)):
                    forms += [(lds[2], 0, 1, 208), (lds[2], 1, 0, 0)]
                for (lddy, ldx), im, ge, ct in forms:
                    key = f"wgrad {short(n)} {d} B{B} T{T} ld{lddy},{ldx}" + \
                        " dy_img" * im + " grad_end" * ge + f" ctas{ct}" * bool(ct)
                    bias = n.replace("weight", "bias") if n.endswith(".conv.weight") else None
                    dy_img = t("dy_img", (B + 1) * (T + 2 * P), lddy)[T:] if im else None
                    grad_end = t("grad_end", B, dtype=torch.int32) if ge else None
                    do(key, "_wgrad_impl", t("dY", M, lddy), lddy, t("X", M, ldx), ldx, M, T, n,
                       n_cols, None, bias, dy_img, ct, grad_end)
    return out


def trace(gemms=None):
    """every case: both dtypes; the FFN conv1 sites with both switches off and both on, the
    weight-image predicates under all four settings"""
    out = {}
    gemms = {} if gemms is None else gemms
    for adt in (torch.bfloat16, torch.float32):
        for sw in ((0, 0), (1, 1))[:1 + (adt == torch.bfloat16)]:   # fp32 reads no switch
            out.update(cases(adt, sw, gemms))
        for sw in ((1, 0), (0, 1), (1, 1)):
            with switches(*sw):
                out[f"images {_DT[adt]} sw{sw}"] = images(make_stub(adt))
    return out


def split_mismatches(gemms):
    """re-plans every recorded gemm call with fs2_gemm_plan (needs the built library) and returns
    "case id #i: requested -> planned" for the calls into split-K slices (split_stride > 0) whose slice count the plan does not keep, and
    "case id #i: fs2_gemm_plan returned rc" for the calls it refuses"""
    bad = []
    for key, calls in gemms.items():
        for i, (args, kw) in enumerate(calls):
            try:
                pl = real_ops.gemm_plan(*args, **kw)
            except RuntimeError as e:
                bad.append(f"{key} #{i}: {e}")
                continue
            if kw.get("split_stride", 0) > 0 and pl.split_k != kw["split_k"]:
                bad.append(f"{key} #{i}: {kw['split_k']} -> {pl.split_k}")
    return bad


if __name__ == "__main__":
    tr = trace()
    for k in sys.argv[1:] or tr:
        for kk, v in tr.items():
            if k in kk:
                print(kk, v, sep="\n    ")
