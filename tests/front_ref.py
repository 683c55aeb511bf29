"""float64 reference of everything in front of the generator, one function per kind of step, and the step-by-step teacher-forced check —
TEST INFRASTRUCTURE (numpy on the CPU).

The text encoder, the projection, the path expansion, the flow couplings and the duration predictor have no rounding but fp32's own, so a
step that is fed the GPU's own fp32 inputs differs from a float64 evaluation of the same formula by accumulation order and fp32 rounding
only, and the project's op-level rule applies as it stands:   |Δ| ≤ OP_TOL · max(1, ‖ref‖∞)   (conftest). No allowance, no measured constant.

How a schedule is walked (verify): the step names come from the device (`piper_hip_voice_profile` / "@steps"), in order. `Walker.plan` maps
a name to (what the step reads, what it writes, the float64 formula); a name it does not recognise raises UnknownStep, so a new schedule
cannot slip past. Per step the verifier reads the inputs with "<tensor>@<previous step>", the outputs with "<tensor>@<this step>"
(piper_hip_voice_tap's step selector) and compares. Tensors are [C, len] of ONE item cut to its true length; positions past it are zero
inputs — on the device the buffers are NOT zero there, every kernel has to mask by len_ptr.

The flow's latent travels as two physical halves (channels [0, half) and [half, inter)) through the buffers front.zp / front.zflip; Flip is
a reversed channel map, never a copy (csrc/voice.hip build_flow). The walker tracks both the same way the builder does, from the step
names alone. A folded tail (…res_skip_post_sub[_flip_preN]) is referenced by the UNFOLDED composition from the raw blob weights:
res_skip conv → skip sum → post → x1 − m → Flip → next pre.

`Device` is the tap interface: `GpuDevice` serves it from a HipRuntime slot, `SimDevice` is a stand-in that evaluates the same steps in
float32 with another summation order (channels reversed, taps reversed) — the CPU tests run the verifier over it, clean and with planted defects.
"""
import re
import time

import numpy as np
import torch

import katdata as kd
import piper_hip as ph
from conftest import OP_TOL

NOISE_SCALE = 0.667
DUR_REL = 1e-4     # an id whose float64 length_scale · exp(logw) lies within this (relative) of an integer is not compared …
DUR_SHARE = 0.01   # … and at most this share of a case's ids may be left out that way


class UnknownStep(AssertionError):
    pass


class UnitMismatch(AssertionError):
    """A step beyond its bound: .step, .tensor, .item, .result"""

    def __init__(self, msg, step, tensor, item, result):
        super().__init__(msg)
        self.step, self.tensor, self.item, self.result = step, tensor, item, result


def base_tol(ref):
    ref = np.asarray(ref)
    return OP_TOL * max(1.0, float(np.max(np.abs(ref))) if ref.size else 0.0)


def compare(got, ref):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    tol = base_tol(ref)
    if not ref.size:
        return dict(err=0.0, bound=tol, ratio=0.0, ok=True, columns=np.zeros(0, np.int64), worst=())
    d = np.abs(got - ref)
    d = np.where(np.isfinite(d), d, np.inf)  # NaN counts as beyond
    bad = ~(d <= tol)
    return dict(err=float(d.max()), bound=tol, ratio=float(d.max() / tol), ok=not bad.any(), columns=np.unique(np.nonzero(bad)[-1]),
                worst=tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape)))


# ------------------------------------------------------------------------------------------------ the units
class FrontRef:
    """dtype float64: the reference. float32 with reverse=True: an honest fp32 implementation in another summation order (the stand-in)."""

    def __init__(self, cfg, blob, dtype=np.float64, reverse=False):
        self.cfg, self.dt, self.rev = cfg, dtype, reverse
        blob = np.asarray(blob, np.float32)
        self.raw = {e["name"]: blob[e["offset"]:e["offset"] + e["count"]].reshape(e["shape"]) for e in ph.blob_layout(cfg)}
        self._w = {}

    def W(self, name):
        if name not in self._w:
            self._w[name] = np.asarray(self.raw[name], self.dt)
        return self._w[name]

    def A(self, x):
        return np.asarray(x, self.dt)

    # ---- primitives
    def conv(self, x, name, pad=0, bias=True):
        """'same' conv of x [Cin, L] with weight [Cout, Cin, K], zero padding `pad` either side."""
        w = self.W(name + ".weight")
        x = self.A(x)
        K, L = w.shape[2], x.shape[1]
        xp = np.pad(x, ((0, 0), (pad, pad)))
        y = np.zeros((w.shape[0], L), self.dt)
        for k in (range(K - 1, -1, -1) if self.rev else range(K)):
            y += (w[:, ::-1, k] @ xp[::-1, k:k + L]) if self.rev else (w[:, :, k] @ xp[:, k:k + L])
        if bias:
            y = y + self.W(name + ".bias")[:, None]
        return y

    def layernorm(self, x, gname, bname, eps=1e-5):
        x = self.A(x)
        xs = x[::-1] if self.rev else x
        mean = xs.sum(0, dtype=self.dt) / self.dt(x.shape[0])
        var = ((xs - mean) ** 2).sum(0, dtype=self.dt) / self.dt(x.shape[0])
        return (x - mean) / np.sqrt(var + self.dt(eps)) * self.W(gname)[:, None] + self.W(bname)[:, None]

    def ln_enc(self, x, which, l, eps=1e-5):
        return self.layernorm(x, f"enc_p.encoder.norm_layers_{which}.{l}.gamma", f"enc_p.encoder.norm_layers_{which}.{l}.beta", eps)

    # ---- encoder
    def embed(self, ids):
        """Gather · √H; a negative id wraps once, what is still out of range gathers 0.0 (pinned in test_gpu_voice.py)."""
        c = self.cfg
        emb = self.W("enc_p.emb.weight")
        ids = np.asarray(ids, np.int64).copy()
        ids[ids < 0] += c.n_vocab
        ok = (ids >= 0) & (ids < c.n_vocab)
        x = emb[np.where(ok, ids, 0)] * ok[:, None]
        return (x * self.dt(np.sqrt(self.dt(c.hidden)))).T.copy()

    def qkv(self, x, l):
        P = f"enc_p.encoder.attn_layers.{l}."
        return np.concatenate([self.conv(x, P + n) for n in ("conv_q", "conv_k", "conv_v")], 0)

    def attention(self, qkv, l, length=None):
        """Relative-position attention of one item from its [3H, T] q ; k ; v (window-limited learned key / value offsets).
        length: keys at and past it are excluded (None: every column is real)."""
        c = self.cfg
        H, nh = c.hidden, c.n_heads
        d, w = H // nh, c.window
        qkv = self.A(qkv)
        T = qkv.shape[1]
        P = f"enc_p.encoder.attn_layers.{l}."
        ek, ev = self.W(P + "emb_rel_k").reshape(-1, d), self.W(P + "emb_rel_v").reshape(-1, d)
        q, k, v = (qkv[i * H:(i + 1) * H].reshape(nh, d, T).transpose(0, 2, 1) for i in range(3))
        qs = q / self.dt(np.sqrt(self.dt(d)))
        scores = qs @ k.transpose(0, 2, 1)
        rel = qs @ ek.T  # [nh, T, 2w + 1]
        off = np.arange(T)[None, :] - np.arange(T)[:, None] + w  # [i, j] → index of the offset j − i
        valid = (off >= 0) & (off <= 2 * w)
        offc = np.clip(off, 0, 2 * w)
        scores = scores + np.where(valid[None], np.take_along_axis(rel, np.broadcast_to(offc[None], scores.shape), 2), 0)
        if length is not None:
            scores = np.where((np.arange(T) < length)[None, None, :], scores, -np.inf)
        scores = scores - scores.max(-1, keepdims=True)
        p = np.exp(scores)
        p = p / p.sum(-1, keepdims=True)
        out = p @ v
        for r in range(2 * w + 1):
            i = np.arange(max(0, w - r), min(T, T + w - r))
            if i.size:
                out[:, i] += p[:, i, i + r - w][..., None] * ev[r][None, None, :]
        return out.transpose(0, 2, 1).reshape(H, T)

    def conv_o(self, att, l):
        return self.conv(att, f"enc_p.encoder.attn_layers.{l}.conv_o")

    def ffn1(self, x1, l):
        kf = self.cfg.ffn_kernel
        return np.maximum(self.conv(x1, f"enc_p.encoder.ffn_layers.{l}.conv_1", (kf - 1) // 2), 0)

    def ffn2(self, ff, l):
        kf = self.cfg.ffn_kernel
        return self.conv(ff, f"enc_p.encoder.ffn_layers.{l}.conv_2", (kf - 1) // 2)

    def proj(self, x):
        return self.conv(x, "enc_p.proj")

    # ---- expansion and flow
    def expand_noise(self, stats, durations, noise, noise_scale):
        I = self.cfg.inter
        stats = self.A(stats)
        f2i = np.repeat(np.arange(len(durations)), np.asarray(durations, np.int64))
        return stats[:I, f2i] + (self.A(noise) * np.exp(stats[I:, f2i])) * self.dt(noise_scale)

    def flow_pre(self, f, x0):
        return self.conv(x0, f"flow.flows.{2 * f}.pre")

    def in_gate(self, f, i, h):
        H = self.cfg.hidden
        K = self.cfg.wn_kernel
        a = self.conv(h, f"flow.flows.{2 * f}.enc.in_layers.{i}", (K - 1) // 2)
        return np.tanh(a[:H]) * (1 / (1 + np.exp(-a[H:])))

    def res_skip(self, f, i, acts):
        return self.conv(acts, f"flow.flows.{2 * f}.enc.res_skip_layers.{i}")

    def post(self, f, skip):
        return self.conv(skip, f"flow.flows.{2 * f}.post")

    # ---- duration predictor
    def dds_layer(self, base, i, x):
        c = self.cfg
        K = c.dp_kernel
        dil = K ** i
        x = self.A(x)
        w, b = self.W(f"{base}.convs.convs_sep.{i}.weight"), self.W(f"{base}.convs.convs_sep.{i}.bias")
        pad = (K * dil - dil) // 2
        L = x.shape[1]
        xp = np.pad(x, ((0, 0), (pad, pad)))
        y = np.zeros_like(x)
        for k in (range(K - 1, -1, -1) if self.rev else range(K)):
            y += w[:, 0, k][:, None] * xp[:, k * dil:k * dil + L]
        y = y + b[:, None]
        y = self.gelu(self.layernorm(y, f"{base}.convs.norms_1.{i}.gamma", f"{base}.convs.norms_1.{i}.beta"))
        y = self.conv(y, f"{base}.convs.convs_1x1.{i}")
        y = self.gelu(self.layernorm(y, f"{base}.convs.norms_2.{i}.gamma", f"{base}.convs.norms_2.{i}.beta"))
        return x + y

    def gelu(self, x):
        x = np.asarray(x, self.dt)
        return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / np.sqrt(self.dt(2.0))))).numpy())

    def spline_inverse(self, x, h, bin_shift=0):
        """x [T] (the half to transform), h [3·bins − 1, T] → inverse rational-quadratic spline with linear tails."""
        c = self.cfg
        nb, B, fc = c.dp_bins, self.dt(c.dp_tail_bound), self.dt(c.hidden)
        h = self.A(h).T
        x = self.A(x)
        uw, uh, ud = h[:, :nb] / np.sqrt(fc), h[:, nb:2 * nb] / np.sqrt(fc), h[:, 2 * nb:]
        mb = self.dt(1e-3)

        def softmax(a):
            e = np.exp(a - a.max(-1, keepdims=True))
            return e / e.sum(-1, keepdims=True)

        def softplus(a):
            return np.where(a > 0, a + np.log1p(np.exp(-np.abs(a))), np.log1p(np.exp(-np.abs(a))))

        const = np.log(np.exp(1 - mb) - 1)
        ud = np.pad(ud, ((0, 0), (1, 1)), constant_values=const)
        inside = (x >= -B) & (x <= B)

        def knots(u):
            wd = mb + (1 - mb * nb) * softmax(u)
            cw = np.pad(np.cumsum(wd, -1), ((0, 0), (1, 0))) * (2 * B) - B
            cw[:, 0], cw[:, -1] = -B, B
            return cw, cw[:, 1:] - cw[:, :-1]

        cw, widths = knots(uw)
        chh, heights = knots(uh)
        derivs = mb + softplus(ud)
        loc = chh.copy()
        loc[:, -1] += 1e-6
        idx = np.clip(np.sum(x[:, None] >= loc, -1) - 1 + bin_shift, 0, nb - 1)[:, None]
        g = lambda a: np.take_along_axis(a, idx, -1)[:, 0]
        icw, ibw, ich, ih = g(cw), g(widths), g(chh), g(heights)
        idl = ih / ibw
        d0, d1 = g(derivs), g(derivs[:, 1:])
        i1 = d0 + d1 - 2 * idl
        i2 = x - ich
        i3 = i2 * i1
        a = ih * (idl - d0) + i3
        b = ih * d0 - i3
        cc = -idl * i2
        with np.errstate(invalid="ignore", divide="ignore"):
            root = (2 * cc) / (-b - np.sqrt(b * b - 4 * a * cc))
        return np.where(inside, root * ibw + icw, x).astype(self.dt)


# ------------------------------------------------------------------------------------------------ the schedule walker
class Inputs:
    """What prepare staged for ONE item: ids; durations + noise [inter, F] + noise_scale (a plan with a flow); dp_noise [2, T] + noise_w +
    length_scale (the predictor plan)."""

    def __init__(self, ids, durations=None, noise=None, noise_scale=NOISE_SCALE, dp_noise=None, noise_w=0.8, length_scale=1.0):
        self.ids = np.asarray(ids, np.int64)
        self.durations = None if durations is None else np.asarray(durations, np.int64)
        self.noise, self.noise_scale = noise, noise_scale
        self.dp_noise, self.noise_w, self.length_scale = dp_noise, noise_w, length_scale


KINDS = {}  # step kind → description (the table of the module docstring of tests/test_gpu_front_exact.py)


class Walker:
    """Fed the step names of a schedule in order; plan(name) → (kind, reads, writes, fn). reads / writes: tap names.
    fn(R, bufs, inp) → {tap name: array or (array, channel slice)} of ONE item, bufs = {tap name: [C, len]} of what it reads."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.cur_f = None
        self.flipped = False
        self.zloc = ["front.zp", "front.zp"]  # the buffer physical half k was last written to
        self.dds_src = None

    # the physical latent from its two halves, and the logical one the coupling sees
    def _phys(self, bufs, zloc):
        half = self.cfg.inter // 2
        return np.concatenate([bufs[zloc[0]][:half], bufs[zloc[1]][half:]], 0)

    def _enter(self, f):
        if f != self.cur_f:
            self.cur_f = f
            self.flipped = not self.flipped

    def plan(self, name):
        c = self.cfg
        H, I = c.hidden, c.inter
        half = I // 2
        X, X1, QKV, ATT, Y, FF, ST = ("front." + n for n in ("x", "x1", "qkv", "att", "y", "ff", "stats"))
        Hh, ACTS, SKIP = "front.h", "front.acts", "front.skip"
        if name == "embed":
            return "embed", [], [X], lambda R, b, inp: {X: R.embed(inp.ids)}
        m = re.fullmatch(r"enc(\d+)\.(\w+)", name)
        if m:
            l, op = int(m.group(1)), m.group(2)
            if op == "qkv":
                return "qkv", [X], [QKV], lambda R, b, inp: {QKV: R.qkv(b[X], l)}
            if op == "ln2_qkv":
                def fn(R, b, inp):
                    x = R.ln_enc(b[Y], 2, l - 1)
                    return {X: x, QKV: R.qkv(x, l)}
                return "ln2_qkv", [Y], [X, QKV], fn
            if op == "rel_attention":
                return "rel_attention", [QKV], [ATT], lambda R, b, inp: {ATT: R.attention(b[QKV], l)}
            if op == "attention_o_add_ln1":
                return "attention_o_add_ln1", [QKV, X], [X1], lambda R, b, inp: {X1: R.ln_enc(R.A(b[X]) + R.conv_o(R.attention(b[QKV], l), l), 1, l)}
            if op in ("o_add", "o_add_stats"):
                return op, [ATT, X], [Y], lambda R, b, inp: {Y: R.A(b[X]) + R.conv_o(b[ATT], l)}
            if op == "o":
                return "o", [ATT], [Y], lambda R, b, inp: {Y: R.conv_o(b[ATT], l)}
            if op == "add_ln1":
                return "add_ln", [X, Y], [X1], lambda R, b, inp: {X1: R.ln_enc(R.A(b[X]) + R.A(b[Y]), 1, l)}
            if op == "ln1_ffn1_relu":
                def fn(R, b, inp):
                    x1 = R.ln_enc(b[Y], 1, l)
                    return {X1: x1, FF: R.ffn1(x1, l)}
                return "ln1_ffn1_relu", [Y], [X1, FF], fn
            if op == "ffn1_relu":
                return "ffn1_relu", [X1], [FF], lambda R, b, inp: {FF: R.ffn1(b[X1], l)}
            if op in ("ffn2_add", "ffn2_add_stats"):
                return op, [FF, X1], [Y], lambda R, b, inp: {Y: R.A(b[X1]) + R.ffn2(b[FF], l)}
            if op == "ffn2":
                return "ffn2", [FF], [Y], lambda R, b, inp: {Y: R.ffn2(b[FF], l)}
            if op == "add_ln2":
                return "add_ln", [X1, Y], [X], lambda R, b, inp: {X: R.ln_enc(R.A(b[X1]) + R.A(b[Y]), 2, l)}
            raise UnknownStep(name)
        last_l = c.n_layers - 1
        if name == "enc.ln2_final":
            return "ln2_final", [Y], [X], lambda R, b, inp: {X: R.ln_enc(b[Y], 2, last_l)}
        if name == "enc.ln2_proj":
            def fn(R, b, inp):
                x = R.ln_enc(b[Y], 2, last_l)
                return {X: x, ST: R.proj(x)}
            return "ln2_proj", [Y], [X, ST], fn
        if name == "enc.proj":
            return "proj", [X], [ST], lambda R, b, inp: {ST: R.proj(b[X])}
        if name == "expand_noise":
            def fn(R, b, inp):
                zp = R.expand_noise(b[ST], inp.durations, inp.noise, inp.noise_scale)
                return {"front.zp": zp, "z_p": zp}
            return "expand_noise", [ST], ["front.zp", "z_p"], fn
        if name == "flow.final_flip":
            src = self.zloc[0]
            assert self.zloc[1] == src and self.flipped, "final_flip: both halves in one buffer after an odd number of couplings"
            dst = "front.zflip" if src == "front.zp" else "front.zp"
            self.zloc = [dst, dst]
            self.flipped = False
            return "final_flip", [src], [dst], lambda R, b, inp: {dst: R.A(b[src])[::-1]}
        m = re.fullmatch(r"flow(\d+)\.(.+)", name)
        if m:
            f, op = int(m.group(1)), m.group(2)
            self._enter(f)
            flipped, zloc = self.flipped, list(self.zloc)
            zbufs = sorted(set(zloc))
            logical = (lambda P: P[::-1]) if flipped else (lambda P: P)
            phys = lambda b: self._phys(b, zloc)
            xh = 0 if flipped else 1  # the physical half this coupling's x1 is

            def coupling(R, b, skip_total):
                """→ the physical latent after the coupling, from the physical one in front of it and the complete skip sum"""
                z = logical(R.A(phys(b)))
                out = np.concatenate([z[:half], z[half:] - R.post(f, skip_total)], 0)
                return logical(out)

            def next_h(R, Pn, g):  # the pre of coupling g, which runs next (one more Flip)
                zl = Pn if flipped else Pn[::-1]
                return R.flow_pre(g, zl[:half])

            if op == "pre":
                return "flow_pre", zbufs, [Hh], lambda R, b, inp: {Hh: R.flow_pre(f, logical(R.A(phys(b)))[:half])}
            mm = re.fullmatch(r"wn(\d+)\.(\w+)", op)
            if mm:
                i, sub = int(mm.group(1)), mm.group(2)
                lastl = i + 1 == c.wn_layers
                if sub == "in_gate":
                    return "in_gate", [Hh], [ACTS], lambda R, b, inp: {ACTS: R.in_gate(f, i, b[Hh])}
                if sub == "res_skip" and not lastl:
                    def fn(R, b, inp):
                        rs = R.res_skip(f, i, b[ACTS])
                        return {Hh: R.A(b[Hh]) + rs[:H], SKIP: rs[H:] + (R.A(b[SKIP]) if i else 0)}
                    return "res_skip", [ACTS, Hh] + ([SKIP] if i else []), [Hh, SKIP], fn
                if sub == "res_skip" and lastl:
                    return "res_skip_last", [ACTS] + ([SKIP] if i else []), [SKIP], \
                        lambda R, b, inp: {SKIP: R.res_skip(f, i, b[ACTS]) + (R.A(b[SKIP]) if i else 0)}
                mt = re.fullmatch(r"res_skip_post_sub(?:_flip_pre(\d+))?", sub)
                if mt and lastl:
                    seam = mt.group(1) is not None
                    assert seam == (f > 0) and (not seam or int(mt.group(1)) == f - 1), name
                    zin = zloc[xh]
                    zout = ("front.zflip" if zin == "front.zp" else "front.zp") if seam else zloc[1 - xh]
                    self.zloc[xh] = zout
                    sl = slice(xh * half, (xh + 1) * half)

                    def fn(R, b, inp):
                        Pn = coupling(R, b, R.res_skip(f, i, b[ACTS]) + (R.A(b[SKIP]) if i else 0))
                        out = {zout: (Pn[sl], sl)}
                        if seam:
                            out[Hh] = next_h(R, Pn, f - 1)
                        return out
                    return "folded_tail", [ACTS] + ([SKIP] if i else []) + zbufs, [zout] + ([Hh] if seam else []), fn
                raise UnknownStep(name)
            mt = re.fullmatch(r"post_sub(?:_flip_pre(\d+))?", op)
            if mt:
                seam = mt.group(1) is not None
                assert not seam or int(mt.group(1)) == f - 1, name
                assert zloc[0] == zloc[1], "an unfolded coupling keeps both halves in one buffer"
                zb = zloc[0]

                def fn(R, b, inp):
                    Pn = coupling(R, b, b[SKIP])
                    out = {zb: Pn}
                    if seam:
                        out[Hh] = next_h(R, Pn, f - 1)
                    return out
                return ("seam" if seam else "post_sub"), [SKIP, zb], [zb] + ([Hh] if seam else []), fn
            raise UnknownStep(name)
        # ---- duration predictor
        A0, A1, COND, HSP, Z, LOGW, DUR = ("dp." + n for n in ("a0", "a1", "cond", "hsp", "z", "logw", "dur"))
        if name == "dp.pre":
            self.dds_src = A0
            return "dp_k1", [X], [A0], lambda R, b, inp: {A0: R.conv(b[X], "dp.pre")}
        m = re.fullmatch(r"dp(?:\.flow(\d+))?\.dds(\d+)", name)
        if m:
            base = "dp" if m.group(1) is None else f"dp.flows.{m.group(1)}"
            i = int(m.group(2))
            src = self.dds_src
            dst = A1 if src == A0 else A0
            self.dds_src = dst
            return "dds", [src], [dst], lambda R, b, inp: {dst: R.dds_layer(base, i, b[src])}
        if name == "dp.proj":
            src = self.dds_src
            return "dp_k1", [src], [COND], lambda R, b, inp: {COND: R.conv(b[src], "dp.proj")}
        if name == "dp.init_latent":
            # rows already flipped for the first ConvFlow: row 0 ← noise row 1
            return "init_latent", [], [Z], lambda R, b, inp: {Z: (R.A(inp.dp_noise).reshape(2, -1) * R.dt(np.float32(inp.noise_w)))[::-1]}
        m = re.fullmatch(r"dp\.flow(\d+)\.(\w+)", name)
        if m:
            k, op = int(m.group(1)), m.group(2)
            base = f"dp.flows.{k}"
            if op == "pre_add_cond":
                self.dds_src = A0
                return "dp_k1", [Z, COND], [A0], lambda R, b, inp: {A0: R.conv(R.A(b[Z])[:1], base + ".pre") + R.A(b[COND])}
            if op == "proj":
                src = self.dds_src
                return "dp_k1", [src], [HSP], lambda R, b, inp: {HSP: R.conv(b[src], base + ".proj")}
            if op == "spline_flip":
                # z1 ← spline⁻¹(z1; h), then the Flip in front of the next module as a row swap
                return "spline_flip", [HSP, Z], [Z], lambda R, b, inp: {Z: np.stack([R.spline_inverse(R.A(b[Z])[1], b[HSP]), R.A(b[Z])[0]], 0)}
            raise UnknownStep(name)
        if name == "dp.affine_exp_ceil":
            def fn(R, b, inp):
                lw = (R.A(b[Z])[0] - R.W("dp.flows.0.m").reshape(-1)[0]) * np.exp(-R.W("dp.flows.0.logs").reshape(-1)[0])
                w = np.exp(lw) * R.dt(np.float32(inp.length_scale))
                return {LOGW: lw[None], DUR: np.ceil(w)[None], "_w": w}
            return "affine_exp_ceil", [Z], [LOGW, DUR], fn
        raise UnknownStep(name)


def is_front_step(name):
    return not name.startswith("dec.")


# ------------------------------------------------------------------------------------------------ devices
class GpuDevice:
    """The tap interface over a prepared, launched and collected HipRuntime slot (predict=True: the cached predictor plan of its bucket)."""

    def __init__(self, rt, slot, lensT, lensF, predict=False):
        self.rt, self.slot, self.lensT, self.lensF = rt, slot, list(lensT), list(lensF)
        self.prefix = "predict:" if predict else ""
        self._steps = rt.steps(slot, predict)

    def steps(self):
        return self._steps

    def read(self, tensor, step):
        raw = self.rt.tap(self.slot, f"{self.prefix}{tensor}@{step}")
        lens = self.lensF if tensor in ("z_p", "z") or tensor.split(".")[-1] in ("zp", "zflip", "h", "acts", "skip") and tensor.startswith("front.") \
            else self.lensT
        assert raw.size % max(sum(lens), 1) == 0, (tensor, raw.size, lens)
        C = raw.size // max(sum(lens), 1)
        offs = np.concatenate([[0], np.cumsum([C * n for n in lens])])
        out = [raw[offs[b]:offs[b + 1]].reshape(C, -1) for b in range(len(lens))]
        if tensor == "dp.dur":
            out = [o.view(np.int32).astype(np.float64) for o in out]
        return out


class SimDevice:
    """A stand-in for the device: the steps of `names` evaluated by R (an honest float32 FrontRef in another summation order) over buffers
    that persist from step to step, each stored tensor rounded to fp32; every step's outcome is kept, so read(tensor, step) serves the tap
    interface. defect(step name, R, bufs, inp, out) may alter what a step writes (the planted defects of the CPU tests). Columns past an
    item's true length do not exist here: a defect that reads them plants what it needs itself."""

    def __init__(self, cfg, R, names, inputs, defect=None):
        self.names = list(names)
        self.snap = {}
        for b, inp in enumerate(inputs):
            W = Walker(cfg)
            bufs = {}
            for name in self.names:
                kind, reads, writes, fn = W.plan(name)
                out = fn(R, {k: bufs[k] for k in reads}, inp)
                if defect:
                    out = defect(name, R, {k: bufs[k] for k in reads}, inp, out) or out
                for k, v in out.items():
                    if k.startswith("_"):
                        continue
                    if isinstance(v, tuple):
                        if k not in bufs:
                            bufs[k] = np.zeros((cfg.inter, v[0].shape[1]), np.float32)
                        bufs[k] = bufs[k].copy()
                        bufs[k][v[1]] = np.asarray(v[0], np.float32)
                    else:
                        bufs[k] = np.asarray(v, np.float32)
                self.snap[(name, b)] = dict(bufs)
        self.n = len(inputs)

    def steps(self):
        return self.names

    def read(self, tensor, step):
        return [self.snap[(step, b)][tensor] for b in range(self.n)]


# ------------------------------------------------------------------------------------------------ the verifier
def add_floorless(r, got, ref):
    """The compare dict r of (got, ref) with the rule WITHOUT the floor on top: |Δ| ≤ OP_TOL · ‖ref‖∞ (tests/att_ref.py says why the attention
    core is held to it). r["floorless"] is max|Δ| over that bound; ok and columns then answer for both rules."""
    ref = np.asarray(ref, np.float64)
    if not ref.size:
        return dict(r, floorless=0.0)
    d = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    d = np.where(np.isfinite(d), d, np.inf)
    tol = OP_TOL * float(np.max(np.abs(ref)))
    bad = ~(d <= tol)
    ratio = float(d.max() / tol) if tol > 0 else (0.0 if d.max() == 0 else float("inf"))
    return dict(r, floorless=ratio, ok=r["ok"] and not bad.any(), columns=np.union1d(r["columns"], np.unique(np.nonzero(bad)[-1])))


def verify(dev, cfg, blob, inputs, label="", items=None, report=print, R=None, att_floorless=False):
    """Every front step of the device's schedule, every item of `items`: inputs read with @previous step, outputs with @this step, compared
    with the float64 formula under the plain rule. → (rows [(step, tensor, item, kind, compare dict)], seconds of reference + comparison).
    att_floorless: steps of kind `rel_attention` are held to the rule without the floor IN ADDITION (add_floorless).
    Raises UnknownStep for a step name the walker does not know, UnitMismatch at the first step beyond its bound."""
    R = R or FrontRef(cfg, blob)
    items = list(range(len(inputs))) if items is None else list(items)
    names = [n for n in dev.steps() if is_front_step(n)]
    W = Walker(cfg)
    rows, t_ref, prev = [], 0.0, None
    dur_total = dur_skipped = 0
    for name in names:
        kind, reads, writes, fn = W.plan(name)
        src = {k: dev.read(k, prev if prev is not None else name) for k in reads}  # (the first step reads nothing but staged inputs)
        got = {k: dev.read(k, name) for k in writes}
        t0 = time.time()
        for b in items:
            out = fn(R, {k: src[k][b] for k in reads}, inputs[b])
            for k in writes:
                ref, g = out[k], got[k][b]
                if isinstance(ref, tuple):
                    ref, g = ref[0], g[ref[1]]
                if k == "dp.dur":
                    w = np.asarray(out["_w"], np.float64)
                    near = np.abs(w - np.rint(w)) <= DUR_REL * np.maximum(np.abs(w), 1e-30)
                    dur_total += w.size
                    dur_skipped += int(near.sum())
                    bad = (np.asarray(g).reshape(-1) != np.asarray(ref).reshape(-1)) & ~near
                    r = dict(err=float(bad.sum()), bound=0.0, ratio=float(bad.any()), ok=not bad.any(), columns=np.nonzero(bad)[0], worst=())
                else:
                    r = compare(g, ref)
                    if att_floorless and kind == "rel_attention":
                        r = add_floorless(r, g, ref)
                rows.append((name, k, b, kind, r))
                fl = f"  without the floor {r['floorless']:.4f}" if "floorless" in r else ""
                report(f"  {label}[{b}] {name:44s} {k:12s} {kind:14s} max|Δ| {r['err']:.3e}  bound {r['bound']:.3e}  |Δ|/bound {r['ratio']:.4f}{fl}")
                if not r["ok"]:
                    cols = r["columns"]
                    raise UnitMismatch(f"{label}[{b}] step {name} → {k}: beyond the bound in columns {cols[:8].tolist()}…{cols[-3:].tolist()} of "
                                       f"{np.asarray(ref).shape[-1]}, worst at {r['worst']}: max|Δ| {r['err']:.3e}, |Δ|/bound {r['ratio']:.2f}{fl}",
                                       name, k, b, r)
        t_ref += time.time() - t0
        prev = name
    assert dur_skipped <= DUR_SHARE * max(dur_total, 1) or dur_skipped == 0, \
        f"{label}: {dur_skipped} of {dur_total} ids lie within {DUR_REL} of an integer duration (> 1 %): choose another seed"
    return rows, t_ref


def worst_by_kind(rows):
    out = {}
    for _, _, _, kind, r in rows:
        out[kind] = max(out.get(kind, 0.0), r["ratio"])
        if "floorless" in r:
            out[kind + " (no floor)"] = max(out.get(kind + " (no floor)", 0.0), r["floorless"])
    return out


# ------------------------------------------------------------------------------------------------ inputs and expected schedules
def utterance(cfg, T, F, seed, durations=None):
    """T ids, durations that sum to F frames (or the ones given) and the injected noise [inter, F]."""
    rng = np.random.RandomState(seed)
    if durations is None:
        dur = np.full(T, F // T, np.int32)
        dur[:F - int(dur.sum())] += 1
    else:
        dur = np.asarray(durations, np.int32)
        F = int(dur.sum())
    return list(rng.randint(1, 130, size=T)), [int(d) for d in dur], kd.sym(kd.case_seed("cfg", 61) + seed, (cfg.inter, F), 1.7320508)


def dp_noise(T, seed):
    return kd.sym(kd.case_seed("cfg", 62) + seed, (2, T), 1.7320508)


def default_steps(cfg, predict=False, fold=True, ln="self"):
    """The front schedule a small single utterance gets by default (csrc/voice.hip), for the CPU stand-in: ln = "self" / "stats" (LayerNorm
    folded into its consumers) or "plain" (add_layernorm kernels); fold: the flow's folded tails, else seam + EPI_WN_SKIP_LAST."""
    if predict:
        ln = "stats" if ln == "self" else ln
    s = ["embed"]
    fused = ln != "plain"
    sfx = "" if ln == "self" else "_stats"
    for l in range(cfg.n_layers):
        p = f"enc{l}."
        s.append(p + ("ln2_qkv" if fused and l else "qkv"))
        s.append(p + "rel_attention")
        s += [p + "o_add" + sfx, p + "ln1_ffn1_relu", p + "ffn2_add" + sfx] if fused else [p + "o", p + "add_ln1", p + "ffn1_relu", p + "ffn2", p + "add_ln2"]
    if predict:
        s += (["enc.ln2_final"] if fused else []) + ["enc.proj", "dp.pre"] + [f"dp.dds{i}" for i in range(cfg.dp_dds_layers)] + ["dp.proj", "dp.init_latent"]
        for k in range(2 * cfg.dp_n_flows - 1, 1, -2):
            s += [f"dp.flow{k}.pre_add_cond"] + [f"dp.flow{k}.dds{i}" for i in range(cfg.dp_dds_layers)] + [f"dp.flow{k}.proj", f"dp.flow{k}.spline_flip"]
        return s + ["dp.affine_exp_ceil"]
    s += ["enc.ln2_proj" if fused else "enc.proj", "expand_noise"]
    n = cfg.wn_layers
    for f in range(cfg.n_flows - 1, -1, -1):
        p = f"flow{f}."
        if f == cfg.n_flows - 1:
            s.append(p + "pre")
        for i in range(n):
            s.append(p + f"wn{i}.in_gate")
            if i + 1 < n or not fold:
                s.append(p + f"wn{i}.res_skip")
        tail = f"post_sub_flip_pre{f - 1}" if f else "post_sub"
        s.append(p + (f"wn{n - 1}.res_skip_" + tail if fold else tail))
    if cfg.n_flows % 2:
        s.append("flow.final_flip")
    return s
