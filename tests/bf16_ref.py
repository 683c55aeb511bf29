"""Rounding-exact reference of the bf16 generator, one function per unit — TEST INFRASTRUCTURE (torch on the CPU).

The bf16 generator (csrc/voice.hip build_generator_bf16) rounds contraction INPUTS only: every conv reads
bf16(LeakyReLU(x)) of an fp32 tensor and bf16 weights, accumulates in fp32 and adds bias / residual / MRF mean in fp32. A product of two
bf16 values is exact in fp32, so a unit that is fed the GPU's own fp32 input ("teacher forcing") differs from this reference by
accumulation order only, and the op-level rule of conftest.assert_close applies:  |Δ| ≤ OP_TOL · max(1, ‖ref‖∞).

Rounding points (taken from the builder, not assumed):
  conv_pre        W16 ⋆ bf16(z) + b                                        (pack_act_c8 with slope 1)
  ConvTranspose   W16 ⋆ᵀ bf16(lrelu(x, 0.1)) + b                           x = conv_pre output, or the MRF mean of the previous stage
  ResBlock2 step  x + W16 ⋆ bf16(lrelu(x, 0.1)) + b
  ResBlock1 step  x + Wb16 ⋆ bf16(lrelu(fp32(Wa16 ⋆ bf16(lrelu x) + ba))) + bb   (one launch in rb_pair_bf16_kernel, two in conv_bf16_kernel)
  MRF mean        ((r0 + r1) + r2) / 3 in fp32 — a true division (`/ 3.0f`), the form every bf16 kernel uses; the `·(1/3)` of DESIGN §5 is an
                  fp32 kernel's. fp32 add and divide are correctly rounded on both sides, so this unit is reproduced bit for bit.
  conv_post       tanh(W32 ⋆ lrelu(mean, 0.01)) with fp32 weights (conv_cout1 kernel), no bias
LeakyReLU is `v >= 0 ? v : v * alpha` in fp32 and is evaluated here in fp32 as well, so bf16(lrelu(x)) of a given fp32 x is exact.
A tensor handed to a unit is one batch item cut to its true length [C, len]: positions at or past the true length are zero inputs,
which is what the zero tail of the C8 images means.

Units with an INTERNAL rounding (the ResBlock1 pair; anything referenced across the bf16 image of the MRF mean) get a per-element
allowance for legitimate rounding flips on top of the OP_TOL rule:
  * the value v that is rounded carries an error bound err(v). An element is AMBIGUOUS when v lies within err(v) of a bf16 rounding
    midpoint: the GPU may round it the other way, which moves it by one ulp_bf16(v);
  * allowance = Σ over the ambiguous elements of the consumer's receptive field of |w| · ulp_bf16(v): ONE conv of the ambiguity map with |W|.
  * err(v) of a contraction result is ε = κ · 2⁻²⁴ · Σ|w·x|. The SHAPE Σ|w·x| is the standard bound of a floating-point sum; the
    worst-case factor n_terms would make ε exceed half a bf16 ulp for most elements (n_terms up to 2816), so κ is MEASURED, as the issue allows:
    κ = 2 · max over the tensor of |fp64 − fp32 accumulation| / (2⁻²⁴ · Σ|w·x|) of this reference's own contraction — the largest relative
    spread torch's fp32 order shows, doubled because the GPU sums in another order (MFMA blocks of 16, taps outermost). κ comes out near 0.1–0.3.
    tests/test_bf16_ref.py validates the choice on the CPU with a third summation order (channels reversed) that took no part in measuring κ.
    Errors inherited from upstream (an allowance already granted, fp32 rounding of adds) are added to err(v).
"""
import numpy as np
import torch
import torch.nn.functional as Fn

import katdata as kd
import piper_hip as ph
from conftest import OP_TOL

U24 = 2.0 ** -24
SLOPE = 0.1


def lrelu32(x, alpha):
    x = np.asarray(x, np.float32)
    return np.where(x >= 0, x, x * np.float32(alpha)).astype(np.float32)


def bf16_ulp(v):
    """Spacing of bf16 numbers at |v| (8 significant bits): 2^(e−8) for |v| in [2^(e−1), 2^e)."""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.where(np.asarray(v) == 0, 0.0, np.ldexp(1.0, e - 8))


def base_tol(ref):
    return OP_TOL * max(1.0, float(np.max(np.abs(ref)))) if ref.size else OP_TOL


class Unit:
    """ref, per-element tol = base + allow, eps (accumulation-error bound of ref itself), allow (flip allowance)."""

    def __init__(self, ref, allow=None, eps=None, base=None):
        self.ref = np.asarray(ref, np.float64)
        self.allow = np.zeros_like(self.ref) if allow is None else np.asarray(allow, np.float64)
        self.eps = np.zeros_like(self.ref) if eps is None else np.asarray(eps, np.float64)
        self.base = base_tol(self.ref) if base is None else base
        self.tol = self.base + self.allow

    def compare(self, got):
        """→ dict(err, bound, allow_share, needed_share, ok, median_ok, worst) for a GPU tensor of the same shape."""
        got = np.asarray(got, np.float64).reshape(self.ref.shape)
        d = np.abs(got - self.ref)
        over = d > self.tol
        worst = np.unravel_index(int(np.argmax(d - self.tol)), d.shape) if d.size else ()
        return dict(err=float(d.max()) if d.size else 0.0, bound=float(self.tol.max()) if d.size else self.base, base=self.base,
                    allow_share=float(np.mean(self.allow > 0)) if d.size else 0.0,
                    needed_share=float(np.mean(d > self.base)) if d.size else 0.0,
                    ok=bool(np.all(np.isfinite(got)) and not over.any()), n_over=int(over.sum()), worst=tuple(int(i) for i in worst),
                    median_ok=bool(d.size == 0 or float(np.median(self.tol)) <= 2.0 * self.base), median_tol=float(np.median(self.tol)) if d.size else 0.0)


class Bf16Ref:
    """acc: "f64" (the reference), "f32" (torch's fp32 order) or "f32r" (fp32 with the channel order reversed: a second, unrelated order).
    rounding=False switches every bf16 rounding off (then it is the plain fp32 generator, torch_ref.Ref.generator)."""

    def __init__(self, cfg, blob, acc="f64", rounding=True):
        self.cfg, self.acc, self.rounding = cfg, acc, rounding
        self.w = {e["name"]: np.asarray(blob[e["offset"]:e["offset"] + e["count"]], np.float32).reshape(e["shape"])
                  for e in ph.blob_layout(cfg) if e["name"].startswith("dec.")}

    # ---------------------------------------------------------------- pieces
    def rnd(self, a):
        return kd.bf16_round(np.asarray(a, np.float32)) if self.rounding else np.asarray(a, np.float32)

    def _run(self, x, w, acc, dil, pad, stride):
        dt = torch.float64 if acc == "f64" else torch.float32
        xt, wt = torch.from_numpy(np.ascontiguousarray(x)).to(dt)[None], torch.from_numpy(np.ascontiguousarray(w)).to(dt)
        if acc == "f32r":
            xt, wt = torch.flip(xt, [1]), torch.flip(wt, [0 if stride else 1])
        if stride:
            y = Fn.conv_transpose1d(xt, wt, None, stride=stride, padding=pad)
        else:
            y = Fn.conv1d(xt, wt, None, dilation=dil, padding=pad)
        return y[0].to(torch.float64).numpy()

    def contract(self, x, wname, dil=1, pad=0, stride=0, want_eps=False, w32=False):
        """W ⋆ x + b for one item x [Cin, L] (stride > 0: ConvTranspose1d) → (value fp64 in the configured accumulation, eps or None)."""
        w = self.w[wname + ".weight"]
        w = w if w32 else self.rnd(w)
        b = self.w.get(wname + ".bias")
        if x.shape[1] == 0:
            L = 0
            z = np.zeros((w.shape[1] if stride else w.shape[0], L))
            return z, (z if want_eps else None)
        v = self._run(x, w, self.acc, dil, pad, stride)
        eps = None
        if want_eps:
            v64 = v if self.acc == "f64" else self._run(x, w, "f64", dil, pad, stride)
            v32 = self._run(x, w, "f32", dil, pad, stride)
            s = self._run(np.abs(x), np.abs(w), "f64", dil, pad, stride)
            kappa = 2.0 * float(np.max(np.abs(v64 - v32) / np.maximum(U24 * s, 1e-300))) if s.size else 0.0
            eps = kappa * U24 * s
        if b is not None:
            v = v + b.astype(np.float64)[:, None]
        return v, eps

    def spread(self, cost, wname, dil=1, pad=0, stride=0):
        """Σ over the receptive field of |w| · cost: the flip allowance of a consumer of an ambiguity map."""
        if cost.shape[1] == 0 or not cost.any():
            w = self.w[wname + ".weight"]
            return np.zeros((w.shape[1] if stride else w.shape[0], cost.shape[1] * (stride or 1)))
        return self._run(cost, np.abs(self.rnd(self.w[wname + ".weight"])), "f64", dil, pad, stride)

    def round_amb(self, h32, err):
        """bf16 of the fp32 tensor h32 whose true value is only known to ±err → (rounded fp32, cost map: ulp where ambiguous, else 0)."""
        hb = self.rnd(h32)
        if not self.rounding:
            return hb, np.zeros(h32.shape)
        h = h32.astype(np.float64)
        ulp = bf16_ulp(h)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(ulp > 0, h / np.where(ulp > 0, ulp, 1.0), 0.0)
        dist = np.abs(q - np.floor(q) - 0.5) * ulp  # distance to the nearest rounding midpoint of its binade
        err = err + np.abs(h) * 2 * U24  # (+ the fp32 cast in front of the bf16 rounding)
        amb = (ulp > 0) & (dist <= err)
        # one flip moves the value by exactly one ulp; a small value whose error spans several ulps moves by at most err + an ulp either side
        cost = np.where(amb, np.where(err <= 0.5 * ulp, ulp, err + 2.0 * ulp), 0.0)
        # h32 == 0 exactly (three ResBlock outputs that cancel in fp32): it has no binade and no midpoint, but its true value is still only
        # known to ±err — the device's sum of the same terms in another order lands within err of 0, and its bf16 image within an ulp of that
        zero = (ulp == 0) & (err > 0)
        return hb, np.where(zero, err + bf16_ulp(err), cost)

    def rb_names(self, u, j, d):
        rb = u * self.cfg.n_rb + j
        if self.cfg.resblock_type == 1:
            return f"dec.resblocks.{rb}.convs1.{d}", f"dec.resblocks.{rb}.convs2.{d}"
        return (f"dec.resblocks.{rb}.convs.{d}",)

    # ---------------------------------------------------------------- units (inputs: the GPU's fp32 tensors of ONE item, [C, len])
    def conv_pre(self, z):
        v, _ = self.contract(self.rnd(z), "dec.conv_pre", pad=3)
        return Unit(v)

    def _up(self, u, a, cost=None):
        k, s = self.cfg.up_kernels[u], self.cfg.up_rates[u]
        v, eps = self.contract(a, f"dec.ups.{u}", pad=(k - s) // 2, stride=s, want_eps=True)
        allow = None if cost is None else self.spread(cost, f"dec.ups.{u}", pad=(k - s) // 2, stride=s)
        return Unit(v, allow, eps)

    def up(self, u, x):
        """ConvTranspose of stage u from the fp32 tensor whose lrelu it reads (conv_pre output)."""
        return self._up(u, self.rnd(lrelu32(x, SLOPE)))

    def rb_step(self, u, j, d, x):
        """Dilation step d of ResBlock j of stage u from its fp32 input stream x."""
        c = self.cfg
        K, dl = c.rb_kernels[j], c.rb_dilations[j][d]
        names = self.rb_names(u, j, d)
        a = self.rnd(lrelu32(x, SLOPE))
        x64 = np.asarray(x, np.float64)
        if c.resblock_type != 1:
            v, eps = self.contract(a, names[0], dil=dl, pad=(K * dl - dl) // 2, want_eps=True)
            return Unit(x64 + v, None, eps)
        t, eps_t = self.contract(a, names[0], dil=dl, pad=(K * dl - dl) // 2, want_eps=True)
        t32 = t.astype(np.float32)
        h32 = lrelu32(t32, SLOPE)
        hb, cost = self.round_amb(h32, eps_t * np.where(t + eps_t >= 0, 1.0, SLOPE))  # (slope 1 wherever the value may be positive)
        v, eps = self.contract(hb, names[1], pad=(K - 1) // 2, want_eps=True)
        return Unit(x64 + v, self.spread(cost, names[1], pad=(K - 1) // 2), eps)

    @staticmethod
    def mean32(r0, r1, r2):
        r0, r1, r2 = (np.asarray(r, np.float32) for r in (r0, r1, r2))
        return ((r0 + r1) + r2) / np.float32(3.0)

    def mean(self, r0, r1, r2):
        """fp32 MRF mean of three tapped ResBlock outputs: bit-exact form, checked at the OP_TOL rule like every other unit."""
        return Unit(self.mean32(r0, r1, r2))

    def mean_from_rb(self, u, r0, r1, x2):
        """The last stage's mean where the last ResBlock's closing step is folded into it: r2 = rb_step(x2) is not materialised."""
        j, d = self.cfg.n_rb - 1, self.cfg.rb_n_dil - 1
        r2 = self.rb_step(u, j, d, x2)
        m = (np.asarray(r0, np.float64) + np.asarray(r1, np.float64) + r2.ref) / 3.0
        return Unit(m, r2.allow / 3.0, r2.eps / 3.0)

    def up_from_act(self, u, act):
        """ConvTranspose of stage u from the GPU's own bf16 image of lrelu(MRF mean) of stage u−1 (tap "dec.s{u−1}.mean_act")."""
        return self._up(u, np.asarray(act, np.float32))

    def mean_act(self, u, r0, r1, r2=None, x2=None):
        """The bf16 image bf16(lrelu(MRF mean)) that stage u writes for stage u+1, compared as VALUES with base tolerance 0.
        r2 tapped: the fp32 mean is reproduced bit for bit, so every element must be equal. r2 folded into the mean's producer (x2 = the
        input of its closing step): the mean carries r2's accumulation error and flip allowance; an element may differ by ONE bf16 ulp
        where the mean lies that close to a rounding midpoint, and must be equal everywhere else. (Referencing the next ConvTranspose
        across this image instead was measured on the CPU: three roundings deep on ResBlock1 voices, median tol 3.4e-4 against a cap
        of 3.0e-4 — the image tap keeps every link one contraction deep.)"""
        if r2 is not None:
            return Unit(self.rnd(lrelu32(self.mean32(r0, r1, r2), SLOPE)), base=0.0)
        j, d = self.cfg.n_rb - 1, self.cfg.rb_n_dil - 1
        r2u = self.rb_step(u, j, d, x2)
        r0, r1 = np.asarray(r0, np.float32), np.asarray(r1, np.float32)
        r2f = r2u.ref.astype(np.float32)
        m32 = self.mean32(r0, r1, r2f)
        err = (r2u.eps + r2u.allow) / 3.0 + 3 * U24 * (np.abs(r0) + np.abs(r1) + np.abs(r2f)).astype(np.float64)
        h32 = lrelu32(m32, SLOPE)
        hb, cost = self.round_amb(h32, err * np.where(m32 + err >= 0, 1.0, SLOPE))  # (slope 1 wherever the mean may be positive)
        return Unit(hb, cost, base=0.0)

    def conv_post(self, mean):
        v, _ = self.contract(lrelu32(mean, 0.01), "dec.conv_post", pad=3, w32=True)
        return Unit(np.tanh(v))

    # ---------------------------------------------------------------- the whole generator, free running (CPU tests)
    def generator(self, z):
        """→ {tap name: fp32 tensor [C, L]} under the names the GPU plan uses, plus "audio". Every rb step is materialised."""
        c = self.cfg
        out = {"z": np.asarray(z, np.float32)}
        x = self.conv_pre(z).ref.astype(np.float32)
        out["dec_pre"] = x
        a = self.rnd(lrelu32(x, SLOPE))
        for u in range(c.n_ups):
            x = self._up(u, a).ref.astype(np.float32)
            out[f"dec.s{u}.up"] = x
            rs = []
            for j in range(c.n_rb):
                y = x
                for d in range(c.rb_n_dil):
                    y = self.rb_step(u, j, d, y).ref.astype(np.float32)
                    out[f"dec.s{u}.rb{j}.c{d}"] = y
                rs.append(y)
            m = self.mean32(*rs)
            a = self.rnd(lrelu32(m, SLOPE))
            if u + 1 < c.n_ups:
                out[f"dec.s{u}.mean_act"] = a
        out["dec.mean"] = m
        out["audio"] = self.conv_post(m).ref.astype(np.float32).reshape(-1)
        return out


# -------------------------------------------------------------------- the chained, teacher-forced check of one item
def verify_item(R, T, audio, label="", report=print, hooks=None):
    """T: {tap name: [C, len]} of ONE batch item as read from the GPU (or produced by another Bf16Ref), audio: its waveform.
    Every unit is referenced from the tensors upstream of it IN T; the first link is T["z"], the last the waveform, none is skipped.
    Returns the list of (unit name, compare dict); raises AssertionError on the first unit beyond its bound or its median condition.
    hooks: {unit name: function(Unit) → Unit} — used by the sensitivity test to plant a defect in the REFERENCE."""
    c = R.cfg
    assert c.n_rb == 3 and c.rb_n_dil <= 3, "taps cover the presets' shape: three ResBlocks of at most three steps"
    rows = []

    def check(name, unit, got):
        if hooks and name in hooks:
            unit = hooks[name](unit)
        r = unit.compare(got)
        rows.append((name, r))
        report(f"  {label} {name:22s} max|Δ| {r['err']:.3e}  bound {r['bound']:.3e} (base {r['base']:.3e}, median {r['median_tol']:.3e})  "
               f"allowance on {100 * r['allow_share']:.2f} %, needed by {100 * r['needed_share']:.3f} %")
        assert r["median_ok"], f"{label} {name}: median tol {r['median_tol']:.3e} > 2 · {r['base']:.3e}: the allowance would swallow defects"
        assert r["ok"], f"{label} {name}: {r['n_over']} elements beyond tol, worst at {r['worst']}: max|Δ| {r['err']:.3e}, bound {r['bound']:.3e}"

    check("dec.conv_pre", R.conv_pre(T["z"]), T["dec_pre"])
    prev = None  # (r0, r1, r2 or None, x2) of the previous stage
    for u in range(c.n_ups):
        up = T[f"dec.s{u}.up"]
        if prev is None:
            check(f"dec.s{u}.up", R.up(u, T["dec_pre"]), up)
        else:
            act = T[f"dec.s{u - 1}.mean_act"]
            check(f"dec.s{u - 1}.mean_act", R.mean_act(u - 1, *prev), act)
            check(f"dec.s{u}.up", R.up_from_act(u, act), up)
        outs, x2 = [], None
        for j in range(c.n_rb):
            x = up
            for d in range(c.rb_n_dil):
                name = f"dec.s{u}.rb{j}.c{d}"
                if name not in T:  # only the closing step of the last ResBlock may be folded into the mean
                    assert j == c.n_rb - 1 and d == c.rb_n_dil - 1, f"tap {name} is missing"
                    x2, x = x, None
                    break
                check(name, R.rb_step(u, j, d, x), T[name])
                x = T[name]
            outs.append(x)
        prev = (outs[0], outs[1], outs[2], x2)
    if prev[2] is not None:
        check("dec.mean", R.mean(*prev[:3]), T["dec.mean"])
    else:
        check("dec.mean", R.mean_from_rb(c.n_ups - 1, prev[0], prev[1], prev[3]), T["dec.mean"])
    check("audio", R.conv_post(T["dec.mean"]), np.asarray(audio).reshape(1, -1))
    return rows


def tap_names(cfg):
    """Every tap name a bf16 plan may register, with (channels, positions per frame)."""
    names = [("z", cfg.inter, 1), ("dec_pre", cfg.up_initial, 1)]
    mul, ch = 1, cfg.up_initial
    for u in range(cfg.n_ups):
        mul, ch = mul * cfg.up_rates[u], ch // 2
        names.append((f"dec.s{u}.up", ch, mul))
        names += [(f"dec.s{u}.rb{j}.c{d}", ch, mul) for j in range(cfg.n_rb) for d in range(cfg.rb_n_dil)]
        if u + 1 < cfg.n_ups:
            names.append((f"dec.s{u}.mean_act", ch, mul))
    names.append(("dec.mean", ch, mul))
    return names


def decode_c8(raw, C):
    """A "mean_act" tap of one item (raw bits, [C/8][len][8] bf16 read as float32 words) → fp32 values [C, len]."""
    u = np.ascontiguousarray(raw, np.float32).view(np.uint16).reshape(C // 8, -1, 8)
    return (u.transpose(0, 2, 1).reshape(C, -1).astype(np.uint32) << 16).view(np.float32)


class TapSizeMismatch(AssertionError):
    """A tap whose total size is not Σ C · len_b · positions per unit of the lengths the caller expects: .name, .got, .sizes."""

    def __init__(self, name, got, sizes):
        super().__init__(f"tap {name}: {got} floats, expected {sum(sizes)} = Σ {list(sizes)}")
        self.name, self.got, self.sizes = name, got, list(sizes)


def read_named_taps(rt, slot, names, lengths, items=None, prefix=""):
    """The taps `names` = [(name, channels, positions per unit of length)] of a slot → one {name: [C, len]} per item (lengths: the length
    each item is compacted to — the true frame counts of a launched slot, or, with prefix "window:", the window lengths of the slot's latest
    stream step, 0 for a row that contributes nothing; items not asked for stay empty). The library sizes the buffer, so a tap that holds
    more or less than Σ C · len · positions raises TapSizeMismatch instead of being cut. A name the plan did not register (a tensor its
    schedule never materialises) is absent; every other refusal of the selector is raised. "mean_act" images are decoded (decode_c8)."""
    want = range(len(lengths)) if items is None else items
    out = [{} for _ in lengths]
    for name, C, mul in names:
        packed = name.endswith("mean_act")
        sizes = [C * f * mul // (2 if packed else 1) for f in lengths]
        try:
            raw = rt.tap(slot, prefix + name)
        except ph.InvalidArgument as e:
            if "unknown tap" in str(e):
                continue
            raise
        if raw.size != sum(sizes):
            raise TapSizeMismatch(prefix + name, raw.size, sizes)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        for b in want:
            part = raw[offs[b]:offs[b + 1]]
            out[b][name] = decode_c8(part, C) if packed else part.reshape(C, -1).copy()
    return out


def read_taps(rt, slot, frames, items=None, prefix=""):
    """Every registered tap of a prepared and launched bf16 slot → one {name: [C, len]} per batch item (frames: true frame count per item);
    prefix "window:": of the generator window plan of the slot's latest stream step (frames: the rows' window lengths).
    A name the plan did not register is simply absent; verify_item decides whether that is allowed."""
    return read_named_taps(rt, slot, tap_names(rt.cfg), frames, items, prefix)


def verify_slot(rt, blob, slot, frames, audio, label="", items=None, report=print):
    """The chained exact check of a launched and collected bf16 slot: audio = collect(slot), items back to back at their true lengths."""
    R = Bf16Ref(rt.cfg, blob)
    taps = read_taps(rt, slot, frames)
    offs = np.concatenate([[0], np.cumsum([f * rt.cfg.hop for f in frames])])
    assert audio.size == offs[-1], (audio.size, offs[-1])
    rows = []
    for b in (range(len(frames)) if items is None else items):
        rows += verify_item(R, taps[b], audio[offs[b]:offs[b + 1]], f"{label}[{b}]", report)
    return rows
