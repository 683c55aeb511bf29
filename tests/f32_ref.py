"""float64 reference of the fp32 generator, one function per unit, and the chained teacher-forced check — TEST INFRASTRUCTURE (torch on the CPU).

The fp32 generator (csrc/voice.hip build_generator_merged and the per-conv half of build_schedule) has no rounding but fp32's own, so a
unit that is fed the GPU's own fp32 input ("teacher forcing") differs from a float64 evaluation of the same formula by accumulation order
and fp32 rounding only, and the project's op-level rule applies as it stands:   |Δ| ≤ OP_TOL · max(1, ‖ref‖∞)   (conftest.assert_close).
There is NO flip allowance and NO measured constant here: `F32Ref` is `bf16_ref.Bf16Ref(rounding=False)` (tied to torch_ref at 1e-5 by
test_bf16_ref.py and to the C oracle by test_f32_ref.py) with units that keep float64 between the links they compose.

Units (inputs: the GPU's fp32 tensors of ONE item cut to its true length [C, len]; positions past it are zero inputs — the fp32 streams
are NOT zero there on the device, every kernel has to mask by len_ptr · len_mul, and a kernel that does not shows in the last `reach`
columns of its output):
  conv_pre        W ⋆ z + b
  up              ConvTranspose(lrelu(x, 0.1)),  x = conv_pre output, or (r0 + r1 + r2) / 3 of the previous stage's three ResBlock outputs
                  (merged schedule: the average-of-three prologue), or ConvTranspose(a) of the stored a = lrelu(mean) (per-conv schedule)
  rb_chain        ResBlock steps d0 … d1 from the nearest tapped tensor upstream; the reference makes the middle itself, in float64.
                  One step of ResBlock2: x + W ⋆ lrelu(x) + b;  of ResBlock1: x + Wb ⋆ lrelu(Wa ⋆ lrelu(x) + ba) + bb
  mean_lrelu      per-conv schedule: lrelu((r0 + r1 + r2) / 3, α) with r2 = the closing step(s) of the last ResBlock, folded into its epilogue
  waveform        tanh(v),  v = W ⋆ lrelu(mean, 0.01)  (no bias), see `Waveform`
"""
import time

import numpy as np

import bf16_ref as br
import katdata as kd
from conftest import OP_TOL

SLOPE = 0.1
POST_SLOPE = 0.01
# Error floor of the waveform link: fp32 rounding of the output (half an ulp just below 1.0 = 2⁻²⁵) plus the error of the device tanhf.
# No accuracy table of the HIP device math library is installed with the toolchain this was written against, so the fallback the
# project agreed on is used: 4 · 2⁻²⁴ for both together (tanhf is documented at 1–2 ulp by the vendors that publish a table).
WAVE_FLOOR = 4.0 * 2.0 ** -24
FLOOR_SHARE_MAX = 0.10
NOISE_SCALE = 0.667  # of the GPU cases; test_f32_ref.py checks that their waveforms meet FLOOR_SHARE_MAX at it

base_tol = br.base_tol


class UnitMismatch(AssertionError):
    """A unit beyond its bound: .unit (name), .result (compare dict), .columns (positions with an element beyond the bound)."""

    def __init__(self, msg, unit, result, columns):
        super().__init__(msg)
        self.unit, self.result, self.columns = unit, result, columns


def lrelu64(x, alpha):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, x, x * alpha)


class Plain:
    """ref with the plain rule: one bound OP_TOL · max(1, ‖ref‖∞) for every element."""

    def __init__(self, ref, kind):
        self.ref, self.kind = np.asarray(ref, np.float64), kind
        self.tol = np.full(self.ref.shape, base_tol(self.ref))

    def compare(self, got):
        got = np.asarray(got, np.float64).reshape(self.ref.shape)
        d = np.abs(got - self.ref)
        bad = ~(d <= self.tol)  # (NaN counts as beyond)
        ratio = d / self.tol
        worst = np.unravel_index(int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf))), d.shape) if d.size else ()
        return dict(kind=self.kind, err=float(d.max()) if d.size else 0.0, bound=float(self.tol.max()) if d.size else OP_TOL,
                    ratio=float(np.max(np.where(np.isfinite(ratio), ratio, np.inf))) if d.size else 0.0, ok=not bad.any(), n_over=int(bad.sum()),
                    worst=tuple(int(i) for i in worst), columns=np.unique(np.nonzero(bad)[-1]) if d.size else np.zeros(0, np.int64))


class Waveform(Plain):
    """audio against tanh(v) under the per-sample bound  base_tol(v) · (1 − tanh²(v)) + WAVE_FLOOR:  the op-level bound on the
    pre-activation v carried through the slope of tanh, so that the link is not blind where tanh saturates (a plain OP_TOL on the
    waveform lets an error in front of tanh grow by 1 / slope — 10 to 1000 on the synthetic voices — before it shows).
    floor_share: the share of samples where the floor exceeds the slope term, from the reference alone; verify_item asserts ≤ 10 %."""

    def __init__(self, v):
        self.v = np.asarray(v, np.float64)
        self.ref, self.kind = np.tanh(self.v), "waveform"
        self.slope_term = base_tol(self.v) * (1.0 - self.ref ** 2)
        self.tol = self.slope_term + WAVE_FLOOR
        self.floor_share = float(np.mean(WAVE_FLOOR > self.slope_term)) if self.v.size else 0.0

    def compare(self, got):
        r = super().compare(got)
        r["floor_share"] = self.floor_share
        return r


class F32Ref(br.Bf16Ref):
    """acc "f64": the reference. "f32" / "f32r": two honest fp32 implementations (torch's order; channels reversed) for the CPU tests."""

    def __init__(self, cfg, blob, acc="f64"):
        super().__init__(cfg, blob, acc=acc, rounding=False)

    def conv(self, x, wname, **kw):
        return self.contract(np.asarray(x, np.float64 if self.acc == "f64" else np.float32), wname, w32=True, **kw)[0]

    def reach(self, j, d):
        """Columns either side that one step d of ResBlock j reads (ResBlock1: both convs)."""
        c = self.cfg
        K = c.rb_kernels[j]
        return (K - 1) // 2 * c.rb_dilations[j][d] + ((K - 1) // 2 if c.resblock_type == 1 else 0)

    # ---------------------------------------------------------------- units
    def conv_pre(self, z):
        return Plain(self.conv(z, "dec.conv_pre", pad=3), "conv_pre")

    def _convt(self, u, a):
        k, s = self.cfg.up_kernels[u], self.cfg.up_rates[u]
        return self.conv(a, f"dec.ups.{u}", pad=(k - s) // 2, stride=s)

    @staticmethod
    def mean64(xs):
        xs = [np.asarray(x, np.float64) for x in xs]
        return xs[0] if len(xs) == 1 else (xs[0] + xs[1] + xs[2]) / 3.0

    def up(self, u, xs):
        """xs: [conv_pre output] or the previous stage's three ResBlock outputs."""
        return Plain(self._convt(u, lrelu64(self.mean64(xs), SLOPE)), "up")

    def up_from_act(self, u, act):
        return Plain(self._convt(u, np.asarray(act, np.float64)), "up")

    def _chain(self, u, j, d0, d1, x):
        c = self.cfg
        K = c.rb_kernels[j]
        x = np.asarray(x, np.float64)
        for d in range(d0, d1 + 1):
            dl = c.rb_dilations[j][d]
            names = self.rb_names(u, j, d)
            t = self.conv(lrelu64(x, SLOPE), names[0], dil=dl, pad=(K * dl - dl) // 2)
            if c.resblock_type == 1:
                t = self.conv(lrelu64(t, SLOPE), names[1], pad=(K - 1) // 2)
            x = x + t
        return x

    def rb_chain(self, u, j, d0, d1, x):
        return Plain(self._chain(u, j, d0, d1, x), "rb_step" if d0 == d1 else "rb_composed")

    def mean_lrelu(self, u, r0, r1, r2=None, x2=None, d0=None):
        """r2 tapped, or made here from x2 = the last ResBlock's stream in front of its untapped closing steps d0 … last."""
        c = self.cfg
        if r2 is None:
            r2 = self._chain(u, c.n_rb - 1, d0, c.rb_n_dil - 1, x2)
        alpha = POST_SLOPE if u + 1 == c.n_ups else SLOPE
        return Plain(lrelu64(self.mean64([r0, r1, r2]), alpha), "mean_lrelu")

    def post(self, a):
        """conv_post pre-activation v from a = lrelu(mean, 0.01)."""
        return self.conv(a, "dec.conv_post", pad=3)

    def waveform(self, xs=None, act=None):
        return Waveform(self.post(lrelu64(self.mean64(xs), POST_SLOPE) if act is None else np.asarray(act, np.float64)))

    # ---------------------------------------------------------------- the whole generator, free running (CPU tests)
    def generator(self, z, third=1.0 / 3.0):
        """→ {tap name: [C, L]} with every tensor either schedule may keep, plus "audio" and "v" (conv_post's pre-activation).
        acc "f64": float64 throughout. Otherwise every stored tensor is rounded to fp32, the mean is (r0 + r1 + r2) · third in fp32."""
        c = self.cfg
        f = (lambda a: np.asarray(a, np.float64)) if self.acc == "f64" else (lambda a: np.asarray(a, np.float64).astype(np.float32))
        out = {"z": np.asarray(z, np.float32)}
        x = f(self.conv_pre(z).ref)
        out["dec_pre"] = x
        a = f(lrelu64(x, SLOPE))
        for u in range(c.n_ups):
            x = f(self._convt(u, a))
            out[f"dec.s{u}.up"] = x
            rs = []
            for j in range(c.n_rb):
                y = x
                for d in range(c.rb_n_dil):
                    y = f(self._chain(u, j, d, d, y))
                    out[f"dec.s{u}.rb{j}.c{d}"] = y
                rs.append(y)
            if self.acc == "f64":
                m = (rs[0] + rs[1] + rs[2]) * third
            else:
                m = ((rs[0] + rs[1]) + rs[2]) * np.float32(third)
            a = f(lrelu64(m, POST_SLOPE if u + 1 == c.n_ups else SLOPE))
            out[f"dec.s{u}.mean_lrelu"] = a
        out["v"] = self.post(a).reshape(-1)
        out["audio"] = f(np.tanh(out["v"]))
        return out


def schedule_view(cfg, G, schedule):
    """The taps of a free-running generator G that a plan of the given schedule registers (csrc/voice.hip):
    "all": the merged schedule conv by conv with every step kept (what a two-step ResBlock2 stage keeps);
    "merged": the merged schedule's ping-pong buffers — the last two steps; "pair": the merged pair plan — ResBlock2 keeps only the last
    step of each pair launch, ResBlock1 the last two steps; "per_conv": every step but the last ResBlock's closing one, plus mean_lrelu."""
    keep = {"z", "dec_pre"}
    n = cfg.rb_n_dil
    for u in range(cfg.n_ups):
        keep.add(f"dec.s{u}.up")
        for j in range(cfg.n_rb):
            for d in range(n):
                if schedule == "all":
                    ok = True
                elif schedule == "merged":
                    ok = d + 2 >= n
                elif schedule == "pair":
                    ok = d + 2 >= n and (cfg.resblock_type == 1 or d % 2 == 1)
                else:
                    ok = not (j == cfg.n_rb - 1 and d == n - 1)
                if ok:
                    keep.add(f"dec.s{u}.rb{j}.c{d}")
        if schedule == "per_conv":
            keep.add(f"dec.s{u}.mean_lrelu")
    return {k: v for k, v in G.items() if k in keep}


# -------------------------------------------------------------------- the chained, teacher-forced check of one item
def verify_item(R, T, audio, label="", report=print):
    """T: {tap name: [C, len]} of ONE batch item as read from the GPU (or made by another F32Ref), audio: its waveform.
    Every unit is referenced from the nearest tensors upstream of it IN T; the first link is T["z"], the last the waveform, none is skipped.
    Returns [(unit name, compare dict)]; raises UnitMismatch at the first unit beyond its bound."""
    c = R.cfg
    assert c.n_rb == 3, "the fp32 schedules tapped here advance three ResBlocks"
    rows = []

    def check(name, unit, got):
        r = unit.compare(got)
        rows.append((name, r))
        extra = f"  floor-dominated {100 * r['floor_share']:.2f} %" if "floor_share" in r else ""
        report(f"  {label} {name:24s} {r['kind']:11s} max|Δ| {r['err']:.3e}  bound {r['bound']:.3e}  worst |Δ|/bound {r['ratio']:.4f}{extra}")
        if "floor_share" in r:
            assert r["floor_share"] <= FLOOR_SHARE_MAX, (f"{label} {name}: the error floor exceeds the slope term on {100 * r['floor_share']:.1f} % of the "
                                                         f"samples (> 10 %): the input saturates tanh too often for this check; lower noise_scale")
        if not r["ok"]:
            cols = r["columns"]
            raise UnitMismatch(f"{label} {name}: {r['n_over']} elements beyond the bound in columns {cols[:8].tolist()}…{cols[-3:].tolist()} of "
                               f"{unit.ref.shape[-1]}, worst at {r['worst']}: max|Δ| {r['err']:.3e}, |Δ|/bound {r['ratio']:.2f}", name, r, cols)

    check("dec_pre", R.conv_pre(T["z"]), T["dec_pre"])
    xs, act = [T["dec_pre"]], None
    for u in range(c.n_ups):
        p = f"dec.s{u}."
        up = T[p + "up"]
        check(p + "up", R.up(u, xs) if act is None else R.up_from_act(u, act), up)
        outs, pending = [], None
        for j in range(c.n_rb):
            x, d0 = up, 0  # x: the nearest tapped tensor upstream; steps d0 … are still to be accounted for
            for d in range(c.rb_n_dil):
                name = f"{p}rb{j}.c{d}"
                if name in T:
                    check(name, R.rb_chain(u, j, d0, d, x), T[name])
                    x, d0 = T[name], d + 1
            if d0 < c.rb_n_dil:  # closing step(s) without a tensor: only where the mean is folded into the last ResBlock's epilogue
                assert j == c.n_rb - 1 and p + "mean_lrelu" in T, f"tap {p}rb{j}.c{c.rb_n_dil - 1} is missing"
                pending = (x, d0)
                x = None
            outs.append(x)
        if p + "mean_lrelu" in T:
            act = T[p + "mean_lrelu"]
            unit = R.mean_lrelu(u, outs[0], outs[1], outs[2]) if pending is None else R.mean_lrelu(u, outs[0], outs[1], None, *pending)
            check(p + "mean_lrelu", unit, act)
        else:
            xs, act = outs, None
    check("audio", R.waveform(xs, act), np.asarray(audio).reshape(-1))
    return rows


def tap_names(cfg):
    """Every tap name an fp32 plan may register, with (channels, positions per frame)."""
    names = [("z", cfg.inter, 1), ("dec_pre", cfg.up_initial, 1)]
    mul, ch = 1, cfg.up_initial
    for u in range(cfg.n_ups):
        mul, ch = mul * cfg.up_rates[u], ch // 2
        names.append((f"dec.s{u}.up", ch, mul))
        names += [(f"dec.s{u}.rb{j}.c{d}", ch, mul) for j in range(cfg.n_rb) for d in range(cfg.rb_n_dil)]
        names.append((f"dec.s{u}.mean_lrelu", ch, mul))
    return names


def read_taps(rt, slot, frames, items=None, prefix=""):
    """Every registered tap of a prepared and launched fp32 slot → one {name: [C, len]} per batch item (frames: true frame count per item;
    items not asked for stay empty); prefix "window:": of the generator window plan of the slot's latest stream step (frames: the rows'
    window lengths). A name the plan did not register is absent; verify_item decides whether that is allowed."""
    return br.read_named_taps(rt, slot, tap_names(rt.cfg), frames, items, prefix)


def verify_slot(rt, blob, slot, frames, audio, label="", items=None, report=print):
    """The chained check of a launched and collected fp32 slot: audio = collect(slot), items back to back at their true lengths.
    → (rows, seconds the float64 reference and the comparisons took, the tap names the plan registered)."""
    R = F32Ref(rt.cfg, blob)
    items = list(range(len(frames))) if items is None else list(items)
    taps = read_taps(rt, slot, frames, items)
    offs = np.concatenate([[0], np.cumsum([f * rt.cfg.hop for f in frames])])
    assert audio.size == offs[-1], (audio.size, offs[-1])
    rows, t0 = [], time.time()
    for b in items:
        rows += verify_item(R, taps[b], audio[offs[b]:offs[b + 1]], f"{label}[{b}]", report)
    return rows, time.time() - t0, sorted(taps[items[0]])


def utterance(cfg, F, seed, T=None):
    """T ids with durations that sum to F frames (at least one id per 3 frames) and the injected noise [inter, F] — the inputs of
    tests/test_gpu_f32_exact.py, here so that the CPU tests can check the same inputs against the saturation condition."""
    T = T or max(1, -(-F // 3))
    rng = np.random.RandomState(seed)
    dur = np.full(T, F // T, np.int32)
    dur[:F - int(dur.sum())] += 1
    return list(rng.randint(1, 130, size=T)), list(int(d) for d in dur), kd.sym(kd.case_seed("cfg", 60) + seed, (cfg.inter, F), 1.7320508)


def worst_by_kind(rows):
    out = {}
    for _, r in rows:
        out[r["kind"]] = max(out.get(r["kind"], 0.0), r["ratio"])
    return out
