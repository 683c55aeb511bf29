"""The streaming contract restated, and the per-unit check of one stream step — TEST INFRASTRUCTURE (numpy and torch on the CPU, no GPU).

A stream (single, group or pool) runs encoder + flow once and then the generator window by window on PLAN_GENERATOR plans
(csrc/voice.hip stream_step / batched_step). This module restates, independently of that code,
  * the window rule (`window_of`), the row bookkeeping of a group or pool with drops and joins, the plan's bucket and the generator's
    batch (`schedule`);
  * the generator's true receptive field by integer interval arithmetic (`exact_reach`) next to the formula the library uses for its
    halo (`halo_formula`, used only to assert formula ≥ exact and library == formula);
and checks ONE step through the "window:" selector of piper_hip_voice_tap (`verify_step`):
  size    every "window:" tap holds exactly Σ C · Fc_r · positions per frame floats for the Fc of `schedule` — this checks the lengths the
          device wrote (a row of length 0 contributes nothing) without a tap for them; every delivered chunk holds n_r samples;
  1       the gather is a move: window:z of a row is z_of(src)[:, a : a + Fc] bit for bit;
  2       every unit of the window's generator under the EXISTING rules, unchanged: f32_ref.verify_item (OP_TOL · max(1, ‖ref‖∞) per
          unit, the slope-weighted waveform rule, floor share ≤ 10 %) or bf16_ref.verify_item (per-element allowance, median_ok), with
          window:audio as the waveform;
  3       the chunk is a slice: the delivered chunk of a row is window:audio[skip : skip + n] bit for bit.
No tolerance is defined here.

`StandIn` serves "window:" taps from tensors made on the CPU, so the CPU tests can run verify_step with another F32Ref in the GPU's place
and plant defects in ITS tensors (`Planted`), never in a kernel. `CASES` are the inputs of tests/test_gpu_stream_windows.py, here so that
tests/test_stream_ref.py can hold them to the saturation condition of the waveform rule."""
import collections
import time

import numpy as np

import bf16_ref as br
import f32_ref as fr
import piper_hip as ph

Window = collections.namedtuple("Window", "a Fc skip n end")
Row = collections.namedtuple("Row", "src a Fc skip n")  # one generator row of one step; Fc = 0: src is None and the row runs nothing
Step = collections.namedtuple("Step", "rows Fb NBg")    # rows [NBg], the bucket of the step's plan, the generator's batch
IDLE = Row(None, 0, 0, 0, 0)


def bucket_f(F):
    """Frame rows come in steps of 16 up to 1024 frames and of 64 beyond."""
    return -(-F // 16) * 16 if F <= 1024 else -(-F // 64) * 64


def group_batch(n):
    """The generator's batch of a batched stream of n rows: n rounded up to a power of two."""
    NBg = 1
    while NBg < n:
        NBg *= 2
    return NBg


def window_of(F, next, chunk, halo, hop):
    """What one step decodes of an utterance of F frames whose next frame is `next`: latent frames [a, a + Fc) — the chunk's frames plus
    `halo` either side, clamped to the utterance — of whose audio the first `skip` samples are dropped and the following `n` delivered."""
    f0, f1 = next, min(F, next + chunk)
    a, b = max(0, f0 - halo), min(F, f1 + halo)
    return Window(a, b - a, (f0 - a) * hop, (f1 - f0) * hop, f1)


def schedule(Fs, chunk, halo, hop, events=(), NBg=None):
    """The steps of a batched stream of len(Fs) rows (a single stream: one row) → [Step]. Fs[r]: the frames of the item that holds row r
    from the start (0 / None: a free pool row). events, applied once `k` steps have run (k = 0: before the first):
      ("drop", k, row)            stream_drop on a group's item: the row runs and delivers nothing from then on (Fc = 0), but until the
                                  frame where its stream would have ended its window still counts for the bucket of the step's plan,
                                  so the other rows run the plans they would have run without the drop;
      ("join", k, row, F, src)    a pool session of F frames takes the (free) row; `src` names it for verify_step's z_of.
    Rows past len(Fs) up to NBg = group_batch(len(Fs)) are pad rows. A row's src is its index unless a join named it. The stream ends
    when no row is active and no event is left (events due while the pool is idle apply at once: an idle pool runs no step)."""
    n = len(Fs)
    NBg = NBg or group_batch(n)
    rows = [dict(F=int(F or 0), next=0, active=bool(F), ghost=False, src=r) for r, F in enumerate(Fs)]
    events = sorted(events, key=lambda e: e[1])
    steps = []
    while True:
        k = len(steps)
        due = [e for e in events if e[1] <= k]
        events = [e for e in events if e[1] > k]
        for e in due:
            if e[0] == "drop":
                rows[e[2]]["ghost"] = rows[e[2]]["active"] and rows[e[2]]["next"] < rows[e[2]]["F"]
                rows[e[2]]["active"] = False
            else:
                assert e[0] == "join" and not rows[e[2]]["active"], e
                rows[e[2]] = dict(F=int(e[3]), next=0, active=True, ghost=False, src=e[4])
        out, ends, Fplan = [], {}, 0
        for r in range(NBg):
            if r >= n or not rows[r]["active"]:
                out.append(IDLE)
                if r < n and rows[r]["ghost"]:
                    g = window_of(rows[r]["F"], rows[r]["next"], chunk, halo, hop)
                    Fplan, ends[r] = max(Fplan, g.Fc), g.end
                continue
            w = window_of(rows[r]["F"], rows[r]["next"], chunk, halo, hop)
            out.append(Row(rows[r]["src"], w.a, w.Fc, w.skip, w.n))
            ends[r] = w.end
        Fmax = max(o.Fc for o in out)
        if Fmax == 0:
            if not events:
                return steps
            events = [(e[0], k) + tuple(e[2:]) for e in events]  # an idle pool: the next events apply now
            continue
        steps.append(Step(out, bucket_f(max(Fmax, Fplan)), NBg))
        for r, end in ends.items():
            rows[r]["next"] = end
            if end >= rows[r]["F"]:
                rows[r]["active"] = rows[r]["ghost"] = False


def reused_after_longer(steps):
    """Indices of the steps whose plan (Fb, NBg) last held, in some row, a longer row than the step gives it (0 included): the step has to
    cope with what the longer row left past the new true length."""
    held, out = {}, []
    for i, st in enumerate(steps):
        prev = held.get((st.Fb, st.NBg))
        if prev is not None and any(p > r.Fc for p, r in zip(prev, st.rows)):
            out.append(i)
        held[(st.Fb, st.NBg)] = [r.Fc for r in st.rows]
    return out


# ------------------------------------------------------------------------ the receptive field
def halo_formula(cfg):
    """The library's halo (generator_halo_frames) restated — used ONLY to assert formula ≥ exact_reach and library == formula."""
    r = 3
    for u in range(cfg.n_ups - 1, -1, -1):
        rb = 0
        for j in range(cfg.n_rb):
            reach = 0
            for d in range(cfg.rb_n_dil):
                k, dl = cfg.rb_kernels[j], cfg.rb_dilations[j][d]
                reach += (k * dl - dl) // 2 + ((k - 1) // 2 if cfg.resblock_type == 1 else 0)
            rb = max(rb, reach)
        r += rb
        r = (r + cfg.up_kernels[u]) // cfg.up_rates[u] + 1
    return r + 3


def exact_reach_sides(cfg):
    """(left, right): the latent frames before / after frame f that the samples of output frame f depend on, by integer interval
    arithmetic from the waveform back to z. A 'same' conv of kernel K, dilation d widens an interval of positions by (K − 1) / 2 · d
    either side; ConvTranspose1d(kernel k, stride s, padding p) writes output o = i · s − p + t, t ∈ [0, k), so outputs [lo, hi] read
    inputs ⌈(lo + p − k + 1) / s⌉ … ⌊(hi + p) / s⌋. All hop samples of the frame are taken together: the bound holds for every phase."""
    f = 1000  # any frame: the arithmetic is translation invariant in whole frames
    lo, hi = f * cfg.hop, f * cfg.hop + cfg.hop - 1
    lo, hi = lo - 3, hi + 3  # conv_post, kernel 7
    for u in range(cfg.n_ups - 1, -1, -1):
        widest = 0
        for j in range(cfg.n_rb):
            K, reach = cfg.rb_kernels[j], 0
            for d in range(cfg.rb_n_dil):
                reach += (K - 1) // 2 * cfg.rb_dilations[j][d] + ((K - 1) // 2 if cfg.resblock_type == 1 else 0)
            widest = max(widest, reach)
        lo, hi = lo - widest, hi + widest
        k, s = cfg.up_kernels[u], cfg.up_rates[u]
        p = (k - s) // 2
        lo, hi = -((-(lo + p - k + 1)) // s), (hi + p) // s
    lo, hi = lo - 3, hi + 3  # conv_pre, kernel 7
    return f - lo, hi - f


def exact_reach(cfg):
    """The generator's true receptive field in latent frames per side (the larger of the two sides)."""
    return max(exact_reach_sides(cfg))


# ------------------------------------------------------------------------ the check of one step
class StepMismatch(AssertionError):
    """A step that fails outside the units: .check ("size", "gather" or "chunk"), .row (generator row, or None), .columns."""

    def __init__(self, msg, check, row=None, columns=None):
        super().__init__(msg)
        self.check, self.row, self.columns = check, row, columns


def unit_kind(name):
    """The kind of unit a bf16 row checks, by its name (bf16_ref.verify_item keeps none)."""
    if name == "audio":
        return "waveform"
    if name == "dec.conv_pre":
        return "conv_pre"
    if name == "dec.mean":
        return "mean"
    return "up" if name.endswith(".up") else "mean_act" if name.endswith("mean_act") else "rb_step"


def verify_step(rt, blob, slot, rows, chunks, z_of, precision, label="", report=print, full=True, only=None):
    """The check of the stream step that `slot` ran last. rows: the step's generator rows [NBg] from `schedule`; chunks: {row: the chunk
    the step delivered}; z_of(src) → the latent [inter, F] of the item in that row (the `z` tap of the slot whose front ran);
    precision "f32" / "bf16". full=False: checks 1 and 2 are left out (size and chunk = slice only). only: the generator rows that
    checks 1 – 3 look at (default: every row with Fc > 0); the size checks always cover every row.
    → dict(rows=[(unit name, compare dict)], ref_s=seconds of reference and comparison, names=the tap names the plan registered).
    Raises StepMismatch (size, check 1, check 3), f32_ref.UnitMismatch or bf16_ref's AssertionError (check 2)."""
    cfg = rt.cfg
    lens = [r.Fc for r in rows]
    live = [i for i, r in enumerate(rows) if r.Fc > 0 and (only is None or i in only)]
    for i, r in enumerate(rows):
        got = np.asarray(chunks.get(i, ())).size
        if got != r.n:
            raise StepMismatch(f"{label} row {i}: a chunk of {got} samples where the step delivers {r.n}", "size", i)
    mod = fr if precision == "f32" else br
    names = [("audio", 1, cfg.hop)] + ([("z", cfg.inter, 1)] if not full else mod.tap_names(cfg))
    try:
        taps = br.read_named_taps(rt, slot, names, lens, live, "window:")
    except br.TapSizeMismatch as e:
        raise StepMismatch(f"{label}: {e} — the window lengths on the device are not the schedule's {lens}", "size") from e
    R = (fr.F32Ref if precision == "f32" else br.Bf16Ref)(cfg, blob)
    out, t0 = [], time.time()
    for i in live:
        r, T = rows[i], taps[i]
        audio = T.pop("audio").reshape(-1)
        lab = f"{label}[row {i}]"
        if full:
            want = np.asarray(z_of(r.src), np.float32)[:, r.a:r.a + r.Fc]
            if not np.array_equal(T["z"], want):
                cols = np.unique(np.nonzero(T["z"] != want)[1]) if T["z"].shape == want.shape else None
                raise StepMismatch(f"{lab}: window:z is not z[{r.src}][:, {r.a}:{r.a + r.Fc}] (columns {None if cols is None else cols[:8].tolist()}…)",
                                   "gather", i, cols)
            out += mod.verify_item(R, T, audio, lab, report)
        chunk = np.asarray(chunks[i], np.float32).reshape(-1)
        if not np.array_equal(chunk, audio[r.skip:r.skip + r.n]):
            cols = np.nonzero(chunk != audio[r.skip:r.skip + r.n])[0]
            raise StepMismatch(f"{lab}: the chunk is not window:audio[{r.skip}:{r.skip + r.n}] ({cols.size} samples differ, first {cols[:4].tolist()})",
                               "chunk", i, cols)
    return dict(rows=out, ref_s=time.time() - t0, names=sorted(taps[live[0]]) if live else [])


def summary(rows, precision):
    """Worst figures of verify_step rows per kind of unit. fp32: |Δ| / bound, and the waveform's floor share. bf16: max|Δ| over the
    largest bound of the unit, the shares of elements that carry / needed the allowance, and median tolerance over the plain rule."""
    if precision == "f32":
        shares = [r["floor_share"] for _, r in rows if "floor_share" in r]
        return dict(worst={k: round(v, 5) for k, v in fr.worst_by_kind(rows).items()}, floor_share=round(max(shares), 5) if shares else 0.0)
    worst, allow, needed, med = {}, 0.0, 0.0, 0.0
    for name, r in rows:
        k = unit_kind(name)
        ratio = r["err"] / r["bound"] if r["bound"] > 0 else (0.0 if r["err"] == 0 else float("inf"))
        worst[k] = max(worst.get(k, 0.0), ratio)
        allow, needed = max(allow, r["allow_share"]), max(needed, r["needed_share"])
        if r["base"] > 0:
            med = max(med, r["median_tol"] / r["base"])
    return dict(worst={k: round(v, 5) for k, v in worst.items()}, allow_share=round(allow, 5), needed_share=round(needed, 5), median_ratio=round(med, 4))


# ------------------------------------------------------------------------ a stand-in for the GPU, and defects planted in it (CPU tests)
class StandIn:
    """Serves the "window:" taps of one step from tensors made on the CPU: rows[r] = {tap name: [C, len]} (with "audio": [1, len · hop]),
    None for a row that contributes nothing. Only what verify_step uses of HipRuntime: .cfg and .tap()."""

    def __init__(self, cfg):
        self.cfg, self.rows = cfg, []

    def tap(self, slot, name, max_floats=None):
        assert name.startswith("window:"), name
        parts = [np.asarray(T[name[7:]], np.float32).reshape(-1) for T in self.rows if T is not None and name[7:] in T]
        if not parts:
            raise ph.InvalidArgument(f"unknown tap '{name}'")
        return np.concatenate(parts)


class Planted(fr.F32Ref):
    """An fp32 generator with ONE defect of a window plan that was reused after a longer row: `prev` holds the tensors the plan's
    buffers kept of that longer row ({tap name: [C, len_prev]}), and the defective unit reads or keeps them past the new true length.
      ("input",)        the window's input is not zeroed past Fc: conv_pre convolves the previous window's latent columns in;
      ("rb", u, j, d)   step d of ResBlock j of stage u convolves its input's stale columns past the true length;
      ("up", u)         the ConvTranspose of stage u skips its last `pad` outputs, which keep the previous row's values
                        (the streaming kernel's bug of profiles/f32_exact_units.md)."""

    def __init__(self, cfg, blob, defect, prev, acc="f32"):
        super().__init__(cfg, blob, acc=acc)
        self.defect, self.prev = defect, prev

    def _tail(self, name, L):
        return np.asarray(self.prev[name], np.float64)[:, L:]

    def conv_pre(self, z):
        if self.defect[0] != "input":
            return super().conv_pre(z)
        L = np.asarray(z).shape[1]
        zz = np.concatenate([np.asarray(z, np.float64), self._tail("z", L)], axis=1)
        return fr.Plain(self.conv(zz, "dec.conv_pre", pad=3)[:, :L], "conv_pre")

    def _chain(self, u, j, d0, d1, x):
        if self.defect[0] != "rb" or self.defect[1:] != (u, j, d0) or d0 != d1:
            return super()._chain(u, j, d0, d1, x)
        L = np.asarray(x).shape[1]
        src = f"dec.s{u}.up" if d0 == 0 else f"dec.s{u}.rb{j}.c{d0 - 1}"
        return super()._chain(u, j, d0, d1, np.concatenate([np.asarray(x, np.float64), self._tail(src, L)], axis=1))[:, :L]

    def _convt(self, u, a):
        y = super()._convt(u, a)
        if self.defect[0] == "up" and self.defect[1] == u:
            pad, Lo = (self.cfg.up_kernels[u] - self.cfg.up_rates[u]) // 2, y.shape[1]
            y = np.array(y)
            y[:, Lo - pad:] = np.asarray(self.prev[f"dec.s{u}.up"], np.float64)[:, Lo - pad:Lo]
        return y


def window_taps(G, cfg, view):
    """A free-running generator's tensors as the taps of one window-plan row: what a plan of schedule `view` registers, plus the waveform."""
    T = {k: np.asarray(v, np.float32) for k, v in fr.schedule_view(cfg, G, view).items()}
    T["audio"] = np.asarray(G["audio"], np.float32).reshape(1, -1)
    return T


def fp32_view(cfg, st):
    """The taps an fp32 window plan of a step registers: the pair plan from NBg · Fb ≥ 128, the merged plan conv by conv below."""
    return "pair" if st.NBg * st.Fb >= 128 else "merged"


# ------------------------------------------------------------------------ the inputs of the GPU cases
# name → frames per item, chunk, seed of fr.utterance. The GPU tests take their inputs from here; test_stream_ref.py checks the windows
# they verify against the saturation condition of the waveform rule (floor share ≤ FLOOR_SHARE_MAX) from the oracle's z alone.
CASES = {
    "reuse": dict(Fs=(70,), chunk=20, seed=700),
    "pair": dict(Fs=(230,), chunk=100, seed=710),
    "group": dict(Fs=(70, 9, 41), chunk=20, seed=720),
    "one_frame": dict(Fs=(40,), chunk=1, seed=730, voices=("medium",)),
    "one_frame_group": dict(Fs=(40, 40), chunk=1, seed=735, voices=("medium",)),
    "pool": dict(Fs=(60, 25, 11), chunk=16, seed=740),  # sessions A, B, C
    "per_conv": dict(Fs=(90,) * 32, chunk=40, seed=750, items=(0, 7, 31), steps=(0, 1)),
}
POOL_EVENTS = (("join", 0, 0, 60, "A"), ("join", 0, 1, 25, "B"), ("join", 2, 1, 11, "C"))  # C takes B's row once B has ended (2 steps)


def case_utterances(cfg, name):
    c = CASES[name]
    return [fr.utterance(cfg, F, c["seed"] + 17 * i + F) for i, F in enumerate(c["Fs"])]


def per_conv_chunk(halo, F=90, chunk=40, batch=32):
    """Case "per_conv": the largest chunk ≤ 40 at which step 2 of a group of F-frame items runs a 64-frame plan (NBg · Fb = 2048 > 1536)."""
    for c in range(chunk, 0, -1):
        w = window_of(F, c, c, halo, 1)
        if c < F and bucket_f(w.Fc) == 64:
            return c
    raise AssertionError("no chunk puts step 2 on a 64-frame plan")


def case_schedule(cfg, name, halo):
    """→ (chunk, [Step]) of a case as the GPU test runs it (the pool with POOL_EVENTS; the drop run of "group" is the test's own)."""
    c = CASES[name]
    chunk = per_conv_chunk(halo) if name == "per_conv" else c["chunk"]
    if name == "pool":
        return chunk, schedule((0, 0, 0, 0), chunk, halo, cfg.hop, POOL_EVENTS)
    return chunk, schedule(c["Fs"], chunk, halo, cfg.hop)


def one_frame_steps(steps):
    """The steps of a one-frame-chunk case that are verified in full: the first, the last, and for each of a mod 4 = 0 … 3 the first
    step whose window starts at such an a > 0 (the gather's vector branch at a ≠ 0 and its scalar branch at every misalignment)."""
    pick = {0, len(steps) - 1}
    for m in range(4):
        pick.add(next(i for i, st in enumerate(steps) if st.rows[0].a > 0 and st.rows[0].a % 4 == m))
    return sorted(pick)


def verified_windows(cfg, name, halo):
    """[(step index, generator row, item index of case_utterances, a, Fc)] of the windows the GPU case checks unit by unit."""
    c = CASES[name]
    chunk, steps = case_schedule(cfg, name, halo)
    pick = range(len(steps))
    if name.startswith("one_frame"):
        pick = one_frame_steps(steps)
    elif "steps" in c:
        pick = c["steps"]
    out = []
    for i in pick:
        for r, row in enumerate(steps[i].rows):
            if row.Fc == 0:
                continue
            item = "ABC".index(row.src) if name == "pool" else row.src
            if "items" in c and item not in c["items"]:
                continue
            out.append((i, r, item, row.a, row.Fc))
    return out
