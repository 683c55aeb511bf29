"""GPU: every unit of the streaming window plans against the float64 (fp32) and the rounding-exact (bf16) reference, step by step.

A stream runs the generator on PLAN_GENERATOR window plans; the "window:" selector of piper_hip_voice_tap reaches the plan of a slot's
latest step. Every case below checks each step with stream_ref.verify_step: the tap sizes against the window lengths of the restated rule
(which checks the lengths the device wrote), the gather bit for bit, every unit of the window's generator teacher-forced from the GPU's
own taps under the rules of f32_ref / bf16_ref as they stand (no tolerance is defined here), and the delivered chunk bit for bit against
the window's waveform. The schedule each window takes is asserted from "window:@steps" and the restated rule, so a case cannot silently
stop running what it was chosen for:
  fp32   NBg · Fb ≥ 128: the pair kernel on the 32- and 64-channel stages, conv by conv below (three convs per launch either way);
  bf16   NBg · Fb ≤ 1536: the merged schedule ("rb012" launches), one launch per conv above.
What window plans add to the whole-utterance cases of test_gpu_f32_exact.py / test_gpu_bf16_exact.py: lengths written on the device and
changing at every step, rows of true length 0 next to live ones (pad, finished, dropped and free rows), a plan reused at every step —
often after a longer row —, window starts off the 4-frame grid, and schedules chosen by NBg · Fb with short rows.
Inputs: stream_ref.CASES (tests/test_stream_ref.py holds every verified window to the saturation condition of the waveform rule).
Per case one `STREAMWIN {json}` line: worst ratio per kind of unit, the seconds the reference took and the wall time."""
import json
import time

import numpy as np
import pytest

import bf16_ref as br
import f32_ref as fr
import piper_hip as ph
import stream_ref as sr

pytestmark = pytest.mark.gpu
PAIR_NAMES = {1: "ab_lrelu_conv_lrelu_conv_res_x3", 2: "_lrelu_conv_res_pair_x3"}
QUIET = lambda s: None
BOTH = [(q, p) for q in ("medium", "high") for p in ("f32", "bf16")]


@pytest.fixture(scope="module")
def rts(backend, voices):
    out = {}
    for q, p in BOTH:
        out[q, p] = ph.HipRuntime(backend, *voices[q])
        if p == "bf16":
            out[q, p].set_precision("bf16")
    yield out
    for rt in out.values():
        rt.close()


def assert_schedule(cfg, prec, st, launches):
    """The launches of the step's window plan are those of the schedule that the restated rule gives the step. → its name."""
    assert launches and all(n.startswith("dec.") for n in launches), launches
    rb = [n for n in launches if ".rb" in n]
    if prec == "bf16":
        merged = st.NBg * st.Fb <= 1536
        assert rb and all(("rb012." in n) == merged for n in rb), (st.NBg, st.Fb, rb)
        return "merged" if merged else "per_conv"
    pair = st.NBg * st.Fb >= 128
    for u in range(cfg.n_ups):
        su = [n for n in rb if n.startswith(f"dec.s{u}.")]
        assert su and all(n.endswith("_x3") for n in su), (u, su)
        paired = [n for n in su if PAIR_NAMES[cfg.resblock_type] in n]
        want = pair and (cfg.up_initial >> (u + 1)) in (32, 64)
        assert (len(paired) == len(su)) if want else not paired, (u, st.NBg, st.Fb, su)
    return "pair" if pair else "conv_by_conv"


class Case:
    """One case's bookkeeping: every verified step's rows, the schedules the windows took, the STREAMWIN line."""

    def __init__(self, rt, blob, quality, prec, name):
        self.rt, self.blob, self.quality, self.prec, self.name = rt, blob, quality, prec, name
        self.rows, self.ref_s, self.plans, self.t0, self.bit_only = [], 0.0, [], time.time(), 0
        self.halo = sr.halo_formula(rt.cfg)
        assert rt.lib.piper_hip_voice_receptive_field(rt.voice) == self.halo

    def step(self, slot, st, chunks, z_of, i, full=True, only=None):
        label = f"{self.name} {self.quality} {self.prec} step {i + 1}"
        res = sr.verify_step(self.rt, self.blob, slot, st.rows, chunks, z_of, self.prec, label, QUIET, full=full, only=only)
        kind = assert_schedule(self.rt.cfg, self.prec, st, self.rt.steps(slot, window=True))
        self.rows += res["rows"]
        self.ref_s += res["ref_s"]
        self.plans.append((max(r.Fc for r in st.rows), st.Fb, st.NBg, kind))
        self.bit_only += 0 if full else 1
        return kind

    def report(self):
        print("STREAMWIN " + json.dumps(dict(case=self.name, voice=self.quality, precision=self.prec, plans=self.plans, bit_checked_only=self.bit_only,
                                             ref_s=round(self.ref_s, 2), wall_s=round(time.time() - self.t0, 2), **sr.summary(self.rows, self.prec))))


def latents(rt, slot, Fs):
    """The z tap of the slot whose front ran, per item [inter, F]."""
    return [t["z"] for t in br.read_named_taps(rt, slot, [("z", rt.cfg.inter, 1)], list(Fs))]


def stream_single(case, utt, chunk, slot, steps, full=None):
    """One pass of a single stream, every step checked (full: the step indices checked unit by unit; None = all). → the chunks."""
    rt, z, out = case.rt, None, []
    for i, audio in enumerate(rt.synthesize_stream(*utt, fr.NOISE_SCALE, chunkFrames=chunk, slot=slot)):
        assert i < len(steps), "more steps than the rule gives"
        if z is None:
            z = latents(rt, slot, [sum(utt[1])])[0]
        case.step(slot, steps[i], {0: audio}, lambda src: z, i, full=full is None or i in full)
        out.append(audio)
    assert len(out) == len(steps)
    return out


def stream_group(case, utts, chunk, slot, steps, full=None, only=None, drop=None):
    """One pass of a group. drop = (steps run, item): stream_drop after that many steps. → [per step: the items' chunks]."""
    rt, zs, out = case.rt, None, []
    for i, chunks in enumerate(rt.synthesize_stream_batch(utts, fr.NOISE_SCALE, chunkFrames=chunk, slot=slot)):
        assert i < len(steps), "more steps than the rule gives"
        if zs is None:
            zs = latents(rt, slot, [sum(u[1]) for u in utts])
        case.step(slot, steps[i], {r: c for r, c in enumerate(chunks) if c.size}, lambda src: zs[src], i, full=full is None or i in full, only=only)
        out.append(chunks)
        if drop and i + 1 == drop[0]:
            rt.stream_drop(slot, drop[1])
    assert len(out) == len(steps)
    return out


@pytest.mark.parametrize("quality,prec", BOTH)
def test_single_stream_short_windows_on_reused_plans(quality, prec, rts, voices):
    """F = 70, chunk 20. Medium: 32, 44, 42 and 22 frames on plans of 32, 48, 48 and 32 — steps 3 and 4 run a plan that last held a longer
    row. High (halo 15): 35, 50, 45, 25 frames on plans of 48, 64, 48, 32 — no such step in one pass, so the stream runs a second time and
    the steps of the second pass that follow a longer row (by the restated rule) are checked unit by unit, the others bit for bit."""
    cfg, blob = voices[quality]
    case = Case(rts[quality, prec], blob, quality, prec, "reuse")
    utt = sr.case_utterances(cfg, "reuse")[0]
    chunk, steps = sr.case_schedule(cfg, "reuse", case.halo)
    passes = 1 if sr.reused_after_longer(steps) else 2
    reuse = sr.reused_after_longer(steps * passes)
    assert reuse, "the case must run a plan that last held a longer row"
    first = stream_single(case, utt, chunk, 0, steps)
    if passes == 2:
        again = stream_single(case, utt, chunk, 0, steps, full={i - len(steps) for i in reuse if i >= len(steps)})
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a reused plan must give what it gave before"
    case.report()


@pytest.mark.parametrize("quality,prec", BOTH)
def test_single_stream_on_the_pair_kernel(quality, prec, rts, voices):
    """F = 230, chunk 100: medium's second window (124 frames, Fb = 128) runs the pair kernel on the 32- and 64-channel stages, its first
    (Fb = 112) is still conv by conv; the last window is short (and conv by conv on both voices)."""
    cfg, blob = voices[quality]
    case = Case(rts[quality, prec], blob, quality, prec, "pair")
    chunk, steps = sr.case_schedule(cfg, "pair", case.halo)
    stream_single(case, sr.case_utterances(cfg, "pair")[0], chunk, 1, steps)
    kinds = [p[3] for p in case.plans]
    if prec == "f32":
        assert "pair" in kinds and kinds[-1] == "conv_by_conv", kinds
        assert quality != "medium" or kinds == ["conv_by_conv", "pair", "conv_by_conv"], kinds
    case.report()


@pytest.mark.parametrize("quality,prec", BOTH)
def test_group_with_a_pad_row_ragged_ends_and_a_drop(quality, prec, rts, voices):
    """n = 3 (NBg = 4: row 3 has length 0 at every step), F = 70, 9, 41 at chunk 20: item 1 ends after step 1 and item 2 after step 3, so
    rows of length 0 appear next to live ones; NBg · Fb ≥ 128 puts the short rows on fp32's pair kernel. Then the same group with
    stream_drop(slot, 0) after step 2: the dropped row's window length is 0 from then on (the tap sizes), rows 1 and 2 stay bit-equal.

    This case found the step choosing its plan from the rows that still deliver: without row 0's 42- / 45-frame window, step 3 of the
    drop run took the 16-frame plan (NBg · Fb = 64: conv by conv) where the first run took the 48-frame plan (192: the pair kernel), and
    row 2's fp32 chunk came out 9.8e-07 (medium) / 1.3e-06 (high) away from the first run's — another kernel, another summation order.
    batched_step now lets a dropped item's window size the plan until the frame where the item would have ended; the restated rule
    (stream_ref.schedule) says the same, and the drop run's plans are asserted equal to the first run's."""
    cfg, blob = voices[quality]
    case = Case(rts[quality, prec], blob, quality, prec, "group")
    utts = sr.case_utterances(cfg, "group")
    chunk, steps = sr.case_schedule(cfg, "group", case.halo)
    assert steps[0].NBg == 4 and all(st.rows[3].Fc == 0 for st in steps) and any(st.rows[1].Fc == 0 and st.rows[0].Fc > 0 for st in steps)
    first = stream_group(case, utts, chunk, 2, steps)
    if prec == "f32":
        assert "pair" in [p[3] for p in case.plans]
    dropped = sr.schedule(sr.CASES["group"]["Fs"], chunk, case.halo, cfg.hop, [("drop", 2, 0)])
    assert all(st.rows[0].Fc == 0 for st in dropped[2:]) and len(dropped) > 2
    assert [st.Fb for st in dropped] == [st.Fb for st in steps[:len(dropped)]], "a drop must not move the other rows to another plan"
    second = stream_group(case, utts, chunk, 2, dropped, full=set(range(2, len(dropped))), drop=(2, 0))
    case.report()
    unequal = []
    for i, chunks in enumerate(second):
        assert chunks[0].size == (first[i][0].size if i < 2 else 0)
        for r in (1, 2):
            assert chunks[r].size == first[i][r].size
            if not np.array_equal(chunks[r], first[i][r]):
                d = float(np.max(np.abs(chunks[r] - first[i][r])))
                print(f"DROP {quality} {prec} step {i + 1} row {r}: max|Δ| {d:.3e} against the first run, plan Fb {steps[i].Fb} there and {dropped[i].Fb} here")
                unequal.append((i + 1, r, d, steps[i].Fb, dropped[i].Fb))
    assert not unequal, f"rows 1 and 2 must stay bit-equal to the first run: (step, row, max|Δ|, Fb first run, Fb drop run) {unequal}"


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_one_frame_chunks(prec, rts, voices):
    """Medium, F = 40, chunk 1, a single stream and a group of 2: window starts at every a mod 4 (the gather's scalar branch) and skips that
    are no multiple of 4 samples. Checked unit by unit: the first and the last step and the first step at each a mod 4 with a > 0; the
    other steps by the tap sizes and the bit-equality of chunk and window:audio."""
    cfg, blob = voices["medium"]
    for name, slot in (("one_frame", 3), ("one_frame_group", 4)):
        case = Case(rts["medium", prec], blob, "medium", prec, name)
        utts = sr.case_utterances(cfg, name)
        chunk, steps = sr.case_schedule(cfg, name, case.halo)
        full = set(sr.one_frame_steps(steps))
        assert {steps[i].rows[0].a % 4 for i in full if steps[i].rows[0].a > 0} == {0, 1, 2, 3} and len(steps) == 40
        if len(utts) == 1:
            stream_single(case, utts[0], chunk, slot, steps, full=full)
        else:
            stream_group(case, utts, chunk, slot, steps, full=full)
        case.report()


@pytest.mark.parametrize("quality,prec", BOTH)
def test_pool_row_taken_over_by_a_shorter_session(quality, prec, rts, voices):
    """Capacity 4, chunk 16, plain joins through one work slot: A (F = 60) and B (F = 25) join; B ends after step 2 and C (F = 11) joins
    into B's row while A is mid-stream — C's first window follows B's longer ones in the same generator row and the same row store."""
    cfg, blob = voices[quality]
    rt = rts[quality, prec]
    case = Case(rt, blob, quality, prec, "pool")
    uA, uB, uC = sr.case_utterances(cfg, "pool")
    chunk, steps = sr.case_schedule(cfg, "pool", case.halo)
    assert steps[2].rows[1].src == "C" and steps[1].rows[1].src == "B" and steps[1].rows[1].Fc > steps[2].rows[1].Fc and steps[2].rows[0].src == "A"
    pool = rt.stream_pool(5, 4, chunkFrames=chunk, work_slot=6)
    with pytest.raises(ph.InvalidArgument, match="no stream step"):
        rt.tap(5, "window:z")
    assert [r for r, _ in pool.join([uA, uB], fr.NOISE_SCALE)] == [0, 1]
    z = dict(zip("AB", latents(rt, 6, [60, 25])))  # the work slot's z, after the join and before the next prepare on it
    for i, st in enumerate(steps):
        if i == 2:
            assert [r for r, _ in pool.join([uC], fr.NOISE_SCALE)] == [1], "C takes B's row"
            z["C"] = latents(rt, 6, [11])[0]
        case.step(5, st, pool.step(), lambda src: z[src], i)
    assert pool.step() == {} and pool.free_rows == 4
    pool.close()
    case.report()


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_bf16_per_conv_schedule_on_window_plans(quality, rts, voices):
    """A group of 32 items of F = 90: at step 2 every window runs a 64-frame plan, NBg · Fb = 2048 > 1536 — one launch per conv. Medium:
    chunk 40 (62-frame windows); high: the largest chunk ≤ 40 that puts step 2 on a 64-frame plan. Items 0, 7, 31 at steps 1 and 2."""
    cfg, blob = voices[quality]
    case = Case(rts[quality, "bf16"], blob, quality, "bf16", "per_conv")
    c = sr.CASES["per_conv"]
    chunk, steps = sr.case_schedule(cfg, "per_conv", case.halo)
    assert steps[1].Fb == 64 and steps[1].NBg == 32 and (quality != "medium" or (chunk == 40 and steps[1].rows[0].Fc == 62))
    rt, zs = case.rt, None
    for i, chunks in enumerate(rt.synthesize_stream_batch(sr.case_utterances(cfg, "per_conv"), fr.NOISE_SCALE, chunkFrames=chunk, slot=7)):
        if i in c["steps"]:
            zs = zs or latents(rt, 7, c["Fs"])
            case.step(7, steps[i], {r: ch for r, ch in enumerate(chunks) if ch.size}, lambda src: zs[src], i, only=c["items"])
    assert case.plans[1][3] == "per_conv", case.plans
    case.report()


def test_the_selector_refuses_what_it_cannot_reach(backend, voices):
    cfg, blob = voices["medium"]
    utt, other = fr.utterance(cfg, 70, 70), fr.utterance(cfg, 33, 71)
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        halo = rt.lib.piper_hip_voice_receptive_field(rt.voice)
        assert halo == sr.halo_formula(cfg) >= sr.exact_reach(cfg)
        with pytest.raises(ph.InvalidArgument):
            rt.tap(0, "window:z")  # nothing on the slot
        rt.prepare(0, *utt, fr.NOISE_SCALE)
        with pytest.raises(ph.InvalidArgument, match="no stream step"):
            rt.tap(0, "window:z")
        a = rt.synthesize_stream(*utt, fr.NOISE_SCALE, chunkFrames=20, slot=0)
        next(a)
        w = sr.window_of(70, 0, 20, halo, cfg.hop)
        assert rt.tap(0, "window:z").size == cfg.inter * w.Fc and rt.tap(0, "window:audio").size == w.Fc * cfg.hop  # (sized by the library)
        launches = rt.steps(0, window=True)
        assert launches and all(n.startswith("dec.") for n in launches)
        with pytest.raises(ph.UnsupportedOp):
            rt.tap(0, "window:z@dec.conv_pre")
        with pytest.raises(ph.InvalidArgument, match="unknown tap"):
            rt.tap(0, "window:enc_out")
        # another stream runs the same window plan (one item, 32 frames): slot 0's step is no longer what the plan holds
        b = rt.synthesize_stream(*utt, fr.NOISE_SCALE, chunkFrames=20, slot=2)
        next(b)
        with pytest.raises(ph.InvalidArgument, match="another step since"):
            rt.tap(0, "window:z")
        assert rt.tap(2, "window:z").size == cfg.inter * w.Fc
        # a prepare on the slot forgets its stream's step
        next(a)
        assert rt.tap(0, "window:z").size == cfg.inter * sr.window_of(70, 20, 20, halo, cfg.hop).Fc
        # eviction: one cached plan, and an unrelated prepare — the idle window plans go
        rt.set_plan_cache(1)
        rt.prepare(3, *other, fr.NOISE_SCALE)
        with pytest.raises(ph.InvalidArgument, match="evicted"):
            rt.tap(0, "window:z")
        rt.prepare(0, *utt, fr.NOISE_SCALE)
        with pytest.raises(ph.InvalidArgument, match="no stream step"):
            rt.tap(0, "window:z")
    finally:
        rt.close()
