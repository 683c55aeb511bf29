"""CPU: the streaming contract restated (tests/stream_ref.py) validated on its own, before it judges a stream step on the GPU.

* the window rule: the chunks of `window_of` cover [0, F · hop) exactly once and no window leaves [0, F);
* the halo is enough, shown on the float64 reference: one perturbed latent frame moves no sample further away than `exact_reach`, and the
  library's formula (restated as `halo_formula`) is at least `exact_reach` for the four presets;
* self-consistency: an honest fp32 generator run window by window passes verify_step with the taps of the plan each step takes;
* planted defects, applied to the stand-in's tensors of one row of one step, fail verify_step where they were planted, by at least 5 × the
  bound where a bound applies — while the whole-stream checks that streams had before (2e-5 · max(1, ‖whole‖∞) for fp32, 40 dB for bf16)
  are printed next to them: those take the defective stream against the whole utterance;
* the windows that the GPU cases verify meet the saturation condition of the waveform rule (floor share ≤ 10 %)."""
import numpy as np
import pytest

import f32_ref as fr
import oracle as orc
import piper_hip as ph
import stream_ref as sr

QUIET = dict(report=lambda s: None)
STREAM_TOL = 2e-5   # the fp32 streams' whole-utterance check (test_gpu_voice.py, test_gpu_stream_batch.py)
STREAM_SNR_DB = 40  # the bf16 streams'


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10.0 * np.log10(np.sum(ref ** 2) / max(np.sum((got - ref) ** 2), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("chunk", [1, 7, 16, 20, 64])
@pytest.mark.parametrize("halo", [12, 15])
def test_window_chunks_cover_the_utterance_exactly_once(chunk, halo):
    hop = 4
    for F in range(1, 3 * (chunk + 2 * halo) + 1):
        covered, nxt = np.zeros(F * hop, np.int32), 0
        while nxt < F:
            w = sr.window_of(F, nxt, chunk, halo, hop)
            assert 0 <= w.a and w.a + w.Fc <= F and w.Fc >= 1, (F, nxt, w)
            assert w.a <= nxt and w.end <= w.a + w.Fc and w.skip == (nxt - w.a) * hop, (F, nxt, w)
            assert nxt - w.a == min(halo, nxt) and w.a + w.Fc - w.end == min(halo, F - w.end), "the halo is whole wherever the utterance has it"
            assert 0 < w.n <= chunk * hop and w.skip + w.n <= w.Fc * hop, (F, nxt, w)
            covered[w.a * hop + w.skip:w.a * hop + w.skip + w.n] += 1
            assert w.end > nxt
            nxt = w.end
        assert np.all(covered == 1), (F, chunk)
        single = sr.schedule([F], chunk, halo, hop)
        assert len(single) == -(-F // chunk) and all(st.NBg == 1 and st.Fb == sr.bucket_f(st.rows[0].Fc) for st in single)


def test_schedule_of_a_group_with_a_pad_row_a_drop_and_pool_joins():
    hop, halo = 256, 12
    st = sr.schedule((70, 9, 41), 20, halo, hop)
    assert [s.NBg for s in st] == [4] * 4 and all(s.rows[3] == sr.IDLE for s in st)
    assert [[r.Fc for r in s.rows] for s in st] == [[32, 9, 32, 0], [44, 0, 33, 0], [42, 0, 13, 0], [22, 0, 0, 0]]
    assert [s.Fb for s in st] == [32, 48, 48, 32]
    dropped = sr.schedule((70, 9, 41), 20, halo, hop, [("drop", 2, 0)])
    assert [[r.Fc for r in s.rows] for s in dropped] == [[32, 9, 32, 0], [44, 0, 33, 0], [0, 0, 13, 0]]
    assert [s.Fb for s in dropped] == [32, 48, 48], "the dropped item's window still sizes step 3's plan: row 2 runs what it ran without the drop"
    assert [s.Fb for s in sr.schedule((9, 70), 20, halo, hop, [("drop", 1, 1)])] == [32], "dropped items alone run no step"
    pool = sr.schedule((0, 0, 0, 0), 16, halo, hop, sr.POOL_EVENTS)
    assert [[r.src for r in s.rows] for s in pool] == [["A", "B", None, None], ["A", "B", None, None], ["A", "C", None, None], ["A", None, None, None]]
    assert [r.Fc for r in pool[2].rows] == [40, 11, 0, 0] and pool[1].rows[1].Fc > pool[2].rows[1].Fc, "C's window follows B's longer one in row 1"
    assert sr.reused_after_longer(sr.schedule([70], 20, halo, hop)) == [2, 3], "medium F = 70, chunk 20: 32, 44, 42, 22 frames on plans of 32, 48, 48, 32"


# ---------------------------------------------------------------------------------------------------------------- the halo is enough
def test_the_halo_formula_covers_the_exact_reach_on_every_preset():
    for q in ("x_low", "low", "medium", "high"):
        cfg = ph.voice_config(q)
        left, right = sr.exact_reach_sides(cfg)
        print(f"{q}: exact reach {left} frames before, {right} after; halo formula {sr.halo_formula(cfg)}")
        assert sr.halo_formula(cfg) >= sr.exact_reach(cfg) >= 1
    assert sr.halo_formula(ph.voice_config("medium")) == 12 and sr.halo_formula(ph.voice_config("high")) == 15  # (by hand)


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_a_perturbed_latent_frame_moves_nothing_beyond_the_exact_reach(quality, voices):
    """Free-running float64 generator: z perturbed in ONE frame f; the samples that change lie in frames [f − right, f + left] of the exact
    reach (a sample of frame g reads z frames g − left … g + right). The measured reach may be smaller: exact_reach bounds every phase."""
    cfg, blob = voices[quality]
    left, right = sr.exact_reach_sides(cfg)
    F, f = left + right + 9, right + 4
    R = fr.F32Ref(cfg, blob)
    z = np.asarray(fr.utterance(cfg, F, 5)[2], np.float32)
    base = R.generator(z)["audio"]
    z2 = z.copy()
    z2[:, f] += 0.5
    moved = np.nonzero(R.generator(z2)["audio"] != base)[0]
    g0, g1 = int(moved.min()) // cfg.hop, int(moved.max()) // cfg.hop
    m_left, m_right = g1 - f, f - g0  # frames g that read z frame f: g − left ≤ f ≤ g + right
    print(f"{quality}: measured reach {m_left} frames before / {m_right} after, exact {left} / {right}, halo {sr.halo_formula(cfg)}")
    assert 0 <= m_left <= left and 0 <= m_right <= right
    assert m_left >= left - 1 and m_right >= right - 1, "the interval arithmetic is a whole frame wider than what the generator shows"


# ---------------------------------------------------------------------------------------------------------------- verify_step on a stand-in
class Streamed:
    """An utterance of F frames streamed window by window by an fp32 generator on the CPU (acc f32: torch's order), each step's row as the
    taps of the plan it takes; `defect` = (step, kind …) plants one in that step's generator (stream_ref.Planted)."""

    def __init__(self, cfg, blob, F, chunk, seed, defect=None, gather_off=0, skip_off=0):
        self.cfg, self.blob = cfg, blob
        ids, dur, noise = fr.utterance(cfg, F, seed)
        self.z = np.asarray(orc.synthesize(cfg, blob, ids, dur, noise, fr.NOISE_SCALE, taps=True)[1]["z"], np.float32)
        self.halo = sr.halo_formula(cfg)
        self.steps = sr.schedule([F], chunk, self.halo, cfg.hop)
        self.taps, self.chunks, held = [], [], {}
        for i, st in enumerate(self.steps):
            r = st.rows[0]
            off = gather_off if defect is None or defect[0] == i else 0
            zw = self.z[:, r.a + off:r.a + off + r.Fc]
            if defect is not None and defect[0] == i and len(defect) > 1:
                G = sr.Planted(cfg, blob, defect[1:], held[st.Fb]).generator(zw)
            else:
                G = fr.F32Ref(cfg, blob, acc="f32").generator(zw)
            held[st.Fb] = {k: v for k, v in G.items() if k not in ("v", "audio")}  # what the plan's buffers keep of this row
            self.taps.append(sr.window_taps(G, cfg, sr.fp32_view(cfg, st)))
            s_off = skip_off if defect is None or defect[0] == i else 0
            self.chunks.append(np.asarray(G["audio"], np.float32)[r.skip + s_off:r.skip + s_off + r.n])

    def audio(self):
        return np.concatenate(self.chunks)

    def verify(self, i, rows=None, chunks=None, taps=None):
        rt = sr.StandIn(self.cfg)
        rt.rows = [self.taps[i]] if taps is None else taps
        return sr.verify_step(rt, self.blob, 0, self.steps[i].rows if rows is None else rows, {0: self.chunks[i]} if chunks is None else chunks,
                              lambda src: self.z, "f32", f"step {i + 1}", **QUIET)


@pytest.fixture(scope="module")
def clean(voices):
    return {q: Streamed(*voices[q], 70, 20, 70) for q in ("medium", "high")}


@pytest.fixture(scope="module")
def wholes(voices, clean):
    return {q: fr.F32Ref(*voices[q], acc="f32").generator(clean[q].z)["audio"] for q in ("medium", "high")}


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_an_honest_streamed_generator_passes_every_step(quality, clean, wholes):
    s = clean[quality]
    worst = {}
    for i in range(len(s.steps)):
        for k, v in fr.worst_by_kind(s.verify(i)["rows"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    d = float(np.max(np.abs(s.audio() - wholes[quality])))
    print(f"{quality} F=70 chunk=20: worst |Δ|/bound per kind {({k: round(v, 4) for k, v in worst.items()})}; stream vs whole max|Δ| {d:.2e}")
    assert s.audio().size == wholes[quality].size and d <= STREAM_TOL * max(1.0, float(np.max(np.abs(wholes[quality]))))


def old_checks(s, whole, what):
    """The whole-stream checks that streams had before, on a defective stream: → (fp32 check passes, bf16 check passes), printed."""
    d = float(np.max(np.abs(s.audio() - whole)))
    bound = STREAM_TOL * max(1.0, float(np.max(np.abs(whole))))
    snr = snr_db(s.audio(), whole)
    print(f"DEFECT {what}: whole-stream max|Δ| {d:.3e} against {bound:.1e} ({'passes' if d <= bound else 'FAILS'}), "
          f"SNR {snr:.1f} dB against {STREAM_SNR_DB} ({'passes' if snr >= STREAM_SNR_DB else 'FAILS'})")
    return d <= bound, snr >= STREAM_SNR_DB


def reuse_step(s):
    """The step of the stream whose plan last held a longer row (stream_ref.reused_after_longer) — None if the stream has none."""
    steps = sr.reused_after_longer(s.steps)
    return steps[0] if steps else None


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_defect_a_gather_offset_fails_check_1(quality, voices):
    s = Streamed(*voices[quality], 70, 20, 70, defect=(1,), gather_off=1)
    with pytest.raises(sr.StepMismatch) as e:
        s.verify(1)
    assert e.value.check == "gather" and e.value.row == 0
    s.verify(0)
    s.verify(2)


def test_defects_b_c_d_fail_at_their_unit_by_five_bounds_and_pass_the_old_stream_checks(voices, clean, wholes):
    """Medium F = 70, chunk 20: step 3 (42 frames) runs the 48-frame plan that step 2 left 44 frames in. On the high voice no step of this
    stream follows a longer row on its plan (35, 50, 45, 25 frames on plans of 48, 64, 48, 32), so the defects are planted on medium."""
    quality = "medium"
    cfg, blob = voices[quality]
    i = reuse_step(clean[quality])
    assert i == 2 and reuse_step(clean["high"]) is None
    Fc, last = clean[quality].steps[i].rows[0].Fc, cfg.rb_n_dil - 1
    R = fr.F32Ref(cfg, blob)
    seen = {}
    for what, defect, unit, width in (
            ("(b) input not zeroed past Fc", ("input",), "dec_pre", 3),
            ("(c) ResBlock step on stale columns", ("rb", 1, 1, last), f"dec.s1.rb1.c{last}", R.reach(1, last)),
            ("(d) ConvTranspose keeps its last pad outputs", ("up", 1), "dec.s1.up", (cfg.up_kernels[1] - cfg.up_rates[1]) // 2)):
        s = Streamed(cfg, blob, 70, 20, 70, defect=(i,) + defect)
        with pytest.raises(fr.UnitMismatch) as e:
            s.verify(i)
        L = s.taps[i][unit].shape[1]
        cols, ratio = e.value.columns, e.value.result["ratio"]
        print(f"DEFECT {what}: fails {e.value.unit} in columns {cols.min()}…{cols.max()} of {L}, |Δ|/bound {ratio:.1f}")
        assert e.value.unit == unit and cols.max() == L - 1 and cols.min() >= L - width, (what, e.value.unit, cols.min(), L - width)
        assert ratio >= 5.0, (what, ratio)
        for k in range(len(s.steps)):  # every other step of the stream is clean
            if k != i:
                s.verify(k)
        seen[what] = old_checks(s, wholes[quality], what)
    # (measured, see profiles/stream_window_units.md) none of them is seen by the checks streams had: the stale columns lie at the window's end,
    # the chunk ends a halo before it
    assert all(f32_ok and bf16_ok for f32_ok, bf16_ok in seen.values()), seen


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_defect_e_skip_off_by_one_sample_fails_check_3(quality, voices, wholes):
    s = Streamed(*voices[quality], 70, 20, 70, defect=(1,), skip_off=1)
    with pytest.raises(sr.StepMismatch) as e:
        s.verify(1)
    assert e.value.check == "chunk" and e.value.row == 0
    old_checks(s, wholes[quality], f"(e) skip off by one sample, {quality}")


def test_defect_f_a_length_0_row_that_delivers_fails_the_size_check(voices, clean):
    """A group of two where row 1 has ended: its window length is 0, it contributes nothing to a tap and delivers nothing. A device
    length that stayed at the previous step's (the tap holds a second row), or a chunk out of the row's stale audio, trips the size check."""
    s = clean["medium"]
    rows = [s.steps[2].rows[0], sr.IDLE]
    s.verify(2, rows=rows, taps=[s.taps[2], None])
    with pytest.raises(sr.StepMismatch) as e:
        s.verify(2, rows=rows, taps=[s.taps[2], s.taps[1]])
    assert e.value.check == "size" and "window:" in str(e.value)
    with pytest.raises(sr.StepMismatch) as e:
        s.verify(2, rows=rows, taps=[s.taps[2], None], chunks={0: s.chunks[2], 1: s.chunks[1]})
    assert e.value.check == "size" and e.value.row == 1


# ---------------------------------------------------------------------------------------------------------------- the inputs of the GPU cases
@pytest.mark.parametrize("quality,name", [(q, n) for n in sorted(sr.CASES) for q in sr.CASES[n].get("voices", ("medium", "high"))])
def test_gpu_case_windows_meet_the_saturation_condition(quality, name, voices):
    """Every window that tests/test_gpu_stream_windows.py checks unit by unit: the share of samples where the floor of the waveform rule
    exceeds its slope term, from the oracle's z and the float64 reference alone."""
    cfg, blob = voices[quality]
    utts = sr.case_utterances(cfg, name)
    R, zs, worst = fr.F32Ref(cfg, blob), {}, 0.0
    for step, row, item, a, Fc in sr.verified_windows(cfg, name, sr.halo_formula(cfg)):
        if item not in zs:
            zs[item] = orc.synthesize(cfg, blob, *utts[item], fr.NOISE_SCALE, taps=True)[1]["z"]
        w = fr.Waveform(R.generator(zs[item][:, a:a + Fc])["v"])
        worst = max(worst, w.floor_share)
        assert w.floor_share <= fr.FLOOR_SHARE_MAX, (name, quality, step, row, w.floor_share)
    print(f"{name} {quality}: worst floor share of a verified window {100 * worst:.2f} %")
