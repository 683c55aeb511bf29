"""GPU: multi-speaker voices (include/piper_hip.h "Multi-speaker voices").

1. The request-path kernel (csrc/speaker.hip) against float64 recomputed from the blobs, with an a-priori bound and no measured
   tolerance: |e − ref| ≤ (gin + 8) · 2⁻²⁴ · (|b| + |bc| + Σ_j |W_cj| · Σ_k |w_k · emb_jk|) for every element of every item's speaker row.
2. End to end, bit for bit: item i's speaker row, as the GPU computed it, is written into the dp.pre / in_layers / dec.conv_pre biases of
   a copy of the voice blob (spk_ref.fold). That is a plain single-speaker voice, and the single-speaker path is checked against the
   oracle and the float64 references elsewhere; since a consumer adds one float per channel where it adds its bias, the conditioned run
   must equal that voice's run in the same plan shape — on every route.
3. Speakers matter, nothing leaks between items, and a voice without a table is the voice it was."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import piper_hip as ph
import spk_ref as sr

pytestmark = pytest.mark.gpu

S = 5
IDS = list(kd.FIXTURE_IDS)                      # 14 ids
DUR = [2] * 12 + [3] * 2                        # 30 frames
SPK3 = [4, 0, 2]                                # the speakers of the batches of 3
CHUNK = 16


def noise_of(cfg, F, seed=4321):
    return kd.sym(seed, (cfg.inter, F), 1.7320508)


def utts3(cfg):
    """A ragged batch of 3: 14 ids / 30 frames, 9 ids / 21 frames, 12 ids / 33 frames."""
    out = []
    for k, (n, dur) in enumerate(((14, DUR), (9, [2, 3] * 4 + [1]), (12, [3] * 9 + [2] * 3))):
        out.append((IDS[:n], dur, noise_of(cfg, sum(dur), 100 + k)))
    return out


class World:
    """One quality: the voice blob, a speaker blob, the conditioned runtime and the folded plain voices made so far (by speaker row)."""

    def __init__(self, backend, quality, gin, cfg=None, blob=None):
        self.backend = backend
        self.cfg = cfg if cfg is not None else ph.voice_config(quality)
        self.blob = blob if blob is not None else ph.synthetic_blob(self.cfg, 1234)
        self.lay = ph.blob_layout(self.cfg)
        self.gin = gin
        self.scfg = ph.speaker_config(S, gin)
        self.sblob = ph.synthetic_speaker_blob(self.cfg, self.scfg, 4321)
        self.emb, self.W, self.bc, self.b = sr.row_tables(self.cfg, S, gin, self.sblob, self.lay, self.blob)
        self.rt = ph.HipRuntime(backend, self.cfg, self.blob)
        self.rt.attach_speakers(self.scfg, self.sblob)
        self.folded = {}
        self.H = sr.dp_rows(self.cfg)

    def row(self, slot, item, predict):
        """Item `item`'s speaker row of the slot's last run as the GPU computed it: the flow and generator rows from the slot's plan, the
        dp.pre rows from the predictor plan when it ran (otherwise the voice's own dp.pre bias: that run does not read them)."""
        ctot = sr.row_floats(self.cfg)
        main = self.rt.tap(slot, "spk.bias").reshape(-1, ctot)[item]
        assert not np.any(main[:self.H]) and np.all(np.isfinite(main))  # a plan leaves the rows it does not compute 0.0
        row = main.copy()
        if predict:
            dp = self.rt.tap(slot, "predict:spk.bias").reshape(-1, ctot)[item]
            assert not np.any(dp[self.H:])
            row[:self.H] = dp[:self.H]
        else:
            row[:self.H] = self.b[:self.H]
        return row

    def plain(self, row, precision="f32"):
        """The plain single-speaker voice with `row` folded into its biases (made once per row and precision)."""
        key = (row.tobytes(), precision)
        if key not in self.folded:
            rt = ph.HipRuntime(self.backend, self.cfg, sr.fold(self.cfg, self.lay, self.blob, row))
            if precision != "f32":
                rt.set_precision(precision)
            self.folded[key] = rt
        return self.folded[key]

    def close(self):
        for rt in self.folded.values():
            rt.close()
        self.rt.close()


@pytest.fixture(scope="module")
def medium(backend, voices):
    w = World(backend, "medium", 512, *voices["medium"])
    yield w
    w.close()


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    assert a.size > 0 and np.all(np.isfinite(a)), what
    assert np.array_equal(a, b), f"{what}: {int(np.sum(a != b))} of {a.size} samples differ, max |Δ| = {float(np.max(np.abs(a - b))):.3e}"


# ---------------------------------------------------------------------------------------------- 1. the kernel against float64
MIXES = {1: [[(3, 1.0), (0, 0.5), (4, -0.25), (1, 1.5)]],                          # one item: a mix of 4
         3: [[(2, 1.0)], [(0, 0.25), (4, 0.75)], [(1, 0.4), (2, -0.3), (3, 1.2), (0, 0.1)]]}  # mixes of 1, 2 and 4


@pytest.fixture(scope="module")
def narrow(backend, voices):
    w = World(backend, "medium", 36, *voices["medium"])  # gin = 36: one partial sweep of the 64 lanes
    yield w
    w.close()


@pytest.mark.parametrize("gin", [512, 36])
@pytest.mark.parametrize("N", [1, 3])
def test_speaker_rows_against_float64(gin, N, medium, narrow):
    w = medium if gin == 512 else narrow
    rt, cfg = w.rt, w.cfg
    mixes = MIXES[N]
    items = utts3(cfg)[:N]
    rt.slot_speakers(6, [dict(m) for m in mixes])
    rt.prepare_batch(6, items)
    rt.launch(6)
    rt.collect(6)
    rt.predict_durations([(ids, None) for ids, _d, _n in items], speakers=[dict(m) for m in mixes])  # the predictor plan of the same bucket
    ctot = sr.row_floats(cfg)
    g = rt.tap(6, "spk.g").reshape(N, gin)
    e_main = rt.tap(6, "spk.bias").reshape(N, ctot)
    e_dp = rt.tap(6, "predict:spk.bias").reshape(N, ctot)
    assert np.array_equal(rt.tap(6, "predict:spk.g").reshape(N, gin), g)
    worst = 0.0
    for i, mix in enumerate(mixes):
        assert np.array_equal(g[i], sr.mix_f32(w.emb, mix)), f"item {i}: g is not the fp32 mix in ascending k"
        if len(mix) == 1 and mix[0][1] == 1.0:
            assert np.array_equal(g[i], w.emb[mix[0][0]])  # a single id at weight 1: the table row, bit for bit
        g64, e64, bound = sr.reference(w.emb, w.W, w.bc, w.b, mix)
        assert np.max(np.abs(g[i] - g64)) <= 4 * 2.0 ** -24 * np.max(np.abs(g64)) + 1e-30
        e = np.concatenate([e_dp[i, :w.H], e_main[i, w.H:]])  # every element of the row: no element is left out
        assert not np.any(e_main[i, :w.H]) and not np.any(e_dp[i, w.H:])
        err = np.abs(e.astype(np.float64) - e64)
        worst = max(worst, float(np.max(err / bound)))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, f"gin {gin} N {N} item {i}: {bad.size} rows over the bound, first {bad[0]}: {err[bad[0]]:.3e} > {bound[bad[0]]:.3e}"
    print(f"gin {gin} N {N}: worst |e - ref| / bound = {worst:.4f}")
    rt.slot_speakers(6, None)


# ---------------------------------------------------------------------------------------------- 2. end to end, bit for bit
def test_synthesize_given_and_predicted_durations(medium):
    w, cfg = medium, medium.cfg
    noise = noise_of(cfg, sum(DUR))
    got = w.rt.synthesize(IDS, DUR, noise, 0.667, speaker=3)
    plain = w.plain(w.row(0, 0, predict=False))
    same(got, plain.synthesize(IDS, DUR, noise, 0.667), "synthesize, given durations, speaker 3")
    assert got.size == sum(DUR) * cfg.hop
    # predicted durations: the predictor is conditioned too (dp.pre), the durations must be equal as well
    got = w.rt.synthesize(IDS, None, None, 0.667, noise_mode="device", seed=7, speaker={1: 0.5, 3: 0.5})
    dur = w.rt.durations(0)
    plain = w.plain(w.row(0, 0, predict=True))
    ref = plain.synthesize(IDS, None, None, 0.667, noise_mode="device", seed=7)
    assert np.array_equal(dur, plain.durations(0)) and dur.sum() >= 1
    same(got, ref, "synthesize, predicted durations, a mix of speakers 1 and 3")
    w.rt.slot_speakers(0, None)


@pytest.fixture(scope="module")
def batch3(medium):
    """The ragged batch of 3 with speakers (4, 0, 2) on the conditioned voice: waveform, sample counts, the three folded voices."""
    w = medium
    items = utts3(w.cfg)
    w.rt.slot_speakers(1, SPK3)
    w.rt.prepare_batch(1, items)
    w.rt.launch(1)
    audio = w.rt.collect(1).copy()
    pcm = w.rt.collect_pcm16(1).copy()
    per, _tot = w.rt.prepared_samples(1)
    plains = [w.plain(w.row(1, i, predict=False)) for i in range(3)]
    return items, audio, pcm, per, plains


def test_ragged_batch_item_by_item(medium, batch3):
    items, audio, pcm, per, plains = batch3
    assert per == [sum(d) * medium.cfg.hop for _i, d, _n in items]
    off = np.concatenate([[0], np.cumsum(per)])
    for i, plain in enumerate(plains):  # the same batch shape on the folded voice of item i: item i must be equal
        plain.prepare_batch(1, items)
        plain.launch(1)
        ref = plain.collect(1)
        same(audio[off[i]:off[i + 1]], ref[off[i]:off[i + 1]], f"ragged batch, item {i} (speaker {SPK3[i]})")
        same(pcm[off[i]:off[i + 1]], plain.collect_pcm16(1)[off[i]:off[i + 1]], f"collect_pcm16, item {i}")
    # the three speakers are three voices: item 0 on item 1's folded voice is something else
    assert not np.array_equal(audio[off[0]:off[1]], ref[off[0]:off[1]])


def test_bounded_prepare(medium):
    w = medium
    texts = [(IDS, None), (IDS[:9], None), (IDS[:12], None)]
    w.rt.slot_speakers(2, SPK3)
    w.rt.prepare_batch_bounded(2, texts, 256, noise_mode="device", seed=11)
    w.rt.launch(2)
    audio = w.rt.collect(2).copy()
    per, _tot = w.rt.prepared_samples(2)
    dur = w.rt.durations(2)
    off = np.concatenate([[0], np.cumsum(per)])
    for i in range(3):
        plain = w.plain(w.row(2, i, predict=True))
        plain.prepare_batch_bounded(2, texts, 256, noise_mode="device", seed=11)
        plain.launch(2)
        ref = plain.collect(2)
        per_p, _ = plain.prepared_samples(2)
        assert per_p[i] == per[i]
        o = int(np.sum(per_p[:i]))
        same(audio[off[i]:off[i + 1]], ref[o:o + per_p[i]], f"bounded prepare, item {i} (speaker {SPK3[i]})")
        t0 = sum(len(t[0]) for t in texts[:i])
        assert np.array_equal(dur[t0:t0 + len(texts[i][0])], plain.durations(2)[t0:t0 + len(texts[i][0])])
    w.rt.slot_speakers(2, None)


def test_single_stream_and_group(medium, batch3):
    w = medium
    items, _audio, _pcm, per, plains = batch3
    ids, dur, noise = items[2]
    w.rt.slot_speakers(3, [SPK3[2]])
    got = list(w.rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=CHUNK, slot=3))
    ref = list(plains[2].synthesize_stream(ids, dur, noise, 0.667, chunkFrames=CHUNK, slot=3))
    assert len(got) == len(ref) == -(-sum(dur) // CHUNK) and sum(c.size for c in got) == per[2]
    for k, (a, b) in enumerate(zip(got, ref)):
        same(a, b, f"single stream, chunk {k}")
    # a group of 3: every step's chunk of item i against the same group on item i's folded voice
    w.rt.slot_speakers(3, SPK3)
    got = list(w.rt.synthesize_stream_batch(items, 0.667, chunkFrames=CHUNK, slot=3))
    for i, plain in enumerate(plains):
        ref = list(plain.synthesize_stream_batch(items, 0.667, chunkFrames=CHUNK, slot=3))
        assert len(ref) == len(got)
        for k in range(len(got)):
            if got[k][i].size or ref[k][i].size:
                same(got[k][i], ref[k][i], f"group of 3, item {i}, step {k}")
        assert sum(step[i].size for step in got) == per[i]
    w.rt.slot_speakers(3, None)


def pool_scenario(rt, items, speakers):
    """Capacity 4, chunk 16: A joins alone; B and C one step later; when A has delivered its last chunk its row is free and D — another
    speaker — takes it. speakers: {name: speaker} or None (a plain voice). Returns {name: (row, [chunks])}."""
    utt = {"A": items[1], "B": items[0], "C": items[2], "D": items[0]}  # A: 21 frames = 2 chunks
    pool = rt.stream_pool(4, 4, chunkFrames=CHUNK, work_slot=5)
    live, out = {}, {}

    def join(*names):
        if speakers is not None:
            rt.slot_speakers(5, [speakers[n] for n in names])
        for name, (row, _samples) in zip(names, pool.join([utt[n] for n in names], 0.667)):
            live[row] = name
            out[name] = (row, [])

    def step():
        got = pool.step()
        for row, chunk in got.items():
            out[live[row]][1].append(chunk)
        return got

    join("A")
    step()
    join("B", "C")
    step()  # A's last chunk: row 0 is free
    assert pool.free_rows == 2
    join("D")
    assert out["D"][0] == out["A"][0] == 0  # the freed row, retaken
    for _ in range(16):
        if not step():
            break
    pool.close()
    return out


def test_stream_pool_rows_keep_and_change_speakers(medium, batch3):
    w = medium
    items, _audio, _pcm, _per, _plains = batch3
    speakers = {"A": 4, "B": 0, "C": 2, "D": 1}
    got = pool_scenario(w.rt, items, speakers)
    # the speaker rows of the four sessions, from the work slot's join plans (B and C shared one join)
    rows = {}
    rt = w.rt
    for names in (("A",), ("B", "C"), ("D",)):
        utt = {"A": items[1], "B": items[0], "C": items[2], "D": items[0]}
        rt.slot_speakers(7, [speakers[n] for n in names])
        rt.prepare_batch(7, [utt[n] for n in names])
        rt.launch(7)
        rt.collect(7)
        for k, n in enumerate(names):
            rows[n] = w.row(7, k, predict=False)
    rt.slot_speakers(7, None)
    for name in "ABCD":  # the same scenario on the session's folded voice: that session must be equal, chunk by chunk
        ref = pool_scenario(w.plain(rows[name]), items, None)
        assert got[name][0] == ref[name][0] and len(got[name][1]) == len(ref[name][1]) > 0
        for k, (a, b) in enumerate(zip(got[name][1], ref[name][1])):
            same(a, b, f"pool session {name} (speaker {speakers[name]}), chunk {k}")
    # D sits in the row A had and is another speaker: on A's folded voice session D is something else
    refA = pool_scenario(w.plain(rows["A"]), items, None)
    assert not np.array_equal(np.concatenate(got["D"][1]), np.concatenate(refA["D"][1]))
    rt.slot_speakers(5, None)


def test_bf16_generator(medium):
    w, cfg = medium, medium.cfg
    noise = noise_of(cfg, sum(DUR))
    w.rt.set_precision("bf16")
    try:
        got = w.rt.synthesize(IDS, DUR, noise, 0.667, speaker=4)
        row = w.row(0, 0, predict=False)
        same(got, w.plain(row, "bf16").synthesize(IDS, DUR, noise, 0.667), "bf16 generator, speaker 4")
        chunks = list(w.rt.synthesize_stream(IDS, DUR, noise, 0.667, chunkFrames=CHUNK, slot=0))
        ref = list(w.plain(row, "bf16").synthesize_stream(IDS, DUR, noise, 0.667, chunkFrames=CHUNK, slot=0))
        same(np.concatenate(chunks), np.concatenate(ref), "bf16 generator, single stream")
    finally:
        w.rt.set_precision("f32")
        w.rt.slot_speakers(0, None)


@pytest.mark.parametrize("quality,gin", [("high", 512), ("x_low", 36)])
def test_other_qualities(quality, gin, backend):
    w = World(backend, quality, gin)
    try:
        noise = noise_of(w.cfg, sum(DUR))
        got = w.rt.synthesize(IDS, None, None, 0.667, noise_mode="device", seed=3, speaker={2: 0.7, 4: 0.3})
        plain = w.plain(w.row(0, 0, predict=True))
        same(got, plain.synthesize(IDS, None, None, 0.667, noise_mode="device", seed=3), f"{quality}: predicted durations")
        got = w.rt.synthesize(IDS, DUR, noise, 0.667)  # the assignment persists
        same(got, plain.synthesize(IDS, DUR, noise, 0.667), f"{quality}: given durations")
        chunks = list(w.rt.synthesize_stream(IDS, DUR, noise, 0.667, chunkFrames=CHUNK, slot=0))
        same(np.concatenate(chunks), np.concatenate(list(plain.synthesize_stream(IDS, DUR, noise, 0.667, chunkFrames=CHUNK, slot=0))),
             f"{quality}: single stream")
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------- 3. speakers matter, nothing leaks
def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def test_speakers_differ_and_items_do_not_leak(medium, batch3):
    w, cfg = medium, medium.cfg
    noise = noise_of(cfg, sum(DUR))
    a = w.rt.synthesize(IDS, DUR, noise, 0.667, speaker=0)
    b = w.rt.synthesize(IDS, DUR, noise, 0.667, speaker=1)
    assert rms(a - b) > 0.01 * rms(a), f"speakers 0 and 1: RMS of the difference {rms(a - b):.3e} against {rms(a):.3e}"
    w.rt.slot_speakers(0, None)
    same(w.rt.synthesize(IDS, DUR, noise, 0.667), a, "the default assignment is speaker 0 alone")
    # item 1 changes its speaker: items 0 and 2 stay bit-identical, item 1 does not
    items, audio, _pcm, per, _plains = batch3
    off = np.concatenate([[0], np.cumsum(per)])
    w.rt.slot_speakers(1, [SPK3[0], 3, SPK3[2]])
    w.rt.prepare_batch(1, items)
    w.rt.launch(1)
    again = w.rt.collect(1)
    for i in (0, 2):
        same(again[off[i]:off[i + 1]], audio[off[i]:off[i + 1]], f"item {i} after item 1 changed its speaker")
    assert not np.array_equal(again[off[1]:off[2]], audio[off[1]:off[2]])
    # items past the assignment take its last entry
    w.rt.slot_speakers(1, [SPK3[0], 3])
    w.rt.prepare_batch(1, items)
    w.rt.launch(1)
    last = w.rt.collect(1)
    same(last[off[1]:off[2]], again[off[1]:off[2]], "item 1")
    assert np.array_equal(w.rt.tap(1, "spk.g").reshape(3, -1)[2], w.emb[3])
    w.rt.slot_speakers(1, SPK3)


def test_voice_without_table_is_unchanged(medium, voices, backend):
    cfg, blob = voices["medium"]
    noise = noise_of(cfg, sum(DUR))
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        before = rt.synthesize(IDS, DUR, noise, 0.667)
        steps = rt.steps(0)
        assert rt.num_speakers() == 0
        with pytest.raises(ph.UnsupportedOp):
            rt.slot_speakers(0, [0])
        with pytest.raises(ph.UnsupportedOp):
            rt.predict_durations([(IDS, None)], speakers=[0])
        with pytest.raises(ph.InvalidArgument):
            rt.tap(0, "spk.bias")
        with pytest.raises(ph.InvalidArgument):  # the table comes before the first prepare
            rt.attach_speakers(medium.scfg, medium.sblob)
        same(rt.synthesize(IDS, DUR, noise, 0.667), before, "a voice without a table, after the new calls")
        assert rt.steps(0) == steps and "spk.rows" not in steps
        # … and its schedule is the conditioned voice's without the one new step, which comes first
        medium.rt.synthesize(IDS, DUR, noise, 0.667)
        csteps = medium.rt.steps(0)
        assert csteps[0] == "spk.rows" and csteps[1:] == steps
        rt.predict_durations([(IDS, None)])
        medium.rt.predict_durations([(IDS, None)])
        rt.prepare(0, IDS, None, None, 0.667, noise_mode="device")
        medium.rt.prepare(0, IDS, None, None, 0.667, noise_mode="device")
        psteps, cpsteps = rt.steps(0, predict=True), medium.rt.steps(0, predict=True)
        assert cpsteps[0] == "spk.rows" and cpsteps[1:] == psteps
    finally:
        rt.close()


def test_refusals_on_the_device_side(medium):
    rt = medium.rt
    assert rt.num_speakers() == S
    with pytest.raises(ph.InvalidArgument):  # twice
        rt.attach_speakers(medium.scfg, medium.sblob)
    rt.slot_speakers(8, [1])
    for bad in ([S], [-1], [{0: float("nan")}], [{0: float("inf")}], [[(0, 1.0)] * 5], [1, {2: 0.5, S: 0.5}]):
        with pytest.raises(ph.InvalidArgument):
            rt.slot_speakers(8, bad)
    empty = ph.Speaker()  # n = 0 in an entry
    assert rt.lib.piper_hip_voice_slot_speakers(rt.voice, 8, C.byref(empty), 1) == ph.InvalidArgument.code
    assert rt.lib.piper_hip_voice_slot_speakers(rt.voice, 16, C.byref(empty), 0) == ph.InvalidArgument.code
    assert rt.lib.piper_hip_voice_slot_speakers(rt.voice, 8, None, 257) == ph.InvalidArgument.code
    with pytest.raises(ph.InvalidArgument):
        rt.predict_durations([(IDS, None)], speakers=[S])
    # a refused assignment leaves the one in place
    rt.prepare_batch(8, [(IDS, DUR, None)])
    rt.launch(8)
    rt.collect(8)
    assert np.array_equal(rt.tap(8, "spk.g"), medium.emb[1])
    rt.slot_speakers(8, None)
