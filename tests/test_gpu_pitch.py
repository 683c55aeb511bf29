"""GPU: the pitch (include/piper_hip.h "Pitch") as a per-op and on every whole-item voice route. The per-op is compared with
tests/pitch_ref.py bit for bit. On the voice routes the raw reference is the GPU's own audio: pitch_ref.item applied to the plan's raw
`audio` tap (or to the collect that lacks only the pitch) must equal what the device delivers, zero tail included, and every later
stage's existing host twin or numpy reference, applied to the pitch-only float collect, must equal the pitched route.

The voice is the scaled-output-conv medium voice of tests/test_gpu_level.py at factor 1, in batches of 3."""
import ctypes as C

import numpy as np
import pytest

import join_ref as jr
import katdata as kd
import level_ref as lr
import loudness_ref as ld
import mixed_ref as mr
import pitch_ref as pr
import piper_hip as ph
from test_gpu_level import DEV, SINKS, collect_as, item, level_for, rt_medium, same  # noqa: F401  (rt_medium: a fixture)
from test_gpu_resample import same_bits
from test_gpu_stream_mixed import TABLES

pytestmark = pytest.mark.gpu

F32 = np.float32
SHIFTS3 = [(3.0, 0), (0.0, 0), (-5.0, 0)]  # varispeed: supplied durations
EQ = [(ph.EQ_HIGHPASS, 120.0, 0.707), (ph.EQ_PEAKING, 3000.0, 1.0, 6.0)]
SLOT, FIX = 5, 7  # FIX: the slot of the module's pitched batch, prepared and launched once


def signal(n, seed):
    x = pr.noise(n, seed)
    if n >= 23:
        x[[1, 7, n - 2, 11, 12]] = [np.nan, np.inf, -np.inf, 1e-42, -0.0]
    return x


def pitched_items(items, shifts, hop):
    return [pr.item(x, st, hop)[0] for x, (st, _keep) in zip(items, shifts)]


def split(x, per):
    return np.split(x, np.cumsum(per)[:-1])


def clear(rt, *slots):
    for s in slots:
        rt.slot_eq(s, None)
        rt.slot_level(s, None)
        rt.slot_loudness(s, None)
        rt.slot_join(s, None)


def batch(cfg):
    return [item(cfg, n, k) for k, n in enumerate((40, 14, 23))]


# ---- per-op

def test_per_op_is_the_reference_on_the_grid(backend):
    for n in pr.SIZES:
        x = signal(n, n + 1)
        buf = backend.uploadFloat32(x if n else np.zeros(1, F32))
        for st in pr.SHIFTS:
            out = backend.pitch_f32(buf, st, count=n)
            want = pr.apply(x, st)
            assert out.count == want.size == ph.pitch_count(st, n), (n, st)
            got = backend.downloadFloat32(out, out.count) if out.count else np.empty(0, F32)
            assert same_bits(got, want), (n, st)
            out.free()
        buf.free()


@pytest.mark.parametrize("st", [-12.0, 0.01, 7.0, 12.0])
def test_per_op_unaligned_source_and_destination(backend, st):
    """Every phase of the source and of the destination against 16 bytes, over more tiles than one block takes in one pass"""
    n = 9001
    x = signal(n, 77)
    want = pr.apply(x, st)
    for a in range(4):  # the source a floats, the destination 1 + a floats off a 16-byte boundary
        src = backend.uploadFloat32(np.concatenate([np.zeros(a, F32), x]))
        dst = backend.uploadFloat32(np.full(want.size + 8, 7.0, F32))
        xin = ph.DeviceBuffer(backend, src.ptr + 4 * a, n, owned=False)
        yout = ph.DeviceBuffer(backend, dst.ptr + 4 * (1 + a), want.size, owned=False)
        backend.pitch_f32(xin, st, out=yout)
        full = backend.downloadFloat32(dst, want.size + 8)
        assert same_bits(full[1 + a:1 + a + want.size], want), (st, a)
        assert (full[:1 + a] == 7.0).all() and (full[1 + a + want.size:] == 7.0).all(), (st, a)  # nothing outside the row is written
        src.free()
        dst.free()


def test_per_op_refusals(backend):
    buf = backend.uploadFloat32(np.zeros(8, F32))
    for st in (12.5, float("nan")):
        with pytest.raises(ph.InvalidArgument):
            backend.pitch_f32(buf, st)
    assert b"semitones" in backend.lib.piper_hip_last_error()


# ---- whole items: varispeed on a batch of 3 with supplied durations

@pytest.fixture(scope="module")
def fix(rt_medium):
    """The module's pitched batch on slot FIX, launched once: raw = the plan's audio tap per item, y = the pitch-only float collect per
    item, want = the reference applied to raw."""
    rt, hop = rt_medium, rt_medium.cfg.hop
    clear(rt, FIX)
    rt.prepare_batch(FIX, batch(rt.cfg), 0.667, pitch=SHIFTS3)
    rt.launch(FIX)
    got = rt.collect(FIX).copy()
    per, total = rt.pitch_samples(FIX)
    raw_per, _ = rt.prepared_samples(FIX)
    raw = split(rt.tap(FIX, "audio").reshape(-1), raw_per)
    return dict(got=got, per=per, total=total, raw=raw, raw_per=raw_per, y=split(got, per), want=pitched_items(raw, SHIFTS3, hop))


def test_collect_is_the_reference_on_the_raw_audio(rt_medium, fix):
    rt, hop = rt_medium, rt_medium.cfg.hop
    assert fix["raw_per"] == [40 * 3 * hop, 14 * 3 * hop, 23 * 3 * hop]  # prepared_samples stays raw
    assert fix["per"] == [w.size for w in fix["want"]] and fix["total"] == fix["got"].size == sum(fix["per"])
    for b, (st, _k) in enumerate(SHIFTS3):
        n = pr.count(fix["raw"][b].size, pr.step(st))
        assert fix["per"][b] == -(-n // hop) * hop
        assert same_bits(fix["y"][b], fix["want"][b]), b
        assert not fix["y"][b][n:].any() and not np.signbit(fix["y"][b][n:]).any()  # the zero tail
    assert fix["per"][0] < fix["raw_per"][0] and fix["per"][1] == fix["raw_per"][1] and fix["per"][2] > fix["raw_per"][2]
    # the item with pitch 0 is the un-pitched collect, bit for bit; and so is the whole batch without a pitch
    rt.prepare_batch(SLOT, batch(rt.cfg), 0.667)
    rt.launch(SLOT)
    plain = split(rt.collect(SLOT), fix["raw_per"])
    assert same_bits(fix["y"][1], plain[1])
    for b in range(3):
        assert same_bits(fix["raw"][b], plain[b]), b
    # a second collect, and the audio tap, after the pitched one
    assert same_bits(rt.collect(FIX), fix["got"])
    assert same_bits(rt.tap(FIX, "audio").reshape(-1), np.concatenate(fix["raw"]))
    short = np.empty(fix["total"] - 1, F32)
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rt.lib.piper_hip_voice_collect(rt.voice, FIX, short.ctypes.data_as(ph.c_f32p), short.size))


def test_volume_then_pitch(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    clear(rt, SLOT)
    items = batch(rt.cfg)
    vols = [np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], F32), len(it[0])) for it in items]
    rt.prepare_batch(SLOT, items, 0.667, volume=vols)
    rt.launch(SLOT)
    raw_per, _ = rt.prepared_samples(SLOT)
    shaped = split(rt.collect(SLOT).copy(), raw_per)
    rt.prepare_batch(SLOT, items, 0.667, volume=vols, pitch=SHIFTS3)
    rt.launch(SLOT)
    got = rt.collect(SLOT)
    want = pitched_items(shaped, SHIFTS3, hop)
    assert same_bits(got, np.concatenate(want))
    assert not same_bits(got[:want[0].size], pitched_items(split(rt.tap(SLOT, "audio").reshape(-1), raw_per), SHIFTS3, hop)[0])  # (the volume shows)


def test_eq_reads_the_pitched_items(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    want = np.concatenate([ph.eq_from_f32(y, EQ, rate) for y in fix["y"]])
    assert same_bits(rt.collect(FIX, eq=EQ), want)
    assert same_bits(rt.collect(FIX, eq=None), fix["got"])


def test_loudness_measures_and_gains_the_pitched_items(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    rt.slot_loudness(FIX, (-16.0, 0.0))
    lufs, g = rt.loudness(FIX)
    for b, y in enumerate(fix["y"]):
        L = ld.lufs(y, rate)
        print(f"item {b}: L device {float(lufs[b]):.4f}, loudness_ref {L:.4f}")
        assert abs(float(lufs[b]) - L) <= 0.002, (b, lufs[b], L)
    want = np.concatenate([ld.apply(y, gk) for y, gk in zip(fix["y"], g)])
    assert same_bits(rt.collect(FIX), want)
    assert same_bits(rt.collect(FIX, loudness=None), fix["got"])


def test_level_limits_the_pitched_items(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    level = (3.0 / max(float(np.abs(y).max()) for y in fix["y"]), 0.5, 50.0)
    want = np.concatenate([lr.apply(y, level, rate) for y in fix["y"]])
    assert same_bits(rt.collect(FIX, level=level), want)
    assert same_bits(rt.collect(FIX, level=None), fix["got"])


def test_join_takes_the_pitched_items(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    J = dict(lead_ms=1.5, gap_ms=20.0, tail_ms=3.0, trim=1, trim_threshold=float(np.abs(fix["got"]).max()) * 0.05, trim_pad_ms=2.0, fade_ms=3.0)
    y, start, length, total = ph.join_from_f32(fix["y"], J, rate)
    rt.slot_join(FIX, J)
    assert rt.join_capacity(FIX) == ph.join_capacity(J, rate, fix["per"])
    got = rt.collect(FIX)
    assert same_bits(got, y[:total])
    s, l, t = rt.join_report(FIX)
    assert t == total and list(s) == list(start) and list(l) == list(length)
    assert same(rt.collect_pcm16(FIX, rate=8000), mr.whole(y[:total], SINKS["s16@8000"], rate, TABLES))
    assert same_bits(rt.collect(FIX, join=None), fix["got"])


def test_every_stage_together(rt_medium):
    """Volume, pitch, EQ, loudness, level and join on one launch: every sink, in two orders, equals the existing references chained on the
    float collect that has only the volume and the pitch."""
    rt, rate, hop = rt_medium, rt_medium.cfg.sample_rate, rt_medium.cfg.hop
    clear(rt, SLOT)
    items = batch(rt.cfg)
    vols = [np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], F32), len(it[0])) for it in items]
    rt.prepare_batch(SLOT, items, 0.667, volume=vols, pitch=SHIFTS3)
    rt.launch(SLOT)
    got = rt.collect(SLOT).copy()  # volume and pitch only
    per, total = rt.pitch_samples(SLOT)
    raw_per, _ = rt.prepared_samples(SLOT)
    assert got.size == total and per != raw_per  # (the pitch shows)
    assert not same_bits(got, np.concatenate(pitched_items(split(rt.tap(SLOT, "audio").reshape(-1), raw_per), SHIFTS3, hop)))  # (the volume shows)
    y = split(got, per)
    e = [ph.eq_from_f32(x, EQ, rate) for x in y]
    rt.slot_eq(SLOT, EQ)
    rt.slot_loudness(SLOT, (-16.0, 0.0))
    lufs, g = rt.loudness(SLOT)
    for b, x in enumerate(e):
        L = ld.lufs(x, rate)
        print(f"item {b}: L device {float(lufs[b]):.4f}, loudness_ref {L:.4f}, gain {float(g[b]):.4f}")
        assert abs(float(lufs[b]) - L) <= 0.002, (b, lufs[b], L)
    u = [ld.apply(x, gk) for x, gk in zip(e, g)]
    level = level_for(u)  # (asserts that the limiter works on some blocks and rests on others)
    lim = [lr.apply(x, level, rate) for x in u]
    J = dict(lead_ms=1.5, gap_ms=20.0, tail_ms=3.0, trim=1, trim_threshold=max(float(np.abs(x).max()) for x in lim) * 0.05, trim_pad_ms=2.0,
             fade_ms=3.0)
    prog, start, length, jtotal = jr.join(lim, J, rate)
    print(f"items {per}, kept {list(length)}, programme {jtotal}")
    for b in range(3):  # every stage changes the signal: one that was skipped would be seen
        assert not same_bits(e[b], y[b]) and not same_bits(u[b], e[b]) and not same_bits(lim[b], u[b]), b
    assert sum(int(n) for n in length) < total  # (the trim removes something)
    want = {name: mr.whole(prog[:jtotal], f, rate, TABLES) for name, f in SINKS.items()}
    rt.slot_level(SLOT, level)
    rt.slot_join(SLOT, J)
    for name in list(SINKS) + list(SINKS)[::-1]:
        assert same(collect_as(rt, SLOT, name), want[name]), name
        s, l, t = rt.join_report(SLOT)
        assert t == jtotal and list(s) == list(start) and list(l) == list(length), name
    clear(rt, SLOT)
    assert same_bits(rt.collect(SLOT), got)


def test_collect_pcm16(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    assert same(rt.collect_pcm16(FIX), np.concatenate([mr.whole(y, SINKS["s16"], rate, TABLES) for y in fix["y"]]))
    got = rt.collect_pcm16(FIX, gain=0.5, normalize=True)  # the peaks are those of the pitched items
    peaks = rt.peaks(FIX)
    for b, y in enumerate(fix["y"]):
        assert peaks[b] == np.abs(y).max(), b
    assert got.size == fix["total"]


def test_collect_pcm16_rate(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    assert same(rt.collect_pcm16(FIX, rate=8000), np.concatenate([mr.whole(y, SINKS["s16@8000"], rate, TABLES) for y in fix["y"]]))


def test_collect_g711(rt_medium, fix):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    assert same(collect_as(rt, FIX, "mulaw@8000"), np.concatenate([mr.whole(y, SINKS["mulaw@8000"], rate, TABLES) for y in fix["y"]]))
    alaw = mr.Format(0, "alaw", 1.0)
    assert same(rt.collect_g711(FIX, "alaw"), np.concatenate([mr.whole(y, alaw, rate, TABLES) for y in fix["y"]]))


def test_synthesize_twins(rt_medium):
    rt, rate, hop = rt_medium, rt_medium.cfg.sample_rate, rt_medium.cfg.hop
    clear(rt, 0)
    ids, dur, noise = item(rt.cfg, 14, 1)
    raw = rt.synthesize(ids, dur, noise, 0.667).copy()
    want = pr.item(raw, 7.0, hop)[0]
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, pitch=(7.0, 0)), want)
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, pitch=(7.0, 0)), mr.whole(want, SINKS["s16"], rate, TABLES))
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000, pitch=(7.0, 0)), mr.whole(want, SINKS["s16@8000"], rate, TABLES))
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000, pitch=(7.0, 0)), mr.whole(want, SINKS["mulaw@8000"], rate, TABLES))
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667), raw)  # the pitch was that call's alone


# ---- tempo

def test_keep_tempo_scales_the_predicted_durations(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    clear(rt, SLOT)
    id_lists = [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS, kd.FIXTURE_IDS * 3]
    ls = [1.0, 0.0, 1.25]  # (0 is taken as 1.0)
    shifts = [(3.0, 1), (-5.0, 1), (0.0, 1)]
    with_pitch = [(ids, None, None, dict(DEV, length_scale=l)) for ids, l in zip(id_lists, ls)]
    scaled = [(ids, None, None, dict(DEV, length_scale=float(pr.length_scale(l, st)))) for ids, l, (st, _k) in zip(id_lists, ls, shifts)]
    rt.prepare_batch(SLOT, scaled, 0.667)
    rt.launch(SLOT)
    dur = rt.durations(SLOT).copy()
    raw_per, _ = rt.prepared_samples(SLOT)
    raw = split(rt.collect(SLOT).copy(), raw_per)
    plain = [(ids, None, None, dict(DEV, length_scale=l)) for ids, l in zip(id_lists, ls)]
    rt.prepare_batch(SLOT, plain, 0.667)
    dur_plain = rt.durations(SLOT).copy()
    assert not np.array_equal(dur, dur_plain)  # the factor shows in the durations
    rt.prepare_batch(SLOT, with_pitch, 0.667, pitch=shifts)
    assert np.array_equal(rt.durations(SLOT), dur)
    assert rt.prepared_samples(SLOT)[0] == raw_per
    rt.launch(SLOT)
    got = rt.collect(SLOT)
    want = pitched_items(raw, shifts, hop)
    assert same_bits(got, np.concatenate(want))
    # the item keeps its length: each id's ceil moves its frames by less than max(1, ρ), so F' by less than max(1, 1/ρ) per id, plus the tail
    for b in (0, 1):
        n_plain = int(dur_plain[sum(len(i) for i in id_lists[:b]):sum(len(i) for i in id_lists[:b + 1])].sum()) * hop
        rq = pr.step(shifts[b][0]) / 2.0 ** 32
        assert abs(want[b].size - n_plain) <= (max(1.0, 1.0 / rq) * len(id_lists[b]) + 1) * hop, (b, want[b].size, n_plain)
    # supplied durations: the caller owns them
    rt.slot_pitch(SLOT, [(3.0, 1)])
    with pytest.raises(ph.InvalidArgument):
        rt.prepare(SLOT, *item(rt.cfg, 14, 1), 0.667)
    assert b"keep_tempo" in rt.lib.piper_hip_last_error()
    rt.prepare(SLOT, *item(rt.cfg, 14, 1), 0.667)  # the refused call took the pitch with it
    assert rt.pitch_samples(SLOT) == rt.prepared_samples(SLOT)


# ---- bounded

def test_bounded_equals_prepare_batch(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT, 6)
    id_lists = [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS, kd.FIXTURE_IDS * 3]
    shifts = [(-7.0, 1), (4.0, 0), (0.0, 0)]
    rt.prepare_batch(SLOT, [(ids, None, None, dict(DEV)) for ids in id_lists], 0.667, pitch=shifts)
    rt.launch(SLOT)
    # exactly enough frames: the bounded plan is the bucket prepare_batch chose, so both run the same kernels (another bucket may pick
    # other tile shapes, and the waveform then agrees only up to summation order, with or without a pitch)
    bound = max(n // hop for n in rt.prepared_samples(SLOT)[0])
    want = rt.collect(SLOT).copy()
    want_per, want_total = rt.pitch_samples(SLOT)
    want_s16 = rt.collect_pcm16(SLOT, rate=8000).copy()
    rt.prepare_batch_bounded(6, [(ids, None) for ids in id_lists], bound, 0.667, **DEV, pitch=shifts)
    cap_raw, _ = rt.prepared_samples(6)
    cap, cap_total = rt.pitch_samples(6)
    assert cap == [pr.frames(n, pr.step(st), hop) * hop for n, (st, _k) in zip(cap_raw, shifts)] and cap_total == sum(cap)  # the capacity
    rt.launch(6)
    short = np.empty(cap_total - 1, F32)
    assert rt.lib.piper_hip_voice_collect(rt.voice, 6, short.ctypes.data_as(ph.c_f32p), short.size) == ph.ShapeMismatch.code
    assert same(rt.collect_pcm16(6, rate=8000), want_s16)  # (the collecting call of the bounded slot)
    assert rt.pitch_samples(6) == (want_per, want_total)
    assert same_bits(rt.collect(6), want)
    assert np.array_equal(rt.durations(6), rt.durations(SLOT))
    rt.prepare_batch_bounded(6, [(ids, None) for ids in id_lists], bound, 0.667, **DEV, pitch=shifts)
    rt.launch(6)
    assert same_bits(rt.collect(6), want)  # the float collect as the collecting call


# ---- no pitch

def test_neutral_pitch_is_no_pitch(rt_medium, backend):
    rt = rt_medium
    clear(rt, SLOT)
    items = batch(rt.cfg)
    backend.arm_routes(True)
    try:
        rt.prepare_batch(SLOT, items, 0.667)
        rt.launch(SLOT)
        plain = {name: collect_as(rt, SLOT, name).copy() for name in SINKS}
        routes, steps = backend.last_routes(), rt.steps(SLOT)
        info = rt.plan_info(SLOT)
        for neutral in ([(0.0, 0)] * 3, [(1e-9, 0), (-0.0, 0)], (0.0, 0)):
            rt.prepare_batch(SLOT, items, 0.667, pitch=neutral)
            rt.launch(SLOT)
            for name in SINKS:
                assert same(collect_as(rt, SLOT, name), plain[name]), (neutral, name)
            assert backend.last_routes() == routes and rt.steps(SLOT) == steps
            assert rt.pitch_samples(SLOT) == rt.prepared_samples(SLOT)
            assert rt.plan_info(SLOT)["cached_bytes"] == info["cached_bytes"]  # the plan carries nothing new
    finally:
        backend.arm_routes(False)


# ---- streams and the lifecycle

def test_streams_refuse_and_leave_the_slot_usable(rt_medium):
    rt = rt_medium
    ids, dur, noise = item(rt.cfg, 14, 1)
    u, _k = rt._utt(ids, dur, noise, 0.667)
    lib, code = rt.lib, ph.UnsupportedOp.code
    rt.slot_pitch(3, [3.0])
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 4) == code
    assert b"pitch" in lib.piper_hip_last_error()
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 4) >= 0  # the refusal cleared the pitch
    chunks = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3))
    rt.prepare(3, ids, dur, noise, 0.667)
    rt.launch(3)
    whole = rt.collect(3)
    assert same_bits(np.concatenate(chunks), whole)
    arr = (ph.Utterance * 2)(u, u)
    rt.slot_pitch(3, [(3.0, 0), (-2.0, 0)])
    assert lib.piper_hip_voice_stream_begin_batch(rt.voice, arr, 2, 3, 4) == code
    assert lib.piper_hip_voice_stream_begin_batch(rt.voice, arr, 2, 3, 4) >= 0
    pool = rt.stream_pool(4, 2, chunkFrames=8, work_slot=6)
    rt.slot_pitch(6, [3.0])
    with pytest.raises(ph.UnsupportedOp):
        pool.join([(ids, dur, noise)])
    assert pool.free_rows == 2
    (row, samples), = pool.join([(ids, dur, noise)])
    assert samples == whole.size
    pool.close()


def test_lifecycle_and_refusals(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    lib = rt.lib
    for bad, field in (([(12.5, 0)], b"semitones"), ([(0.0, 0), (float("nan"), 0)], b"entry 1"), ([(3.0, 2)], b"keep_tempo")):
        with pytest.raises(ph.InvalidArgument):
            rt.slot_pitch(SLOT, bad)
        assert field in lib.piper_hip_last_error(), (bad, lib.piper_hip_last_error())
    it = ph.Pitch(3.0, 0)
    assert lib.piper_hip_voice_slot_pitch(rt.voice, -1, C.byref(it), 1) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_pitch(rt.voice, SLOT, C.byref(it), 257) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_pitch(rt.voice, SLOT, None, 1) == ph.InvalidArgument.code
    # a pitch is taken by the next staging call alone; entries past the batch are ignored, items past the entries have none
    ids, dur, noise = item(rt.cfg, 14, 1)
    rt.prepare(SLOT, ids, dur, noise, 0.667)
    rt.launch(SLOT)
    raw = rt.collect(SLOT).copy()
    rt.slot_pitch(SLOT, [(-12.0, 0), (5.0, 0)])
    rt.prepare(SLOT, ids, dur, noise, 0.667)
    rt.launch(SLOT)
    assert same_bits(rt.collect(SLOT), pr.item(raw, -12.0, hop)[0])
    rt.prepare(SLOT, ids, dur, noise, 0.667)
    rt.launch(SLOT)
    assert same_bits(rt.collect(SLOT), raw)
    rt.slot_pitch(SLOT, [(5.0, 0)])
    rt.slot_pitch(SLOT, None)  # cleared
    rt.prepare(SLOT, ids, dur, noise, 0.667)
    rt.launch(SLOT)
    assert same_bits(rt.collect(SLOT), raw)
    # a lower pitch on a plan whose later stages were sized for shorter rows
    rt.slot_eq(SLOT, EQ)
    eq_raw = rt.collect(SLOT).copy()
    assert same_bits(eq_raw, ph.eq_from_f32(raw, EQ, rt.cfg.sample_rate))
    rt.prepare(SLOT, ids, dur, noise, 0.667, pitch=(-12.0, 0))
    rt.launch(SLOT)
    assert same_bits(rt.collect(SLOT), ph.eq_from_f32(pr.item(raw, -12.0, hop)[0], EQ, rt.cfg.sample_rate))
    rt.slot_eq(SLOT, None)
