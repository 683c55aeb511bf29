"""GPU: batched streaming (piper_hip_voice_stream_*_batch) — a group of utterances on one slot, encoder + flow once, every active
item's next chunk in one generator launch. Each item must stream what it streams alone and what synthesize() gives."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import piper_hip as ph
from conftest import assert_close

pytestmark = pytest.mark.gpu

SD = kd.case_seed("mod", 0) + 5000
TOL = 2e-5  # the single-stream test's tolerance: fp32 summation order (tile splits depend on the window length)


def snr_db(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return 10.0 * np.log10((ref ** 2).sum() / max(((x - ref) ** 2).sum(), 1e-300))


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


def ragged_group(cfg):
    """Five items at factors 1, 2 and 8: F = 42, 30 (ragged durations), 84, 70, 336 — none a multiple of 32 or 64, two shorter than
    one chunk of 64 and one (F = 30) shorter than a chunk of 32."""
    ids1 = kd.FIXTURE_IDS
    items = [(ids1, [3] * 14), (ids1, [0, 5, 1, 2, 0, 4, 3, 1, 2, 6, 0, 1, 2, 3]), (ids1 * 2, [3] * 28), (ids1 * 2, [2, 3] * 14),
             (ids1 * 8, [3] * 112)]
    out = []
    for k, (ids, dur) in enumerate(items):
        out.append((ids, dur, kd.sym(SD + k, (cfg.inter, sum(dur)), 1.7320508)))
    return out


def run_group(rt, group, chunk, slot):
    """All steps of a batched stream → per-item chunk lists and the step count."""
    per = [[] for _ in group]
    steps = 0
    for chunks in rt.synthesize_stream_batch(group, 0.667, chunkFrames=chunk, slot=slot):
        assert len(chunks) == len(group)
        for i, c in enumerate(chunks):
            if c.size:
                per[i].append(c)
        steps += 1
    return per, steps


@pytest.mark.parametrize("chunk", [32, 64])
def test_ragged_group_matches_whole_utterances(rt_medium, chunk):
    rt, cfg = rt_medium, rt_medium.cfg
    group = ragged_group(cfg)
    per, steps = run_group(rt, group, chunk, slot=2)
    Fs = [sum(d) for _, d, _ in group]
    assert steps == max(-(-F // chunk) for F in Fs)
    for i, (ids, dur, noise) in enumerate(group):
        assert len(per[i]) == -(-Fs[i] // chunk)
        assert all(c.size == chunk * cfg.hop for c in per[i][:-1])
        got = np.concatenate(per[i])
        whole = rt.synthesize(ids, dur, noise, 0.667)
        assert got.size == whole.size == Fs[i] * cfg.hop
        assert_close(got, whole, TOL, f"item {i} (F = {Fs[i]}, chunk {chunk}) vs whole utterance")
    # the same item through the single-slot stream
    ids, dur, noise = group[0]
    single = np.concatenate(list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3)))
    assert_close(np.concatenate(per[0]), single, TOL, "item 0 vs stream_begin / stream_next")


def test_predicted_durations_item(rt_medium, voices):
    rt, cfg = rt_medium, rt_medium.cfg
    ids = kd.FIXTURE_IDS * 2
    dev = {"noise_mode": "device", "seed": 4242}
    group = [(kd.FIXTURE_IDS, [3] * 14, kd.sym(SD + 20, (cfg.inter, 42), 1.7320508)), (ids, None, None, dev)]
    per, _ = run_group(rt, group, 64, slot=4)
    dur_group = rt.durations(4)
    whole = rt.synthesize(ids, None, None, 0.667, noise_mode="device", seed=4242)
    dur_single = rt.durations(0)
    assert np.array_equal(dur_group[14:], dur_single)
    got = np.concatenate(per[1])
    assert got.size == whole.size == int(dur_single.sum()) * cfg.hop
    assert_close(got, whole, TOL, "predicted-duration item vs whole utterance")


def test_high_voice_fp32_and_bf16(backend, voices):
    cfg, blob = voices["high"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        group = []
        for k, f in enumerate((1, 2, 4)):
            dur = [3] * (14 * f)
            group.append((kd.FIXTURE_IDS * f, dur, kd.sym(SD + 40 + k, (cfg.inter, sum(dur)), 1.7320508)))
        wholes = [rt.synthesize(ids, dur, nz, 0.667) for ids, dur, nz in group]
        per, _ = run_group(rt, group, 32, slot=1)
        for i in range(3):
            assert_close(np.concatenate(per[i]), wholes[i], TOL, f"high fp32 item {i}")
        rt.set_precision("bf16")
        per_b, _ = run_group(rt, group, 32, slot=1)
        for i in range(3):
            got = np.concatenate(per_b[i])
            assert got.size == wholes[i].size
            assert snr_db(got, wholes[i]) >= 40.0, (i, snr_db(got, wholes[i]))
    finally:
        rt.close()


def test_repeat_same_slot_and_plan_count(rt_medium):
    rt, cfg = rt_medium, rt_medium.cfg
    group = ragged_group(cfg)
    first, _ = run_group(rt, group, 64, slot=6)
    plans = rt.plan_info(6)["cached_plans"]
    again, _ = run_group(rt, group, 64, slot=6)
    for a, b in zip(first, again):
        assert np.array_equal(np.concatenate(a), np.concatenate(b))
    assert rt.plan_info(6)["cached_plans"] == plans
    # n = 6 rounds to the same generator batch (8) as n = 5 and has the same windows: only its own encoder + flow plan is new
    bigger = group + [group[2]]
    more, _ = run_group(rt, bigger, 64, slot=6)
    assert rt.plan_info(6)["cached_plans"] <= plans + 1
    for i in range(len(group)):
        assert_close(np.concatenate(more[i]), np.concatenate(first[i]), TOL, f"item {i} in a group of 6")


def test_drop(rt_medium):
    """Item 3 (F = 70: three chunks of 32) is dropped after step 1: it reports 0 samples from then on, the others are unchanged."""
    rt, cfg = rt_medium, rt_medium.cfg
    group = ragged_group(cfg)
    ref, _ = run_group(rt, group, 32, slot=7)
    assert len(ref[3]) == 3
    per = [[] for _ in group]
    for step, chunks in enumerate(rt.synthesize_stream_batch(group, 0.667, chunkFrames=32, slot=7)):
        if step >= 2:
            assert chunks[3].size == 0
        for i, c in enumerate(chunks):
            if c.size:
                per[i].append(c)
        if step == 1:
            rt.stream_drop(7, 3)
    assert len(per[3]) == 2
    assert np.array_equal(np.concatenate(per[3]), np.concatenate(ref[3][:2]))
    for i in (0, 1, 2, 4):
        assert_close(np.concatenate(per[i]), np.concatenate(ref[i]), TOL, f"item {i} with item 3 dropped")


def test_limits_and_errors(rt_medium):
    rt, cfg = rt_medium, rt_medium.cfg
    # n = 256 at factor 1 (device noise, one seed per item)
    group = [(kd.FIXTURE_IDS, [3] * 14, None, {"noise_mode": "device", "seed": 100 + i}) for i in range(256)]
    per, steps = run_group(rt, group, 64, slot=8)
    assert steps == 1
    assert all(len(p) == 1 and p[0].size == 42 * cfg.hop for p in per)
    for i in (0, 255):
        whole = rt.synthesize(kd.FIXTURE_IDS, [3] * 14, None, 0.667, noise_mode="device", seed=100 + i)
        assert_close(per[i][0], whole, TOL, f"item {i} of 256")
    with pytest.raises(ph.ShapeMismatch):
        list(rt.synthesize_stream_batch(group + group[:1], 0.667, chunkFrames=64, slot=8))
    small = ragged_group(cfg)[:3]
    with pytest.raises(ph.ExecutionError):
        list(rt.synthesize_stream_batch(small, 0.667, chunkFrames=0, slot=8))
    lib, v = rt.lib, rt.voice
    it = rt.synthesize_stream_batch(small, 0.667, chunkFrames=16, slot=9)
    next(it)  # the group is running on slot 9
    got = (C.c_int64 * 3)()
    buf = np.empty(16, np.float32)
    rc = lib.piper_hip_voice_stream_next_batch(v, 9, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, got)
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rc)
    one = C.c_int64()
    assert lib.piper_hip_voice_stream_next(v, 9, None, 0, C.byref(one)) != 0  # a group slot refuses the single-stream call
    with pytest.raises(ph.ExecutionError):
        rt.stream_drop(9, 3)
    with pytest.raises(ph.ExecutionError):
        rt.stream_drop(9, -1)
    assert lib.piper_hip_voice_stream_next_batch(v, 12, None, 0, got) != 0  # slot 12 holds no stream
    rest = list(it)  # the refused calls left the group intact
    assert len(rest) == -(-84 // 16) - 1


def test_repeated_streams_keep_buffers_and_bits(backend, voices):
    """Who owns a stream's device buffers, across repeated streams on one slot id: three factor-1 items at chunk 8 as a group in fp32, at
    8000 Hz int16 and mixed (s16 at 8000, mu-law, f32), then through a mixed pool of 4 on another slot id that is closed again. Three
    such cycles: the third delivers the first's chunks bit for bit, and neither the context pool's live bytes nor the plan cache grow
    from the second to the third (a plan keeps its stream buffers across streams; a pool's go back when it closes)."""
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        group = [(kd.FIXTURE_IDS, [3] * 14, kd.sym(SD + 60 + k, (cfg.inter, 42), 1.7320508)) for k in range(3)]
        fmts = [ph.stream_format(rate=8000, encoding="s16"), ph.stream_format(encoding="mulaw"), ph.stream_format(encoding="f32")]

        def cycle():
            out = []
            for kw in ({}, {"rate": 8000}, {"formats": fmts}):
                for chunks in rt.synthesize_stream_batch(group, 0.667, chunkFrames=8, slot=2, **kw):
                    out.extend(chunks)
            pool = rt.stream_pool(4, 4, chunkFrames=8, work_slot=5, mixed=True)
            assert [r for r, _ in pool.join(group, formats=fmts)] == [0, 1, 2]
            while True:
                chunks = pool.step_mixed()
                if not any(c.size for c in chunks):
                    break
                out.extend(chunks)
            pool.close()
            return out, (backend.memory_stats()["live"], rt.plan_info(2)["cached_plans"])

        first, _ = cycle()
        _, second = cycle()
        third, after = cycle()
        assert sum(c.size for c in first if c.dtype == np.float32) == (3 + 1 + 1) * 42 * cfg.hop  # fp32 group, the two f32 rows
        assert {c.dtype for c in first if c.size} == {np.dtype(t) for t in (np.float32, np.int16, np.uint8)}
        assert len(third) == len(first)
        for i, (a, b) in enumerate(zip(first, third)):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"chunk {i} of cycle 3 differs from cycle 1"
        print(f"after cycle 2: live bytes, cached plans = {second}; after cycle 3: {after}")
        assert after == second
    finally:
        rt.close()
