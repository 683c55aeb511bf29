"""GPU: the device buffers of a stream (voice.hip: Stream and its StreamRate, StreamLevel, StreamEq — descriptor, packed chunks, volume,
EQ, level, history and the mixed table), which stay with their owner from one stream to the next: a plan keeps them across the streams of
its slot id, a pool gives them back when it closes. Nothing here has a tolerance: every stream's chunks, concatenated per item, are held
with np.array_equal to the SAME stream on a fresh HipRuntime, whose plans own nothing yet — the same kernels read the same inputs.

One slot id runs the same utterances at 2, then 5, then 2 frames a chunk (2 frames of 256 samples: the 512-sample minimum of a stream
level), so the same front plan sees every buffer first allocated, then regrown, then reused while too large; each pass has a sink of its
own, so the history halves and the mixed table are first allocated on a plan that already holds the others. A pool does the same over
open … close, and an identical third cycle must leave the context's live bytes where they were: every buffer was given back."""
import numpy as np
import pytest

import katdata as kd
import piper_hip as ph

pytestmark = pytest.mark.gpu

IDS = list(kd.FIXTURE_IDS)
SLOT, WORK = 5, 6
CHUNKS = (2, 5, 2)
EQ = [(ph.EQ_HIGHPASS, 120.0, 0.707), (ph.EQ_PEAKING, 2500.0, 1.0, 6.0), (ph.EQ_HIGHSHELF, 6000.0, 0.707, -3.0)]
LEVEL = (2.0, 0.5, 50.0)
MIXED = [dict(rate=8000, encoding="mulaw"), dict(encoding="s16"), dict(rate=16000, encoding="alaw")]
# one sink per pass; a single stream has no mixed step: its third pass is the mixed group's first row
SINGLE_SINKS = (dict(), dict(rate=8000), dict(rate=8000, encoding="mulaw"))
GROUP_SINKS = (dict(), dict(rate=8000), dict(formats=MIXED))
DROP = (2, 3)  # item 2 leaves behind the third step


def utt(k, n, dur):
    return ((IDS * 2)[:n], [dur] * n, kd.sym(7300 + k, (ph.voice_config("medium").inter, dur * n), 1.7320508))


GROUP = [utt(0, 14, 3), utt(1, 10, 2), utt(2, 18, 2)]  # F = 42, 20, 36: a generator batch of 4 with one pad row
GAINS = np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], np.float32), 10)  # the volume of item 1


def single_stream(rt, chunk, sink):
    ids, dur, noise = GROUP[0]
    return [np.concatenate(list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=SLOT, eq=EQ, level=LEVEL, **sink)))]


def group_stream(rt, chunk, sink):
    per = [[] for _ in GROUP]
    for k, chunks in enumerate(rt.synthesize_stream_batch(GROUP, 0.667, chunkFrames=chunk, slot=SLOT, eq=EQ, level=LEVEL,
                                                           volume=[None, GAINS], **sink)):
        for i, c in enumerate(chunks):
            per[i].append(c)
        if k == DROP[1] - 1:
            rt.stream_drop(SLOT, DROP[0])
    return [np.concatenate(p) for p in per]


def pool_cycle(rt, chunk):
    """open … close of a mixed pool of 3 rows (a generator batch of 4) with a level and an EQ: two sessions join and run to their ends"""
    pool = rt.stream_pool(SLOT, 3, chunkFrames=chunk, work_slot=WORK, mixed=True, eq=EQ, level=LEVEL)
    try:
        rows = [r for r, _ in pool.join(GROUP[:2], 0.667, formats=MIXED[:2], volume=[None, GAINS])]
        per = {r: [] for r in rows}
        for _ in range(64):
            out = pool.step_mixed()
            if not any(c.size for c in out):
                break
            for r in rows:
                per[r].append(out[r])
    finally:
        pool.close()
    return [np.concatenate(per[r]) for r in rows]


def make(backend, voice):
    cfg, blob = voice
    return ph.HipRuntime(backend, cfg, blob)


def same(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == r.dtype and g.size > 0 and np.array_equal(g, r), (what, i)


def held_to_fresh(backend, voice, rt, run, passes):
    for k, args in enumerate(passes):
        got = run(rt, *args)
        fresh = make(backend, voice)
        try:
            ref = run(fresh, *args)
        finally:
            fresh.close()
        same(got, ref, (run.__name__, k) + tuple(args[:1]))


@pytest.mark.parametrize("run, sinks", [(single_stream, SINGLE_SINKS), (group_stream, GROUP_SINKS)], ids=["single", "group of 3"])
def test_one_plan_keeps_its_stream_buffers(backend, voices, run, sinks):
    rt = make(backend, voices["medium"])
    try:
        held_to_fresh(backend, voices["medium"], rt, run, list(zip(CHUNKS, sinks)))
    finally:
        rt.close()


def test_a_pool_gives_every_stream_buffer_back(backend, voices):
    """The live bytes are read around the THIRD cycle, identical to the second: by then the work slot's plan and the window plans of both
    chunk sizes exist, so a cycle that gives back all it took leaves the count where it was."""
    rt = make(backend, voices["medium"])
    try:
        held_to_fresh(backend, voices["medium"], rt, pool_cycle, [(2,), (5,)])
        before = backend.memory_stats()["live"]
        again = pool_cycle(rt, 5)
        after = backend.memory_stats()["live"]
        print("live bytes before / after the repeated cycle:", before, after)
        assert before == after, (before, after)
        fresh = make(backend, voices["medium"])
        try:
            same(again, pool_cycle(fresh, 5), "repeated cycle")
        finally:
            fresh.close()
    finally:
        rt.close()
