"""GPU: the staging of a request (voice.hip: a slot id's page-locked buffers, the pending prosody / volume / pitch of its next staging call,
the inputs of a predictor plan, the whole-plan request scalars). Nothing here has a tolerance: every result is held, with np.array_equal,
to the SAME request on a fresh HipRuntime, whose staging is fresh and which has nothing cached — the same kernels read the same inputs.

One slot id goes through every staging route with its buckets growing, then shrinking: every page-locked buffer is first allocated,
regrown with its contents dropped, and reused while too large. A refused staging call must leave none of the three controls behind."""
import numpy as np
import pytest

import katdata as kd
import piper_hip as ph

pytestmark = pytest.mark.gpu

IDS = list(kd.FIXTURE_IDS)
SLOT = 6
LENS = (14, 40, 23)  # T buckets 16 / 48 / 32
DEV = {"noise_mode": "device", "seed": 2718}
MIX = {1: 0.75, 3: 0.25}
PITCH = [(3.0, 1), (0.0, 0), (-5.0, 0)]


def ids_of(n):
    return (IDS * 3)[:n]


def dpn(k, n):
    return kd.sym(7100 + k, (2, n), 1.7320508)


def cycle(n):
    return np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], np.float32), n)


def make(backend, voice, speakers):
    cfg, blob = voice
    r = ph.HipRuntime(backend, cfg, blob)
    if speakers:
        scfg = ph.speaker_config(4, 16)
        r.attach_speakers(scfg, ph.synthetic_speaker_blob(cfg, scfg, 4321))
        r.slot_speakers(SLOT, [0, MIX])  # item 2 takes the last entry too
    return r


def collected(rt, pcm):
    rt.launch(SLOT)
    out = {"f32": rt.collect(SLOT).copy(), "durations": rt.durations(SLOT).copy(), "pitch_samples": rt.pitch_samples(SLOT)}
    if pcm:
        out["s16@8000"] = rt.collect_pcm16(SLOT, rate=8000).copy()
        out["prosody_report"] = rt.prosody_report(SLOT)
    return out


def step_single(rt, _sp):
    n = LENS[0]
    rt.prepare_batch(SLOT, [(ids_of(n), [3] * n, kd.sym(7001, (rt.cfg.inter, 3 * n), 1.7320508))], 0.667)
    return collected(rt, False)


def step_predict(rt, sp):
    got = rt.predict_durations([(ids_of(n), dpn(k, n)) for k, n in enumerate(LENS)], speakers=[0, MIX, MIX] if sp else None)
    return {"dur%d" % i: d for i, (d, _) in enumerate(got)} | {"logw%d" % i: w for i, (_, w) in enumerate(got)}


def step_ragged(rt, _sp):
    t0 = LENS[1]
    items = [(ids_of(t0), None, None, dict(dp_noise=dpn(1, t0), length_scale=1.1, **DEV)),
             (ids_of(LENS[0]), [3] * LENS[0], None, DEV), (ids_of(LENS[2]), [3] * LENS[2], None, dict(noise_mode="device", seed=99))]
    pro = [dict(length=np.resize(np.array([1.0, 1.5, 0.5, 2.0], np.float32), t0), min_frames=np.resize(np.array([0, 2, 0, 1], np.int32), t0),
                noise=np.resize(np.array([1.0, 0.0, 0.5], np.float32), t0))]
    rt.prepare_batch(SLOT, items, 0.667, prosody=pro, volume=[None, cycle(LENS[0])], pitch=PITCH)
    return collected(rt, True)


def step_bounded(rt, sp):
    """Item 0 (40 ids) at three times its predicted length against a bound just over the longest plain prediction: fit compresses it."""
    utts = [(ids_of(n), dpn(k, n)) for k, n in enumerate((LENS[1], LENS[0], LENS[2]))]
    pred = rt.predict_durations(utts, speakers=[0, MIX, MIX] if sp else None, **DEV)
    bound = max(max(int(d.sum()), 1) for d, _ in pred) + 8
    pro = [dict(length=np.full(LENS[1], 3.0, np.float32), fit=1)]
    rt.prepare_batch_bounded(SLOT, utts, bound, 0.667, prosody=pro, volume=[None, cycle(LENS[0])], pitch=PITCH, **DEV)
    out = collected(rt, True)
    wanted, fitted = out["prosody_report"]
    assert wanted[0] > bound and fitted == [1, 0, 0], (wanted, fitted, bound)
    return out


def step_stream(rt, _sp):
    a, b = LENS[0], LENS[2]
    utts = [(ids_of(a), [3] * a, kd.sym(7002, (rt.cfg.inter, 3 * a), 1.7320508)), (ids_of(b), [3] * b, None, DEV)]
    rows = [[], []]
    for chunks in rt.synthesize_stream_batch(utts, 0.667, chunkFrames=16, slot=SLOT, volume=[cycle(a), None]):
        for i, c in enumerate(chunks):
            rows[i].append(c)
    return {"row%d" % i: np.concatenate(r) for i, r in enumerate(rows)}


def same(got, ref, what):
    assert got.keys() == ref.keys(), what
    for k in got:
        if isinstance(got[k], np.ndarray):
            assert got[k].dtype == ref[k].dtype and got[k].size > 0 and np.array_equal(got[k], ref[k]), (what, k)
        else:  # (per item, total) of pitch_samples, (wanted, fitted) of prosody_report: every part element by element
            assert len(got[k]) == len(ref[k]) and all(np.array_equal(np.asarray(g), np.asarray(r)) for g, r in zip(got[k], ref[k])), (what, k)


ROUTE = [("single", step_single), ("predict", step_predict), ("ragged", step_ragged), ("bounded", step_bounded), ("stream", step_stream),
         ("single again", step_single)]


@pytest.mark.parametrize("speakers", [False, True], ids=["plain", "speaker-table"])
def test_one_slot_id_through_every_staging_route(backend, voices, speakers):
    route = ROUTE[1:4] if speakers else ROUTE
    rt = make(backend, voices["medium"], speakers)
    try:
        for name, step in route:
            got = step(rt, speakers)
            fresh = make(backend, voices["medium"], speakers)
            try:
                ref = step(fresh, speakers)
            finally:
                fresh.close()
            same(got, ref, name)
    finally:
        rt.close()


# ------------------------------------------------------------------------------------------------ refusals
T = LENS[0]
PITCH_PENDING = "%s: slot %d has a pitch pending (piper_hip_voice_slot_pitch), and streams have no pitch: it has been cleared"
PROSODY_T = "utterance 0: its prosody has %d entries, the utterance %d ids" % (T - 1, T)
WORK = SLOT + 1


def stage_controls(rt, slot, bad_prosody, pitch):
    t = T - 1 if bad_prosody else T
    rt.slot_prosody(slot, [dict(noise=np.zeros(t, np.float32))])
    rt.slot_volume(slot, [np.full(T, 0.25, np.float32)])
    if pitch:
        rt.slot_pitch(slot, [(3.0, 0)])


def refused_prepare(rt, stage):
    n = kd.sym(7003, (rt.cfg.inter, 3 * T), 1.7320508)
    if stage:
        stage_controls(rt, SLOT, True, True)
        with pytest.raises(ph.ShapeMismatch) as e:
            rt.prepare_batch(SLOT, [(ids_of(T), [3] * T, n)], 0.667)
        assert e.value.code == -1 and str(e.value) == PROSODY_T
    rt.prepare_batch(SLOT, [(ids_of(T), [3] * T, n)], 0.667)
    return collected(rt, False)


def refused_bounded(rt, stage):
    utts = [(ids_of(T), dpn(0, T))]
    if stage:
        stage_controls(rt, SLOT, True, True)
        with pytest.raises(ph.ShapeMismatch) as e:
            rt.prepare_batch_bounded(SLOT, utts, 256, 0.667, **DEV)
        assert e.value.code == -1 and str(e.value) == PROSODY_T
    rt.prepare_batch_bounded(SLOT, utts, 256, 0.667, **DEV)
    return collected(rt, False)


def refused_stream(rt, stage):
    utts = [(ids_of(T), [3] * T, kd.sym(7004, (rt.cfg.inter, 3 * T), 1.7320508))]
    if stage:
        stage_controls(rt, SLOT, False, True)
        with pytest.raises(ph.UnsupportedOp) as e:
            list(rt.synthesize_stream_batch(utts, 0.667, chunkFrames=16, slot=SLOT))
        assert e.value.code == -3 and str(e.value) == PITCH_PENDING % ("stream_begin_batch", SLOT)
    return {"row0": np.concatenate([c[0] for c in rt.synthesize_stream_batch(utts, 0.667, chunkFrames=16, slot=SLOT)])}


def refused_join(rt, stage):
    utts = [(ids_of(T), [3] * T, kd.sym(7005, (rt.cfg.inter, 3 * T), 1.7320508))]
    pool = rt.stream_pool(SLOT, 2, chunkFrames=16, work_slot=WORK)
    try:
        if stage:
            stage_controls(rt, WORK, False, True)
            with pytest.raises(ph.UnsupportedOp) as e:
                pool.join(utts, 0.667)
            assert e.value.code == -3 and str(e.value) == PITCH_PENDING % ("stream_pool_join", WORK)
        (row, samples), = pool.join(utts, 0.667)
        chunks = []
        for _ in range(64):
            out = pool.step()
            if not out:
                break
            chunks.append(out[row])
    finally:
        pool.close()
    got = np.concatenate(chunks)
    assert got.size == samples
    return {"row": got}


@pytest.mark.parametrize("call", [refused_prepare, refused_bounded, refused_stream, refused_join],
                         ids=["prepare_batch", "prepare_batch_bounded", "synthesize_stream_batch", "pool join"])
def test_a_refused_staging_call_clears_all_three_controls(backend, voices, call):
    rt = make(backend, voices["medium"], False)
    try:
        got = call(rt, True)
    finally:
        rt.close()
    never = make(backend, voices["medium"], False)  # no control was ever staged on this one
    try:
        ref = call(never, False)
    finally:
        never.close()
    same(got, ref, call.__name__)
