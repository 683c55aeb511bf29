"""GPU: bounded pool joins (include/piper_hip.h "Streaming pool: joins with predicted durations that never wait") — a session whose durations
are predicted joins a running pool without the host round trip: the frame count reaches the row on the device (stream_adopt_bounded_kernel)
and the host learns it at the next step. Each session must stream what its utterance gives alone, within fp32 summation order of
synthesize(); an item the predictor makes longer than the join's bound fails alone.

Every test first learns the item's true frame count F* with predict_durations and picks max_frames from it."""
import numpy as np
import pytest

import katdata as kd
import mixed_ref as mr
import piper_hip as ph
from conftest import assert_close
from mixed_ref import Format
from test_gpu_stream_mixed import TABLES, lib_format
from test_gpu_stream_pool import NAMES, Sessions, TOL, check_session, frames, ragged_group

pytestmark = pytest.mark.gpu

DEV = {"noise_mode": "device", "seed": 4242}
IDS = list(kd.FIXTURE_IDS)
P_IDS = IDS * 2
CHUNK = 32


def predicted_frames(rt, id_lists, speakers=None):
    """F* per utterance from ONE predict_durations call over the list: the predictor plan (phoneme bucket, batch) a join of the same list uses"""
    outs = rt.predict_durations([(ids, None) for ids in id_lists], noise_mode="device", seed=4242, speakers=speakers)
    return [max(int(np.sum(dur)), 1) for dur, _logw in outs]


def whole_of(rt, ids, **kw):
    """(the whole-utterance waveform, its durations), read-only"""
    audio = rt.synthesize(ids, None, None, 0.667, noise_mode="device", seed=4242, **kw)
    dur = rt.durations(0).copy()
    audio.setflags(write=False)
    dur.setflags(write=False)
    return audio, dur


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


@pytest.fixture(scope="module")
def utts(rt_medium):
    group = ragged_group(rt_medium.cfg)
    return {name: group[k] for name, k in NAMES.items()}


@pytest.fixture(scope="module")
def wholes(rt_medium, utts):
    out = {}
    for name in "AB":
        ids, dur, noise = utts[name]
        out[name] = rt_medium.synthesize(ids, dur, noise, 0.667)
        out[name].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def pred(rt_medium):
    """The predicted-duration utterance P of test_gpu_stream_pool: its F*, waveform and durations, computed once"""
    (F,) = predicted_frames(rt_medium, [P_IDS])
    audio, dur = whole_of(rt_medium, P_IDS)
    assert audio.size == F * rt_medium.cfg.hop and int(dur.sum()) == F
    return {"utt": (P_IDS, None, None, DEV), "F": F, "audio": audio, "dur": dur}


def join_bounded(s, names, utterances, max_frames, expect, formats=None):
    """pool.join_bounded with the bookkeeping of Sessions.join. expect: {name: F*} of the items that fit — the others are never entered
    into s.live, so Sessions.step refuses any sample a step reports for them."""
    hop = s.pool.rt.cfg.hop
    items = s.pool.join_bounded(utterances, max_frames, 0.667, formats=formats)
    assert len(items) == len(names) == len(set(items))
    for name, item in zip(names, items):
        assert item not in s.live, f"row {item} handed out while {s.live.get(item)} holds it"
        s.item[name] = item
        if name in expect:
            s.live[item], s.samples[name], s.chunks[name] = name, expect[name] * hop, []
    return items


def check_bounded(s, name, audio, F, hop, what=""):
    got = s.audio(name)
    assert len(s.chunks[name]) == -(-F // s.pool.chunk_frames), (name, len(s.chunks[name]))
    assert got.size == audio.size == F * hop, (name, got.size, audio.size, F)
    assert_close(got, audio, TOL, f"bounded session {name} (F = {F}) vs whole utterance{what}")


def test_equivalence_joined_mid_stream(rt_medium, utts, wholes, pred):
    rt, hop, F = rt_medium, rt_medium.cfg.hop, pred["F"]
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11)
    s = Sessions(pool, utts)
    s.join("A")
    s.step()
    (item,) = join_bounded(s, ["P"], [pred["utt"]], F + 40, {"P": F})  # mid-stream
    assert pool.free_rows == 0
    s.drain()
    assert pool.item_samples(item) == F * hop
    assert np.array_equal(rt.durations(11), pred["dur"])  # the work slot learnt its durations when the join resolved
    assert rt.prepared_samples(11) == ([F * hop], F * hop)
    pool.close()
    check_bounded(s, "P", pred["audio"], F, hop)
    check_session(s, "A", wholes["A"], frames(utts, "A"), CHUNK, hop, " next to a bounded join")


@pytest.fixture(scope="module")
def odd(rt_medium):
    """An utterance whose F* is not a multiple of 4 (the float4 tail of the adopt): the first of a fixed list of candidates"""
    cands = [P_IDS, P_IDS[:-1], IDS, IDS * 3, P_IDS[:-3], IDS[:-1]]
    for ids in cands:
        (F,) = predicted_frames(rt_medium, [ids])
        if F % 4:
            audio, _dur = whole_of(rt_medium, ids)
            return {"utt": (ids, None, None, DEV), "F": F, "audio": audio}
    raise AssertionError("no candidate has F* % 4 != 0")


@pytest.mark.parametrize("edge", ["fits_exactly", "plus_1", "next_16", "next_16_plus_1"])
def test_length_edges_of_the_adopt(rt_medium, odd, edge):
    rt, hop, F = rt_medium, rt_medium.cfg.hop, odd["F"]
    assert F % 4 != 0
    up16 = (F // 16 + 1) * 16  # the next multiple of 16 above F*
    max_frames = {"fits_exactly": F, "plus_1": F + 1, "next_16": up16, "next_16_plus_1": up16 + 1}[edge]
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11)
    s = Sessions(pool, {})
    (item,) = join_bounded(s, ["P"], [odd["utt"]], max_frames, {"P": F})
    assert pool.item_samples(item) == F * hop
    s.drain()
    pool.close()
    check_bounded(s, "P", odd["audio"], F, hop, f" (max_frames = {max_frames})")


def over_bound_scenario(rt, utts, pred, with_failing_join):
    hop, F = rt.cfg.hop, pred["F"]
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11)
    s = Sessions(pool, utts)
    s.join("A")
    s.step()
    if with_failing_join:
        (item,) = join_bounded(s, ["P"], [pred["utt"]], F - 1, {})
        assert pool.free_rows == 0  # taken until the host knows better
        assert sorted(s.step()) == [s.item["A"]]  # the step resolves the join, returns OK and reports nothing for P
        assert pool.free_rows == 1
        with pytest.raises(ph.ShapeMismatch) as e:
            pool.item_samples(item)
        assert str(F) in str(e.value) and str(F - 1) in str(e.value), str(e.value)
        assert pool.free_rows == 1
    else:
        s.step()
    s.drain()  # (Sessions.step refuses samples for a row that is not live: no step ever reports any for P)
    assert pool.free_rows == 2
    pool.close()
    return s


def test_over_the_bound(rt_medium, utts, wholes, pred):
    rt, hop = rt_medium, rt_medium.cfg.hop
    plain = over_bound_scenario(rt, utts, pred, False)
    s = over_bound_scenario(rt, utts, pred, True)
    assert "P" not in s.chunks
    assert len(s.chunks["A"]) == len(plain.chunks["A"]) > 1
    for k, (a, b) in enumerate(zip(s.chunks["A"], plain.chunks["A"])):
        assert np.array_equal(a, b), f"session A, chunk {k}: differs next to a failing join"
    check_session(s, "A", wholes["A"], frames(utts, "A"), CHUNK, hop, " next to a failing join")


def test_three_items_the_middle_one_over_its_bound(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    ids3 = [IDS, IDS * 3, P_IDS[:-1]]  # ragged, the middle one the longest
    Fs = predicted_frames(rt, ids3)
    max_frames = Fs[1] - 1
    assert Fs[0] <= max_frames and Fs[2] <= max_frames and Fs[0] != Fs[2], Fs
    refs = [whole_of(rt, ids)[0] for ids in (ids3[0], ids3[2])]
    pool = rt.stream_pool(10, 4, chunkFrames=CHUNK, work_slot=11)
    s = Sessions(pool, {})
    items = join_bounded(s, ["X", "Y", "Z"], [(ids, None, None, DEV) for ids in ids3], max_frames, {"X": Fs[0], "Z": Fs[2]})
    assert items == [0, 1, 2] and pool.free_rows == 1
    with pytest.raises(ph.ShapeMismatch) as e:  # resolves the join before any step
        pool.item_samples(1)
    assert str(Fs[1]) in str(e.value) and str(max_frames) in str(e.value), str(e.value)
    assert pool.free_rows == 2
    assert [pool.item_samples(0), pool.item_samples(2)] == [Fs[0] * hop, Fs[2] * hop]
    s.drain()
    assert pool.free_rows == 4
    pool.close()
    check_bounded(s, "X", refs[0], Fs[0], hop, " (item 0 of 3)")
    check_bounded(s, "Z", refs[1], Fs[2], hop, " (item 2 of 3)")


def test_row_reuse(rt_medium, utts, wholes, pred):
    """Row 0 holds E (336 frames), then C (30), then the bounded P: a stale tail of E beyond P's true length would reach P's last windows.
    Then a bounded join is dropped while it is still pending and an ordinary join takes its row."""
    rt, hop, F = rt_medium, rt_medium.cfg.hop, pred["F"]
    assert frames(utts, "C") < F < frames(utts, "E")
    pool = rt.stream_pool(10, 3, chunkFrames=CHUNK, work_slot=11)
    for name in ("E", "C"):
        s = Sessions(pool, utts)
        assert s.join(name) == [0]
        s.drain()
    s = Sessions(pool, utts)
    assert join_bounded(s, ["P"], [pred["utt"]], F + 40, {"P": F}) == [0]
    s.drain()
    check_bounded(s, "P", pred["audio"], F, hop, " in a row that held a longer and a shorter item")
    assert pool.free_rows == 3
    s = Sessions(pool, utts)
    (item,) = join_bounded(s, ["P"], [pred["utt"]], F + 40, {})
    assert item == 0 and pool.free_rows == 2
    pool.drop(item)  # still pending
    assert pool.free_rows == 3
    with pytest.raises(ph.InvalidArgument):
        pool.item_samples(item)  # nothing in the row has a known length
    assert s.join("B") == [0]
    s.drain()
    pool.close()
    check_session(s, "B", wholes["B"], frames(utts, "B"), CHUNK, hop, " in the row of a dropped pending join")


def test_formats_on_a_mixed_pool(rt_medium, pred):
    rt, hop, rate, F = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate, pred["F"]
    f32, law = Format(0, "f32", 1.0), Format(8000, "mulaw", 1.0)
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11, mixed=True)
    items = pool.join_bounded([pred["utt"], pred["utt"]], F + 40, 0.667, formats=[lib_format(f32), lib_format(law)])
    assert items == [0, 1] and pool.free_rows == 0
    share = mr.step_bound_bytes(f32, rate, CHUNK * hop) + mr.step_bound_bytes(law, rate, CHUNK * hop)
    assert rt.stream_step_capacity_bytes(10) == share  # a pending row's share counts
    per = [[], []]
    for _ in range(64):
        out = pool.step_mixed()
        if not any(c.size for c in out):
            break
        for r in (0, 1):
            if out[r].size:
                per[r].append(out[r])
    assert pool.item_samples(0) == F * hop
    assert pool.item_samples(1) == ph.resample_count(rate, 8000, F * hop)
    pool.close()
    assert all(c.dtype == np.float32 for c in per[0]) and all(c.dtype == np.uint8 for c in per[1])
    x = np.concatenate(per[0])
    assert x.size == F * hop
    assert_close(x, pred["audio"], TOL, "the f32 row of a mixed bounded join vs whole utterance")
    want = mr.row_steps(per[0], law, rate, hop, CHUNK, True, TABLES)  # the μ-law row from the f32 row's samples, step by step
    want = [w for w in want if w.size]
    assert len(per[1]) == len(want)
    for k, (g, w) in enumerate(zip(per[1], want)):
        assert np.array_equal(g, w), f"μ-law row, step {k}: {int(np.count_nonzero(g != w)) if g.size == w.size else (g.size, w.size)}"
    assert sum(c.size for c in per[1]) == ph.resample_count(rate, 8000, F * hop)


def test_speakers(backend, voices):
    cfg, blob = voices["medium"]
    scfg = ph.speaker_config(5, 512)
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        rt.attach_speakers(scfg, ph.synthetic_speaker_blob(cfg, scfg, 4321))
        (F,) = predicted_frames(rt, [P_IDS], speakers=[3])
        audio, _dur = whole_of(rt, P_IDS, speaker=3)
        pool = rt.stream_pool(4, 2, chunkFrames=CHUNK, work_slot=5)
        rt.slot_speakers(5, [3])
        s = Sessions(pool, {})
        (item,) = join_bounded(s, ["P"], [(P_IDS, None, None, DEV)], F + 40, {"P": F})
        assert pool.item_samples(item) == F * cfg.hop
        s.drain()
        pool.close()
        check_bounded(s, "P", audio, F, cfg.hop, " (speaker 3)")
    finally:
        rt.close()


def test_bookkeeping_and_refused_calls(rt_medium, utts, wholes, pred):
    rt, hop, F = rt_medium, rt_medium.cfg.hop, pred["F"]
    pool = rt.stream_pool(10, 3, chunkFrames=CHUNK, work_slot=11)
    s = Sessions(pool, utts)
    s.join("A")
    s.step()
    assert pool.joins_pending() == 0  # the step waited for A's join
    (item,) = join_bounded(s, ["P"], [pred["utt"]], F + 40, {"P": F})
    assert pool.joins_pending() in (0, 1)
    assert pool.free_rows == 1  # a pending row is taken
    assert pool.item_samples(item) == F * hop
    assert pool.joins_pending() == 0
    assert pool.item_samples(s.item["A"]) == frames(utts, "A") * hop  # an ordinary row answers too
    with pytest.raises(ph.InvalidArgument):
        pool.item_samples(2)  # never held an item
    with pytest.raises(ph.InvalidArgument):
        pool.item_samples(3)  # out of range
    ids, dur, noise = utts["B"]
    refused = [
        (ph.InvalidArgument, dict(utterances=[(ids, dur, None, DEV)])),                       # supplied durations
        (ph.InvalidArgument, dict(utterances=[(ids, None, noise)])),                          # a host noise tensor
        (ph.InvalidArgument, dict(utterances=[(ids, None, None, DEV)], formats=[None])),      # formats on a pool that is not mixed
        (ph.ShapeMismatch, dict(utterances=[(ids, None, None, DEV)] * 2)),                    # 2 items, 1 free row
        (ph.ShapeMismatch, dict(utterances=[(ids, None, None, DEV)], max_frames=0)),          # prepare_batch_bounded's range check
    ]
    for exc, kw in refused:
        with pytest.raises(exc):
            pool.join_bounded(kw["utterances"], kw.get("max_frames", F + 40), 0.667, formats=kw.get("formats"))
        assert pool.free_rows == 1
    s.drain()  # the refused calls left the pool intact
    assert pool.free_rows == 3
    pool.close()
    check_bounded(s, "P", pred["audio"], F, hop, " after refused calls")
    check_session(s, "A", wholes["A"], frames(utts, "A"), CHUNK, hop, " after refused calls")
