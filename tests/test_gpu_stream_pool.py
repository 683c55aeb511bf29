"""GPU: the streaming pool (piper_hip_voice_stream_pool_*) — sessions join a running batched stream and leave it, rows are reused.
Each session must stream what its utterance gives alone: within fp32 summation order of synthesize()."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import piper_hip as ph
from conftest import assert_close
from test_gpu_stream_batch import SD, TOL, ragged_group, snr_db

pytestmark = pytest.mark.gpu

# ragged_group's items by the names used below: F = 84, 42, 30 (ragged durations), 70, 336
NAMES = {"A": 2, "B": 0, "C": 1, "D": 3, "E": 4}


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
    """The whole-utterance waveform of every item, computed once and only read by the tests."""
    out = {}
    for name, (ids, dur, noise) in utts.items():
        out[name] = rt_medium.synthesize(ids, dur, noise, 0.667)
        out[name].setflags(write=False)
    return out


class Sessions:
    """Bookkeeping of a test's sessions on one pool: who sits in which row, the chunks each has received."""

    def __init__(self, pool, utts):
        self.pool, self.utts = pool, utts
        self.live, self.chunks, self.samples, self.item = {}, {}, {}, {}

    def join(self, *names, utterances=None):
        got = self.pool.join(utterances if utterances is not None else [self.utts[n] for n in names], 0.667)
        assert len(got) == len(names)
        for name, (item, samples) in zip(names, got):
            assert item not in self.live, f"row {item} handed out while {self.live.get(item)} holds it"
            self.live[item], self.item[name], self.samples[name], self.chunks[name] = name, item, samples, []
        return [item for item, _ in got]

    def step(self):
        out = self.pool.step()
        assert set(out) <= set(self.live), (sorted(out), self.live)
        for item, chunk in out.items():
            name = self.live[item]
            self.chunks[name].append(chunk)
            if sum(c.size for c in self.chunks[name]) >= self.samples[name]:
                del self.live[item]  # last chunk: the row is free
        return out

    def drop(self, name):
        self.pool.drop(self.item[name])
        del self.live[self.item[name]]

    def drain(self, limit=64):
        for _ in range(limit):
            if not self.step():
                return
        raise AssertionError("the pool did not go idle")

    def audio(self, name):
        return np.concatenate(self.chunks[name])


def check_session(s, name, whole, F, chunk, hop, what=""):
    ch = s.chunks[name]
    assert len(ch) == -(-F // chunk), (name, len(ch))
    assert all(c.size == chunk * hop for c in ch[:-1]), name
    assert s.samples[name] == F * hop, name
    got = s.audio(name)
    assert got.size == whole.size == F * hop
    assert_close(got, whole, TOL, f"session {name} (F = {F}, chunk {chunk}) vs whole utterance{what}")


def frames(utts, name):
    return sum(utts[name][1])


def staggered(rt, utts, slot, work_slot):
    """The scenario of the first test: capacity 4, chunk 32. A joins alone; B and C join one step later; when A has finished D joins
    and must get A's row, E joins as soon as a row is free; then steps until the pool is idle."""
    pool = rt.stream_pool(slot, 4, chunkFrames=32, work_slot=work_slot)
    s = Sessions(pool, utts)
    assert pool.free_rows == 4
    assert s.join("A") == [0]
    assert pool.free_rows == 3
    assert sorted(s.step()) == [0]
    assert s.join("B", "C") == [1, 2]  # lowest free rows first
    assert pool.free_rows == 1
    while "A" in s.live.values():
        out = s.step()
        assert 0 in out
    # A (3 chunks) finished on step 3; B (2 chunks) and C (1 chunk) joined on step 2 and have finished too
    assert pool.free_rows == 4 and not s.live
    assert s.join("D") == [s.item["A"]]
    assert pool.free_rows == 3
    assert s.join("E") == [1]
    assert pool.free_rows == 2
    s.drain()
    assert pool.free_rows == 4
    assert pool.step() == {}  # idle, not closed
    pool.close()
    return s


def test_staggered_joins_and_row_reuse(rt_medium, utts, wholes):
    rt, hop = rt_medium, rt_medium.cfg.hop
    s = staggered(rt, utts, slot=10, work_slot=11)
    for name in "ABCDE":
        check_session(s, name, wholes[name], frames(utts, name), 32, hop)
    ids, dur, noise = utts["A"]
    single = np.concatenate(list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=32, slot=3)))
    assert_close(s.audio("A"), single, TOL, "session A vs stream_begin / stream_next")


def test_stale_rows(rt_medium, utts, wholes):
    """Capacity 3 (generator batch 4, one pad row), chunk 16. Row 0 holds E (336 frames), then C (30): a shorter item after a longer one
    must not pick up a stale tail; then E again: a longer item after a shorter one."""
    rt, hop = rt_medium, rt_medium.cfg.hop
    pool = rt.stream_pool(10, 3, chunkFrames=16, work_slot=11)
    for k, name in enumerate(("E", "C", "E")):
        s = Sessions(pool, utts)
        assert s.join(name) == [0]
        assert pool.free_rows == 2
        s.drain()
        assert pool.free_rows == 3
        check_session(s, name, wholes[name], frames(utts, name), 16, hop, f" (round {k})")
    pool.close()


def test_drop_frees_the_row(rt_medium, utts, wholes):
    rt, hop = rt_medium, rt_medium.cfg.hop
    pool = rt.stream_pool(10, 4, chunkFrames=32, work_slot=11)
    s = Sessions(pool, utts)
    assert s.join("A", "D", "B") == [0, 1, 2]
    assert sorted(s.step()) == [0, 1, 2]
    s.drop("D")  # after its first chunk
    assert pool.free_rows == 2
    assert sorted(s.step()) == [0, 2]  # D reports 0
    assert s.join("E") == [1]  # D's row, not the never-used row 3
    s.drain()
    assert len(s.chunks["D"]) == 1
    assert_close(s.chunks["D"][0], wholes["D"][:32 * hop], TOL, "D's only chunk")
    for name in "ABE":
        check_session(s, name, wholes[name], frames(utts, name), 32, hop, " with D dropped")
    pool.close()


def test_full_pool_and_bad_arguments(rt_medium, utts, wholes):
    rt, hop = rt_medium, rt_medium.cfg.hop
    lib, v = rt.lib, rt.voice
    pool = rt.stream_pool(10, 2, chunkFrames=32, work_slot=11)
    s = Sessions(pool, utts)
    assert s.join("A") == [0]
    with pytest.raises(ph.ShapeMismatch):
        pool.join([utts["B"], utts["C"]], 0.667)  # 2 items, 1 free row
    assert pool.free_rows == 1
    with pytest.raises(ph.ExecutionError):
        rt.stream_pool(12, 2, chunkFrames=32, work_slot=12).join([utts["B"]], 0.667)  # work_slot == slot
    with pytest.raises(ph.ExecutionError):
        rt.stream_pool(12, 2, chunkFrames=32, work_slot=10).join([utts["B"]], 0.667)  # the work slot holds a pool
    one = C.c_int64()
    with pytest.raises(ph.ExecutionError):
        ph._check(lib.piper_hip_voice_stream_next(v, 10, None, 0, C.byref(one)))
    for bad in (-1, 2):
        with pytest.raises(ph.ExecutionError):
            pool.drop(bad)
    s.drain()  # the refused calls left the pool intact
    check_session(s, "A", wholes["A"], frames(utts, "A"), 32, hop, " after refused calls")
    pool.close()
    with pytest.raises(ph.ExecutionError):
        pool.step()  # stream_next_batch after close
    with pytest.raises(ph.ExecutionError):
        pool.close()
    for cap, chunk in ((0, 32), (257, 32), (2, 0)):
        with pytest.raises(ph.ExecutionError):
            rt.stream_pool(10, cap, chunkFrames=chunk, work_slot=11)
    rt.stream_pool(12, 1).close()


def test_predicted_durations_join(rt_medium, utts, wholes):
    rt, hop = rt_medium, rt_medium.cfg.hop
    ids = kd.FIXTURE_IDS * 2
    dev = {"noise_mode": "device", "seed": 4242}
    pool = rt.stream_pool(10, 2, chunkFrames=32, work_slot=11)
    s = Sessions(pool, utts)
    s.join("A")
    s.step()
    s.join("P", utterances=[(ids, None, None, dev)])  # mid-stream
    dur_join = rt.durations(11)
    per, total = rt.prepared_samples(11)
    assert per == [s.samples["P"]] and total == s.samples["P"]
    s.drain()
    pool.close()
    whole = rt.synthesize(ids, None, None, 0.667, noise_mode="device", seed=4242)
    dur_single = rt.durations(0)
    assert np.array_equal(dur_join, dur_single)
    got = s.audio("P")
    assert got.size == whole.size == s.samples["P"] == int(dur_single.sum()) * hop
    assert_close(got, whole, TOL, "predicted-duration session vs whole utterance")
    check_session(s, "A", wholes["A"], frames(utts, "A"), 32, hop, " next to a predicted-duration join")


def test_plans_and_determinism(rt_medium, utts):
    rt = rt_medium
    first = staggered(rt, utts, slot=10, work_slot=11)
    plans = rt.plan_info(10)["cached_plans"]
    again = staggered(rt, utts, slot=10, work_slot=11)
    for name in "ABCDE":
        assert np.array_equal(first.audio(name), again.audio(name)), name
    assert rt.plan_info(10)["cached_plans"] <= plans
    # a group of 4 has the pool's generator batch and, at the same chunk, windows the pool has decoded: only its front plan is new
    group = [utts[n] for n in "ABCD"]
    for _ in rt.synthesize_stream_batch(group, 0.667, chunkFrames=32, slot=13):
        pass
    assert rt.plan_info(13)["cached_plans"] <= plans + 1


@pytest.mark.parametrize("pcm", [False, True], ids=["fp32", "pcm16_gain_0.5"])
def test_group_and_pool_steps_are_bit_equal(rt_medium, utts, pcm):
    """C, A, E (F = 30, 84, 336: ragged, none a multiple of 32, C shorter than one chunk, E longer than three) at chunk 32 as a group of 3
    and joined at once into an empty pool of capacity 3 — generator batch 4, one pad row. A group and a pool run the same step on the same
    generator plans with equal inputs: the same number of steps, and every step's n_samples and packed chunks equal bit for bit."""
    rt = rt_medium
    items = [utts[name] for name in "CAE"]
    Fs = [frames(utts, name) for name in "CAE"]
    halo = rt.lib.piper_hip_voice_receptive_field(rt.voice)
    assert len(set(Fs)) == 3 and any(F % 32 for F in Fs) and min(Fs) < 32 + halo and max(Fs) > 3 * 32
    kw = {"pcm": True, "gain": 0.5} if pcm else {}
    group = [(tuple(c.size for c in chunks), np.concatenate(chunks))
             for chunks in rt.synthesize_stream_batch(items, 0.667, chunkFrames=32, slot=8, **kw)]
    pool = rt.stream_pool(10, 3, chunkFrames=32, work_slot=11)
    assert [item for item, _ in pool.join(items, 0.667)] == [0, 1, 2]
    pooled = []
    while True:
        out = pool.step(**kw)
        if not out:
            break
        pooled.append((tuple(out[i].size if i in out else 0 for i in range(3)), np.concatenate([out[i] for i in sorted(out)])))
    pool.close()
    assert len(group) == len(pooled) == -(-max(Fs) // 32)
    for k, ((n_g, x_g), (n_p, x_p)) in enumerate(zip(group, pooled)):
        assert n_g == n_p, (k, n_g, n_p)
        assert x_g.dtype == x_p.dtype == (np.int16 if pcm else np.float32)
        assert np.array_equal(x_g, x_p), f"step {k}: group and pool differ in {int(np.count_nonzero(x_g != x_p))} of {x_g.size} samples"
    assert sum(sum(n) for n, _ in group) == sum(Fs) * rt.cfg.hop


def test_high_voice_fp32_and_bf16(backend, voices):
    cfg, blob = voices["high"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        items = {}
        for k, f in enumerate((1, 2, 4)):
            dur = [3] * (14 * f)
            items[f] = (kd.FIXTURE_IDS * f, dur, kd.sym(SD + 40 + k, (cfg.inter, sum(dur)), 1.7320508))
        whole = {f: rt.synthesize(ids, dur, nz, 0.667) for f, (ids, dur, nz) in items.items()}

        def run():
            pool = rt.stream_pool(1, 4, chunkFrames=32, work_slot=2)
            s = Sessions(pool, items)
            for f in (1, 2, 4):  # one step apart
                s.join(f)
                s.step()
            s.drain()
            pool.close()
            return s

        s = run()
        for f in (1, 2, 4):
            check_session(s, f, whole[f], 42 * f, 32, cfg.hop, " (high, fp32)")
        rt.set_precision("bf16")
        s = run()
        for f in (1, 2, 4):
            got = s.audio(f)
            assert got.size == whole[f].size
            assert snr_db(got, whole[f]) >= 40.0, (f, snr_db(got, whole[f]))
    finally:
        rt.close()
