"""GPU: level control (include/piper_hip.h "Level control") — the look-ahead limiter on whole items and on every stream route. The raw fp32
reference is always the GPU's own audio: the same slot collected without a level, or the same stream run once without a level. On top
of it tests/level_ref.py and the existing pcm_ref / resample_ref / g711_ref / mixed_ref are applied, and compared bit for bit, counts
included. The drive comes from the measured raw peak (ceiling 0.5, drive = 3 / peak), and the reference alone must show that at least one
block in ten is over the ceiling and at least one block has g = 1: a test that never limits, or always limits, shows nothing.

The stock synthetic voice cannot show both: its output conv drives the final tanh into saturation, every block of its audio peaks near 1.0
and the limiter would sit at 1 / 6 from the first block to the last. The voice here is the same synthetic medium voice with the output
conv's weights scaled by 0.02, so that the waveform follows the size of the latent, and the items' injected noise carries an envelope —
16 on most frames, 0 on a stretch of 16 frames — which gives every item loud stretches and a quiet one. Items whose noise is drawn on
the device (bounded prepares and joins) have no envelope; they get theirs from the noise scale, per item."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import level_ref as lr
import mixed_ref as mr
import piper_hip as ph
import resample_ref as rr
from mixed_ref import Format
from test_gpu_resample import same_bits
from test_gpu_stream_batch import ragged_group
from test_gpu_stream_mixed import TABLES
from test_level_abi import NS, vector

pytestmark = pytest.mark.gpu

F32 = np.float32
SINKS = {"f32": Format(0, "f32", 1.0), "s16": Format(0, "s16", 1.0), "s16@8000": Format(8000, "s16", 1.0), "s16@48000": Format(48000, "s16", 0.5),
         "mulaw@8000": Format(8000, "mulaw", 1.0)}
DEV = {"noise_mode": "device", "seed": 4242}


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    blob = blob.copy()
    (post,) = [e for e in ph.blob_layout(cfg) if e["name"] == "dec.conv_post.weight"]
    blob[post["offset"]:post["offset"] + post["count"]] *= F32(0.02)
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


def shaped(cfg, durs, seed, quiet_at=None):
    """(ids, durations, noise): the noise is 16 × the usual on every frame but a stretch of 16, where it is 0 (items under 24 frames: none).
    The stretch starts a quarter into the item, or at frame quiet_at."""
    F = sum(durs)
    env = np.full(F, 16.0, F32)
    if F >= 24:
        q = F // 4 if quiet_at is None else quiet_at
        env[q:q + 16] = 0.0
    return (kd.FIXTURE_IDS * 4)[:len(durs)], list(durs), kd.sym(900 + seed, (cfg.inter, F), 1.7320508) * env


def item(cfg, n_ids, seed):
    return shaped(cfg, [3] * n_ids, seed)


def level_for(raws):
    """ceiling 0.5, drive 3 / peak of the raw audio; asserts on the reference alone that the limiter works on some blocks and rests on others"""
    peak = max(float(np.abs(x).max()) for x in raws)
    assert 0.003 < peak < 1e6, peak
    level = (3.0 / peak, 0.5, 50.0)
    over = blocks = unity = 0
    for x in raws:
        u, node = lr.gains(x, level, 22050)
        K = x.size // 32
        over += int((np.abs(u[:K * 32]).reshape(-1, 32).max(axis=1) > 0.5).sum())
        blocks += K
        unity += int(((node[:-1] == 1.0) & (node[1:] == 1.0)).sum())
    print(f"level {level}: {over} of {blocks} blocks over the ceiling, {unity} blocks at g = 1")
    assert over * 10 >= blocks and unity >= 1, (over, blocks, unity)
    return level


def stream_kw(fmt):
    return dict(pcm=fmt.enc != "f32", gain=fmt.gain, rate=fmt.rate or None, encoding=fmt.enc if fmt.enc in ("mulaw", "alaw") else None)


def rs_ready(e, L, M, P):
    return 0 if e <= P // 2 else rr.count(e - P // 2, L, M)


def expected_row(raw_chunks, level, fmt, chunk, hop, rate, finished=True):
    """The typed chunk of every step of one row whose un-levelled fp32 chunks are raw_chunks: the limiter's emit rule [lo, hi), then the
    output stage's own rule on that range as if it were the chunk."""
    x = np.concatenate(raw_chunks)
    assert x.size % hop == 0
    frames = x.size // hop
    y = lr.apply(x, level, rate)  # (an unfinished row: final up to ready(e), and no step reads further)
    ranges = lr.step_ranges(frames if finished else frames + chunk, chunk, hop)[:len(raw_chunks)]
    fl = mr.filt(fmt, rate, TABLES)
    out = []
    for k, (lo, hi) in enumerate(ranges):
        last = finished and k == len(ranges) - 1
        assert hi > lo and (hi == x.size) == last
        if fl is None:
            out.append(mr.sink(y[lo:hi], fmt))
            continue
        tab, L, M, P = fl
        j0 = 0 if lo == 0 else rs_ready(lo, L, M, P)
        j1 = rr.count(x.size, L, M) if last else max(j0, rs_ready(hi, L, M, P))
        out.append(mr.sink(rr.apply(y[:hi], tab, L, M, j0, j1) if j1 > j0 else np.empty(0, F32), fmt))
    return out


def whole_item(x, level, fmt, rate):
    return mr.whole(lr.apply(x, level, rate), fmt, rate, TABLES)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        return got.dtype == np.float32 and same_bits(got, want)
    return got.dtype == want.dtype and np.array_equal(got, want)


def check_row(got_chunks, raw_chunks, level, fmt, chunk, hop, rate, what, finished=True):
    want = expected_row(raw_chunks, level, fmt, chunk, hop, rate, finished)
    assert [c.size for c in got_chunks] == [c.size for c in want], what  # per step n_samples: the composed emit rule
    for k, (g, w) in enumerate(zip(got_chunks, want)):
        assert same(g, w), (what, k)
    if finished:  # the concatenation equals the whole-item conversion
        assert same(np.concatenate(got_chunks), whole_item(np.concatenate(raw_chunks), level, fmt, rate)), what


# ---- per-op

@pytest.mark.parametrize("n", NS)
def test_per_op(backend, n):
    x = vector(n, 300 + n)
    for level, rate in (((3.0, 0.5, 50.0), 22050), ((8.0, 0.25, 5.0), 16000), ((0, 0, 0), 22050)):
        buf = backend.uploadFloat32(x if n else np.zeros(1, F32))
        out = backend.level_f32(buf, rate, level, count=n)
        got = backend.downloadFloat32(out, n) if n else np.empty(0, F32)
        assert same_bits(got, lr.apply(x, level, rate)), (n, level, rate)
        assert same_bits(got, ph.level_from_f32(x, level, rate))
    with pytest.raises(ph.InvalidArgument):
        backend.level_f32(backend.uploadFloat32(np.zeros(4, F32)), 22050, (1.0, 2.0, 50.0))


def test_per_op_long_item_and_unaligned_source(backend):
    x = vector(70001, 5)  # 2188 blocks: more than one pass of the chain, more than one thread block of peaks
    level = (3.0, 0.5, 50.0)
    buf = backend.uploadFloat32(np.concatenate([np.zeros(1, F32), x]))
    whole = backend.downloadFloat32(backend.level_f32(backend.uploadFloat32(x), 22050, level), x.size)
    assert same_bits(whole, lr.apply(x, level, 22050))
    shifted = ph.DeviceBuffer(backend, buf.ptr + 4, x.size, owned=False)  # a source that is not 16-byte aligned
    assert same_bits(backend.downloadFloat32(backend.level_f32(shifted, 22050, level), x.size), whole)


# ---- whole items

def plain(rt, slot):
    rt.prepare(slot, *item(rt.cfg, 14, 1), 0.667)


def ragged(rt, slot):
    rt.prepare_batch(slot, [item(rt.cfg, n, k) for k, n in enumerate((40, 14, 23))], 0.667)


def bounded(rt, slot):
    """prepare_batch_bounded of two items with a noise scale each: a loud one and a quiet one (the device draws the noise: no envelope)"""
    id_lists = [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS]
    bound = max(int(d.sum()) for d, _ in rt.predict_durations([(ids, None) for ids in id_lists], **DEV)) + 5
    arr, keep = (ph.Utterance * 2)(), []
    for i, (ids, scale) in enumerate(zip(id_lists, (0.667 * 16, 0.0))):
        arr[i], k = rt._utt(ids, None, None, scale, **DEV)
        keep.append(k)
    assert rt.lib.piper_hip_voice_prepare_batch_bounded(rt.voice, arr, 2, slot, bound) >= 0
    tot = C.c_int64()
    ph._check(rt.lib.piper_hip_voice_prepared_samples(rt.voice, slot, None, 0, C.byref(tot)))
    rt._keep[slot] = (keep, int(tot.value), True)


def collect_as(rt, slot, name, **kw):
    fmt = SINKS[name]
    if fmt.enc == "f32":
        return rt.collect(slot, **kw)
    if fmt.enc == "s16":
        return rt.collect_pcm16(slot, gain=fmt.gain, rate=fmt.rate or None, **kw)
    return rt.collect_g711(slot, fmt.enc, gain=fmt.gain, rate=fmt.rate or None, **kw)


@pytest.mark.parametrize("prep", [plain, ragged, bounded])
def test_whole_items_in_both_orders(rt_medium, prep):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    prep(rt, 5)
    rt.launch(5)
    raw = rt.collect(5, level=None).copy()  # (a bounded slot: its collecting call)
    per, total = rt.prepared_samples(5)
    assert raw.size == total
    items = np.split(raw, np.cumsum(per)[:-1])
    level = level_for(items)
    steps = rt.steps(5)
    want = {name: np.concatenate([whole_item(it, level, f, rate) for it in items]) for name, f in SINKS.items()}
    plain_bytes = {name: collect_as(rt, 5, name).copy() for name in SINKS}  # without a level, before any level was set
    for name in SINKS:  # raw first, then with a level …
        assert same(collect_as(rt, 5, name, level=level), want[name]), (name, "level after raw")
    assert same_bits(rt.tap(5, "audio").reshape(-1), raw)  # the audio tap stays raw
    with pytest.raises(ph.InvalidArgument):
        rt.collect_pcm16(5, normalize=True)
    for name in SINKS:  # … and the un-levelled bytes are what they were
        assert same(collect_as(rt, 5, name, level=None), plain_bytes[name]), (name, "raw after level")
    assert rt.steps(5) == steps
    # the other order on one launch: the level's collect is the first thing that reads the new run
    for name in SINKS:
        prep(rt, 6)
        rt.launch(6)
        assert same(collect_as(rt, 6, name, level=level), want[name]), (name, "level first")
        assert same_bits(rt.collect(6, level=None), raw), name
    # a neutral level reproduces the un-levelled bytes (the audio is under the ceiling when the drive puts it there)
    peak = max(float(np.abs(it).max()) for it in items)
    if peak < 1.0:
        for name in SINKS:
            assert same(collect_as(rt, 5, name, level=(1.0, 1.0, 20.0)), plain_bytes[name]), (name, "neutral")
    rt.slot_level(5, None)
    rt.slot_level(6, None)


def test_synthesize_twins_take_slot_0_level(rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    ids, dur, noise = item(rt.cfg, 14, 1)
    raw = rt.synthesize(ids, dur, noise, 0.667, level=None)
    level = level_for([raw])
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, level=level), lr.apply(raw, level, rate))
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000), whole_item(raw, level, SINKS["s16@8000"], rate))  # the level stays
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000), whole_item(raw, level, SINKS["mulaw@8000"], rate))
    with pytest.raises(ph.InvalidArgument):
        rt.synthesize_pcm16(ids, dur, noise, 0.667, normalize=True)
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, level=None), raw)


# ---- streams: the twin is the same stream run once without a level

def single_item(cfg):
    return shaped(cfg, [3] * 23 + [1], 3)  # F = 70: not a multiple of 3


@pytest.fixture(scope="module")
def single_twin(rt_medium):
    ids, dur, noise = single_item(rt_medium.cfg)
    return {c: list(rt_medium.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=c, slot=3)) for c in (2, 3)}


@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("chunk", [2, 3])
def test_single_stream(rt_medium, single_twin, chunk, sink):
    rt, hop, fmt = rt_medium, rt_medium.cfg.hop, SINKS[sink]
    ids, dur, noise = single_item(rt.cfg)
    raw = single_twin[chunk]
    level = level_for([np.concatenate(raw)])
    got = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3, level=level, **stream_kw(fmt)))
    assert len(got) == len(raw) == -(-70 // chunk)
    check_row(got, raw, level, fmt, chunk, hop, rt.cfg.sample_rate, (sink, chunk))
    # and a stream without a level on the same slot delivers what it delivered before
    if sink == "f32":
        again = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3))
        assert all(same_bits(a, b) for a, b in zip(again, raw)) and len(again) == len(raw)


def group_items(cfg):
    return [shaped(cfg, ragged_group(cfg)[1][1], 5), shaped(cfg, [1, 1], 6), item(cfg, 14, 7)]  # F = 30, 2 (one step), 42


def run_group(rt, chunk, level=None, fmt=SINKS["f32"], drop=(0, 4)):
    per = [[] for _ in range(3)]
    for k, chunks in enumerate(rt.synthesize_stream_batch(group_items(rt.cfg), 0.667, chunkFrames=chunk, slot=8, level=level, **stream_kw(fmt))):
        for i, c in enumerate(chunks):
            if c.size:
                per[i].append(c)
        if k == drop[1] - 1:
            rt.stream_drop(8, drop[0])
    return per


@pytest.fixture(scope="module")
def group_twin(rt_medium):
    return {c: run_group(rt_medium, c) for c in (2, 3)}


@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("chunk", [2, 3])
def test_ragged_group_with_a_one_step_item_and_a_drop(rt_medium, group_twin, chunk, sink):
    rt, hop, fmt = rt_medium, rt_medium.cfg.hop, SINKS[sink]
    raw = group_twin[chunk]
    assert [len(r) for r in raw] == [4, 1, -(-42 // chunk)]  # item 0 dropped after four steps, item 1 is one step
    level = level_for([np.concatenate(r) for r in raw])
    got = run_group(rt, chunk, level, fmt)
    for i in range(3):
        check_row(got[i], raw[i], level, fmt, chunk, hop, rt.cfg.sample_rate, (sink, chunk, i), finished=i != 0)


def pool_sessions(rt):
    cfg = rt.cfg
    return {"S": item(cfg, 5, 9), "E": item(cfg, 14, 8), "A": shaped(cfg, ragged_group(cfg)[1][1], 5), "B": shaped(cfg, [3] * 9, 4, quiet_at=0),
            "P": (kd.FIXTURE_IDS * 2, None, None, DEV)}  # F = 15, 42, 30, 27 (B starts quiet: an inherited gain would show), predicted


def run_pool(rt, chunk, level=None, fmt=SINKS["f32"], formats=None):
    """Capacity 4: S (15 frames), E and A join, and P by a bounded join; when S has finished B takes its row — a new occupant that must not
    inherit S's carry or gain. formats: {session: Format} on a mixed pool. Returns ({session: [chunk per step]}, [raw step] if mixed)."""
    u = pool_sessions(rt)
    mixed = formats is not None
    pool = rt.stream_pool(10, 4, chunkFrames=chunk, work_slot=11, rate=fmt.rate or None, mixed=mixed, level=level)
    lf = (lambda names: [ph.stream_format(rate=formats[s].rate, encoding=formats[s].enc, gain=formats[s].gain) for s in names]) if mixed else (lambda names: None)
    assert [i for i, _ in pool.join([u["S"], u["E"], u["A"]], 0.667, formats=lf("SEA"))] == [0, 1, 2]
    assert pool.join_bounded([u["P"]], 400, 0.667, formats=lf("P")) == [3]
    who = {0: "S", 1: "E", 2: "A", 3: "P"}
    per, raws, caps = {s: [] for s in "SEABP"}, [], []
    for k in range(256):
        if k == -(-15 // chunk):
            assert pool.free_rows >= 1  # S has finished
            (row, samples), = pool.join([u["B"]], 0.667, formats=lf("B"))
            assert row == 0
            who[0] = "B"
        caps.append(rt.stream_step_capacity_bytes(10) if mixed else rt.stream_step_capacity(10))
        if mixed:
            st = pool.step_mixed(raw=True)
            if not any(st[0]):
                break
            raws.append(st)
            for r, c in enumerate(st[0]):
                if c:
                    f = formats[who[r]]
                    per[who[r]].append(st[2][st[1][r]:st[1][r] + c * mr.ELEM[f.enc]].view(mr.DTYPE[f.enc]).copy())
        else:
            out = pool.step(pcm=fmt.enc != "f32", gain=fmt.gain, encoding=fmt.enc if fmt.enc == "mulaw" else None)
            if not out:
                break
            for r, c in out.items():
                per[who[r]].append(c)
    pool.close()
    return per, raws, caps


@pytest.fixture(scope="module")
def pool_twin(rt_medium):
    return {c: run_pool(rt_medium, c)[0] for c in (2, 3)}


@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("chunk", [2, 3])
def test_pool_with_a_take_over_and_a_bounded_join(rt_medium, pool_twin, chunk, sink):
    rt, hop, fmt = rt_medium, rt_medium.cfg.hop, SINKS[sink]
    raw = pool_twin[chunk]
    assert all(len(raw[s]) for s in "SEABP")
    level = level_for([np.concatenate(raw[s]) for s in "SEABP"])
    got, _, caps = run_pool(rt, chunk, level, fmt)
    for s in "SEABP":
        check_row(got[s], raw[s], level, fmt, chunk, hop, rt.cfg.sample_rate, (sink, chunk, s))
    per_row = lr.step_bound(chunk * hop)
    if fmt.rate:
        per_row = rr.step_bound(per_row, *rr.ratio(rt.cfg.sample_rate, fmt.rate))
    assert set(caps) == {4 * per_row}


def test_pool_row_taken_over_starts_from_nothing(rt_medium, pool_twin):
    """The reference itself: had B's first step seen S's carry — its last samples and the gain they left, in front of B's quiet start —
    the limited samples would differ from the ones test_pool_with_a_take_over_and_a_bounded_join has just found."""
    raw = pool_twin[2]
    s_tail, b = np.concatenate(raw["S"])[-255:], np.concatenate(raw["B"])
    level = level_for([np.concatenate(raw[s]) for s in "SEABP"])
    clean = lr.apply(b, level, 22050)[:256]
    haunted = lr.apply(np.concatenate([np.zeros(1, F32), s_tail, b]), level, 22050)[256:512]
    assert not same_bits(clean, haunted)


MIXED = {"S": Format(48000, "s16", 1.0), "E": Format(8000, "mulaw", 1.0), "A": Format(0, "f32", 1.0), "B": Format(8000, "mulaw", 0.5), "P": Format(48000, "s16", 1.0)}


@pytest.mark.parametrize("chunk", [2, 3])
def test_mixed_pool(rt_medium, pool_twin, chunk):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    raw = pool_twin[chunk]
    level = level_for([np.concatenate(raw[s]) for s in "SEABP"])
    got, steps, caps = run_pool(rt, chunk, level, formats=MIXED)
    for s in "SEABP":
        check_row(got[s], raw[s], level, MIXED[s], chunk, hop, rate, ("mixed", chunk, s))
    who = {0: "S", 1: "E", 2: "A", 3: "P"}
    for k, (counts, offs, data) in enumerate(steps):  # byte_off: the layout of "Mixed formats" over the counts above
        if k == -(-15 // chunk):
            who[0] = "B"
        want_offs, total = mr.layout(counts, [mr.ELEM[MIXED[who[r]].enc] for r in range(4)])
        assert offs == want_offs and data.size == total, k
    share = {s: (mr.step_bound_bytes(MIXED[s], rate, lr.step_bound(chunk * hop))) for s in "SEABP"}
    assert caps[0] == share["S"] + share["E"] + share["A"] + share["P"] and max(d.size for _, _, d in steps) <= max(caps)


# ---- state rules

def test_state_rules(rt_medium):
    rt, lib = rt_medium, rt_medium.lib
    hop, rate = rt.cfg.hop, rt.cfg.sample_rate
    ids, dur, noise = shaped(rt.cfg, ragged_group(rt.cfg)[1][1], 5)  # F = 30
    raw = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=3, slot=3))
    level = level_for([np.concatenate(raw)])
    want = expected_row(raw, level, SINKS["s16"], 3, hop, rate)
    u, keep = rt._utt(ids, dur, noise, 0.667)
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_level(12, level)  # no stream there
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 1) == 30
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_level(3, level)  # chunk_frames · hop = 256 < 512
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 3) == 10
    with pytest.raises(ph.InvalidArgument):
        rt.stream_level(3)  # none yet
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_level(3, (1.0, 2.0, 50.0))
    assert rt.stream_step_capacity(3) == 3 * hop
    rt.stream_set_level(3, (0, 0, 0))
    got = rt.stream_level(3)
    assert (got.drive, got.ceiling, got.release_ms) == (1.0, 1.0, 50.0)
    rt.stream_set_level(3, level)  # before the first step the level may still change
    assert rt.stream_step_capacity(3) == 3 * hop + 255 == ph.level_step_bound(3 * hop)
    rt.stream_set_rate(3, 8000)  # either order
    assert rt.stream_step_capacity(3) == ph.resample_step_bound(rate, 8000, 3 * hop + 255)
    rt.stream_set_rate(3, rate)
    buf, got_n = np.empty(3 * hop + 255, np.int16), C.c_int64()
    with pytest.raises(ph.ShapeMismatch):  # a buffer one sample short consumes nothing
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), want[0].size - 1, C.byref(got_n)))
    with pytest.raises(ph.UnsupportedOp):  # normalize on a step stays what it was
        prm = ph.PcmParams(1.0, 1)
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, C.byref(prm), buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got_n)))
    parts = []
    for k in range(16):
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got_n)))
        if not got_n.value:
            break
        parts.append(buf[:got_n.value].copy())
        with pytest.raises(ph.InvalidArgument):  # after a step the level is fixed
            rt.stream_set_level(3, level)
    assert [p.size for p in parts] == [w.size for w in want] and all(np.array_equal(p, w) for p, w in zip(parts, want))
    # a new begin clears the level
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 3) == 10
    with pytest.raises(ph.InvalidArgument):
        rt.stream_level(3)
    fbuf = np.empty(3 * hop, F32)
    ph._check(lib.piper_hip_voice_stream_next(rt.voice, 3, fbuf.ctypes.data_as(ph.c_f32p), fbuf.size, C.byref(got_n)))
    assert got_n.value == 3 * hop and same_bits(fbuf, raw[0])
    # a pool: the level is fixed from its first join on
    pool = rt.stream_pool(10, 2, chunkFrames=3, work_slot=11)
    pool.join([(ids, dur, noise)], 0.667)
    with pytest.raises(ph.InvalidArgument):
        pool.set_level(level)
    pool.close()
    del keep


def test_window_plans_are_unchanged(rt_medium):
    """The limiter runs behind the window plan's graph and is never captured: the plan's steps are the same with and without a level."""
    rt = rt_medium
    ids, dur, noise = shaped(rt.cfg, ragged_group(rt.cfg)[1][1], 5)
    gen = rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=3, slot=3)
    next(gen)
    plain_steps = rt.steps(3, window=True)
    gen.close()
    gen = rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=3, slot=3, level=(3.0, 0.5, 50.0))
    next(gen)
    assert rt.steps(3, window=True) == plain_steps
    gen.close()
