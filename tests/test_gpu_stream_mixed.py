"""GPU: mixed-format streaming (include/piper_hip.h "Mixed formats") — every row of a group or pool in its own rate, encoding and gain, one
output launch per step. Every comparison is bit for bit: the fp32 twin of a scenario is a plain float group or pool of the same sessions
(the windows are the same, so the fp32 samples are), and tests/mixed_ref.py turns its chunks into the n_samples, byte_off and bytes every
step must deliver, with the library's own filter tables."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import mixed_ref as mr
import piper_hip as ph
import resample_ref as rr
from mixed_ref import Format
from test_gpu_resample import item
from test_gpu_stream_batch import SD, ragged_group

pytestmark = pytest.mark.gpu

CHUNK = 8


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


class Tables(dict):
    """{(in, out): the library's own [L][P] table}, fetched on first use"""

    def __missing__(self, pair):
        self[pair] = ph.resample_taps(*pair)
        return self[pair]


TABLES = Tables()


def lib_format(f):
    return ph.stream_format(rate=f.rate, encoding=f.enc, gain=f.gain)


def begin_group(rt, slot, group, chunk):
    n = len(group)
    arr, keep = (ph.Utterance * n)(), []
    for i, (ids, dur, noise) in enumerate(group):
        arr[i], k = rt._utt(ids, dur, noise, 0.667)
        keep.append(k)
    steps = rt.lib.piper_hip_voice_stream_begin_batch(rt.voice, arr, n, slot, chunk)
    assert steps > 0
    return keep


def mixed_step(rt, slot, n, buf, max_bytes=None):
    """one stream_next_batch_mixed → (n_samples, byte_off, bytes up to the step's total)"""
    got, off = (C.c_int64 * n)(), (C.c_int64 * n)()
    ph._check(rt.lib.piper_hip_voice_stream_next_batch_mixed(rt.voice, slot, buf.ctypes.data_as(ph.c_vp), buf.size if max_bytes is None else max_bytes,
                                                             got, off))
    counts, offs = [int(x) for x in got], [int(x) for x in off]
    return counts, offs, buf[:step_total(rt, slot, counts, offs)].copy()


def step_total(rt, slot, counts, offs):
    total = 0
    for r, c in enumerate(counts):
        if c:
            total = offs[r] + c * np.dtype(rt.stream_item_format(slot, r).dtype).itemsize
    return total


def float_group(rt, group, chunk, slot=8, drop=None):
    """the fp32 twin of a group: per item the chunks of its steps, a dropped item's up to the drop"""
    per = [[] for _ in group]
    for k, chunks in enumerate(rt.synthesize_stream_batch(group, 0.667, chunkFrames=chunk, slot=slot)):
        for i, c in enumerate(chunks):
            if c.size:
                per[i].append(c)
        if drop and k == drop[1] - 1:
            rt.stream_drop(slot, drop[0])
    return per


def run_mixed_group(rt, group, formats, chunk, slot=8, drop=None):
    keep = begin_group(rt, slot, group, chunk)
    rt.stream_set_mixed(slot)
    rt.stream_item_formats(slot, [lib_format(f) for f in formats])
    cap = rt.stream_step_capacity_bytes(slot)
    buf, steps = np.empty(cap, np.uint8), []
    for k in range(1024):
        st = mixed_step(rt, slot, len(group), buf)
        if not any(st[0]):
            break
        steps.append(st)
        if drop and k == drop[1] - 1:
            rt.stream_drop(slot, drop[0])
    del keep
    return steps, cap


def check_steps(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1], (what, k, g[:2], w[:2])
        assert mr.same_step(g, w), (what, k)


def group_sessions(per, formats, drop=None):
    return [dict(row=i, start=0, chunks=per[i], fmt=formats[i], finished=not (drop and drop[0] == i)) for i in range(len(per))]


# ---- 1. a pool with a take-over

POOL_FORMATS = {"S": Format(8000, "mulaw", 1.0), "E": Format(48000, "s16", 0.5), "A": Format(0, "f32", 1.0), "B": Format(16000, "alaw", 1.0)}
POOL_START = {"S": (0, 0), "E": (1, 0), "A": (2, 0), "B": (0, 2)}  # session → (row, first step)


@pytest.fixture(scope="module")
def pool_utts(rt_medium):
    g = ragged_group(rt_medium.cfg)
    return {"S": item(rt_medium.cfg, 5, 9), "E": g[2], "A": g[1], "B": g[0]}  # 15, 84, 30 and 42 frames


def run_pool(rt, utts, formats, step):
    """Capacity 4, chunk 8: S, E and A join; after two steps S has finished and B takes its row. formats: {session: lib format} or None
    (a pool that is not mixed); step(pool) → whatever one step returns, falsy when the pool is idle."""
    pool = rt.stream_pool(10, 4, chunkFrames=CHUNK, work_slot=11, mixed=formats is not None)
    fm = (lambda names: [formats[s] for s in names]) if formats is not None else (lambda names: None)
    joined = pool.join([utts["S"], utts["E"], utts["A"]], 0.667, formats=fm("SEA"))
    assert [i for i, _ in joined] == [0, 1, 2]
    steps, caps = [], []
    for k in range(64):
        if k == 2:
            assert pool.free_rows == 2  # S (15 frames) has finished
            (row, samples), = pool.join([utts["B"]], 0.667, formats=fm("B"))
            assert row == 0
            joined.append((row, samples))
        if formats is not None:
            caps.append(rt.stream_step_capacity_bytes(10))
        out = step(pool)
        if not out:
            break
        steps.append(out)
    pool.close()
    return steps, [s for _, s in joined], caps


def raw_step(pool):
    st = pool.step_mixed(raw=True)
    return st if any(st[0]) else None


@pytest.fixture(scope="module")
def pool_twin(rt_medium, pool_utts):
    """fp32 chunks per session from a plain float pool of the same sessions, computed once"""
    steps, n, _ = run_pool(rt_medium, pool_utts, None, lambda pool: pool.step())
    per = {s: [] for s in "SEAB"}
    for k, out in enumerate(steps):
        for row, c in out.items():
            per[{0: "S" if k < 2 else "B", 1: "E", 2: "A"}[row]].append(c)
    return per, dict(zip("SEAB", n))


def pool_sessions(per, formats, **extra):
    return [dict(row=POOL_START[s][0], start=POOL_START[s][1], chunks=per[s], fmt=formats[s], **extra.get(s, {})) for s in "SEAB"]


def test_pool_with_a_take_over(rt_medium, pool_utts, pool_twin):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    per, n_flt = pool_twin
    assert [len(per[s]) for s in "SEAB"] == [2, 11, 4, 6]
    steps, samples, caps = run_pool(rt, pool_utts, {s: lib_format(f) for s, f in POOL_FORMATS.items()}, raw_step)
    assert samples == [mr.total_samples(n_flt[s], POOL_FORMATS[s], rate) for s in "SEAB"]  # join reports J(N_i) at the item's rate
    want = mr.expected(pool_sessions(per, POOL_FORMATS), 4, rate, hop, CHUNK, TABLES)
    check_steps(steps, want, "pool")
    share = {s: mr.step_bound_bytes(POOL_FORMATS[s], rate, CHUNK * hop) for s in "SEAB"}
    assert caps[0] == caps[1] == share["S"] + share["E"] + share["A"] and caps[2] == share["B"] + share["E"] + share["A"]
    assert all(st[2].size <= cap for st, cap in zip(steps, caps))
    # B's first chunk: had it seen S's last samples before its own sample 0, these bytes would differ
    haunted = mr.expected(pool_sessions(per, POOL_FORMATS, B=dict(inherit=np.concatenate(per["S"]))), 4, rate, hop, CHUNK, TABLES)
    assert not mr.same_step(steps[2], haunted[2]) and mr.same_step(steps[3], haunted[3])


# ---- 2. a group with a drop

GROUP_FORMATS = [Format(32000, "s16", 1.0),   # the largest table, L = 640
                 Format(8000, "alaw", 1.0),   # the longest filter, P = 134; odd byte counts in front of a wider row
                 Format(0, "s16", 1.0), Format(0, "mulaw", 1.0), Format(11025, "f32", 1.0)]


@pytest.fixture(scope="module")
def group_twin(rt_medium):
    return float_group(rt_medium, ragged_group(rt_medium.cfg), CHUNK, drop=(1, 2))


def test_group_with_a_drop(rt_medium, group_twin):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    assert rr.ratio(rate, 32000)[0] == 640 and rr.ratio(rate, 8000)[2] == 134
    assert [len(p) for p in group_twin] == [6, 2, 11, 9, 42]
    steps, cap = run_mixed_group(rt, ragged_group(rt.cfg), GROUP_FORMATS, CHUNK, drop=(1, 2))
    want = mr.expected(group_sessions(group_twin, GROUP_FORMATS, drop=(1, 2)), 5, rate, hop, CHUNK, TABLES)
    check_steps(steps, want, "group")
    assert any(st[0][1] % 2 == 1 and st[1][2] == ((st[0][1] + st[1][1] + 3) & ~3) for st in steps[:2])  # an odd A-law row was padded
    assert cap == sum(mr.step_bound_bytes(f, rate, CHUNK * hop) for f in GROUP_FORMATS) and all(st[2].size <= cap for st in steps)


# ---- 3. the low preset: a 16 000 Hz voice

LOW_FORMATS = [Format(48000, "s16", 1.0),   # L = 3: the pair whose table the uniform kernel stages in LDS
               Format(8000, "mulaw", 1.0), Format(44100, "s16", 0.5)]


def test_low_preset(backend):
    cfg = ph.voice_config("low")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    try:
        assert cfg.sample_rate == 16000 and rr.ratio(16000, 48000)[0] == 3
        group = ragged_group(cfg)[:3]
        per = float_group(rt, group, CHUNK)
        steps, _ = run_mixed_group(rt, group, LOW_FORMATS, CHUNK)
        check_steps(steps, mr.expected(group_sessions(per, LOW_FORMATS), 3, 16000, cfg.hop, CHUNK, TABLES), "low")
        # the same through synthesize_stream_batch(formats=): every item's chunks in its own dtype
        typed = list(rt.synthesize_stream_batch(group, 0.667, chunkFrames=CHUNK, slot=8, formats=[lib_format(f) for f in LOW_FORMATS]))
        assert len(typed) == len(steps)
        for i, f in enumerate(LOW_FORMATS):
            got = np.concatenate([s[i] for s in typed])
            assert got.dtype == mr.DTYPE[f.enc] and np.array_equal(got, mr.whole(np.concatenate(per[i]), f, 16000, TABLES))
    finally:
        rt.close()


# ---- 4. a chunk of one frame

def test_chunk_of_one_frame(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    group = [(kd.FIXTURE_IDS[:5], [1] * 5, kd.sym(SD + 900 + k, (rt.cfg.inter, 5), 1.7320508)) for k in range(2)]
    formats = [Format(8000, "mulaw", 1.0), Format(48000, "s16", 1.0)]
    per = float_group(rt, group, 1)
    assert [len(p) for p in per] == [5, 5]
    steps, _ = run_mixed_group(rt, group, formats, 1)
    check_steps(steps, mr.expected(group_sessions(per, formats), 2, rate, hop, 1, TABLES), "one frame")
    L, M, P = rr.ratio(rate, 8000)
    assert hop < 2 * P and steps[0][0][0] < rr.count(hop, L, M)  # short against the filter; the first step holds outputs back


# ---- 5. a mixed slot whose rows all carry one format is the uniform slot

@pytest.mark.parametrize("f", [Format(8000, "mulaw", 1.0), Format(48000, "s16", 1.0)], ids=lambda f: "%d-%s" % f[:2])
def test_uniform_twin(rt_medium, pool_utts, f):
    rt = rt_medium
    # the existing uniform pool: stream_set_rate plus the matching step call
    pool = rt.stream_pool(10, 4, chunkFrames=CHUNK, work_slot=11, rate=f.rate)
    n_uni = [s for _, s in pool.join([pool_utts["S"], pool_utts["E"], pool_utts["A"]], 0.667)]
    uni = []
    for k in range(64):
        if k == 2:
            n_uni += [s for _, s in pool.join([pool_utts["B"]], 0.667)]
        out = pool.step(pcm=True) if f.enc == "s16" else pool.step(encoding=f.enc)
        if not out:
            break
        uni.append(out)
    pool.close()
    def typed_step(p):
        out = p.step_mixed()
        return out if any(c.size for c in out) else None

    steps, n_mix, _ = run_pool(rt, pool_utts, {s: lib_format(f) for s in "SEAB"}, typed_step)
    assert n_mix == n_uni and len(steps) == len(uni)
    for k, (m, u) in enumerate(zip(steps, uni)):
        for row in range(4):
            if row not in u:  # (a row nobody has taken yet has no format: its empty array is the default's)
                assert m[row].size == 0, (k, row)
                continue
            assert m[row].dtype == u[row].dtype and np.array_equal(m[row], u[row]), (k, row)


# ---- 6. state rules: every refusal consumes nothing, and the next valid step is the expected one

def refused(exc, rc_call):
    with pytest.raises(exc):
        ph._check(rc_call())


def test_state_rules(rt_medium):
    rt, lib, v = rt_medium, rt_medium.lib, rt_medium.voice
    hop, rate = rt.cfg.hop, rt.cfg.sample_rate
    group = ragged_group(rt.cfg)[1::-1]  # F = 30 and 42
    formats = [Format(8000, "mulaw", 1.0), Format(0, "s16", 0.5)]
    per = float_group(rt, group, CHUNK, slot=8)
    want = mr.expected(group_sessions(per, formats), 2, rate, hop, CHUNK, TABLES)
    ARG, SHAPE, UNSUP = ph.InvalidArgument, ph.ShapeMismatch, ph.UnsupportedOp
    got2, off2 = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    fbuf, ibuf, bbuf = np.empty(2 * CHUNK * hop, np.float32), np.empty(2 * CHUNK * hop, np.int16), np.empty(2 * CHUNK * hop, np.uint8)
    one = C.c_int64()

    # where set_mixed is refused: no stream, a single stream, a slot with a rate, a second call
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 12))
    u, keep1 = rt._utt(*group[0], 0.667)
    assert lib.piper_hip_voice_stream_begin(v, C.byref(u), 3, CHUNK) == 4
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 3))
    ph._check(lib.piper_hip_voice_stream_next(v, 3, fbuf.ctypes.data_as(ph.c_f32p), fbuf.size, C.byref(one)))
    assert one.value == CHUNK * hop and np.array_equal(fbuf[:one.value], per[0][0])  # the single stream goes on as it was
    keep = begin_group(rt, 8, group, CHUNK)
    rt.stream_set_rate(8, 8000)
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 8))
    assert rt.stream_rate(8) == 8000
    keep = begin_group(rt, 8, group, CHUNK)  # a new begin: the voice's own rate, not mixed
    refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch_mixed(v, 8, bbuf.ctypes.data_as(ph.c_vp), bbuf.size, got2, off2))
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_formats(v, 8, ph._formats([None]), 1))  # not mixed yet
    refused(ARG, lambda: lib.piper_hip_voice_stream_step_capacity_bytes(v, 8))
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_format(v, 8, 0, C.byref(ph.StreamFormat())))
    rt.stream_set_mixed(8)
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 8))
    # the rate calls of a uniform slot
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_rate(v, 8, 8000))
    refused(ARG, lambda: lib.piper_hip_voice_stream_rate(v, 8))
    refused(ARG, lambda: lib.piper_hip_voice_stream_step_capacity(v, 8))
    # formats: every bad one is refused whole, and nothing changes
    rt.stream_item_formats(8, [lib_format(f) for f in formats])
    bad = [(ARG, ph.StreamFormat(0, 4, 1.0)), (ARG, ph.StreamFormat(0, -1, 1.0)), (ARG, ph.StreamFormat(0, 0, -1.0)),
           (ARG, ph.StreamFormat(0, 0, float("nan"))), (ARG, ph.StreamFormat(0, 0, float("inf"))), (ARG, ph.StreamFormat(8000, 3, 0.5)),
           (UNSUP, ph.StreamFormat(12345, 0, 1.0)), (UNSUP, ph.StreamFormat(7999, 1, 1.0))]
    for exc, b in bad:
        arr = (ph.StreamFormat * 2)(ph.StreamFormat(48000, 3, 1.0), b)
        refused(exc, lambda: lib.piper_hip_voice_stream_item_formats(v, 8, arr, 2))
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_formats(v, 8, None, 1))
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_formats(v, 8, ph._formats([None]), 0))
    held = [rt.stream_item_format(8, i) for i in range(2)]
    assert [(h.out_rate, h.encoding, h.gain) for h in held] == [(8000, ph.ENC_MULAW, 1.0), (0, ph.ENC_S16, 0.5)]
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_format(v, 8, 2, C.byref(ph.StreamFormat())))
    cap = rt.stream_step_capacity_bytes(8)
    assert cap == ((ph.resample_step_bound(rate, 8000, CHUNK * hop) + 3) & ~3) + CHUNK * hop * 2  # the header's formula
    assert cap == sum(mr.step_bound_bytes(f, rate, CHUNK * hop) for f in formats)

    def other_steps():
        """every step call but the mixed one, on the mixed slot"""
        p = lambda a, t: a.ctypes.data_as(t)
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch(v, 8, p(fbuf, ph.c_f32p), fbuf.size, got2))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch_pcm16(v, 8, None, p(ibuf, ph.c_i16p), ibuf.size, got2))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch_g711(v, 8, None, ph.G711_MULAW, p(bbuf, ph.c_u8p), bbuf.size, got2))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next(v, 8, p(fbuf, ph.c_f32p), fbuf.size, C.byref(one)))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_pcm16(v, 8, None, p(ibuf, ph.c_i16p), ibuf.size, C.byref(one)))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_g711(v, 8, None, ph.G711_MULAW, p(bbuf, ph.c_u8p), bbuf.size, C.byref(one)))
        refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch_mixed(v, 8, None, 1 << 20, got2, off2))  # no buffer
        total = want[done][2].size
        refused(SHAPE, lambda: lib.piper_hip_voice_stream_next_batch_mixed(v, 8, p(buf, ph.c_vp), total - 1, got2, off2))  # one byte short

    buf, done, steps = np.empty(cap, np.uint8), 0, []
    other_steps()
    st = mixed_step(rt, 8, 2, buf, max_bytes=want[0][2].size)  # a buffer of exactly the step's total is enough
    assert mr.same_step(st, want[0])  # nothing was consumed by the refused calls
    steps.append(st)
    done = 1
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_formats(v, 8, ph._formats([None]), 1))  # a row keeps its format
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 8))
    other_steps()
    for k in range(64):
        st = mixed_step(rt, 8, 2, buf)
        if not any(st[0]):
            break
        steps.append(st)
    check_steps(steps, want, "state rules")
    assert all(s[2].size <= cap for s in steps)
    assert mixed_step(rt, 8, 2, buf)[0] == [0, 0]  # the end, again

    # a begin after a mixed stream is not mixed
    keep = begin_group(rt, 8, group, CHUNK)
    refused(ARG, lambda: lib.piper_hip_voice_stream_next_batch_mixed(v, 8, buf.ctypes.data_as(ph.c_vp), buf.size, got2, off2))
    assert rt.stream_rate(8) == rate and rt.stream_step_capacity(8) == 2 * CHUNK * hop
    ph._check(lib.piper_hip_voice_stream_next_batch(v, 8, fbuf.ctypes.data_as(ph.c_f32p), fbuf.size, got2))
    assert list(got2) == [CHUNK * hop] * 2 and np.array_equal(fbuf, np.concatenate([per[0][0], per[1][0]]))

    # a pool: set_mixed before the first join only; the join brings the formats
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11)
    refused(ARG, lambda: lib.piper_hip_voice_stream_pool_join_formats(v, 10, C.byref(u), 1, 11, ph._formats([None]), None, None))  # not mixed
    assert pool.free_rows == 2
    pool.join([group[0]], 0.667)
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 10))  # joined already
    assert np.array_equal(pool.step()[0], per[0][0])
    pool.close()
    pool = rt.stream_pool(10, 2, chunkFrames=CHUNK, work_slot=11, mixed=True)
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_mixed(v, 10))
    refused(ARG, lambda: lib.piper_hip_voice_stream_set_rate(v, 10, 8000))
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_formats(v, 10, ph._formats([None]), 1))  # a pool's formats come with the join
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_format(v, 10, 0, C.byref(ph.StreamFormat())))  # a free row
    assert rt.stream_step_capacity_bytes(10) == 0  # free rows count 0
    for exc, b in bad:  # a refused join leaves nothing joined
        arr = (ph.StreamFormat * 1)(b)
        refused(exc, lambda: lib.piper_hip_voice_stream_pool_join_formats(v, 10, C.byref(u), 1, 11, arr, None, None))
    refused(ARG, lambda: lib.piper_hip_voice_stream_pool_join_formats(v, 10, C.byref(u), 1, 11, None, None, None))
    assert pool.free_rows == 2 and pool.step_mixed(raw=True)[0] == [0, 0]
    (row0, n0), = pool.join([group[0]], 0.667, formats=[lib_format(formats[0])])
    (row1, n1), = pool.join([group[1]], 0.667)  # a plain join on a mixed pool: the default format
    assert (row0, row1) == (0, 1) and n0 == ph.resample_count(rate, 8000, 30 * hop) and n1 == 42 * hop
    d = rt.stream_item_format(10, 1)
    assert (d.out_rate, d.encoding, d.gain) == (0, ph.ENC_S16, 1.0)
    assert rt.stream_step_capacity_bytes(10) == mr.step_bound_bytes(formats[0], rate, CHUNK * hop) + CHUNK * hop * 2
    refused(ARG, lambda: pool.step())
    refused(ARG, lambda: pool.step(pcm=True))
    refused(ARG, lambda: pool.step(encoding="mulaw"))
    pw = mr.expected(group_sessions(per, [formats[0], Format()]), 2, rate, hop, CHUNK, TABLES)
    assert mr.same_step(pool.step_mixed(raw=True), pw[0])
    pool.drop(0)  # stream_drop works as before: the row is free, the other goes on
    refused(ARG, lambda: lib.piper_hip_voice_stream_item_format(v, 10, 0, C.byref(ph.StreamFormat())))
    st = pool.step_mixed(raw=True)
    assert st[0] == [0, CHUNK * hop] and st[1][1] == 0 and np.array_equal(st[2], pw[1][2][pw[1][1][1]:])
    pool.close()
    del keep, keep1
