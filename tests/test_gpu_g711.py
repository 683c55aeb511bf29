"""GPU: G.711 output — the per-op entry point at equal rates and with a filter, unaligned ends, whole items on plain, ragged and bounded
slots, and μ-law / A-law steps of single, grouped and pooled streams. A byte is law(s) of the int16 sample the PCM contracts define
(include/piper_hip.h "G.711 output"), so every comparison is integer equality against the audioop-made table (tests/golden/g711.npz)
applied to what the PCM entry points return and to the numpy restatement of those contracts."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import g711_ref as g
import katdata as kd
import pcm_ref
import piper_hip as ph
import resample_ref as rr
from test_gpu_resample import inputs, item, ref_pcm, ref_pcm_normalized
from test_gpu_stream_batch import SD, ragged_group

pytestmark = pytest.mark.gpu

LAWS = ["mulaw", "alaw"]
GUARD = 0x5A
FILTER_PAIRS = [(22050, 8000), (16000, 8000), (22050, 48000)]
law_of = g.table_encode  # int16 → bytes through the golden table


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


def u8p(a):
    return a.ctypes.data_as(ph.c_u8p)


# ---- per-op

def every_sample_vector():
    """(k + 0.5·sign k) / 32767 for every k — the middle of the floats that convert to k — then the adversarial vector of the PCM tests"""
    k = np.arange(-32767, 32768, dtype=np.float64)
    return np.concatenate([((k + 0.5 * np.sign(k)) / 32767.0).astype(np.float32), pcm_ref.adversarial_vector()])


@pytest.mark.parametrize("law", LAWS)
def test_per_op_equal_rates(backend, law):
    x = every_sample_vector()
    want = law_of(pcm_ref.pcm16_reference(x), law)
    pcm = pcm_ref.pcm16_reference(x)
    assert np.array_equal(np.unique(pcm[:65535]), np.arange(-32767, 32768))  # every int16 the contract can produce …
    assert np.unique(want).size == (255 if law == "mulaw" else 256)  # … hence every code of the law: no segment is left untested
    buf = backend.uploadFloat32(x)
    for count in (0, 1, 2, 3, 4, 5, 7, 255, 257, 1029, x.size):
        out = backend.g711F32(buf, law, 22050, 22050, count=count)
        assert out.count == count and out.ptr and out.dtype == np.uint8, count
        if count:
            assert np.array_equal(backend.downloadUint8(out), want[:count]), count
        out.free()
    for gain in (0.5, 1.7):
        out = backend.g711F32(buf, law, gain=gain)  # no rates: not a filter
        assert np.array_equal(backend.downloadUint8(out), law_of(pcm_ref.pcm16_reference(x, gain), law)), gain
        out.free()
    out = backend.g711F32(buf, law, 12345, 12345, count=1029)  # equal rates are not looked up in the list
    assert np.array_equal(backend.downloadUint8(out), want[:1029])
    out.free()
    with pytest.raises(ph.InvalidArgument):
        backend.g711F32(buf, law, gain=-1.0)
    with pytest.raises(ph.InvalidArgument):
        backend.g711F32(buf, 3)
    with pytest.raises(ph.UnsupportedOp):
        backend.g711F32(buf, law, 22050, 12345)
    buf.free()


@pytest.mark.parametrize("pair", FILTER_PAIRS, ids=lambda p: "%d-%d" % p)
def test_per_op_with_a_filter(backend, pair):
    L, M, P = rr.ratio(*pair)
    for count in (0, 1, 2, P // 2 - 1, P // 2, P, 255, 257, 1029, 40000):
        for name, x in inputs(max(count, 1)).items():
            buf = backend.uploadFloat32(x)
            pcm = ref_pcm(x[:count], pair) if count else np.empty(0, np.int16)
            for law in LAWS:
                out = backend.g711F32(buf, law, *pair, count=count)
                assert out.count == rr.count(count, L, M) == pcm.size and out.ptr, (count, name, law)
                if count:
                    assert np.array_equal(backend.downloadUint8(out), law_of(pcm, law)), (count, name, law)
                out.free()
            buf.free()
    x = inputs(1029)["adversarial"]
    buf = backend.uploadFloat32(x)
    for gain in (0.5, 1.7):
        out = backend.g711F32(buf, "alaw", *pair, gain=gain)
        assert np.array_equal(backend.downloadUint8(out), law_of(ref_pcm(x, pair, gain), "alaw")), gain
        out.free()
    buf.free()


@pytest.mark.parametrize("pair", [(22050, 22050), (22050, 8000)], ids=lambda p: "%d-%d" % p)
def test_per_op_unaligned_ends(backend, pair):
    """x 4 or 12 bytes into its buffer, *out 1, 2, 3 or 5 bytes into a box of 0x5A: the bytes land there and the guard bytes on both sides
    stay — a word store that covered a byte outside the row would show here."""
    x = inputs(3 + 1029)["noise"]
    buf = backend.uploadFloat32(x)
    for count in (1029, 3):
        J = count if pair[0] == pair[1] else rr.count(count, *rr.ratio(*pair)[:2])
        for x_off in (1, 3):
            pcm = pcm_ref.pcm16_reference(x[x_off:x_off + count]) if pair[0] == pair[1] else ref_pcm(x[x_off:x_off + count], pair)
            for lead in (1, 2, 3, 5):
                for law in LAWS:
                    size = (lead + J + 24 + 3) // 4 * 4
                    box = backend.uploadFloat32(np.full(size, GUARD, np.uint8).view(np.float32))
                    out = backend.g711F32(int(buf.ptr) + 4 * x_off, law, *pair, count=count, out=int(box.ptr) + lead)
                    assert out.ptr == int(box.ptr) + lead and out.count == J and not out.owned
                    got = backend.downloadUint8(box, size)
                    what = (count, x_off, lead, law)
                    assert np.all(got[:lead] == GUARD) and np.all(got[lead + J:] == GUARD), what
                    assert np.array_equal(got[lead:lead + J], law_of(pcm, law)), what
                    box.free()
    buf.free()


# ---- whole items

def rate_count(rt, rate, n):
    return n if rate == rt.cfg.sample_rate else ph.resample_count(rt.cfg.sample_rate, rate, n)


def ref_items(rt, rate, items, gain=1.0, normalize=False):
    """the PCM contract in numpy for each item of fp32 audio, back to back"""
    pair = (rt.cfg.sample_rate, rate)
    if rate == rt.cfg.sample_rate:
        return pcm_ref.pcm16_items(items, gain, normalize)
    f = ref_pcm_normalized if normalize else ref_pcm
    return np.concatenate([f(it, pair, gain) for it in items])


@pytest.mark.parametrize("rate", [8000, 22050])
def test_plain_slot_in_any_order(rt_medium, rate):
    rt = rt_medium
    ids, dur, noise = kd.FIXTURE_IDS, [3] * 14, kd.sym(SD + 700, (rt.cfg.inter, 42), 1.7320508)
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    first = rt.collect_g711(5, "mulaw", rate=rate)  # before any other collect
    audio = rt.collect(5)
    pcm_native = rt.collect_pcm16(5)
    a_first = rt.collect_g711(5, "alaw", rate=rate)
    pcm = rt.collect_pcm16(5, rate=rate)
    n = rate_count(rt, rate, 10752)
    assert audio.size == 10752 and first.size == a_first.size == pcm.size == n and first.dtype == np.uint8
    assert np.array_equal(pcm, ref_items(rt, rate, [audio])) and np.array_equal(pcm_native, ph.pcm16(audio))
    for law, got in (("mulaw", first), ("alaw", a_first)):
        assert np.array_equal(got, law_of(pcm, law)), law  # law(·) of what the PCM entry point returns, which is the reference's
        assert np.array_equal(got, ph.g711_encode(pcm, law)), law
        assert np.array_equal(rt.collect_g711(5, law, rate=rate), got), law  # the fp32 audio stays in the plan
    assert np.array_equal(rt.collect(5), audio)
    for law in LAWS:
        assert np.array_equal(rt.collect_g711(5, law, gain=0.5, rate=rate), law_of(ref_items(rt, rate, [audio], 0.5), law))
        norm = rt.collect_g711(5, law, gain=0.7, normalize=True, rate=rate)
        assert np.array_equal(norm, law_of(rt.collect_pcm16(5, gain=0.7, normalize=True, rate=rate), law))
        assert np.array_equal(norm, law_of(ref_items(rt, rate, [audio], 0.7, True), law))
        assert rt.peaks(5).tolist() == [float(np.abs(audio).max())]
    pinned = rt.pinned_empty(n // 4 + 8).view(np.uint8)  # a destination the caller page-locked takes the kernel's stores
    pinned[:] = 0xA7
    got = rt.collect_g711(5, "alaw", out=pinned, rate=rate)
    assert np.array_equal(got, a_first) and np.all(pinned[n:] == 0xA7)
    for law, want in (("mulaw", first), ("alaw", a_first)):
        assert np.array_equal(rt.synthesize_g711(ids, dur, law, noise, 0.667, rate=rate), want)  # the one-call entry point
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    with pytest.raises(ph.UnsupportedOp):
        rt.collect_g711(5, "mulaw", rate=12345)
    with pytest.raises(ph.InvalidArgument):
        rt.collect_g711(5, 0, rate=rate)
    small = np.empty(n - 1, np.uint8)
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rt.lib.piper_hip_voice_collect_g711(rt.voice, 5, None, 1, rate, u8p(small), small.size))
    assert np.array_equal(rt.collect_g711(5, "mulaw", rate=rate), first)


@pytest.mark.parametrize("rate", [8000, 22050])
def test_ragged_batch(rt_medium, rate):
    rt, hop = rt_medium, rt_medium.cfg.hop
    group = [item(rt.cfg, n, k) for k, n in enumerate((14, 5, 9))]
    rt.prepare_batch(6, group, 0.667)
    rt.launch(6)
    got = {law: rt.collect_g711(6, law, rate=rate) for law in LAWS}  # the collecting calls come first
    audio = rt.collect(6)
    per, _ = rt.prepared_samples(6)
    assert per == [42 * hop, 15 * hop, 27 * hop]
    starts = np.concatenate([[0], np.cumsum([rate_count(rt, rate, p) for p in per])])
    if rate == 8000:
        assert starts.tolist() == [0, 3901, 5295, 7803] and any(s % 4 for s in starts[:3])  # an item begins in the middle of a word
    items = np.split(audio, np.cumsum(per)[:-1])
    pcm = rt.collect_pcm16(6, rate=rate)
    assert np.array_equal(pcm, ref_items(rt, rate, items))
    for law in LAWS:
        assert got[law].size == starts[-1] and np.array_equal(got[law], law_of(pcm, law)), law
        norm = rt.collect_g711(6, law, gain=0.5, normalize=True, rate=rate)
        assert np.array_equal(norm, law_of(ref_items(rt, rate, items, 0.5, True), law)), law
        assert rt.peaks(6).tolist() == [float(np.abs(it).max()) for it in items]
    assert np.array_equal(rt.collect(6), audio)


@pytest.mark.parametrize("rate", [8000, 22050])
def test_bounded_slot(rt_medium, rate):
    rt = rt_medium
    utts = [(kd.FIXTURE_IDS * 2, None), (kd.FIXTURE_IDS, None)]
    kw = dict(noise_mode="device", seed=4242)
    probe = rt.predict_durations(utts, **kw)
    bound = max(int(d.sum()) for d, _ in probe) + 5
    for slot in (6, 7):  # two identically prepared slots
        rt.prepare_batch_bounded(slot, utts, bound, **kw)
        rt.launch(slot)
    got = rt.collect_g711(6, "alaw", rate=rate)  # alone: the collecting call of this slot
    audio = rt.collect(7)
    per, total = rt.prepared_samples(7)
    assert rt.prepared_samples(6) == (per, total) and audio.size == total
    items = np.split(audio, np.cumsum(per)[:-1])
    assert np.array_equal(got, law_of(ref_items(rt, rate, items), "alaw"))
    assert np.array_equal(rt.collect_g711(6, "mulaw", rate=rate), law_of(rt.collect_pcm16(7, rate=rate), "mulaw"))


def test_low_preset_16000_to_8000(backend):
    cfg = ph.voice_config("low")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    try:
        ids, dur = kd.FIXTURE_IDS, [3] * 14
        rt.prepare(1, ids, dur, kd.sym(SD + 740, (cfg.inter, 42), 1.7320508), 0.667)
        rt.launch(1)
        audio = rt.collect(1)
        for law in LAWS:
            got = rt.collect_g711(1, law, rate=8000)
            assert got.size == audio.size // 2 and np.array_equal(got, law_of(ref_pcm(audio, (16000, 8000)), law)), law
            assert np.array_equal(rt.collect_g711(1, law), law_of(ph.pcm16(audio), law)), law
    finally:
        rt.close()


# ---- streams: the oracle is a twin stream of the same items delivering int16 (tests/test_gpu_resample.py and test_gpu_pcm16.py check those)

RATES = [8000, None]  # None: the voice's own


def whole_item(rt, rate, flt_steps, law):
    """the whole-item conversion of the fp32 samples a row's float twin delivered, as tests/test_gpu_resample.py takes it (a window's
    samples are those of the whole-utterance run within the waveform tolerance, not bit for bit, so the stream's own are the input)"""
    return law_of(ref_items(rt, rate or rt.cfg.sample_rate, [np.concatenate(flt_steps)]), law)


def same_steps(law_steps, pcm_steps, law, what):
    assert [c.size for c in law_steps] == [c.size for c in pcm_steps], what
    for k, (b, p) in enumerate(zip(law_steps, pcm_steps)):
        assert b.dtype == np.uint8 and np.array_equal(b, law_of(p, law)), (what, k)


@pytest.fixture(scope="module")
def single_twin(rt_medium):
    ids, dur, noise = ragged_group(rt_medium.cfg)[3]
    return {(rate, c): list(rt_medium.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=c, slot=3, pcm=True, rate=rate))
            for rate in RATES for c in (1, 3)}


@pytest.fixture(scope="module")
def single_float(rt_medium):
    ids, dur, noise = ragged_group(rt_medium.cfg)[3]
    return {c: list(rt_medium.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=c, slot=3)) for c in (1, 3)}


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("chunk", [1, 3])
def test_single_stream(rt_medium, single_twin, single_float, rate, chunk):
    rt = rt_medium
    ids, dur, noise = ragged_group(rt.cfg)[3]  # F = 70: not a multiple of 3
    pcm = single_twin[(rate, chunk)]
    assert len(pcm) == -(-70 // chunk)
    for law in LAWS:
        got = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3, rate=rate, encoding=law))
        same_steps(got, pcm, law, (rate, chunk, law))
        assert np.array_equal(np.concatenate(got), whole_item(rt, rate, single_float[chunk], law)), (rate, chunk, law)


@pytest.mark.parametrize("rate", RATES)
def test_single_stream_alternating_pcm_and_g711_steps(rt_medium, single_twin, rate):
    """The law is an argument of the step: PCM, μ-law and A-law steps (and float steps on a slot at the voice's own rate) in turn consume
    the stream alike; decoded through the table they are the twin's sequence."""
    rt, lib = rt_medium, rt_medium.lib
    ids, dur, noise = ragged_group(rt.cfg)[3]
    twin = single_twin[(rate, 3)]
    u, keep = rt._utt(ids, dur, noise, 0.667)
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 3) == 24
    if rate:
        rt.stream_set_rate(3, rate)
    cap = rt.stream_step_capacity(3)
    bbuf, sbuf, fbuf, got = np.empty(cap, np.uint8), np.empty(cap, np.int16), np.empty(cap, np.float32), C.c_int64()
    kinds = ["pcm", "mulaw", "alaw"] + ([] if rate else ["float"])
    for k, want in enumerate(twin):
        kind = kinds[k % len(kinds)]
        if kind == "pcm":
            ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, sbuf.ctypes.data_as(ph.c_i16p), cap, C.byref(got)))
            assert got.value == want.size and np.array_equal(sbuf[:got.value], want), k
        elif kind == "float":
            ph._check(lib.piper_hip_voice_stream_next(rt.voice, 3, fbuf.ctypes.data_as(ph.c_f32p), cap, C.byref(got)))
            assert got.value == want.size and np.array_equal(ph.pcm16(fbuf[:got.value]), want), k
        else:
            ph._check(lib.piper_hip_voice_stream_next_g711(rt.voice, 3, None, g.LAWS[kind], u8p(bbuf), cap, C.byref(got)))
            assert got.value == want.size and np.array_equal(bbuf[:got.value], law_of(want, kind)), k
            assert np.array_equal(g.table_decode(bbuf[:got.value], kind), g.table_decode(law_of(want, kind), kind)), k
    ph._check(lib.piper_hip_voice_stream_next_g711(rt.voice, 3, None, 1, u8p(bbuf), cap, C.byref(got)))
    assert got.value == 0  # end of stream


def run_group(rt, group, rate, encoding, chunk=8, drop_after=2, drop_item=1, pcm=True):
    steps = []
    for k, chunks in enumerate(rt.synthesize_stream_batch(group, 0.667, chunkFrames=chunk, slot=8, pcm=pcm, rate=rate, encoding=encoding)):
        steps.append(chunks)
        if k == drop_after - 1:
            rt.stream_drop(8, drop_item)
    return steps


@pytest.fixture(scope="module")
def group_float(rt_medium):
    return run_group(rt_medium, ragged_group(rt_medium.cfg)[1:4], None, None, pcm=False)


@pytest.mark.parametrize("rate", RATES)
def test_ragged_group_with_a_drop(rt_medium, group_float, rate):
    rt = rt_medium
    group = ragged_group(rt.cfg)[1:4]  # F = 30, 84, 70; item 1 dropped after two steps
    pcm = run_group(rt, group, rate, None)
    assert len(pcm) == 9 and len([s for s in pcm if s[1].size]) == 2
    for law in LAWS:
        got = run_group(rt, group, rate, law)
        assert len(got) == len(pcm)
        for i in range(3):
            same_steps([s[i] for s in got], [s[i] for s in pcm], law, (rate, law, i))
        for i in (0, 2):  # the finished rows: the concatenation is the whole-item conversion
            whole = whole_item(rt, rate, [s[i] for s in group_float], law)
            assert np.array_equal(np.concatenate([s[i] for s in got]), whole), (rate, law, i)


def run_pool(rt, utts, rate, encoding, pcm=True):
    """Capacity 4, chunk 8: S (15 frames), E (84) and A (30) join; after two steps S has finished and B (42) takes its row. encoding: a law,
    None for int16, or "mixed": the steps take PCM, μ-law and A-law in turn and are returned as (kind, chunk)."""
    pool = rt.stream_pool(10, 4, chunkFrames=8, work_slot=11, rate=rate)
    joined = pool.join([utts["S"], utts["E"], utts["A"]], 0.667)
    assert [i for i, _ in joined] == [0, 1, 2]
    rows = {0: [], 1: [], 2: [], "B": []}
    for k in range(64):
        if k == 2:
            (row, samples), = pool.join([utts["B"]], 0.667)
            assert row == 0  # the row of a finished session
            joined.append((row, samples))
        kind = (None, "mulaw", "alaw")[k % 3] if encoding == "mixed" else encoding
        out = pool.step(pcm=pcm, encoding=kind)
        if not out:
            break
        for i, c in out.items():
            rows["B" if (i == 0 and k >= 2) else i].append((kind, c) if encoding == "mixed" else c)
    pool.close()
    return rows, [s for _, s in joined]


@pytest.fixture(scope="module")
def pool_utts(rt_medium):
    grp = ragged_group(rt_medium.cfg)
    return {"S": item(rt_medium.cfg, 5, 9), "E": grp[2], "A": grp[1], "B": grp[0]}


@pytest.fixture(scope="module")
def pool_float(rt_medium, pool_utts):
    return run_pool(rt_medium, pool_utts, None, None, pcm=False)[0]


@pytest.mark.parametrize("rate", RATES)
def test_pool_with_a_join_into_a_finished_row(rt_medium, pool_utts, pool_float, rate):
    rt = rt_medium
    pcm, n_pcm = run_pool(rt, pool_utts, rate, None)
    for law in LAWS:
        got, n_got = run_pool(rt, pool_utts, rate, law)
        assert n_got == n_pcm
        for key in (0, 1, 2, "B"):
            same_steps(got[key], pcm[key], law, (rate, law, key))
            assert sum(c.size for c in got[key]) == n_pcm[{0: 0, 1: 1, 2: 2, "B": 3}[key]]
            assert np.array_equal(np.concatenate(got[key]), whole_item(rt, rate, pool_float[key], law)), (rate, law, key)
    mixed, _ = run_pool(rt, pool_utts, rate, "mixed")  # PCM, μ-law and A-law steps in turn on one pool
    for key in (0, 1, 2, "B"):
        assert len(mixed[key]) == len(pcm[key])
        for (kind, c), want in zip(mixed[key], pcm[key]):
            assert np.array_equal(c, want if kind is None else law_of(want, kind)), (rate, key, kind)


# ---- state rules: each refused call consumes nothing, and the stream then finishes correctly

def test_state_rules(rt_medium):
    rt, lib = rt_medium, rt_medium.lib
    hop, rate = rt.cfg.hop, 8000
    pair = (rt.cfg.sample_rate, rate)
    ids, dur, noise = ragged_group(rt.cfg)[1]  # F = 30
    want = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3, rate=rate))
    u, keep = rt._utt(ids, dur, noise, 0.667)
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 8) == 4
    rt.stream_set_rate(3, rate)
    cap = rt.stream_step_capacity(3)
    assert cap == ph.resample_step_bound(*pair, 8 * hop)  # samples, which are bytes here
    buf, got = np.empty(cap, np.uint8), C.c_int64()
    nxt = lib.piper_hip_voice_stream_next_g711
    prm = ph.PcmParams(1.0, 1)
    assert nxt(rt.voice, 3, C.byref(prm), 1, u8p(buf), cap, C.byref(got)) == ph.UnsupportedOp.code  # normalize on a step
    assert nxt(rt.voice, 3, None, 1, u8p(buf), want[0].size - 1, C.byref(got)) == ph.ShapeMismatch.code  # a buffer one sample short
    assert nxt(rt.voice, 3, None, 1, None, 0, C.byref(got)) == ph.InvalidArgument.code  # a rated slot needs a buffer
    for law in (0, 3, -1):
        assert nxt(rt.voice, 3, None, law, u8p(buf), cap, C.byref(got)) == ph.InvalidArgument.code  # a bad law
    parts = []
    for k in range(8):
        ph._check(nxt(rt.voice, 3, None, 1 + k % 2, u8p(buf), cap, C.byref(got)))
        if not got.value:
            break
        parts.append(buf[:got.value].copy())
    assert len(parts) == 4
    for k, (b, p) in enumerate(zip(parts, want)):  # nothing was consumed by the refused calls
        assert np.array_equal(b, law_of(p, LAWS[k % 2])), k
    # a pool and a group take the batch call; the single-stream call is refused on a pool
    pool = rt.stream_pool(10, 2, chunkFrames=8, work_slot=11, rate=rate)
    pool.join([(ids, dur, noise)], 0.667)
    got_n = (C.c_int64 * 2)()
    nxb = lib.piper_hip_voice_stream_next_batch_g711
    assert nxt(rt.voice, 10, None, 1, u8p(buf), cap, C.byref(got)) == ph.InvalidArgument.code
    assert nxb(rt.voice, 10, None, 2, None, 0, got_n) == ph.InvalidArgument.code
    assert nxb(rt.voice, 10, None, 5, u8p(buf), cap, got_n) == ph.InvalidArgument.code
    assert nxb(rt.voice, 10, C.byref(prm), 2, u8p(buf), cap, got_n) == ph.UnsupportedOp.code
    assert nxb(rt.voice, 10, None, 2, u8p(buf), want[0].size - 1, got_n) == ph.ShapeMismatch.code
    with pytest.raises(ph.UnsupportedOp):
        pool.step(encoding="alaw", normalize=True)
    steps = []
    while True:
        out = pool.step(encoding="alaw")
        if not out:
            break
        steps.append(out[0])
    pool.close()
    same_steps(steps, want, "alaw", "pool")


# ---- command line

def test_cli_output_encoding(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    ids = ",".join(str(i) for i in kd.FIXTURE_IDS + kd.FIXTURE_IDS[:5])
    s16, ul, wav = tmp_path / "a.s16le", tmp_path / "b.ul", tmp_path / "b.wav"
    common = ["--phoneme-ids", ids, "--output-rate", "8000", "--volume", "0.8", "--normalize"]
    out = subprocess.run([str(exe)] + common + ["--output-raw", str(s16), "--output-encoding", "s16le"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([str(exe)] + common + ["--output-raw", str(ul), "--output", str(wav), "--output-encoding", "mulaw"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    pcm = np.frombuffer(s16.read_bytes(), "<i2")
    n = ph.resample_count(22050, 8000, 19 * 3 * 256)
    assert pcm.size == n and ul.read_bytes() == g.encode(pcm, "mulaw").tobytes()
    raw = wav.read_bytes()
    assert struct.unpack_from("<HHI", raw, 20) == (7, 1, 8000) and struct.unpack_from("<I", raw, 54)[0] == n
    assert raw[58:58 + n] == ul.read_bytes()
