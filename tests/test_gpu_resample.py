"""GPU: the output rate — the per-op resampler, collect_pcm16 at a rate on plain, ragged and bounded slots, and resampling steps of single,
grouped and pooled streams. Every comparison is exact: both sides start from the same fp32 bits and the library's own filter table, and the
conversion is a contract (include/piper_hip.h "Output rate"; tests/resample_ref.py restates it)."""
import ctypes as C

import numpy as np
import pytest

import katdata as kd
import pcm_ref
import piper_hip as ph
import resample_ref as rr
from test_gpu_stream_batch import SD, ragged_group

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A
OP_PAIRS = [(22050, 8000), (22050, 48000), (22050, 32000), (16000, 8000), (16000, 44100), (16000, 11025)]


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


_tables = {}


def table(pair):
    if pair not in _tables:
        _tables[pair] = (ph.resample_taps(*pair),) + rr.ratio(*pair)[:2]
    return _tables[pair]


def ref_f32(x, pair, j0=0, j1=None):
    tab, L, M = table(pair)
    return rr.apply(x, tab, L, M, j0, j1)


def ref_pcm(x, pair, gain=1.0):
    return pcm_ref.pcm16_reference(ref_f32(x, pair), gain)


def ref_pcm_normalized(x, pair, gain=1.0):
    """normalize = 1 at a rate: the scale comes from the peak of the waveform at the voice's rate, the samples are y's"""
    s, g = pcm_ref.normalize_scale(pcm_ref.peak(x)), pcm_ref.effective_gain(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (ref_f32(x, pair) * s).astype(np.float32)
        if g != 1:
            v = (v * g).astype(np.float32)
        v = np.where(np.isnan(v), np.float32(0.0), np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.float32)
        return np.trunc(v).astype(np.int16)


def same_bits(got, want):
    """float32 arrays equal bit for bit; a NaN matches a NaN (its sign and payload are the adder's business, not the contract's)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def inputs(count):
    rng = np.random.default_rng(count + 11)
    return {"adversarial": np.resize(pcm_ref.adversarial_vector(), count).astype(np.float32),
            "noise": (rng.standard_normal(count) * 0.4).astype(np.float32)}


# ---- per-op

@pytest.mark.parametrize("pair", OP_PAIRS, ids=lambda p: "%d-%d" % p)
def test_per_op_counts(backend, pair):
    """0, 1, 2, around the filter's half length and length, around a tile edge of the conversion, an odd length, and 40 000 samples:
    several blocks and many periods of L."""
    L, M, P = rr.ratio(*pair)
    for count in (0, 1, 2, P // 2 - 1, P // 2, P, 255, 257, 1029, 40000):
        for name, x in inputs(max(count, 1)).items():
            buf = backend.uploadFloat32(x)
            yf = backend.resampleF32(buf, *pair, count=count)
            yp = backend.resamplePcm16F32(buf, *pair, count=count)
            J = rr.count(count, L, M)
            assert yf.count == yp.count == J == ph.resample_count(*pair, count) and yf.ptr and yp.ptr, (count, name)
            if count:
                want = ref_f32(x[:count], pair)
                assert same_bits(backend.downloadFloat32(yf), want), (count, name)
                assert np.array_equal(backend.downloadInt16(yp), pcm_ref.pcm16_reference(want)), (count, name)
            for b in (yf, yp, buf):
                b.free()


@pytest.mark.parametrize("pair", [(22050, 8000), (16000, 44100)], ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("x_off,lead", [(0, 7), (1, 0), (3, 2)])
def test_per_op_unaligned_source_and_destination(backend, pair, x_off, lead):
    """x 4 or 12 bytes into its buffer, *out 14 or 4 bytes into a guarded one (2-byte, not 4-byte aligned): the samples land there and the
    guard words on both sides stay."""
    count = 1029
    x = inputs(x_off + count)["noise"]
    J = rr.count(count, *rr.ratio(*pair)[:2])
    trail = 24 + (lead + J) % 2  # (the guarded box is uploaded as whole floats)
    buf = backend.uploadFloat32(x)
    box = backend.uploadFloat32(np.full(lead + J + trail, GUARD, np.uint16).view(np.float32))
    out = backend.resamplePcm16F32(int(buf.ptr) + 4 * x_off, *pair, count=count, out=int(box.ptr) + 2 * lead)
    assert out.ptr == int(box.ptr) + 2 * lead and out.count == J and not out.owned
    got = backend.downloadInt16(box, lead + J + trail).view(np.uint16)
    assert np.all(got[:lead] == GUARD) and np.all(got[lead + J:] == GUARD)
    assert np.array_equal(got[lead:lead + J].view(np.int16), ref_pcm(x[x_off:], pair))
    box.free()
    buf.free()


@pytest.mark.parametrize("gain", [0.5, 1.7])
def test_per_op_gain(backend, gain):
    pair = (22050, 8000)
    x = inputs(1029)["adversarial"]
    buf = backend.uploadFloat32(x)
    out = backend.resamplePcm16F32(buf, *pair, gain=gain)
    assert np.array_equal(backend.downloadInt16(out), ref_pcm(x, pair, gain))
    with pytest.raises(ph.InvalidArgument):
        backend.resamplePcm16F32(buf, *pair, gain=-1.0)
    with pytest.raises(ph.UnsupportedOp):
        backend.resamplePcm16F32(buf, 22050, 12345)
    out.free()
    buf.free()


def test_per_op_same_rate_is_the_plain_conversion(backend):
    x = inputs(1029)["adversarial"]
    buf = backend.uploadFloat32(x)
    a, b = backend.resamplePcm16F32(buf, 22050, 22050, gain=0.5), backend.pcm16F32(buf, gain=0.5)
    assert a.count == b.count == x.size and np.array_equal(backend.downloadInt16(a), backend.downloadInt16(b))
    f = backend.resampleF32(buf, 16000, 16000)
    assert same_bits(backend.downloadFloat32(f), x)
    for d in (a, b, f, buf):
        d.free()


# ---- whole utterances

def item(cfg, n_ids, seed):
    ids = (kd.FIXTURE_IDS * 4)[:n_ids]
    dur = [3] * n_ids
    return ids, dur, kd.sym(SD + 700 + seed, (cfg.inter, sum(dur)), 1.7320508)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_plain_slot_in_any_order(rt_medium, rate):
    rt = rt_medium
    pair = (rt.cfg.sample_rate, rate)
    ids, dur, noise = kd.FIXTURE_IDS, [3] * 14, kd.sym(SD + 700, (rt.cfg.inter, 42), 1.7320508)
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    first = rt.collect_pcm16(5, rate=rate)  # before any other collect
    audio = rt.collect(5)
    plain = rt.collect_pcm16(5)
    assert audio.size == 10752 and first.size == ph.resample_count(*pair, 10752)
    assert np.array_equal(first, ref_pcm(audio, pair))
    assert np.array_equal(plain, ph.pcm16(audio))
    assert np.array_equal(rt.collect_pcm16(5, rate=rate), first) and np.array_equal(rt.collect(5), audio)  # the fp32 audio stays in the plan
    assert np.array_equal(rt.collect_pcm16(5, gain=0.5, rate=rate), ref_pcm(audio, pair, 0.5))
    assert np.array_equal(rt.collect_pcm16(5, rate=rt.cfg.sample_rate), plain)  # the voice's own rate is not a filter
    norm = rt.collect_pcm16(5, normalize=True, rate=rate)
    assert np.array_equal(norm, ref_pcm_normalized(audio, pair))
    assert rt.peaks(5).tolist() == [float(np.abs(audio).max())]  # the peak means the same at every rate
    pinned = rt.pinned_empty(first.size // 2 + 8).view(np.int16)  # a destination the caller page-locked takes the kernel's stores
    pinned[:] = 0x1234
    got = rt.collect_pcm16(5, out=pinned, rate=rate)
    assert np.array_equal(got, first) and np.all(pinned[first.size:] == 0x1234)
    assert np.array_equal(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=rate), first)  # the one-call entry point
    with pytest.raises(ph.UnsupportedOp):
        rt.collect_pcm16(5, rate=12345)
    small = np.empty(first.size - 1, np.int16)
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rt.lib.piper_hip_voice_collect_pcm16_rate(rt.voice, 5, None, rate, small.ctypes.data_as(ph.c_i16p), small.size))


@pytest.mark.parametrize("rate", [8000, 48000])
def test_ragged_batch(rt_medium, rate):
    rt, hop = rt_medium, rt_medium.cfg.hop
    pair = (rt.cfg.sample_rate, rate)
    group = [item(rt.cfg, n, k) for k, n in enumerate((14, 5, 9))]
    rt.prepare_batch(6, group, 0.667)
    rt.launch(6)
    audio = rt.collect(6)
    per, _ = rt.prepared_samples(6)
    assert per == [42 * hop, 15 * hop, 27 * hop]
    items = np.split(audio, np.cumsum(per)[:-1])
    got = rt.collect_pcm16(6, rate=rate)
    assert np.array_equal(got, np.concatenate([ref_pcm(it, pair) for it in items]))  # packed at J(true length), every sample
    norm = rt.collect_pcm16(6, gain=0.5, normalize=True, rate=rate)
    assert np.array_equal(norm, np.concatenate([ref_pcm_normalized(it, pair, 0.5) for it in items]))
    assert rt.peaks(6).tolist() == [float(np.abs(it).max()) for it in items]
    assert np.array_equal(rt.collect(6), audio)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_bounded_slot(rt_medium, rate):
    rt = rt_medium
    pair = (rt.cfg.sample_rate, rate)
    utts = [(kd.FIXTURE_IDS * 2, None), (kd.FIXTURE_IDS, None)]
    kw = dict(noise_mode="device", seed=4242)
    probe = rt.predict_durations(utts, **kw)
    bound = max(int(d.sum()) for d, _ in probe) + 5
    for slot in (6, 7):  # two identically prepared slots
        rt.prepare_batch_bounded(slot, utts, bound, **kw)
        rt.launch(slot)
    pcm = rt.collect_pcm16(6, rate=rate)  # alone: the collecting call of this slot
    audio = rt.collect(7)
    per, total = rt.prepared_samples(7)
    assert rt.prepared_samples(6) == (per, total) and audio.size == total
    items = np.split(audio, np.cumsum(per)[:-1])
    assert np.array_equal(pcm, np.concatenate([ref_pcm(it, pair) for it in items]))
    assert np.array_equal(rt.collect_pcm16(6), ph.pcm16(audio))


def test_low_preset_16000_to_8000(backend):
    cfg = ph.voice_config("low")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    try:
        assert cfg.sample_rate == 16000
        ids, dur = kd.FIXTURE_IDS, [3] * 14
        rt.prepare(1, ids, dur, kd.sym(SD + 740, (cfg.inter, 42), 1.7320508), 0.667)
        rt.launch(1)
        audio = rt.collect(1)
        got = rt.collect_pcm16(1, rate=8000)
        assert got.size == audio.size // 2 and np.array_equal(got, ref_pcm(audio, (16000, 8000)))
    finally:
        rt.close()


# ---- streams: the oracle is a twin stream of the same items delivering fp32

def check_row(pcm_steps, flt_steps, pair, chunk, hop, what, finished=True):
    """One row's steps: the concatenated PCM is the conversion of the concatenated fp32, and every step's count is stream_ranges'."""
    L, M, P = rr.ratio(*pair)
    x = np.concatenate(flt_steps)
    assert x.size % hop == 0 and len(pcm_steps) == len(flt_steps), what
    frames = x.size // hop
    got = np.concatenate(pcm_steps)
    ranges = rr.stream_ranges(frames if finished else frames + chunk, chunk, hop, L, M, P)[:len(pcm_steps)]
    assert [c.size for c in pcm_steps] == [b - a for a, b in ranges], what
    want = ref_pcm(x, pair)  # (an unfinished row: the outputs whose taps end inside x are a prefix of this)
    assert got.size == (want.size if finished else ranges[-1][1]) and np.array_equal(got, want[:got.size]), what


@pytest.fixture(scope="module")
def single_twin(rt_medium):
    """fp32 chunks of the single-stream item (F = 70) per chunk size, computed once"""
    ids, dur, noise = ragged_group(rt_medium.cfg)[3]
    return {c: list(rt_medium.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=c, slot=3)) for c in (1, 3)}


@pytest.mark.parametrize("rate", [8000, 48000])
@pytest.mark.parametrize("chunk", [1, 3])
def test_single_stream(rt_medium, single_twin, rate, chunk):
    rt = rt_medium
    ids, dur, noise = ragged_group(rt.cfg)[3]  # F = 70: not a multiple of 3
    flt = single_twin[chunk]
    pcm = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3, rate=rate))
    assert len(flt) == -(-70 // chunk)
    check_row(pcm, flt, (rt.cfg.sample_rate, rate), chunk, rt.cfg.hop, (rate, chunk))
    assert max(c.size for c in pcm) <= ph.resample_step_bound(rt.cfg.sample_rate, rate, chunk * rt.cfg.hop)


def run_group(rt, group, rate, chunk=8, drop_after=2, drop_item=1):
    steps = []
    for k, chunks in enumerate(rt.synthesize_stream_batch(group, 0.667, chunkFrames=chunk, slot=8, rate=rate)):
        steps.append(chunks)
        if k == drop_after - 1:
            rt.stream_drop(8, drop_item)
    return steps


@pytest.fixture(scope="module")
def group_twin(rt_medium):
    return run_group(rt_medium, ragged_group(rt_medium.cfg)[1:4], None)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_ragged_group_with_a_drop(rt_medium, group_twin, rate):
    rt = rt_medium
    group = ragged_group(rt.cfg)[1:4]  # F = 30, 84, 70; item 1 dropped after two steps
    flt, pcm = group_twin, run_group(rt, group, rate)
    assert len(flt) == len(pcm) == 9
    for i in range(3):
        fs, ps = [s[i] for s in flt if s[i].size], [s[i] for s in pcm if s[i].size]
        assert [bool(s[i].size) for s in flt] == [bool(s[i].size) for s in pcm], i
        check_row(ps, fs, (rt.cfg.sample_rate, rate), 8, rt.cfg.hop, (rate, i), finished=i != 1)
    assert len([s for s in pcm if s[1].size]) == 2


def run_pool(rt, utts, rate):
    """Capacity 4, chunk 8: S (15 frames), E (84) and A (30) join; after two steps S has finished and B (42) takes its row."""
    pool = rt.stream_pool(10, 4, chunkFrames=8, work_slot=11, rate=rate)
    joined = pool.join([utts["S"], utts["E"], utts["A"]], 0.667)
    assert [i for i, _ in joined] == [0, 1, 2]
    rows = {0: [], 1: [], 2: [], "B": []}
    for k in range(64):
        if k == 2:
            (row, samples), = pool.join([utts["B"]], 0.667)
            assert row == 0  # the row of a finished session
            joined.append((row, samples))
        out = pool.step(pcm=rate is not None)
        if not out:
            break
        for i, c in out.items():
            rows["B" if (i == 0 and k >= 2) else i].append(c)
    pool.close()
    return rows, [s for _, s in joined]


@pytest.fixture(scope="module")
def pool_utts(rt_medium):
    g = ragged_group(rt_medium.cfg)
    return {"S": item(rt_medium.cfg, 5, 9), "E": g[2], "A": g[1], "B": g[0]}


@pytest.fixture(scope="module")
def pool_twin(rt_medium, pool_utts):
    return run_pool(rt_medium, pool_utts, None)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_pool_with_a_join_into_a_finished_row(rt_medium, pool_utts, pool_twin, rate):
    rt = rt_medium
    pair = (rt.cfg.sample_rate, rate)
    (flt, n_flt), (pcm, n_pcm) = pool_twin, run_pool(rt, pool_utts, rate)
    assert n_pcm == [ph.resample_count(*pair, n) for n in n_flt]  # join reports J(N_i)
    for key in (0, 1, 2, "B"):
        check_row(pcm[key], flt[key], pair, 8, rt.cfg.hop, (rate, key))
        assert sum(c.size for c in pcm[key]) == n_pcm[{0: 0, 1: 1, 2: 2, "B": 3}[key]]


# ---- state rules: each refused call consumes nothing, and the stream then continues correctly

def test_state_rules(rt_medium):
    rt, lib = rt_medium, rt_medium.lib
    hop, rate = rt.cfg.hop, 8000
    pair = (rt.cfg.sample_rate, rate)
    ids, dur, noise = ragged_group(rt.cfg)[1]  # F = 30
    flt = np.concatenate(list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3)))
    want = ref_pcm(flt, pair)
    u, keep = rt._utt(ids, dur, noise, 0.667)
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_rate(12, rate)  # no stream there
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 8) == 4
    assert rt.stream_rate(3) == rt.cfg.sample_rate and rt.stream_step_capacity(3) == 8 * hop
    with pytest.raises(ph.UnsupportedOp):
        rt.stream_set_rate(3, 12345)
    rt.stream_set_rate(3, 48000)
    rt.stream_set_rate(3, rate)  # before the first step the rate may still change
    cap = rt.stream_step_capacity(3)
    assert rt.stream_rate(3) == rate and cap == ph.resample_step_bound(*pair, 8 * hop)
    buf, fbuf, got = np.empty(cap, np.int16), np.empty(8 * hop, np.float32), C.c_int64()
    first = rr.stream_ranges(30, 8, hop, *rr.ratio(*pair))[0][1]
    with pytest.raises(ph.InvalidArgument):  # a float step on a rated slot
        ph._check(lib.piper_hip_voice_stream_next(rt.voice, 3, fbuf.ctypes.data_as(ph.c_f32p), fbuf.size, C.byref(got)))
    with pytest.raises(ph.ShapeMismatch):  # a buffer one sample short
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), first - 1, C.byref(got)))
    with pytest.raises(ph.UnsupportedOp):  # normalize on a step
        prm = ph.PcmParams(1.0, 1)
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, C.byref(prm), buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got)))
    parts = []
    for k in range(8):
        ph._check(lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got)))
        if not got.value:
            break
        parts.append(buf[:got.value].copy())
        with pytest.raises(ph.InvalidArgument):  # after a step the rate is fixed
            rt.stream_set_rate(3, 48000)
    assert len(parts) == 4 and parts[0].size == first
    assert np.array_equal(np.concatenate(parts), want)  # nothing was consumed by the refused calls
    # a new begin is back at the voice's own rate
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 8) == 4
    assert rt.stream_rate(3) == rt.cfg.sample_rate
    ph._check(lib.piper_hip_voice_stream_next(rt.voice, 3, fbuf.ctypes.data_as(ph.c_f32p), fbuf.size, C.byref(got)))
    assert got.value == 8 * hop and np.array_equal(fbuf, flt[:8 * hop])
    # a pool: the rate is fixed from its first join on; a float step on a rated pool is refused
    pool = rt.stream_pool(10, 2, chunkFrames=8, work_slot=11, rate=rate)
    with pytest.raises(ph.InvalidArgument):
        pool.step(pcm=False)
    pool.join([(ids, dur, noise)], 0.667)
    with pytest.raises(ph.InvalidArgument):
        pool.set_rate(48000)
    got_n = (C.c_int64 * 2)()
    with pytest.raises(ph.InvalidArgument):  # a rated step needs a buffer, on a pool as on a single stream; nothing is consumed
        ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(rt.voice, 10, None, None, 0, got_n))
    out = pool.step(pcm=True)
    assert np.array_equal(out[0], want[:first])
    pool.close()
    # the voice's own rate is not a filter: the pool stays native, float steps and their buffer included
    pool = rt.stream_pool(10, 2, chunkFrames=8, work_slot=11, rate=rt.cfg.sample_rate)
    assert rt.stream_rate(10) == rt.cfg.sample_rate
    pool.join([(ids, dur, noise)], 0.667)
    out = pool.step(pcm=False)
    assert out[0].dtype == np.float32 and np.array_equal(out[0], flt[:8 * hop])
    assert np.array_equal(pool.step(pcm=True)[0], ph.pcm16(flt[8 * hop:16 * hop]))
    pool.close()
