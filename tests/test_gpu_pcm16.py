"""GPU: 16-bit PCM straight from the device — the per-op conversion, collect_pcm16 on plain, ragged and bounded slots, and the PCM steps of
single, grouped and pooled streams. Every comparison is exact: both sides start from the same fp32 bits, and the conversion is a
contract (include/piper_hip.h; tests/pcm_ref.py restates it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import katdata as kd
import pcm_ref
import piper_hip as ph
from test_gpu_stream_batch import SD, ragged_group

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A


@pytest.fixture(scope="module")
def rt_medium(backend, voices):
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    yield rt
    rt.close()


def item(cfg, n_ids, seed):
    ids = (kd.FIXTURE_IDS * 4)[:n_ids]
    dur = [3] * n_ids
    return ids, dur, kd.sym(SD + 300 + seed, (cfg.inter, sum(dur)), 1.7320508)


# ---- per-op

def tiled(count):
    v = pcm_ref.adversarial_vector()
    return np.resize(v, count).astype(np.float32)


def test_per_op_adversarial_vector(backend):
    v = pcm_ref.adversarial_vector()
    buf = backend.uploadFloat32(v)
    out = backend.pcm16F32(buf)
    got = backend.downloadInt16(out)
    assert np.array_equal(got, ph.pcm16(v))
    assert np.any(got != pcm_ref.fp32_shortcut(v))  # the device did not take the float32 shortcut either
    out.free()
    buf.free()


@pytest.mark.parametrize("count", [0, 1, 3, 255, 257, 1029])
def test_per_op_counts(backend, count):
    x = tiled(max(count, 1))
    buf = backend.uploadFloat32(x)
    out = backend.pcm16F32(buf, count=count)
    assert out.count == count and out.ptr
    if count:
        assert np.array_equal(backend.downloadInt16(out), ph.pcm16(x[:count]))
    out.free()
    buf.free()


def test_per_op_output_at_a_2_byte_aligned_offset(backend):
    """A caller-supplied *out 14 bytes into a larger buffer (2-byte, not 4-byte aligned): the samples land there, the guards stay."""
    count, lead, trail = 257, 7, 24
    x = tiled(count)
    buf = backend.uploadFloat32(x)
    box = backend.uploadFloat32(np.full(lead + count + trail, GUARD, np.uint16).view(np.float32))
    out = backend.pcm16F32(buf, out=int(box.ptr) + 2 * lead)
    assert out.ptr == int(box.ptr) + 2 * lead and not out.owned
    got = backend.downloadInt16(box, lead + count + trail).view(np.uint16)
    assert np.all(got[:lead] == GUARD) and np.all(got[lead + count:] == GUARD)
    assert np.array_equal(got[lead:lead + count].view(np.int16), ph.pcm16(x))
    box.free()
    buf.free()


@pytest.mark.parametrize("x_off,out_off", [(0, 4), (1, 0), (1, 4), (0, 2), (3, 7)])
def test_per_op_every_alignment_branch(backend, x_off, out_off):
    """The kernel picks its stores by alignment: 16-byte ones where source and destination are 16-byte aligned, 8-byte ones where the
    destination is only 8-byte aligned (*out 8 bytes in), one sample at a time where the source is not 16-byte aligned (x 4 bytes in) or
    the destination not 8-byte aligned. x_off is in floats, out_off in samples; 1029 samples leave a scalar tail on the vector paths."""
    count = 1029
    trail = 24 + (out_off + count) % 2  # (the guarded box is uploaded as whole floats)
    x = tiled(x_off + count)
    buf = backend.uploadFloat32(x)
    box = backend.uploadFloat32(np.full(out_off + count + trail, GUARD, np.uint16).view(np.float32))
    assert int(buf.ptr) % 16 == 0 and int(box.ptr) % 16 == 0
    out = backend.pcm16F32(int(buf.ptr) + 4 * x_off, count=count, out=int(box.ptr) + 2 * out_off)
    assert out.ptr == int(box.ptr) + 2 * out_off and out.dtype == np.int16 and not out.owned
    got = backend.downloadInt16(box, out_off + count + trail).view(np.uint16)
    assert np.all(got[:out_off] == GUARD) and np.all(got[out_off + count:] == GUARD)
    assert np.array_equal(got[out_off:out_off + count].view(np.int16), ph.pcm16(x[x_off:]))
    box.free()
    buf.free()


def test_device_buffer_of_samples_is_not_read_as_floats(backend):
    buf = backend.uploadFloat32(tiled(8))
    out = backend.pcm16F32(buf)
    assert out.count == 8 and out.dtype == np.int16 and buf.dtype == np.float32
    with pytest.raises(TypeError):
        backend.downloadFloat32(out)
    out.free()
    buf.free()


@pytest.mark.parametrize("gain", [0.5, 1.7])
def test_per_op_gain(backend, gain):
    x = tiled(1029)
    buf = backend.uploadFloat32(x)
    out = backend.pcm16F32(buf, gain=gain)
    assert np.array_equal(backend.downloadInt16(out), pcm_ref.pcm16_reference(x, gain))
    out.free()
    buf.free()


def test_per_op_bad_gain(backend):
    buf = backend.uploadFloat32(tiled(8))
    for gain in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ph.InvalidArgument):
            backend.pcm16F32(buf, gain=gain)
    buf.free()


# ---- whole utterance

def test_whole_utterance_both_orders(rt_medium):
    rt = rt_medium
    ids, dur, noise = kd.FIXTURE_IDS, [3] * 14, kd.sym(SD + 300, (rt.cfg.inter, 42), 1.7320508)
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    first = rt.collect_pcm16(5)
    audio = rt.collect(5)
    assert audio.size == first.size == 10752
    assert np.array_equal(first, ph.pcm16(audio))
    assert np.array_equal(rt.collect_pcm16(5), first)  # the fp32 audio stays in the plan
    assert np.array_equal(rt.collect_pcm16(5, gain=0.5), pcm_ref.pcm16_reference(audio, 0.5))
    rt.launch(5)
    audio2 = rt.collect(5)
    assert np.array_equal(audio2, audio)
    assert np.array_equal(rt.collect_pcm16(5), ph.pcm16(audio2))
    # a destination the caller page-locked takes the kernel's stores directly
    pinned = rt.pinned_empty(audio.size // 2 + 8).view(np.int16)
    pinned[:] = 0x1234
    got = rt.collect_pcm16(5, out=pinned)
    assert np.array_equal(got, first) and np.all(pinned[audio.size:] == 0x1234)
    # the one-call entry point
    assert np.array_equal(rt.synthesize_pcm16(ids, dur, noise, 0.667), first)


def test_arguments(rt_medium):
    rt = rt_medium
    ids, dur, noise = item(rt.cfg, 5, 1)
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    n = 15 * rt.cfg.hop
    small = np.empty(n - 1, np.int16)
    prm = ph.PcmParams(1.0, 0)
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rt.lib.piper_hip_voice_collect_pcm16(rt.voice, 5, C.byref(prm), small.ctypes.data_as(ph.c_i16p), small.size))
    with pytest.raises(ph.InvalidArgument):
        rt.peaks(5)  # no normalising collect yet
    for gain in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ph.InvalidArgument):
            rt.collect_pcm16(5, gain=gain)
    with pytest.raises(ph.InvalidArgument):  # slot 9 holds nothing
        ph._check(rt.lib.piper_hip_voice_collect_pcm16(rt.voice, 9, None, small.ctypes.data_as(ph.c_i16p), small.size))
    audio = rt.collect(5)
    assert np.array_equal(rt.collect_pcm16(5, gain=0.0), ph.pcm16(audio))  # gain 0 is taken as 1.0; the refused calls changed nothing
    full = np.empty(n, np.int16)
    ph._check(rt.lib.piper_hip_voice_collect_pcm16(rt.voice, 5, None, full.ctypes.data_as(ph.c_i16p), n))  # NULL params = {1.0, 0}
    assert np.array_equal(full, ph.pcm16(audio))
    rt.collect_pcm16(5, normalize=True)
    assert rt.peaks(5).tolist() == [float(np.abs(audio).max())]
    rt.launch(5)
    rt.collect(5)
    with pytest.raises(ph.InvalidArgument):
        rt.peaks(5)  # they belonged to the previous run


def test_long_utterance_through_the_chunked_copy(rt_medium):
    """2 184 frames: 1.07 MB of int16 into a pageable buffer is past the size where the kernel stores through the host mapping — the samples
    go to the plan's device buffer and cross in chunks."""
    rt = rt_medium
    ids = kd.FIXTURE_IDS * 52
    dur = [3] * len(ids)
    rt.prepare(5, ids, dur, None, 0.667, noise_mode="device", seed=77)
    rt.launch(5)
    audio = rt.collect(5)
    assert audio.size * 2 > 1 << 20
    assert np.array_equal(rt.collect_pcm16(5), ph.pcm16(audio))
    got = rt.collect_pcm16(5, normalize=True)
    assert np.array_equal(got, pcm_ref.pcm16_normalized(audio))
    assert rt.peaks(5)[0] == np.abs(audio).max()


# ---- ragged batch

def test_ragged_batch_and_normalisation(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    group = [item(rt.cfg, n, k) for k, n in enumerate((14, 5, 9))]
    rt.prepare_batch(6, group, 0.667)
    rt.launch(6)
    audio = rt.collect(6)
    per, total = rt.prepared_samples(6)
    assert per == [42 * hop, 15 * hop, 27 * hop] and total == audio.size
    items = np.split(audio, np.cumsum(per)[:-1])
    got = rt.collect_pcm16(6)
    assert got.size == total
    off = 0
    for b, it in enumerate(items):  # packed offsets and every sample
        assert np.array_equal(got[off:off + it.size], ph.pcm16(it)), b
        off += it.size
    for gain in (1.0, 0.5):
        norm = rt.collect_pcm16(6, gain=gain, normalize=True)
        peaks = rt.peaks(6)
        assert peaks.dtype == np.float32 and peaks.tolist() == [float(np.abs(it).max()) for it in items]
        assert np.array_equal(norm, pcm_ref.pcm16_items(items, gain, normalize=True))
        if gain == 1.0:
            for b, pn in enumerate(np.split(norm, np.cumsum(per)[:-1])):
                assert int(np.abs(pn.astype(np.int32)).max()) in (32766, 32767), b
    assert np.array_equal(rt.collect(6), audio)  # still there


# ---- bounded prepare

def test_bounded_prepare_collected_as_pcm_only(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    utts = [(kd.FIXTURE_IDS * 2, None), (kd.FIXTURE_IDS, None)]
    kw = dict(noise_mode="device", seed=4242)
    probe = rt.predict_durations(utts, **kw)
    bound = max(int(d.sum()) for d, _ in probe) + 5
    for slot in (6, 7):  # two identically prepared slots
        rt.prepare_batch_bounded(slot, utts, bound, **kw)
        rt.launch(slot)
    cap = rt.prepared_samples(6)[1]
    pcm = rt.collect_pcm16(6)  # alone: no float collect on this slot
    audio = rt.collect(7)
    assert rt.prepared_samples(6) == rt.prepared_samples(7)
    assert pcm.size == audio.size == rt.prepared_samples(6)[1] <= cap
    assert pcm.size % hop == 0 and np.array_equal(rt.durations(6), rt.durations(7))
    assert np.array_equal(pcm, ph.pcm16(audio))
    # an item over the bound still fails
    rt.prepare_batch_bounded(6, utts, 8, **kw)
    rt.launch(6)
    with pytest.raises(ph.ShapeMismatch):
        rt.collect_pcm16(6)


# ---- streams

def test_single_stream(rt_medium):
    rt = rt_medium
    ids, dur, noise = ragged_group(rt.cfg)[2]  # F = 84: five full chunks of 16 and one of 4
    flt = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=16, slot=3))
    pcm = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=16, slot=3, pcm=True))
    assert len(flt) == len(pcm) == 6
    for k, (f, p) in enumerate(zip(flt, pcm)):
        assert p.dtype == np.int16 and np.array_equal(p, ph.pcm16(f)), k
    half = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=16, slot=3, pcm=True, gain=0.5))
    for k, (f, p) in enumerate(zip(flt, half)):
        assert np.array_equal(p, pcm_ref.pcm16_reference(f, 0.5)), k
    # normalize on a step is refused, so is a buffer too small, and neither consumes the step
    u, keep = rt._utt(ids, dur, noise, 0.667)
    assert rt.lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 16) == 6
    buf, got = np.empty(16 * rt.cfg.hop, np.int16), C.c_int64()
    prm = ph.PcmParams(1.0, 1)
    with pytest.raises(ph.UnsupportedOp):
        ph._check(rt.lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, C.byref(prm), buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got)))
    with pytest.raises(ph.ShapeMismatch):
        ph._check(rt.lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), buf.size - 1, C.byref(got)))
    ph._check(rt.lib.piper_hip_voice_stream_next_pcm16(rt.voice, 3, None, buf.ctypes.data_as(ph.c_i16p), buf.size, C.byref(got)))
    assert got.value == buf.size and np.array_equal(buf, pcm[0])


def run_group(rt, group, pcm, drop_at=1, drop_item=1):
    steps = []
    for k, chunks in enumerate(rt.synthesize_stream_batch(group, 0.667, chunkFrames=32, slot=8, pcm=pcm)):
        steps.append(chunks)
        if k == drop_at - 1:
            rt.stream_drop(8, drop_item)
    return steps


def test_group_with_a_drop(rt_medium):
    rt = rt_medium
    group = ragged_group(rt.cfg)[2:5]  # F = 84, 70, 336
    flt, pcm = run_group(rt, group, False), run_group(rt, group, True)
    assert len(flt) == len(pcm) == 11
    for k, (fs, ps) in enumerate(zip(flt, pcm)):
        assert [c.size for c in fs] == [c.size for c in ps], k  # the n_samples tables
        for i, (f, p) in enumerate(zip(fs, ps)):
            assert p.dtype == np.int16 and np.array_equal(p, ph.pcm16(f)), (k, i)
    assert [c.size for c in pcm[1]][1] == 0  # dropped after its first chunk


def run_pool(rt, utts, mode):
    """Capacity 4, chunk 32: A (84 frames) and E (336) join; B (42) joins after step 2. mode: "float", "pcm", or "mixed" (odd steps PCM)."""
    pool = rt.stream_pool(10, 4, chunkFrames=32, work_slot=11)
    steps = []
    assert [i for i, _ in pool.join([utts["A"], utts["E"]], 0.667)] == [0, 1]
    for k in range(64):
        if k == 2:
            assert [i for i, _ in pool.join([utts["B"]], 0.667)] == [2]
        pcm = mode == "pcm" or (mode == "mixed" and k % 2 == 1)
        if mode != "float" and k == 3:  # refused, nothing consumed: the next plain step still returns this step's chunks
            with pytest.raises(ph.UnsupportedOp):
                pool.step(pcm=True, normalize=True)
        out = pool.step(pcm=pcm)
        if not out:
            break
        steps.append(out)
    pool.close()
    return steps


def test_pool_with_a_join_and_mixed_steps(rt_medium):
    rt = rt_medium
    g = ragged_group(rt.cfg)
    utts = {"A": g[2], "B": g[0], "E": g[4]}
    flt, pcm, mixed = (run_pool(rt, utts, m) for m in ("float", "pcm", "mixed"))
    assert len(flt) == len(pcm) == len(mixed) == 11
    for k, (fs, ps, ms) in enumerate(zip(flt, pcm, mixed)):
        assert {i: c.size for i, c in fs.items()} == {i: c.size for i, c in ps.items()} == {i: c.size for i, c in ms.items()}, k
        for i in fs:
            assert ps[i].dtype == np.int16 and np.array_equal(ps[i], ph.pcm16(fs[i])), (k, i)
            if k % 2 == 1:
                assert ms[i].dtype == np.int16 and np.array_equal(ms[i], ps[i]), (k, i)
            else:
                assert ms[i].dtype == np.float32 and np.array_equal(ms[i], fs[i]), (k, i)
    assert sorted(flt[2]) == [0, 1, 2] and sorted(flt[1]) == [0, 1]  # B active from the step after its join


# ---- high voice, bf16 generator

def test_high_voice_bf16(backend, voices):
    cfg, blob = voices["high"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        rt.set_precision("bf16")
        ids, dur = kd.FIXTURE_IDS, [3] * 14
        rt.prepare(1, ids, dur, kd.sym(SD + 340, (cfg.inter, 42), 1.7320508), 0.667)
        rt.launch(1)
        audio = rt.collect(1)
        assert audio.size == 42 * cfg.hop
        assert np.array_equal(rt.collect_pcm16(1), ph.pcm16(audio))  # the conversion does not care how the waveform was computed
    finally:
        rt.close()


# ---- command line

def test_cli_output_raw(tmp_path):
    import wave
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    ids = ",".join(str(i) for i in kd.FIXTURE_IDS + kd.FIXTURE_IDS[:5])
    wav, raw, loud = tmp_path / "cli.wav", tmp_path / "cli.raw", tmp_path / "loud.raw"
    out = subprocess.run([str(exe), "--phoneme-ids", ids, "--output", str(wav), "--output-raw", str(raw)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    with wave.open(str(wav), "rb") as w:
        ref = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    assert ref.size == 19 * 3 * 256 and raw.read_bytes() == ref.tobytes()  # (after --output: collect_pcm16 on the slot that ran)
    out = subprocess.run([str(exe), "--phoneme-ids", ids, "--output-raw", str(loud)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert loud.read_bytes() == ref.tobytes()  # alone: synthesize_pcm16
    out = subprocess.run([str(exe), "--phoneme-ids", ids, "--output-raw", str(loud), "--normalize", "--volume", "0.5"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.frombuffer(loud.read_bytes(), "<i2")
    assert got.size == ref.size and int(np.abs(got.astype(np.int32)).max()) in (16382, 16383)
