"""GPU: loudness (include/piper_hip.h "Loudness") — BS.1770 integrated loudness measured on the device and the gain it implies on every
whole-item route. The raw fp32 reference is always the GPU's own audio (the same slot collected with neither loudness nor level); on it
tests/loudness_ref.py gives L in float64, and the delivered bytes must be the existing numpy contracts — level_ref, pcm_ref, resample_ref,
g711_ref — applied to fl(raw · g) with g the gain the device reported, bit for bit.

The device's L is held to 0.002 LU of the sequential float64 recurrence: a segmented double restatement differs from it by 1e-12 LU and
the smallest planted defect of tests/test_loudness_ref.py moves L by 0.027 LU.

The voice is the one of tests/test_gpu_level.py (output conv × 0.02, noise envelope 16 / 0): a long quiet stretch in the first two items
puts blocks under the relative gate, the third keeps all its three blocks, the fourth (8448 samples < 400 ms) cannot be measured."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import katdata as kd
import level_ref as lr
import loudness_ref as ld
import mixed_ref as mr
import piper_hip as ph
from test_gpu_level import DEV, SINKS, collect_as, rt_medium, same  # noqa: F401  (rt_medium: the fixture)
from test_gpu_resample import same_bits
from test_gpu_stream_mixed import TABLES

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 0.002
# ids (× 3 frames), the quiet frames, blocks, blocks kept after the relative gate
ITEMS = [(64, (60, 130), 19, 14), (48, (40, 100), 13, 10), (20, None, 3, 3), (11, None, 0, 0)]
ATTENUATE = ((-16.0, 0.0), None)              # a loudness target and the level that goes with it
BOOST = ((-3.0, 6.0), (1.0, 0.5, 50.0))       # boosts into the limiter
NEUTRAL = (1.0, 1.0, 50.0)


def shaped(cfg, k):
    n, quiet, _, _ = ITEMS[k]
    F = 3 * n
    env = np.full(F, 16.0, F32)
    if quiet:
        env[quiet[0]:quiet[1]] = 0.0
    return (kd.FIXTURE_IDS * 5)[:n], [3] * n, kd.sym(940 + k, (cfg.inter, F), 1.7320508) * env


def close(got, want):
    """within TOL, −inf only for −inf"""
    if want == -math.inf or got == -math.inf:
        return got == want
    return abs(float(got) - want) <= TOL


def ulp_apart(a, b):
    a, b = np.asarray([a], F32).view(np.int32)[0], np.asarray([b], F32).view(np.int32)[0]
    return abs(int(a) - int(b))


# ---- per-op

SIGNALS = [(name, rate) for rate in (16000, 22050) for name in ("s1", "s2", "s3")] + [("sine", 48000)]


@pytest.fixture(scope="module")
def per_op_cases():
    """(what, rate, samples, reference L), computed once"""
    cases = [(f"{name}@{rate}", rate, getattr(ld, name)(rate)) for name, rate in SIGNALS]
    long = ld._stretches(22050, [(4.0, 0.1), (2.0, 0.003), (3.1, 0.05)], 7004)
    cases += [(f"edge {n}", 22050, ld.s1(22050)[:n]) for n in (8819, 8820, 11024, 11025)]
    cases += [("empty", 22050, np.empty(0, F32)), ("200001", 22050, long[:200001]),
              ("one pass and a chunk", 16000, ld.s2(16000)[:32768 + 65]), ("exactly one pass", 16000, ld.s2(16000)[:32768])]
    return [(what, rate, x, ld.lufs(x, rate)) for what, rate, x in cases]


def test_per_op_within_tolerance_and_the_same_bits_twice(backend, per_op_cases):
    for what, rate, x, want in per_op_cases:
        buf = backend.uploadFloat32(x if x.size else np.zeros(1, F32))
        got = [backend.loudness_f32(buf, rate, count=x.size) for _ in range(2)]
        print(f"{what}: device {float(got[0]):.6f}, reference {want:.6f}")
        assert close(got[0], want), (what, got[0], want)
        assert same_bits(np.asarray(got[:1], F32), np.asarray(got[1:], F32)), what


def test_per_op_more_passes_than_one_tile_of_the_carry_chain(backend):
    """257 passes of 32 768 samples: the chain over the passes' states runs 256 passes at a time. At this size the reference is the host
    twin, which tests/test_loudness_abi.py holds to 1e-9 LU of loudness_ref."""
    n = 256 * 32768 + 40000
    rng = np.random.default_rng(7005)
    x = (0.05 * rng.standard_normal(n)).astype(F32)
    x[3000000:5000000] *= F32(0.01)  # under the relative gate
    x[5000000:5100000] = 0.0         # under the absolute gate
    buf = backend.uploadFloat32(x)
    got = [backend.loudness_f32(buf, 48000) for _ in range(2)]
    want = float(ph.loudness_from_f32(x, 48000))
    print(f"{n} samples: device {float(got[0]):.6f}, host twin {want:.6f}")
    assert close(got[0], want) and same_bits(np.asarray(got[:1], F32), np.asarray(got[1:], F32))


def test_per_op_unaligned_source_non_finite_samples_and_refusals(backend):
    x = ld.s3(22050)[:70001].copy()
    want = backend.loudness_f32(backend.uploadFloat32(x), 22050)
    buf = backend.uploadFloat32(np.concatenate([np.zeros(1, F32), x]))
    shifted = ph.DeviceBuffer(backend, buf.ptr + 4, x.size, owned=False)  # a source that is not 16-byte aligned
    assert same_bits(np.asarray([backend.loudness_f32(shifted, 22050)], F32), np.asarray([want], F32))
    y = x.copy()
    y[[5, 40000, 70000]] = [np.nan, np.inf, -np.inf]  # read as 0
    z = np.where(np.isfinite(y), y, 0).astype(F32)
    assert close(backend.loudness_f32(backend.uploadFloat32(y), 22050), ld.lufs(z, 22050))
    with pytest.raises(ph.UnsupportedOp):
        backend.loudness_f32(backend.uploadFloat32(x), 11025)


# ---- voice routes

def ragged(rt, slot):
    rt.prepare_batch(slot, [shaped(rt.cfg, k) for k in range(len(ITEMS))], 0.667)
    return list(range(len(ITEMS)))


def alone(k):
    def prep(rt, slot):
        rt.prepare(slot, *shaped(rt.cfg, k), 0.667)
        return [k]
    prep.__name__ = f"alone{k}"
    return prep


def bounded(rt, slot):
    """prepare_batch_bounded of two items whose noise the device draws (no envelope): every block is kept"""
    import ctypes as C
    id_lists = [kd.FIXTURE_IDS * 4, kd.FIXTURE_IDS * 3]
    bound = max(int(d.sum()) for d, _ in rt.predict_durations([(ids, None) for ids in id_lists], **DEV)) + 5
    arr, keep = (ph.Utterance * 2)(), []
    for i, (ids, scale) in enumerate(zip(id_lists, (0.667 * 16, 0.667 * 4))):
        arr[i], k = rt._utt(ids, None, None, scale, **DEV)
        keep.append(k)
    assert rt.lib.piper_hip_voice_prepare_batch_bounded(rt.voice, arr, 2, slot, bound) >= 0
    tot = C.c_int64()
    ph._check(rt.lib.piper_hip_voice_prepared_samples(rt.voice, slot, None, 0, C.byref(tot)))
    rt._keep[slot] = (keep, int(tot.value), True)
    return None


def expected(items, gains, level, rate):
    """every sink's bytes for the raw items, their reported gains and a level (or None)"""
    us = [ld.apply(x, g) for x, g in zip(items, gains)]
    ys = [u if level is None else lr.apply(u, level, rate) for u in us]
    return {name: np.concatenate([mr.whole(y, f, rate, TABLES) for y in ys]) for name, f in SINKS.items()}


@pytest.mark.parametrize("prep", [ragged, alone(0), alone(1), alone(2), alone(3), bounded], ids=lambda f: f.__name__)
def test_voice_routes(rt_medium, prep):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    rt.slot_loudness(5, None)
    rt.slot_level(5, None)
    which = prep(rt, 5)
    if which is None:  # a bounded slot that has not been collected has no lengths to measure by
        with pytest.raises(ph.InvalidArgument):
            rt.loudness(5)
    rt.launch(5)
    raw = rt.collect(5).copy()  # (a bounded slot: its collecting call)
    per, total = rt.prepared_samples(5)
    assert raw.size == total
    items = np.split(raw, np.cumsum(per)[:-1])
    ref = [ld.measure(x, rate) for x in items]
    for k, m in enumerate(ref):
        print(f"item {k}: {items[k].size} samples, {m}")
    if which is not None:  # the gates these items are meant to show, on the GPU's own audio through the reference alone
        for k, m in zip(which, ref):
            assert (m["blocks"], m["rel"]) == ITEMS[k][2:], (k, m)
            assert m["abs"] == m["blocks"]
    else:  # device noise has no envelope: every block is kept
        assert all(m["blocks"] >= 4 and m["abs"] == m["rel"] == m["blocks"] for m in ref), ref
    plain_bytes = {name: collect_as(rt, 5, name).copy() for name in SINKS}  # before any loudness was set

    # 1. the measurement, without a target: g = 1
    lufs, gain = rt.loudness(5)
    for k, m in enumerate(ref):
        assert close(lufs[k], m["L"]), (k, lufs[k], m["L"])
    assert np.all(gain == F32(1.0))
    assert same_bits(rt.loudness(5)[0], lufs)

    for loudness, level in (ATTENUATE, BOOST):
        rt.slot_loudness(5, loudness)
        l2, g = rt.loudness(5)
        assert same_bits(l2, lufs)
        # 2. the gain is the formula's, from the reported L
        for k in range(len(items)):
            assert ulp_apart(g[k], ld.gain(loudness, lufs[k])) <= 1, (k, g[k], ld.gain(loudness, lufs[k]))
            if lufs[k] == -math.inf:
                assert g[k] == F32(1.0)
            elif which is not None:  # −16 attenuates these items, −3 boosts them
                assert (g[k] < 1.0) == (loudness is ATTENUATE[0]), (k, g[k])
        levels = [None, NEUTRAL if level is None else level]
        if level is not None:  # the boost reaches the limiter
            assert any(lr.gains(ld.apply(x, gk), level, rate)[1].min() < 1.0 for x, gk in zip(items, g) if x.size)
        # 3. every collect, with and without a level, after the raw collect …
        want = {lv: expected(items, g, lv, rate) for lv in levels}
        for lv in levels:
            for name in SINKS:
                assert same(collect_as(rt, 5, name, level=lv), want[lv][name]), (loudness, lv, name, "after raw")
        # 5. normalize = 1 is refused
        with pytest.raises(ph.InvalidArgument):
            rt.collect_pcm16(5, normalize=True, level=None)
        with pytest.raises(ph.InvalidArgument):
            rt.collect_g711(5, "mulaw", normalize=True)
        # 6. the audio tap stays raw
        assert same_bits(rt.tap(5, "audio").reshape(-1), raw)
        # … and as the first thing that reads a new run, the raw collect behind it
        rt.slot_loudness(6, loudness)
        for lv in levels:
            for name in SINKS:
                prep(rt, 6)
                rt.launch(6)
                assert same(collect_as(rt, 6, name, level=lv), want[lv][name]), (loudness, lv, name, "first")
            assert same_bits(rt.collect(6, level=None, loudness=None), raw)
            rt.slot_loudness(6, loudness)
        l6, g6 = rt.loudness(6)
        assert same_bits(l6, lufs) and same_bits(g6, g)
        rt.slot_loudness(6, None)
        rt.slot_level(6, None)

    # 4. clearing the loudness returns the bits of a slot that never had one
    rt.slot_loudness(5, None)
    rt.slot_level(5, None)
    for name in SINKS:
        assert same(collect_as(rt, 5, name), plain_bytes[name]), (name, "cleared")
    assert np.all(rt.loudness(5)[1] == F32(1.0))


def test_synthesize_twins_take_slot_0_loudness(rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    ids, dur, noise = shaped(rt.cfg, 2)
    raw = rt.synthesize(ids, dur, noise, 0.667, level=None, loudness=None).copy()
    out = rt.synthesize(ids, dur, noise, 0.667, loudness=-16.0)
    lufs, g = rt.loudness(0)
    assert close(lufs[0], ld.lufs(raw, rate)) and ulp_apart(g[0], ld.gain((-16.0, 0.0), lufs[0])) <= 1
    u = ld.apply(raw, g[0])
    assert same_bits(out, u)
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000), mr.whole(u, SINKS["s16@8000"], rate, TABLES))  # the target stays
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000), mr.whole(u, SINKS["mulaw@8000"], rate, TABLES))
    with pytest.raises(ph.InvalidArgument):
        rt.synthesize_pcm16(ids, dur, noise, 0.667, normalize=True)
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, loudness=None), raw)


def test_state_rules(rt_medium):
    rt = rt_medium
    for bad in ((-71.0, 0.0), (-0.5, 0.0), (-16.0, 61.0), (-16.0, -1.0), (float("nan"), 0.0)):
        with pytest.raises(ph.InvalidArgument):
            rt.slot_loudness(5, bad)
    with pytest.raises(ph.InvalidArgument):
        rt.slot_loudness(-1, -16.0)
    assert rt.lib.piper_hip_voice_loudness(None, 0, None, None, 0) == ph.InvalidArgument.code
    rt.prepare(7, *shaped(rt.cfg, 2), 0.667)
    rt.launch(7)
    import ctypes as C
    one = (C.c_float * 1)()
    assert rt.lib.piper_hip_voice_loudness(rt.voice, 7, one, None, 0) == ph.ShapeMismatch.code
    assert rt.lib.piper_hip_voice_loudness(rt.voice, 7, None, None, 0) == 0  # either array may be NULL
    assert rt.lib.piper_hip_voice_loudness(rt.voice, 7, one, None, 1) == 0 and math.isfinite(one[0])
    rt.collect(7, want_audio=False)


# ---- command line

def test_cli_loudness_equals_the_python_route(backend, voices, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    ids = kd.FIXTURE_IDS * 2
    raw = tmp_path / "a.s16le"
    out = subprocess.run([str(exe), "--phoneme-ids", ",".join(str(i) for i in ids), "--output-raw", str(raw), "--loudness", "-23"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        want = rt.synthesize_pcm16(ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234, loudness=-23.0).copy()
        lufs, g = rt.loudness(0)
    finally:
        rt.close()
    assert np.array_equal(np.frombuffer(raw.read_bytes(), "<i2"), want)
    m = re.search(r"loudness (-?[0-9.]+) LUFS, gain ([0-9.eE+-]+)", out.stderr)
    assert m, out.stderr
    assert abs(float(m.group(1)) - float(lufs[0])) < 1e-3 and abs(float(m.group(2)) / float(g[0]) - 1.0) < 1e-4
