"""CPU: the host-only level entry points of the library (include/piper_hip.h "Level control") against the numpy restatement — the host
twin bit for bit, the constants and counts, every refusal — and the device entry points' answers without a device."""
import ctypes as C

import numpy as np
import pytest

import level_ref as lr
import piper_hip as ph

F32 = np.float32
NS = [0, 1, 31, 32, 33, 255, 256, 257, 5000]
LEVELS = [(3.0, 0.5, 50.0), (0.0, 0.0, 0.0), (8.0, 0.25, 5.0), (0.5, 0.001, 10000.0), (1.0, 1.0, 1.0)]


def vector(n, seed):
    """Quiet and loud stretches, NaN samples, and a peak on a block's first and last sample and on the item's last sample."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = ((0.02 + 0.3 * np.abs(np.sin(t / 700.0)) ** 4) * rng.standard_normal(n)).astype(F32)
    if n > 3:
        x[2] = np.nan
    if n > 100:
        x[64] = 0.9    # a block's first sample
        x[95] = -0.95  # a block's last sample
        x[77] = np.nan
    if n:
        x[n - 1] = 0.97  # the item's last sample
    return x


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("rate", [16000, 22050])
@pytest.mark.parametrize("n", NS)
def test_host_twin_equals_the_reference_bit_for_bit(n, rate):
    x = vector(n, 100 + n)
    for level in LEVELS:
        got = ph.level_from_f32(x, level, rate)
        assert got.size == n
        assert np.array_equal(bits(got), bits(lr.apply(x, level, rate))), (n, rate, level)


def test_info_ready_and_step_bound_follow_the_reference():
    lib = ph.load_library()
    for rate in (8000, 16000, 22050, 48000):
        for level in LEVELS + [(1.0, 1.0, 1.5), (1.0, 1.0, 0.0)]:
            assert ph.level_info(level, rate) == lr.rel(level, rate)
    assert ph.level_info((0, 0, 0), 22050) == F32(min(1.0, 32000.0 / (22050 * 50.0)))
    assert ph.level_info((1, 1, 1), 8000) == F32(1.0)  # 4 > 1: clamped
    for e in list(range(0, 600)) + [2 ** 31 - 1, 2 ** 31, 2 ** 40 + 33]:
        assert ph.level_ready(e) == lr.ready(e)
    assert ph.level_ready(255) == 0 and ph.level_ready(256) == 32
    for n_in in (0, 1, 512, 16384, 2 ** 33):
        assert ph.level_step_bound(n_in) == lr.step_bound(n_in) == n_in + 255
    assert lib.piper_hip_level_ready(-1) == -7 and lib.piper_hip_level_step_bound(-1) == -7
    with pytest.raises(ph.InvalidArgument):
        ph.level_info((1, 1, 50), 0)


@pytest.mark.parametrize("level,field", [
    ((-1.0, 0.5, 50.0), "drive"), ((1000.5, 0.5, 50.0), "drive"), ((float("inf"), 0.5, 50.0), "drive"), ((float("nan"), 0.5, 50.0), "drive"),
    ((1.0, 0.0005, 50.0), "ceiling"), ((1.0, 1.5, 50.0), "ceiling"), ((1.0, -0.5, 50.0), "ceiling"), ((1.0, float("nan"), 50.0), "ceiling"),
    ((1.0, 0.5, 0.5), "release_ms"), ((1.0, 0.5, 10001.0), "release_ms"), ((1.0, 0.5, -1.0), "release_ms"), ((1.0, 0.5, float("nan")), "release_ms"),
])
def test_check_refuses_every_field_by_name(level, field):
    lib = ph.load_library()
    lv = ph.Level(*level)
    assert lib.piper_hip_level_check(C.byref(lv)) == -7
    assert field.encode() in lib.piper_hip_last_error()
    with pytest.raises(ph.InvalidArgument):
        ph.level_from_f32(np.zeros(4, F32), level, 22050)
    with pytest.raises(ph.InvalidArgument):
        ph.level_info(level, 22050)


def test_check_accepts_the_bounds_and_the_defaults():
    for level in [(0, 0, 0), (1000.0, 1.0, 10000.0), (1e-6, 0.001, 1.0)]:
        ph.level_check(level)
    lib = ph.load_library()
    assert lib.piper_hip_level_check(None) == -7
    y = np.zeros(4, F32)
    lv = ph.Level(1, 1, 50)
    assert lib.piper_hip_level_from_f32(None, 22050, y.ctypes.data_as(ph.c_f32p), 4, y.ctypes.data_as(ph.c_f32p)) == -7
    assert lib.piper_hip_level_from_f32(C.byref(lv), 22050, None, 4, y.ctypes.data_as(ph.c_f32p)) == -7
    assert lib.piper_hip_level_from_f32(C.byref(lv), 22050, None, 0, None) == 0


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    lv, p = ph.Level(3.0, 0.5, 50.0), C.c_void_p()
    assert lib.piper_hip_level_f32(None, None, 4, 22050, C.byref(lv), C.byref(p), None) == -7
    assert lib.piper_hip_voice_slot_level(None, 0, C.byref(lv)) == -7
    assert lib.piper_hip_voice_stream_set_level(None, 0, C.byref(lv)) == -7
    assert lib.piper_hip_voice_stream_level(None, 0, C.byref(lv)) == -7


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_points_are_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here, so the
    call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    with pytest.raises(ph.DeviceUnavailable):
        ph.HipBackend(0)
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, p, lv = (C.c_float * 4)(), C.c_void_p(), ph.Level(3.0, 0.5, 50.0)
    assert lib.piper_hip_level_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, 22050, C.byref(lv), C.byref(p), None) == ph.DeviceUnavailable.code
    assert not p.value
