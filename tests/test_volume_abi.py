"""CPU: the host-only volume entry points of the library (include/piper_hip.h "Per-phoneme volume") against the numpy restatement — the
frame gains and the host twin bit for bit, every refusal with its message — and the device entry points' answers without a device."""
import ctypes as C

import numpy as np
import pytest

import piper_hip as ph
import volume_ref as vr
from test_volume_ref import CYCLE, bits, signal

F32 = np.float32
HOPS = [256, 6, 250]
FRAMES = [1, 2, 37]


def gains_for(frames, seed):
    """the cycle, then gains whose differences and products round: the ramp is not exact in fp32"""
    rng = np.random.default_rng(seed)
    return [np.resize(np.array(CYCLE, F32), frames), rng.uniform(0.0, 16.0, frames).astype(F32)]


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("frames", FRAMES)
def test_host_twin_equals_the_reference_bit_for_bit(frames, hop):
    x = signal(frames * hop, 11 * frames + hop)
    for gf in gains_for(frames, frames + hop):
        got = ph.volume_from_f32(x, gf, hop)
        assert got.size == frames * hop
        assert np.array_equal(bits(got), bits(vr.apply(x, gf, hop))), (frames, hop)
    assert np.array_equal(bits(ph.volume_from_f32(x, np.ones(frames, F32), hop)), bits(x))


def test_known_answer():
    assert np.array_equal(ph.volume_from_f32(np.ones(8, F32), [1.0, 0.5], 4), np.array([1, 1, 1, 0.875, 0.75, 0.625, 0.5, 0.5], F32))


@pytest.mark.parametrize("gain,dur", [
    (list(CYCLE), [3] * 6),
    ([1.0, 0.25, 2.0, 0.5, 1.5], [2, 0, 3, 0, 1]),  # ids without frames are skipped
    ([3.0, 0.25, 2.0, 7.0], [0, 2, 2, 0]),          # the first and the last id without frames
    ([0.5, 2.0, 3.0], [0, 0, 0]),                   # an all-zero row: one frame, id 0's
    ([16.0], [37]),
    (None, [2, 0, 5]),                              # no gains: all 1.0
])
def test_frame_gains_equal_the_reference(gain, dur):
    got = ph.volume_frames(gain, dur)
    want = vr.frame_gains(gain, dur)
    assert got.size == max(sum(dur), 1) and np.array_equal(bits(got), bits(want))
    if gain is not None:  # a record without an array is all 1.0 too
        assert np.array_equal(ph.volume_frames(ph.Volume(None, len(dur)), dur), np.ones(want.size, F32))


def test_sizeof_and_layout():
    assert C.sizeof(ph.Volume) == 16
    assert ph.Volume.gain.offset == 0 and ph.Volume.t.offset == 8


def check_fails(rc_want, words, call):
    lib = ph.load_library()
    assert call(lib) == rc_want
    msg = lib.piper_hip_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("bad,at", [(float("nan"), 2), (-0.5, 0), (16.5, 4), (float("inf"), 1), (-float("inf"), 3)])
def test_check_refuses_a_gain_by_field_and_index(bad, at):
    g = np.ones(5, F32)
    g[at] = bad
    rec = ph.Volume(g.ctypes.data_as(ph.c_f32p), 5)
    check_fails(-7, ["gain[%d]" % at], lambda lib: lib.piper_hip_volume_check(C.byref(rec)))
    with pytest.raises(ph.InvalidArgument, match=r"gain\[%d\]" % at):
        ph.volume_check(g)
    with pytest.raises(ph.InvalidArgument, match=r"gain\[%d\]" % at):
        ph.volume_frames(g, [1] * 5)


def test_the_other_refusals_and_their_messages():
    d = np.array([1, 2, 3], np.int32)
    dp = d.ctypes.data_as(ph.c_i32p)
    g3 = np.ones(3, F32)
    rec3, rec2 = ph.Volume(g3.ctypes.data_as(ph.c_f32p), 3), ph.Volume(g3.ctypes.data_as(ph.c_f32p), 2)
    out, frames = np.zeros(8, F32), C.c_int64()
    op = out.ctypes.data_as(ph.c_f32p)
    check_fails(-7, ["null"], lambda lib: lib.piper_hip_volume_check(None))
    check_fails(-7, ["t = 0"], lambda lib: lib.piper_hip_volume_check(C.byref(ph.Volume(None, 0))))
    check_fails(-7, ["t = -3"], lambda lib: lib.piper_hip_volume_check(C.byref(ph.Volume(None, -3))))
    check_fails(-7, ["durations"], lambda lib: lib.piper_hip_volume_frames(C.byref(rec3), None, 3, op, 8, C.byref(frames)))
    check_fails(-7, ["t = 0"], lambda lib: lib.piper_hip_volume_frames(C.byref(rec3), dp, 0, op, 8, C.byref(frames)))
    check_fails(ph.ShapeMismatch.code, ["2 entries", "3 ids"], lambda lib: lib.piper_hip_volume_frames(C.byref(rec2), dp, 3, op, 8, C.byref(frames)))
    check_fails(ph.ShapeMismatch.code, ["5 < 6"], lambda lib: lib.piper_hip_volume_frames(C.byref(rec3), dp, 3, op, 5, C.byref(frames)))
    neg = np.array([1, -2, 3], np.int32)
    check_fails(-7, ["durations[1]"], lambda lib: lib.piper_hip_volume_frames(None, neg.ctypes.data_as(ph.c_i32p), 3, op, 8, C.byref(frames)))
    # the count alone, without a buffer
    assert ph.load_library().piper_hip_volume_frames(C.byref(rec3), dp, 3, None, 0, C.byref(frames)) == 0 and frames.value == 6
    x = np.zeros(12, F32)
    xp = x.ctypes.data_as(ph.c_f32p)
    gp = g3.ctypes.data_as(ph.c_f32p)
    check_fails(ph.ShapeMismatch.code, ["11 samples", "3 frames of 4"], lambda lib: lib.piper_hip_volume_from_f32(gp, 3, 4, xp, 11, xp))
    check_fails(-7, ["hop 0"], lambda lib: lib.piper_hip_volume_from_f32(gp, 3, 0, xp, 12, xp))
    check_fails(-7, ["hop 65537"], lambda lib: lib.piper_hip_volume_from_f32(gp, 3, 65537, xp, 12, xp))
    check_fails(-7, ["null buffer"], lambda lib: lib.piper_hip_volume_from_f32(None, 3, 4, xp, 12, xp))
    assert ph.load_library().piper_hip_volume_from_f32(None, 0, 4, None, 0, None) == 0  # nothing to do
    assert ph.load_library().piper_hip_volume_check(C.byref(ph.Volume(None, 7))) == 0
    for ok in ([0.0], [16.0], [1.0, 0.0, 16.0]):
        ph.volume_check(ok)


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    p, rec = C.c_void_p(), ph.Volume(None, 3)
    assert lib.piper_hip_volume_f32(None, None, 4, None, 1, 4, C.byref(p), None) == -7
    assert lib.piper_hip_voice_slot_volume(None, 0, C.byref(rec), 1) == -7


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_points_are_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot: a zeroed block stands in for the context,
    of which the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, g, p = (C.c_float * 4)(), (C.c_float * 1)(), C.c_void_p()
    rc = lib.piper_hip_volume_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, C.cast(g, C.c_void_p), 1, 4, C.byref(p), None)
    assert rc == ph.DeviceUnavailable.code and not p.value
