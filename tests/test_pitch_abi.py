"""CPU: the host-only pitch entry points of the library (include/piper_hip.h "Pitch") against the numpy restatement (tests/pitch_ref.py)
— the host twin and the table bit for bit, the counts, every refusal by field — and the device entry points' answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_ref as pr
import piper_hip as ph

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["piper_hip_pitch_check", "piper_hip_pitch_info", "piper_hip_pitch_count", "piper_hip_pitch_taps", "piper_hip_pitch_from_f32",
       "piper_hip_pitch_f32", "piper_hip_voice_slot_pitch", "piper_hip_voice_pitch_samples"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def signal(n, seed):
    """Noise with a NaN, both infinities, a denormal and a −0 in it where it is long enough"""
    x = pr.noise(n, seed)
    if n >= 23:
        x[[1, 7, n - 2, 11, 12]] = [np.nan, np.inf, -np.inf, 1e-42, -0.0]
    return x


@pytest.mark.parametrize("st", pr.SHIFTS)
@pytest.mark.parametrize("n", pr.SIZES)
def test_host_twin_is_the_reference(n, st):
    x = signal(n, n + 1)
    got, want = ph.pitch_from_f32(x, st), pr.apply(x, st)
    assert got.size == want.size == ph.pitch_count(st, n) == pr.count(n, pr.step(st))
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("st", pr.SHIFTS + (-7.0, 1e-9))
def test_table_is_the_reference_table(st):
    Q, P, rf = ph.pitch_info(st)
    assert Q == pr.step(st) and P == pr.taps(Q) and rf == F32(Q / 2.0 ** 32)
    got = ph.pitch_taps(st)
    assert got.shape == (129, P) and got.dtype == F32 and got.nbytes <= 49536
    assert np.array_equal(bits(got), bits(pr.table(Q)))


def test_counts():
    for st in pr.SHIFTS:
        Q = pr.step(st)
        for n in (0, 1, 2, 255, 256, 257, 22050, (1 << 30) - 1):
            assert ph.pitch_count(st, n) == pr.count(n, Q)
    assert ph.pitch_count(0.0, 12345) == 12345 and ph.pitch_count(1e-9, 7) == 7
    assert ph.pitch_count(-12.0, 5) == 10 and ph.pitch_count(12.0, 5) == 3


def test_neutral_passes_bit_for_bit():
    x = signal(300, 5)
    for st in (0.0, -0.0, 1e-9):
        assert np.array_equal(bits(ph.pitch_from_f32(x, st)), bits(x))


BAD = [(12.5, 0, "semitones"), (-12.001, 1, "semitones"), (float("nan"), 0, "semitones"), (float("inf"), 0, "semitones"),
       (float("-inf"), 1, "semitones"), (3.0, 2, "keep_tempo"), (0.0, -1, "keep_tempo")]


@pytest.mark.parametrize("st,keep,field", BAD, ids=["%s-%d" % (b[2], i) for i, b in enumerate(BAD)])
def test_every_refusal_names_its_field(st, keep, field):
    lib = ph.load_library()
    p = ph.Pitch(st, keep)
    assert lib.piper_hip_pitch_check(C.byref(p)) == ph.InvalidArgument.code
    assert field.encode() in lib.piper_hip_last_error(), (field, lib.piper_hip_last_error())
    with pytest.raises(ph.InvalidArgument):
        ph.pitch_check(p)
    if field == "semitones":
        x, y = np.zeros(4, F32), np.zeros(16, F32)
        tab = np.zeros(129 * 96, F32)
        for rc in (lib.piper_hip_pitch_info(st, None, None, None), lib.piper_hip_pitch_count(st, 4),
                   lib.piper_hip_pitch_taps(st, tab.ctypes.data_as(ph.c_f32p), tab.size),
                   lib.piper_hip_pitch_from_f32(st, x.ctypes.data_as(ph.c_f32p), x.size, y.ctypes.data_as(ph.c_f32p), y.size, None)):
            assert rc == ph.InvalidArgument.code
            assert b"semitones" in lib.piper_hip_last_error()
        with pytest.raises(ph.InvalidArgument):
            ph.pitch_from_f32(x, st)


def test_bounds_are_accepted_and_the_rest_of_the_refusals():
    for st in (-12.0, 12.0, 0.0):
        for keep in (0, 1):
            ph.pitch_check(ph.Pitch(st, keep))
    ph.pitch_check(3.5)
    ph.pitch_check((3.5, 0))
    lib = ph.load_library()
    assert lib.piper_hip_pitch_check(None) == ph.InvalidArgument.code
    assert lib.piper_hip_pitch_info(3.0, None, None, None) == 0
    assert lib.piper_hip_pitch_count(3.0, -1) == ph.InvalidArgument.code
    assert lib.piper_hip_pitch_count(3.0, 1 << 30) == ph.InvalidArgument.code
    assert lib.piper_hip_pitch_taps(3.0, None, 1 << 20) == ph.InvalidArgument.code
    tab = np.zeros(129 * 58, F32)
    assert lib.piper_hip_pitch_taps(3.0, tab.ctypes.data_as(ph.c_f32p), tab.size - 1) == ph.ShapeMismatch.code
    assert lib.piper_hip_pitch_taps(3.0, tab.ctypes.data_as(ph.c_f32p), tab.size) == 0


def test_host_twin_refuses_a_short_buffer_and_writes_nothing():
    lib = ph.load_library()
    x = np.ones(10, F32)
    y = np.full(32, 7.0, F32)
    got = C.c_size_t()
    args = (-12.0, x.ctypes.data_as(ph.c_f32p), x.size, y.ctypes.data_as(ph.c_f32p))
    assert lib.piper_hip_pitch_from_f32(*args, 19, C.byref(got)) == ph.ShapeMismatch.code
    assert (y == 7.0).all()
    assert lib.piper_hip_pitch_from_f32(*args, 20, C.byref(got)) == 0 and got.value == 20
    assert (y[20:] == 7.0).all() and np.array_equal(bits(y[:20]), bits(pr.apply(x, -12.0)))


def test_header_shim_and_exports_agree():
    src = open(os.path.join(ROOT, "include", "piper_hip.h")).read()
    assert "Pitch: per-item semitone shift" in src
    decl = set(re.findall(r"\b(piper_hip_[a-z0-9_]*pitch[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert decl == set(NEW)
    assert set(NEW) <= set(ph._PROTOS)
    lib = ph.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, nm), name
    assert lib.piper_hip_abi_version() == 3
    assert C.sizeof(ph.Pitch) == 8


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    p, n, t = C.c_void_p(), C.c_size_t(), C.c_int64()
    it = ph.Pitch(3.0, 0)
    assert lib.piper_hip_pitch_f32(None, None, 0, 3.0, C.byref(p), C.byref(n), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_pitch(None, 0, C.byref(it), 1) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_pitch_samples(None, 0, None, 0, C.byref(t)) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_point_is_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here, so the
    call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, p, n = (C.c_float * 4)(), C.c_void_p(), C.c_size_t()
    assert lib.piper_hip_pitch_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, 3.0, C.byref(p), C.byref(n),
                                   None) == ph.DeviceUnavailable.code
