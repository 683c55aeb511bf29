"""CPU: the host-only loudness entry points of the library (include/piper_hip.h "Loudness") against the numpy restatement — the
coefficients, the sequential double twin, the gain formula, every refusal — and the device entry points' answers without a device.

The twin holds L in double and reports it rounded once to fp32, so "within 1e-9 LU of the reference" is checked where it can be seen:
the reported fp32 must be the rounding of some double within 1e-9 of the reference's L."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_ref as ld
import piper_hip as ph

F32 = np.float32


def agrees(got, want, eps=1e-9):
    if want == -math.inf:
        return got == -math.inf
    return F32(want - eps) <= F32(got) <= F32(want + eps)


def cases():
    out = [(f"{name}@{rate}", rate, getattr(ld, name)(rate)) for rate in (16000, 22050) for name in ("s1", "s2", "s3")]
    out += [(f"sine@{rate}", rate, ld.sine(rate)) for rate in (48000, 22050, 16000)]
    out += [(f"tenth sine@{rate}", rate, (0.1 * ld.sine(rate).astype(np.float64)).astype(F32)) for rate in (48000,)]
    out += [(f"edge {n}", 22050, ld.s1(22050)[:n]) for n in (8819, 8820, 11024, 11025)]
    out += [(f"s3@{rate}", rate, ld.s3(rate)) for rate in (8000, 24000, 32000, 44100)]
    out += [("empty", 22050, np.empty(0, F32)), ("silence", 22050, np.zeros(22050, F32))]
    return out


@pytest.mark.parametrize("what,rate,x", cases(), ids=[c[0] for c in cases()])
def test_host_twin_within_1e_9_of_the_reference(what, rate, x):
    assert agrees(ph.loudness_from_f32(x, rate), ld.lufs(x, rate)), (what, ph.loudness_from_f32(x, rate), ld.lufs(x, rate))


def test_host_twin_reads_non_finite_samples_as_zero():
    x = ld.s2(22050).copy()
    x[[0, 777, 50000]] = [np.inf, np.nan, -np.inf]
    assert agrees(ph.loudness_from_f32(x, 22050), ld.lufs(x, 22050))


@pytest.mark.parametrize("rate", ld.RATES)
def test_coefficients_follow_the_reference(rate):
    got, want = ph.loudness_coeffs(rate), ld.coeffs(rate)
    for g, w in zip(got, want):
        assert np.max(np.abs(g - w)) < 1e-14, (rate, g, w)
    if rate == 48000:
        assert abs(got[0][0] - 1.53512485958697) < 1e-12 and abs(got[1][1] + 1.69065929318241) < 1e-12
        assert abs(got[3][1] + 1.99004745483398) < 1e-12 and abs(got[3][2] - 0.99007225036621) < 1e-12


@pytest.mark.parametrize("loudness", [(0.0, 0.0), (-16.0, 0.0), (-23.0, 20.0), (-3.0, 6.0), (-70.0, 60.0), (-1.0, 0.5)])
def test_gain_is_the_formula_exactly(loudness):
    for L in (-8.64, -9.84, -11.07, -23.0, -70.5, -0.25, -36.123456, -math.inf):
        assert ph.loudness_gain(loudness, L) == ld.gain(loudness, L), (loudness, L)
    assert ph.loudness_gain(loudness, -math.inf) == F32(1.0)


@pytest.mark.parametrize("loudness,field", [
    ((-70.5, 0.0), "target_lufs"), ((-0.5, 0.0), "target_lufs"), ((3.0, 0.0), "target_lufs"), ((float("nan"), 0.0), "target_lufs"),
    ((float("-inf"), 0.0), "target_lufs"), ((float("inf"), 0.0), "target_lufs"),
    ((-16.0, -1.0), "max_gain_db"), ((-16.0, 60.5), "max_gain_db"), ((-16.0, float("nan")), "max_gain_db"), ((-16.0, float("inf")), "max_gain_db"),
])
def test_check_refuses_every_field_by_name(loudness, field):
    lib = ph.load_library()
    t = ph.Loudness(*loudness)
    assert lib.piper_hip_loudness_check(C.byref(t)) == ph.InvalidArgument.code
    assert field.encode() in lib.piper_hip_last_error()
    with pytest.raises(ph.InvalidArgument):
        ph.loudness_check(loudness)
    with pytest.raises(ph.InvalidArgument):
        ph.loudness_gain(loudness, -20.0)


def test_check_accepts_the_bounds_and_the_defaults():
    for loudness in [(0, 0), (-70.0, 60.0), (-1.0, 1e-3), -23.0, {"target_lufs": -16.0}]:
        ph.loudness_check(loudness)
    lib = ph.load_library()
    assert lib.piper_hip_loudness_check(None) == ph.InvalidArgument.code
    g, t = C.c_float(), ph.Loudness(-16.0, 0.0)
    assert lib.piper_hip_loudness_gain(None, C.c_float(-20.0), C.byref(g)) == ph.InvalidArgument.code
    assert lib.piper_hip_loudness_gain(C.byref(t), C.c_float(-20.0), None) == ph.InvalidArgument.code
    assert lib.piper_hip_loudness_gain(C.byref(t), C.c_float(float("nan")), C.byref(g)) == ph.InvalidArgument.code
    assert lib.piper_hip_loudness_gain(C.byref(t), C.c_float(float("inf")), C.byref(g)) == ph.InvalidArgument.code


def test_rates_outside_the_contract_are_unsupported():
    x = np.zeros(4410, F32)
    for rate in (11025, 12000, 96000, 0, -1):
        with pytest.raises(ph.UnsupportedOp):
            ph.loudness_from_f32(x, rate)
        with pytest.raises(ph.UnsupportedOp):
            ph.loudness_coeffs(rate)
    lib = ph.load_library()
    out = C.c_float()
    assert lib.piper_hip_loudness_from_f32(22050, None, 4, C.byref(out)) == ph.InvalidArgument.code
    assert lib.piper_hip_loudness_from_f32(22050, x.ctypes.data_as(ph.c_f32p), 4, None) == ph.InvalidArgument.code
    assert lib.piper_hip_loudness_from_f32(22050, None, 0, C.byref(out)) == 0 and out.value == -math.inf


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    t, out = ph.Loudness(-16.0, 0.0), C.c_float()
    assert lib.piper_hip_loudness_f32(None, None, 4, 22050, C.byref(out), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_loudness(None, 0, C.byref(t)) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_loudness(None, 0, None, None, 0) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_points_are_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here, so the
    call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, out = (C.c_float * 4)(), C.c_float(7.0)
    assert lib.piper_hip_loudness_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, 22050, C.byref(out), None) == ph.DeviceUnavailable.code
    assert out.value == 7.0
