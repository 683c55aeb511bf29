"""CPU: the host-only equaliser entry points of the library (include/piper_hip.h "Equaliser") against the numpy restatement
(tests/eq_ref.py) — the design and the host twin bit for bit, every refusal by field and section — and the device entry points'
answers without a device."""
import ctypes as C

import numpy as np
import pytest

import eq_ref as e
import piper_hip as ph

F32 = np.float32
RATES = (8000, 16000, 22050, 48000)


def sections_of_every_type():
    out = []
    for typ in e.TYPES:
        g = (6.0, -7.25) if typ in e.GAIN_TYPES else (0.0, 0.0)
        out.append([(typ, 1000.0, 0.707, g[0])])
        out.append([(typ, 3333.3, 2.5, g[1]), (typ, 10.0, 0.1, g[0]), (typ, 3600.0, 30.0, g[1])])
    return out


@pytest.mark.parametrize("rate", RATES)
def test_design_is_the_reference_bit_for_bit(rate):
    for eq in sections_of_every_type():
        got = ph.eq_design(eq, rate)
        want = np.array(e.design(eq, rate), np.float64)
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), (rate, eq, got, want)


def test_zero_db_peaking_has_b_equal_to_a():
    co = ph.eq_design([(ph.EQ_PEAKING, 440.0, 1.0, 0.0)], 22050)[0]
    assert co[0] == 1.0 and co[1] == co[3] and co[2] == co[4]


@pytest.fixture(scope="module")
def long_signal():
    rng = np.random.default_rng(77)
    x = (0.25 * rng.standard_normal(98404)).astype(F32)
    x[[3, 4500, 70001]] = [np.nan, np.inf, -np.inf]
    return x


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 32769, 98404])
def test_host_twin_is_the_reference_bit_for_bit(long_signal, n):
    x = long_signal[:n]
    for eq in (e.F1, e.F2) if n in (4097, 98404) else (e.F1,):
        got, want = ph.eq_from_f32(x, eq, 22050), e.apply(x, eq, 22050)
        assert got.size == n and np.array_equal(got.view(np.int32), want.view(np.int32)), (n, eq)


def test_host_twin_other_rates_and_section_counts(long_signal):
    x = long_signal[:9000]
    for rate in (8000, 48000):
        for eq in ([(ph.EQ_HIGHPASS, 300.0, 0.707)], [(ph.EQ_LOWSHELF, 200.0, 0.8, 4.0), (ph.EQ_NOTCH, 1000.0, 5.0)]):
            assert np.array_equal(ph.eq_from_f32(x, eq, rate).view(np.int32), e.apply(x, eq, rate).view(np.int32)), (rate, eq)


BAD = [
    ([], 22050, "eq: n "),
    ([(1, 1000.0, 1.0)] * 5, 22050, "eq: n "),
    ([(1, 1000.0, 1.0), (0, 1000.0, 1.0)], 22050, "section[1].type"),
    ([(1, 1000.0, 1.0), (1, 1000.0, 1.0), (8, 1000.0, 1.0)], 22050, "section[2].type"),
    ([(2, 9.5, 1.0)], 22050, "section[0].f0_hz"),
    ([(1, 1000.0, 1.0), (2, 9923.0, 1.0)], 22050, "section[1].f0_hz"),
    ([(2, float("nan"), 1.0)], 22050, "section[0].f0_hz"),
    ([(2, float("inf"), 1.0)], 22050, "section[0].f0_hz"),
    ([(2, 3601.0, 1.0)], 8000, "section[0].f0_hz"),
    ([(2, 100.0, 0.09)], 22050, "section[0].q"),
    ([(1, 1000.0, 1.0), (1, 1000.0, 1.0), (1, 1000.0, 1.0), (2, 100.0, 30.5)], 22050, "section[3].q"),
    ([(2, 100.0, float("nan"))], 22050, "section[0].q"),
    ([(5, 100.0, 1.0, 30.5)], 22050, "section[0].gain_db"),
    ([(6, 100.0, 1.0, -31.0)], 22050, "section[0].gain_db"),
    ([(7, 100.0, 1.0, float("nan"))], 22050, "section[0].gain_db"),
    ([(7, 100.0, 1.0, float("inf"))], 22050, "section[0].gain_db"),
    ([(5, 100.0, 1.0), (1, 100.0, 1.0, 1.0)], 22050, "section[1].gain_db"),
    ([(3, 100.0, 1.0, -0.5)], 22050, "section[0].gain_db"),
    ([(1, 1000.0, 1.0)], 7999, "rate"),
    ([(1, 1000.0, 1.0)], 48001, "rate"),
]


@pytest.mark.parametrize("eq,rate,field", BAD, ids=[f"{b[2]}-{i}" for i, b in enumerate(BAD)])
def test_every_refusal_names_its_field_and_index(eq, rate, field):
    lib = ph.load_library()
    t = ph.Eq(eq)
    if len(eq) > 4:
        t.n = len(eq)
    assert lib.piper_hip_eq_check(C.byref(t), rate) == ph.InvalidArgument.code
    assert field.encode() in lib.piper_hip_last_error(), (field, lib.piper_hip_last_error())
    out = np.zeros((4, 5), np.float64)
    assert lib.piper_hip_eq_design(C.byref(t), rate, out.ctypes.data_as(ph.c_f64p)) == ph.InvalidArgument.code
    x = np.zeros(8, F32)
    assert lib.piper_hip_eq_from_f32(C.byref(t), rate, x.ctypes.data_as(ph.c_f32p), 8, x.ctypes.data_as(ph.c_f32p)) == ph.InvalidArgument.code


def test_bounds_are_accepted():
    for eq, rate in (([(2, 10.0, 0.1), (1, 3600.0, 30.0)], 8000), ([(5, 21600.0, 1.0, 30.0), (6, 10.0, 1.0, -30.0)], 48000),
                     ([(3, 1000.0, 1.0), (4, 1000.0, 1.0), (7, 1000.0, 1.0, 0.0)], 22050)):
        ph.eq_check(eq, rate)
    lib = ph.load_library()
    assert lib.piper_hip_eq_check(None, 22050) == ph.InvalidArgument.code
    t = ph.Eq([(1, 1000.0, 1.0)])
    assert lib.piper_hip_eq_design(C.byref(t), 22050, None) == ph.InvalidArgument.code
    assert lib.piper_hip_eq_from_f32(C.byref(t), 22050, None, 4, None) == ph.InvalidArgument.code
    assert lib.piper_hip_eq_from_f32(C.byref(t), 22050, None, 0, None) == 0


def test_eq_accepts_names_and_tuples():
    assert ph.Eq([("highpass", 40, 0.707), ("peaking", 3000, 1, 6)]).sections() == [(2, 40.0, F32(0.707), 0.0), (5, 3000.0, 1.0, 6.0)]


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    t = ph.Eq([(1, 1000.0, 1.0)])
    p = C.c_void_p()
    assert lib.piper_hip_eq_f32(None, None, 4, 22050, C.byref(t), C.byref(p), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_eq(None, 0, C.byref(t)) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_set_eq(None, 0, C.byref(t)) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_eq(None, 0, C.byref(t)) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_points_are_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here, so the
    call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, t, p = (C.c_float * 4)(), ph.Eq([(1, 1000.0, 1.0)]), C.c_void_p()
    assert lib.piper_hip_eq_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, 22050, C.byref(t), C.byref(p), None) == ph.DeviceUnavailable.code
