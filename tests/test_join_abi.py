"""CPU: the host-only join entry points of the library (include/piper_hip.h "Join") against the numpy restatement (tests/join_ref.py)
— the host twin bit for bit with start / len / total, every refusal by field, the counts, the capacity, the neutral identities — and the
device entry points' answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import join_ref as jr
import piper_hip as ph

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["piper_hip_join_check", "piper_hip_join_counts", "piper_hip_join_capacity", "piper_hip_join_from_f32", "piper_hip_join_f32",
       "piper_hip_voice_slot_join", "piper_hip_voice_join_capacity", "piper_hip_voice_join_report"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def agree(got, want):
    assert got[3] == want[3], (got[3], want[3])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:3], want[1:3])
    assert np.array_equal(bits(got[0]), bits(want[0]))


@pytest.mark.parametrize("name", sorted(jr.VECTORS))
def test_host_twin_is_the_reference_on_every_named_vector(name):
    items, j, rate, gaps = jr.VECTORS[name]
    agree(ph.join_from_f32(items, j, rate, gaps), jr.join(items, j, rate, gaps))


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
def test_host_twin_is_the_reference_on_a_batch(rate):
    rng = np.random.default_rng(rate)
    items = []
    for n, lo, hi in ((0, 0, 0), (1, 0, 1), (3, 1, 2), (255, 0, 100), (256, 100, 256), (257, 90, 180), (1023, 1, 1022), (1025, 512, 513), (700, 0, 0)):
        x = (1e-3 * rng.standard_normal(n)).astype(F32)
        x[lo:hi] = (0.4 + 0.5 * rng.random(hi - lo)).astype(F32)
        items.append(x)
    items[5][[3, 200]] = [np.nan, np.inf]
    for j in (dict(trim=1, trim_threshold=0.05, trim_pad_ms=2.0, fade_ms=3.0, lead_ms=1.5, gap_ms=20.0, tail_ms=0.3),
              dict(trim=1, trim_threshold=0.05, trim_pad_ms=1000.0, fade_ms=100.0),
              dict(trim=0, lead_ms=0.1, gap_ms=0.05, fade_ms=5.0),
              dict(trim=1, trim_threshold=0.0, fade_ms=0.0, gap_ms=0.2)):
        for gaps in (None, [0.0, 0.05, 0.1, 0.15, 0.25], [1.0] * 9):
            agree(ph.join_from_f32(items, j, rate, gaps), jr.join(items, j, rate, gaps))
    agree(ph.join_from_f32(items[3:4], j, rate), jr.join(items[3:4], j, rate))


def test_neutral_identities():
    items = [jr._noise(n, n + 1) for n in (5, 0, 300, 1)]
    items[2][7] = np.nan
    y, start, length, total = ph.join_from_f32(items, ph.Join(), 22050)
    assert np.array_equal(bits(y), bits(np.concatenate(items))) and total == 306
    assert list(start) == [0, 5, 5, 305] and list(length) == [5, 0, 300, 1]
    y, start, length, total = ph.join_from_f32(items[2:3], dict(trim_threshold=0.2, trim_pad_ms=3.0, fade_ms=9.0), 22050)
    assert np.array_equal(bits(y), bits(items[2])) and total == 300 and start[0] == 0 and length[0] == 300


def test_counts_and_capacity():
    j = dict(lead_ms=0.75, gap_ms=200.0, tail_ms=10000.0, trim=1, trim_threshold=0.1, trim_pad_ms=1000.0, fade_ms=100.0)
    for rate in (8000, 22050, 48000):
        c = ph.join_counts(j, rate)
        assert c == dict(lead=jr.S(0.75, rate), gap=jr.S(200.0, rate), tail=jr.S(10000.0, rate), pad=jr.S(1000.0, rate), fade=jr.S(100.0, rate))
        n = [100, 0, 7]
        assert ph.join_capacity(j, rate, n) == jr.capacity(n, j, rate) == c["lead"] + c["tail"] + 107 + 2 * c["gap"]
        assert ph.join_capacity(j, rate, n, gaps=[1.0]) == jr.capacity(n, j, rate, [1.0]) == c["lead"] + c["tail"] + 107 + jr.S(1.0, rate) + c["gap"]
        assert ph.join_capacity(j, rate, [5]) == c["lead"] + c["tail"] + 5
    assert ph.join_counts(dict(lead_ms=0.75), 22050)["lead"] == 17


BAD = [
    (dict(lead_ms=-0.5), None, "lead_ms"), (dict(lead_ms=10000.5), None, "lead_ms"), (dict(lead_ms=float("nan")), None, "lead_ms"),
    (dict(gap_ms=-1.0), None, "gap_ms"), (dict(gap_ms=float("inf")), None, "gap_ms"),
    (dict(tail_ms=10001.0), None, "tail_ms"), (dict(tail_ms=float("nan")), None, "tail_ms"),
    (dict(trim=2), None, "trim "), (dict(trim=-1), None, "trim "),
    (dict(trim=1, trim_threshold=-0.1), None, "trim_threshold"), (dict(trim_threshold=float("inf")), None, "trim_threshold"),
    (dict(trim_threshold=float("nan")), None, "trim_threshold"),
    (dict(trim_pad_ms=1000.5), None, "trim_pad_ms"), (dict(trim_pad_ms=-1.0), None, "trim_pad_ms"),
    (dict(fade_ms=100.5), None, "fade_ms"), (dict(fade_ms=float("nan")), None, "fade_ms"),
    (dict(), [0.0, -1.0], "gaps[1]"), (dict(), [10001.0], "gaps[0]"), (dict(), [1.0, 2.0, float("nan")], "gaps[2]"),
    (dict(), [0.0] * 257, "gaps"),
]


@pytest.mark.parametrize("j,gaps,field", BAD, ids=[f"{b[2].strip()}-{i}" for i, b in enumerate(BAD)])
def test_every_refusal_names_its_field(j, gaps, field):
    lib = ph.load_library()
    jn, g, ng = ph._join(j, gaps)
    assert lib.piper_hip_join_check(C.byref(jn), g, ng) == ph.InvalidArgument.code
    assert field.encode() in lib.piper_hip_last_error(), (field, lib.piper_hip_last_error())
    out = C.c_int64()
    n = np.array([4], np.int64)
    assert lib.piper_hip_join_capacity(C.byref(jn), g, ng, 22050, n.ctypes.data_as(ph.c_i64p), 1, C.byref(out)) == ph.InvalidArgument.code
    with pytest.raises(ph.InvalidArgument):
        ph.join_from_f32([np.zeros(4, F32)], jn, 22050, gaps)


def test_bounds_are_accepted_and_the_rest_of_the_refusals():
    ph.join_check(dict(lead_ms=10000.0, gap_ms=10000.0, tail_ms=10000.0, trim=1, trim_threshold=0.0, trim_pad_ms=1000.0, fade_ms=100.0), [10000.0, 0.0])
    ph.join_check(ph.Join())
    lib = ph.load_library()
    assert lib.piper_hip_join_check(None, None, 0) == ph.InvalidArgument.code
    jn = ph.Join()
    assert lib.piper_hip_join_check(C.byref(jn), None, 2) == ph.InvalidArgument.code
    out = C.c_int64()
    n = np.zeros(300, np.int64)
    for count in (0, 257):
        assert lib.piper_hip_join_capacity(C.byref(jn), None, 0, 22050, n.ctypes.data_as(ph.c_i64p), count, C.byref(out)) == ph.InvalidArgument.code
    assert lib.piper_hip_join_counts(C.byref(jn), 0, None, None, None, None, None) == ph.InvalidArgument.code
    assert lib.piper_hip_join_counts(C.byref(jn), 22050, None, None, None, None, None) == 0


def test_host_twin_refuses_a_short_buffer_and_writes_nothing():
    lib = ph.load_library()
    jn = ph.Join(gap_ms=1.0)
    x = np.ones(10, F32)
    off, ln = np.array([0, 5], np.int64), np.array([5, 5], np.int64)
    y = np.full(32, 7.0, F32)
    total = C.c_int64()
    args = (C.byref(jn), None, 0, 8000, x.ctypes.data_as(ph.c_f32p), off.ctypes.data_as(ph.c_i64p), ln.ctypes.data_as(ph.c_i64p), 2,
            y.ctypes.data_as(ph.c_f32p))
    assert lib.piper_hip_join_from_f32(*args, 17, None, None, C.byref(total)) == ph.ShapeMismatch.code
    assert (y == 7.0).all()
    assert lib.piper_hip_join_from_f32(*args, 18, None, None, C.byref(total)) == 0 and total.value == 18
    assert (y[:5] == 1.0).all() and not y[5:13].any() and (y[13:18] == 1.0).all() and (y[18:] == 7.0).all()


def test_header_shim_and_exports_agree():
    src = open(os.path.join(ROOT, "include", "piper_hip.h")).read()
    assert "Join: trim, fade and gap" in src
    decl = set(re.findall(r"\b(piper_hip_[a-z0-9_]*join[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert {d for d in decl if "stream_pool_join" not in d} == set(NEW)  # (a pool's joins are sessions entering it, another matter)
    assert set(NEW) <= set(ph._PROTOS)
    lib = ph.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, nm), name
    assert lib.piper_hip_abi_version() == 3
    assert C.sizeof(ph.Join) == 28


def test_device_entry_points_refuse_null_handles():
    lib = ph.load_library()
    jn, p, t = ph.Join(), C.c_void_p(), C.c_int64()
    n = np.array([4], np.int64)
    assert lib.piper_hip_join_f32(None, None, n.ctypes.data_as(ph.c_i64p), n.ctypes.data_as(ph.c_i64p), 1, 22050, C.byref(jn), None, 0, C.byref(p),
                                  None, None, C.byref(t), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_join(None, 0, C.byref(jn), None, 0) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_join_capacity(None, 0, 0, C.byref(t)) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_join_report(None, 0, None, None, 0, C.byref(t)) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for the GPU-less build container")
def test_device_entry_point_is_unavailable_without_a_gpu():
    """The per-op call first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here, so the
    call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, jn, p, t = (C.c_float * 4)(), ph.Join(), C.c_void_p(), C.c_int64()
    n, o = np.array([4], np.int64), np.array([0], np.int64)
    assert lib.piper_hip_join_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), o.ctypes.data_as(ph.c_i64p), n.ctypes.data_as(ph.c_i64p), 1,
                                  22050, C.byref(jn), None, 0, C.byref(p), None, None, C.byref(t), None) == ph.DeviceUnavailable.code
