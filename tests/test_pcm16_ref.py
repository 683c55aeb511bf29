"""CPU: the 16-bit PCM contract. tests/pcm_ref.py (the numpy restatement the GPU tests compare against) equals the host conversion
piper_hip_pcm16_from_f32 bit for bit on a vector built to catch a float32 multiply; the new entry points are declared, exported and
bound; without a device they fail loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pcm_ref
import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
NEW = {"piper_hip_pcm16_f32": 6, "piper_hip_voice_collect_pcm16": 5, "piper_hip_voice_synthesize_pcm16": 6,
       "piper_hip_voice_stream_next_pcm16": 6, "piper_hip_voice_stream_next_batch_pcm16": 6, "piper_hip_voice_peaks": 4}


def test_reference_mode_equals_the_host_conversion():
    v = pcm_ref.adversarial_vector()
    assert v.size == 3 * 256 + 14  # k = −32767 + 257·j, j = 0 … 254, plus k = 32767
    want = ph.pcm16(v)
    got = pcm_ref.pcm16_reference(v)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(pcm_ref.pcm16_reference(v, gain=0.0), want)  # gain 0 is taken as 1.0
    # NaN → 0, ±inf and everything beyond ±1 clamp, ±0 and the denormal → 0
    tail = got[-14:]
    assert tail.tolist() == [32767, -32767, 32767, -32767, 32767, -32767, 32767, -32767, 0, 0, 0, 0, 0, 0]


def test_the_vector_catches_a_float32_multiply():
    v = pcm_ref.adversarial_vector()
    want, short = ph.pcm16(v), pcm_ref.fp32_shortcut(v)
    differ = np.flatnonzero(want != short)
    assert differ.size >= 1, "the vector cannot tell x * 32767 in float32 from the contract"
    assert np.all(np.abs(want[differ].astype(np.int32) - short[differ].astype(np.int32)) == 1)


def test_gain_is_one_float32_multiply():
    v = pcm_ref.adversarial_vector()
    for g in (0.5, 1.7):
        y = (v * np.float32(g)).astype(np.float32)
        assert np.array_equal(pcm_ref.pcm16_reference(v, g), ph.pcm16(y))


def test_normalized_mode_properties():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(4099) * 0.2).astype(np.float32)
    x[17] = np.nan
    pk = pcm_ref.peak(x)
    assert pk == np.nanmax(np.abs(x))
    s = pcm_ref.normalize_scale(pk)
    assert s == np.float32(np.float64(32767.0) / np.float64(pk))
    p = pcm_ref.pcm16_normalized(x)
    assert p[17] == 0 and int(np.abs(p.astype(np.int32)).max()) in (32766, 32767)
    assert pcm_ref.peak(np.empty(0, np.float32)) == 0 and pcm_ref.pcm16_normalized(np.empty(0, np.float32)).size == 0
    # a quiet item is scaled by 32767 / 0.01, not by 32767 / peak
    q = np.asarray([0.001, -0.002], np.float32)
    assert pcm_ref.normalize_scale(pcm_ref.peak(q)) == np.float32(3276700.0)
    assert pcm_ref.pcm16_normalized(q).tolist() == [int(np.float32(0.001) * np.float32(3276700.0)), int(np.float32(-0.002) * np.float32(3276700.0))]
    items = [x, q]
    assert np.array_equal(pcm_ref.pcm16_items(items, normalize=True), np.concatenate([p, pcm_ref.pcm16_normalized(q)]))


def test_header_declares_the_pcm_entry_points():
    src = open(HEADER).read()
    assert re.search(r"typedef struct \{\s*float gain;[^}]*int32_t normalize;[^}]*\} piper_hip_pcm_params;", src)
    assert re.search(r"int piper_hip_pcm16_f32\(piper_hip_ctx\* ctx, const float\* x, size_t count, float gain, int16_t\*\* out, piper_hip_stream stream\);", src)
    assert re.search(r"int piper_hip_voice_collect_pcm16\(piper_hip_voice\* v, int slot, const piper_hip_pcm_params\* params, int16_t\* host_pcm, "
                     r"int64_t max_samples\);", src)
    for name in ("synthesize_pcm16", "stream_next_pcm16", "stream_next_batch_pcm16"):
        assert re.search(r"int piper_hip_voice_%s\(piper_hip_voice\* v, [^;]*const piper_hip_pcm_params\* params, int16_t\* host_pcm,\s+"
                         r"int64_t max_samples, int64_t\* n_samples\);" % name, src), name
    assert re.search(r"int piper_hip_voice_peaks\(const piper_hip_voice\* v, int slot, float\* peaks, int max_items\);", src)
    assert re.search(r"#define PIPER_HIP_ABI_VERSION\s+3\b", src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_library_exports_and_shim_binds_the_pcm_entry_points():
    raw = C.CDLL(ph.LIB_PATH)
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    for name, nargs in NEW.items():
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert set(NEW) <= set(ph.exported_symbols())
    assert C.sizeof(ph.PcmParams) == 8
    for name in ("collect_pcm16", "synthesize_pcm16", "peaks"):
        assert callable(getattr(ph.HipRuntime, name, None)), name
    assert callable(getattr(ph.HipBackend, "pcm16F32", None))


def test_null_arguments_are_refused():
    lib = ph.load_library()
    pcm = (C.c_int16 * 4)()
    got = (C.c_int64 * 1)()
    pk = (C.c_float * 1)()
    p = C.c_void_p()
    assert lib.piper_hip_pcm16_f32(None, None, 4, 1.0, C.byref(p), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_collect_pcm16(None, 0, None, pcm, 4) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_synthesize_pcm16(None, None, None, pcm, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_next_pcm16(None, 0, None, pcm, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_next_batch_pcm16(None, 0, None, pcm, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_peaks(None, 0, pk, 1) == ph.InvalidArgument.code
    assert b"null" in lib.piper_hip_last_error()


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for a machine without a GPU")
def test_per_op_is_unavailable_without_a_device():
    """Every compute entry point first selects its context's device and reports UNAVAILABLE when it cannot. No context can be created here,
    so the call gets a zeroed block in its place: the device index (0) is the only thing read before the call gives up."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x = (C.c_float * 4)()
    p = C.c_void_p()
    assert lib.piper_hip_pcm16_f32(C.cast(fake_ctx, C.c_void_p), C.cast(x, C.c_void_p), 4, 1.0, C.byref(p), None) == ph.DeviceUnavailable.code
    assert not p.value
