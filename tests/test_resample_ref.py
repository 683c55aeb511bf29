"""CPU: the output-rate contract (include/piper_hip.h "Output rate"). The library's filter table against the float64 design of
tests/resample_ref.py, the quality that table buys, the reference's own sensitivity to the defects a kernel could have, chunked = whole in
the reference, the counts and bounds, and the new entry points: declared, exported, bound, and loud without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import piper_hip as ph
import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
HOP = 256
NEW = {"piper_hip_resample_info": 5, "piper_hip_resample_taps": 4, "piper_hip_resample_count": 3, "piper_hip_resample_step_bound": 3,
       "piper_hip_wav_write_pcm16": 4, "piper_hip_resample_f32": 8, "piper_hip_resample_pcm16_f32": 9,
       "piper_hip_voice_collect_pcm16_rate": 6, "piper_hip_voice_synthesize_pcm16_rate": 7, "piper_hip_voice_stream_set_rate": 3,
       "piper_hip_voice_stream_rate": 2, "piper_hip_voice_stream_step_capacity": 2}


@pytest.fixture(scope="module")
def tables():
    return {pair: ph.resample_taps(*pair) for pair in rr.PAIRS}


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_there_are_fourteen_pairs():
    assert len(rr.PAIRS) == 14


@pytest.mark.parametrize("pair", rr.PAIRS, ids=lambda p: "%d-%d" % p)
def test_table_equals_the_float64_design(tables, pair):
    """Every entry within one fp32 ulp of the numpy value (libm and np.i0 may differ in the last double bit), nothing larger."""
    L, M, P = rr.ratio(*pair)
    assert ph.resample_info(*pair) == (L, M, P)
    assert L <= 640 and P <= 256 and P % 2 == 0
    got, want = tables[pair], rr.design(*pair).astype(np.float32)
    assert got.shape == (L, P) and got.dtype == np.float32
    assert int(ulps(got, want).max()) <= 1
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 2e-7  # unit DC gain per phase, after rounding


def test_info_formulas():
    assert ph.resample_info(22050, 8000) == (160, 441, 134)
    assert ph.resample_info(16000, 11025) == (441, 640, 70)
    assert max(rr.ratio(*p)[2] for p in rr.PAIRS) == 134
    assert max(rr.ratio(*p)[0] * rr.ratio(*p)[2] * 4 for p in rr.PAIRS) <= 121 * 1024  # the largest table


def settled(P, L, M, n_out):
    """outputs whose taps all lie inside the signal"""
    lo = rr.count(P, L, M) + 1
    return slice(lo, n_out - lo)


@pytest.mark.parametrize("pair", rr.PAIRS, ids=lambda p: "%d-%d" % p)
def test_quality_of_the_library_table(tables, pair):
    """Sines at 0.05, 0.3, 0.6 and 0.8 of the narrower Nyquist come back within 1e-4 (measured: 6.1e-5, two 16-bit steps). What lies above
    the narrower Nyquist is down by 100 dB (measured: 103.9): going down in rate, a tone at 1.15 × the output Nyquist; going up, the image
    of a tone at 0.85 × the input Nyquist, which sits at 1.15 × the input Nyquist (folded at the output Nyquist where it exceeds it).
    Twenty-four zero crossings put it there: sixteen gave 4e-3 and −75 dB."""
    fin, fout = pair
    L, M, P = rr.ratio(*pair)
    tab = tables[pair]
    N = 6000
    n_out = rr.count(N, L, M)
    keep = settled(P, L, M, n_out)
    t_in, t_out = np.arange(N, dtype=np.float64) / fin, np.arange(n_out, dtype=np.float64) * M / L / fin
    nyq = min(fin, fout) / 2.0
    for frac in (0.05, 0.3, 0.6, 0.8):
        f = frac * nyq
        y = rr.apply(np.sin(2 * np.pi * f * t_in + 0.3).astype(np.float32), tab, L, M)
        err = np.abs(y.astype(np.float64) - np.sin(2 * np.pi * f * t_out + 0.3))[keep].max()
        assert err <= 1e-4, (frac, err)
    if fout < fin:
        y = rr.apply(np.sin(2 * np.pi * 1.15 * (fout / 2.0) * t_in).astype(np.float32), tab, L, M)[keep].astype(np.float64)
        level = np.sqrt(2.0 * np.mean(y * y))  # amplitude of what came through, the tone's being 1
    else:
        f = 0.85 * fin / 2.0
        y = rr.apply(np.sin(2 * np.pi * f * t_in).astype(np.float32), tab, L, M).astype(np.float64)
        img = fin - f
        img = img if img <= fout / 2.0 else fout - img
        win = np.hanning(y[keep].size)
        ph_ = 2 * np.pi * img * t_out[keep]
        level = 2.0 * abs(np.sum(win * y[keep] * np.exp(-1j * ph_))) / win.sum()
    assert 20 * np.log10(max(level, 1e-30)) <= -100.0, 20 * np.log10(level)


def noisy(n, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


@pytest.mark.parametrize("defect", [dict(phase_shift=1), dict(swap=True), dict(descending=True), dict(fma=True)],
                         ids=["phase+1", "M-L-swapped", "descending", "fma"])
def test_the_bit_comparison_catches_planted_defects(tables, defect):
    pair = (22050, 8000)
    L, M, _ = rr.ratio(*pair)
    x = noisy(9 * HOP)
    good = rr.apply(x, tables[pair], L, M)
    bad = rr.apply(x, tables[pair], L, M, **defect)
    assert good.size == bad.size and not np.array_equal(good.view(np.int32), bad.view(np.int32))


@pytest.mark.parametrize("pair", [(22050, 8000), (22050, 48000), (22050, 32000), (16000, 8000), (16000, 11025)], ids=lambda p: "%d-%d" % p)
def test_chunked_equals_whole_in_the_reference(tables, pair):
    """A step reads its chunk, the P − 1 samples before it and nothing behind it (zeros on the last step): bit for bit the whole item."""
    L, M, P = rr.ratio(*pair)
    for frames in (1, 5, 7, 9):
        x = noisy(frames * HOP, frames)
        whole = rr.apply(x, tables[pair], L, M)
        assert whole.size == rr.count(frames * HOP, L, M) and not np.any(np.isnan(whole))
        for chunk in (1, 2, 3, 4):
            got = rr.apply_chunked(x, tables[pair], L, M, frames, chunk, HOP)
            assert np.array_equal(got.view(np.int32), whole.view(np.int32)), (frames, chunk)
            for (j0, j1), k in zip(rr.stream_ranges(frames, chunk, HOP, L, M, P), range(99)):
                assert j1 - j0 <= rr.step_bound(min(chunk, frames - k * chunk) * HOP, L, M, P)


def test_counts_and_bounds():
    for pair in rr.PAIRS:
        L, M, P = rr.ratio(*pair)
        for n in (0, 1, 2, 255, 256, 257, 10752, 1 << 33):
            assert ph.resample_count(*pair, n) == rr.count(n, L, M) == -((-n * L) // M)
            assert ph.resample_step_bound(*pair, n) == rr.step_bound(n, L, M, P)
    # 22 050 → 8 000, five frames one at a time
    L, M, P = rr.ratio(22050, 8000)
    r = rr.stream_ranges(5, 1, HOP, L, M, P)
    assert [b - a for a, b in r] == [69, 93, 93, 93, 117] and r[-1][1] == ph.resample_count(22050, 8000, 5 * HOP) == 465
    assert max(b - a for a, b in r) <= ph.resample_step_bound(22050, 8000, HOP) == 93 + 25 + 1


def test_error_paths():
    lib = ph.load_library()
    with pytest.raises(ph.UnsupportedOp):
        ph.resample_info(22050, 12345)
    with pytest.raises(ph.UnsupportedOp):
        ph.resample_taps(16000, 12345)
    with pytest.raises(ph.UnsupportedOp):
        ph.resample_info(22051, 48000)  # L = 48000 phases
    assert lib.piper_hip_resample_count(22050, 12345, 10) == ph.UnsupportedOp.code
    assert lib.piper_hip_resample_count(22050, 8000, -1) < 0 and lib.piper_hip_resample_step_bound(22050, 8000, -1) < 0
    assert lib.piper_hip_resample_count(0, 8000, 1) < 0
    small = (C.c_float * 4)()
    assert lib.piper_hip_resample_taps(22050, 8000, small, 4) == ph.ShapeMismatch.code
    pcm, got, p, cnt = (C.c_int16 * 4)(), (C.c_int64 * 1)(), C.c_void_p(), C.c_size_t()
    assert lib.piper_hip_resample_f32(None, None, 4, 22050, 8000, C.byref(p), C.byref(cnt), None) == ph.InvalidArgument.code
    assert lib.piper_hip_resample_pcm16_f32(None, None, 4, 22050, 8000, 1.0, C.byref(p), C.byref(cnt), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_collect_pcm16_rate(None, 0, None, 8000, pcm, 4) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_synthesize_pcm16_rate(None, None, None, 8000, pcm, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_set_rate(None, 0, 8000) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_rate(None, 0) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_step_capacity(None, 0) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for a machine without a GPU")
def test_per_op_is_unavailable_without_a_device():
    """As pcm16_f32: the context's device is selected before anything else is looked at, so a zeroed block in a context's place gives
    UNAVAILABLE."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, p, cnt = (C.c_float * 4)(), C.c_void_p(), C.c_size_t()
    ctx = C.cast(fake_ctx, C.c_void_p)
    assert lib.piper_hip_resample_f32(ctx, C.cast(x, C.c_void_p), 4, 22050, 8000, C.byref(p), C.byref(cnt), None) == ph.DeviceUnavailable.code
    assert lib.piper_hip_resample_pcm16_f32(ctx, C.cast(x, C.c_void_p), 4, 22050, 8000, 1.0, C.byref(p), C.byref(cnt), None) == ph.DeviceUnavailable.code
    assert not p.value


def test_abi_and_bindings():
    import re
    src = open(HEADER).read()
    assert re.search(r"#define PIPER_HIP_ABI_VERSION\s+3\b", src)
    raw = C.CDLL(ph.LIB_PATH)
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3 and C.sizeof(ph.PcmParams) == 8
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\(" % name, src), name
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert set(NEW) <= set(ph.exported_symbols())
    for name in ("resample_info", "resample_taps", "resample_count", "resample_step_bound", "wav_write_pcm16"):
        assert callable(getattr(ph, name, None)), name
    for name in ("resampleF32", "resamplePcm16F32"):
        assert callable(getattr(ph.HipBackend, name, None)), name
    for name in ("stream_set_rate", "stream_rate", "stream_step_capacity"):
        assert callable(getattr(ph.HipRuntime, name, None)), name
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_wav_write_pcm16(tmp_path):
    import wave
    pcm = (np.arange(-500, 500, dtype=np.int32) * 65).astype(np.int16)
    path = tmp_path / "r.wav"
    ph.wav_write_pcm16(path, pcm, 8000)
    with wave.open(str(path), "rb") as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (8000, 1, 2, pcm.size)
        assert np.array_equal(np.frombuffer(w.readframes(pcm.size), "<i2"), pcm)
    assert path.stat().st_size == 44 + 2 * pcm.size


def test_cli_usage_lists_output_rate(tmp_path):
    lib = os.path.join(ROOT, "piper-swift_amd", "lib")
    cli = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "piper_hip_cli.c"),
                           "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(cli)])
    out = subprocess.run([str(cli)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--output-rate" in out.stderr
