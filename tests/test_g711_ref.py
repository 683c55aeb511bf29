"""CPU: the G.711 contract (include/piper_hip.h "G.711 output"). The numpy restatement against tables made with CPython's audioop, the known
answers, the round trips, a planted defect, the host C functions, the WAV writer field by field, the command line's flag, and the new entry
points: declared, exported, bound, and loud without a device. Every comparison is integer equality."""
import ctypes as C
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import g711_ref as g
import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
LAWS = ["mulaw", "alaw"]
HASHES = {"mulaw": "81d633c9e6972a18c74a58720b96cb8ca0bdd096d4060b646dd708c3b846019a",
          "alaw": "38488f6fd710f4686360edc4d38639f96c491595ef93f8eb8d62d5e07ca6ce7b"}
PINS = {0: (0xFF, 0xD5), -1: (0x7E, 0x55), 32767: (0x80, 0xAA), -32768: (0x00, 0x2A)}
NEW = {"piper_hip_g711_from_pcm16": 4, "piper_hip_g711_to_pcm16": 4, "piper_hip_wav_write_g711": 5, "piper_hip_g711_f32": 10,
       "piper_hip_voice_collect_g711": 7, "piper_hip_voice_synthesize_g711": 8, "piper_hip_voice_stream_next_g711": 7,
       "piper_hip_voice_stream_next_batch_g711": 7}


@pytest.fixture(scope="module")
def golden():
    return g.golden()


@pytest.mark.parametrize("law", LAWS)
def test_golden_tables_are_the_ones_the_contract_names(golden, law):
    enc, dec = golden[law + "_encode"], golden[law + "_decode"]
    assert enc.dtype == np.uint8 and enc.shape == (65536,) and dec.dtype == np.int16 and dec.shape == (256,)
    assert hashlib.sha256(enc.tobytes()).hexdigest() == HASHES[law]


@pytest.mark.parametrize("law", LAWS)
def test_reference_equals_the_golden_tables(golden, law):
    assert np.array_equal(g.encode(g.all_pcm(), law), golden[law + "_encode"])
    assert np.array_equal(g.decode(np.arange(256), law), golden[law + "_decode"])
    assert np.array_equal(g.table_encode(g.all_pcm(), law), golden[law + "_encode"])
    assert np.array_equal(g.table_decode(np.arange(256), law), golden[law + "_decode"])


@pytest.mark.parametrize("law", LAWS)
def test_reference_equals_audioop_where_it_imports(law):
    audioop = pytest.importorskip("audioop")
    x = g.all_pcm()
    lin2, law2 = {"mulaw": (audioop.lin2ulaw, audioop.ulaw2lin), "alaw": (audioop.lin2alaw, audioop.alaw2lin)}[law]
    assert g.encode(x, law).tobytes() == lin2(x.astype("<i2").tobytes(), 2)
    assert g.decode(np.arange(256), law).astype("<i2").tobytes() == law2(bytes(range(256)), 2)


def test_known_answers_and_code_counts():
    for s, (mu, a) in PINS.items():
        assert int(g.encode([s], "mulaw")[0]) == mu and int(g.encode([s], "alaw")[0]) == a, s
    assert int(g.encode([-4], "mulaw")[0]) == 0x7E  # the Sun definition: μ(−1) = μ(−4)
    mu, a = g.encode(g.all_pcm(), "mulaw"), g.encode(g.all_pcm(), "alaw")
    assert np.unique(mu).size == 255 and 0x7F not in mu
    assert np.unique(a).size == 256


@pytest.mark.parametrize("law", LAWS)
def test_round_trips(law):
    c = np.arange(256, dtype=np.uint8)
    d = g.decode(c, law)
    assert np.array_equal(g.decode(g.encode(d, law), law), d)
    keep = c != 0x7F if law == "mulaw" else np.ones(256, bool)
    assert np.array_equal(g.encode(d, law)[keep], c[keep])
    if law == "mulaw":  # 0x7F decodes to 0, whose code is 0xFF
        assert int(d[0x7F]) == 0 and int(g.encode(d[0x7F:0x80], law)[0]) == 0xFF


def test_the_comparison_catches_the_ones_complement_variant():
    """ITU-T G.191's μ-law takes ~v for a negative sample's magnitude; on every negative multiple of 4 minus 1 the magnitude is one less
    than the contract's. Were the reference "fixed" that way, it would no longer match the tables."""
    x = (np.arange(-32768, 0, 4) + 3).astype(np.int16)  # −32765 … −5, −1
    good, bad = g.encode(x, "mulaw"), g.encode(x, "mulaw", ones_complement=True)
    assert np.array_equal(good, g.table_encode(x, "mulaw"))
    assert not np.array_equal(good, bad) and int(bad[-1]) == 0x7F and int(good[-1]) == 0x7E
    assert int((good != bad).sum()) >= 8  # at least the segment boundaries


@pytest.mark.parametrize("law", LAWS)
def test_host_functions_equal_the_reference(law):
    x = g.all_pcm()
    assert np.array_equal(ph.g711_encode(x, law), g.encode(x, law))
    assert np.array_equal(ph.g711_encode(x, g.LAWS[law]), g.encode(x, law))
    c = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ph.g711_decode(c, law), g.decode(c, law))
    assert np.array_equal(ph.g711_decode(bytes(range(256)), law), g.decode(c, law))
    assert ph.g711_encode(np.zeros(0, np.int16), law).size == 0 and ph.g711_decode(np.zeros(0, np.uint8), law).size == 0


def test_host_functions_arguments():
    lib = ph.load_library()
    pcm, out = (C.c_int16 * 4)(1, -1, 2, -2), (C.c_uint8 * 4)(9, 9, 9, 9)
    for law in (0, 3, -1):
        assert lib.piper_hip_g711_from_pcm16(law, pcm, 4, out) == ph.InvalidArgument.code and list(out) == [9, 9, 9, 9]
        assert lib.piper_hip_g711_to_pcm16(law, out, 4, pcm) == ph.InvalidArgument.code and list(pcm) == [1, -1, 2, -2]
        assert lib.piper_hip_wav_write_g711(b"/nonexistent/x.wav", law, out, 4, 8000) == ph.InvalidArgument.code
    assert lib.piper_hip_g711_from_pcm16(1, None, 0, None) == 0 and lib.piper_hip_g711_to_pcm16(2, None, 0, None) == 0  # n = 0
    assert lib.piper_hip_g711_from_pcm16(1, None, 4, out) == ph.InvalidArgument.code
    assert lib.piper_hip_g711_to_pcm16(1, out, 4, None) == ph.InvalidArgument.code
    assert lib.piper_hip_wav_write_g711(b"/nonexistent/x.wav", 1, out, 4, 0) == ph.InvalidArgument.code
    with pytest.raises(ph.InvalidArgument):
        ph.g711_encode([0], "g722")


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("n", [0, 1, 1000, 1001])
def test_wav_file_field_by_field(tmp_path, law, n):
    data = g.encode(((np.arange(n, dtype=np.int32) * 37) % 65536 - 32768).astype(np.int16), law)
    path = tmp_path / "g.wav"
    ph.wav_write_g711(path, data, law, 8000)
    raw = path.read_bytes()
    pad = n & 1
    assert len(raw) == 58 + n + pad
    riff, riff_size, wave = struct.unpack_from("<4sI4s", raw, 0)
    assert (riff, wave) == (b"RIFF", b"WAVE") and riff_size == len(raw) - 8
    fmt_id, fmt_size, tag, channels, rate, byte_rate, align, bits, cb = struct.unpack_from("<4sIHHIIHHH", raw, 12)
    assert (fmt_id, fmt_size, tag, channels, rate, byte_rate, align, bits, cb) == (b"fmt ", 18, 7 if law == "mulaw" else 6, 1, 8000, 8000, 1, 8, 0)
    fact_id, fact_size, fact_n = struct.unpack_from("<4sII", raw, 38)
    assert (fact_id, fact_size, fact_n) == (b"fact", 4, n)
    data_id, data_size = struct.unpack_from("<4sI", raw, 50)
    assert (data_id, data_size) == (b"data", n)
    assert raw[58:58 + n] == data.tobytes() and raw[58 + n:] == b"\0" * pad


def test_cli_knows_the_flag(tmp_path):
    """Without a device the command line gets as far as its arguments: the usage names the flag, a bad encoding is refused by name, a good
    one passes the argument check (and then fails, or not, for the device's reasons). With a device the bytes are compared
    (tests/test_gpu_g711.py)."""
    lib = os.path.join(ROOT, "piper-swift_amd", "lib")
    cli = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "piper_hip_cli.c"),
                           "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(cli)])
    out = subprocess.run([str(cli)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--output-encoding s16le|mulaw|alaw" in out.stderr
    bad = subprocess.run([str(cli), "--phoneme-ids", "1,2", "--output-raw", str(tmp_path / "x"), "--output-encoding", "g722"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "g722" in bad.stderr and "mulaw" in bad.stderr


def test_abi_and_bindings():
    src = open(HEADER).read()
    assert re.search(r"#define PIPER_HIP_ABI_VERSION\s+3\b", src)
    assert re.search(r"#define PIPER_HIP_G711_MULAW\s+1\b", src) and re.search(r"#define PIPER_HIP_G711_ALAW\s+2\b", src)
    assert 'G.711 output' in src and "G.191" in src
    raw = C.CDLL(ph.LIB_PATH)
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\(" % name, src), name
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert set(NEW) <= set(ph.exported_symbols())
    assert (ph.G711_MULAW, ph.G711_ALAW) == (1, 2)
    for name in ("g711_encode", "g711_decode", "wav_write_g711"):
        assert callable(getattr(ph, name, None)), name
    for name in ("g711F32", "downloadUint8"):
        assert callable(getattr(ph.HipBackend, name, None)), name
    for name in ("collect_g711", "synthesize_g711"):
        assert callable(getattr(ph.HipRuntime, name, None)), name
    import inspect
    for fn in (ph.HipRuntime.synthesize_stream, ph.HipRuntime.synthesize_stream_batch, ph.StreamPool.step):
        assert inspect.signature(fn).parameters["encoding"].default is None, fn
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_null_arguments():
    lib = ph.load_library()
    out, got, p, cnt = (C.c_uint8 * 4)(), (C.c_int64 * 1)(), C.c_void_p(), C.c_size_t()
    assert lib.piper_hip_g711_f32(None, None, 4, 22050, 8000, 1.0, 1, C.byref(p), C.byref(cnt), None) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_collect_g711(None, 0, None, 1, 8000, out, 4) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_synthesize_g711(None, None, None, 1, 8000, out, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_next_g711(None, 0, None, 1, out, 4, got) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_stream_next_batch_g711(None, 0, None, 1, out, 4, got) == ph.InvalidArgument.code


@pytest.mark.skipif(ph.device_count() > 0, reason="this check is for a machine without a GPU")
def test_per_op_is_unavailable_without_a_device():
    """As pcm16_f32: the context's device is selected before anything else is looked at — the law included — so a zeroed block in a
    context's place gives UNAVAILABLE, at equal rates and with a filter. piper_hip_g711_f32 is the one compute entry point that can be
    reached without a device: the other four (collect_g711, synthesize_g711, stream_next_g711, stream_next_batch_g711) take a voice, and
    piper_hip_voice_create itself is UNAVAILABLE without a device, so no voice exists to hand them; nothing stands in for one, because
    they read the voice's fields before they reach the device. test_null_arguments checks their refusal of a NULL voice."""
    lib = ph.load_library()
    fake_ctx = C.create_string_buffer(1 << 16)
    x, p, cnt = (C.c_float * 4)(), C.c_void_p(), C.c_size_t()
    ctx = C.cast(fake_ctx, C.c_void_p)
    for law in (1, 2, 7):
        for rates in ((22050, 8000), (8000, 8000)):
            assert lib.piper_hip_g711_f32(ctx, C.cast(x, C.c_void_p), 4, rates[0], rates[1], 1.0, law, C.byref(p), C.byref(cnt), None) == ph.DeviceUnavailable.code
    assert not p.value
