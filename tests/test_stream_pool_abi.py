"""The streaming pool on the C-ABI, checked without a GPU: the header declares the four entry points, the library exports them and
the Python shim binds them and offers HipRuntime.stream_pool. ABI 3 is kept: the entry points are appended."""
import ctypes as C
import os
import re

import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
NEW = ("piper_hip_voice_stream_pool_open", "piper_hip_voice_stream_pool_join", "piper_hip_voice_stream_pool_free_rows",
       "piper_hip_voice_stream_pool_close")


def test_header_declares_stream_pool():
    src = open(HEADER).read()
    assert re.search(r"int piper_hip_voice_stream_pool_open\(piper_hip_voice\* v, int slot, int capacity, int chunk_frames\);", src)
    assert re.search(r"int piper_hip_voice_stream_pool_join\(piper_hip_voice\* v, int slot, const piper_hip_utterance\* utts, int n, "
                     r"int work_slot,\s+int\* items_out, int64_t\* samples_out\);", src)
    assert re.search(r"int piper_hip_voice_stream_pool_free_rows\(const piper_hip_voice\* v, int slot\);", src)
    assert re.search(r"int piper_hip_voice_stream_pool_close\(piper_hip_voice\* v, int slot\);", src)
    assert re.search(r"#define PIPER_HIP_ABI_VERSION\s+3\b", src)


def test_library_exports_stream_pool():
    lib = C.CDLL(ph.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert set(NEW) <= set(ph.exported_symbols())


def test_shim_binds_stream_pool():
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    for name, nargs in zip(NEW, (4, 7, 2, 2)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert len(fn.argtypes) == nargs, name
    assert callable(getattr(ph.HipRuntime, "stream_pool", None))
    for name in ("join", "step", "drop", "free_rows", "close"):
        assert hasattr(ph.StreamPool, name), name


def test_null_voice_is_refused_without_a_device():
    lib = ph.load_library()
    items = (C.c_int * 1)()
    samples = (C.c_int64 * 1)()
    assert lib.piper_hip_voice_stream_pool_open(None, 0, 4, 64) != 0
    assert lib.piper_hip_voice_stream_pool_join(None, 0, None, 1, 1, items, samples) != 0
    assert lib.piper_hip_voice_stream_pool_free_rows(None, 0) < 0
    assert lib.piper_hip_voice_stream_pool_close(None, 0) != 0
