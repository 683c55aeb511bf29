"""Batched streaming on the C-ABI, checked without a GPU: the header declares the three entry points, the library exports them
and the Python shim binds them and offers the runtime methods."""
import ctypes as C
import os
import re

import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
NEW = ("piper_hip_voice_stream_begin_batch", "piper_hip_voice_stream_next_batch", "piper_hip_voice_stream_drop")


def test_header_declares_batched_stream():
    src = open(HEADER).read()
    assert re.search(r"int piper_hip_voice_stream_begin_batch\(piper_hip_voice\* v, const piper_hip_utterance\* utts, int n, int slot, "
                     r"int chunk_frames\);", src)
    assert re.search(r"int piper_hip_voice_stream_next_batch\(piper_hip_voice\* v, int slot, float\* host_audio, int64_t max_samples, "
                     r"int64_t\* n_samples\);", src)
    assert re.search(r"int piper_hip_voice_stream_drop\(piper_hip_voice\* v, int slot, int item\);", src)


def test_library_exports_batched_stream():
    lib = C.CDLL(ph.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert set(NEW) <= set(ph.exported_symbols())


def test_shim_binds_batched_stream():
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    assert lib.piper_hip_voice_stream_begin_batch.restype is C.c_int
    assert len(lib.piper_hip_voice_stream_begin_batch.argtypes) == 5
    assert len(lib.piper_hip_voice_stream_next_batch.argtypes) == 5
    assert len(lib.piper_hip_voice_stream_drop.argtypes) == 3
    assert callable(getattr(ph.HipRuntime, "synthesize_stream_batch", None))
    assert callable(getattr(ph.HipRuntime, "stream_drop", None))


def test_null_arguments_are_refused_without_a_device():
    lib = ph.load_library()
    got = (C.c_int64 * 1)()
    assert lib.piper_hip_voice_stream_begin_batch(None, None, 1, 0, 64) < 0
    assert lib.piper_hip_voice_stream_next_batch(None, 0, None, 0, got) != 0
    assert lib.piper_hip_voice_stream_drop(None, 0, 0) != 0
