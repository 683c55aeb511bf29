"""CPU: the bounded pool join on the C-ABI (include/piper_hip.h "Streaming pool: joins with predicted durations that never wait"): the header
declares the three entry points, the library exports them, null-voice calls are argument errors, and the Python shim binds them and
offers StreamPool.join_bounded / item_samples / joins_pending. ABI 3 is kept: the entry points are appended."""
import ctypes as C
import os
import re

import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")
NEW = ("piper_hip_voice_stream_pool_join_bounded", "piper_hip_voice_stream_pool_item_samples", "piper_hip_voice_stream_pool_joins_pending")
ERR_ARG = -7


def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int piper_hip_voice_stream_pool_join_bounded\(piper_hip_voice\* v, int slot, const piper_hip_utterance\* utts, int n, "
                     r"int work_slot,\s+int max_frames, const piper_hip_stream_format\* fmts, int\* items_out\);", src)
    assert re.search(r"int piper_hip_voice_stream_pool_item_samples\(piper_hip_voice\* v, int slot, int item, int64_t\* samples\);", src)
    assert re.search(r"int piper_hip_voice_stream_pool_joins_pending\(piper_hip_voice\* v, int slot\);", src)
    assert re.search(r"#define PIPER_HIP_ABI_VERSION\s+3\b", src)


def test_library_exports_the_entry_points():
    lib = C.CDLL(ph.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert set(NEW) <= set(ph.exported_symbols())


def test_null_voice_is_an_argument_error():
    lib = ph.load_library()
    items, samples = (C.c_int * 1)(), C.c_int64()
    utt, fmt = ph.Utterance(), ph.StreamFormat()
    assert lib.piper_hip_voice_stream_pool_join_bounded(None, 0, C.byref(utt), 1, 1, 64, None, items) == ERR_ARG
    assert lib.piper_hip_voice_stream_pool_join_bounded(None, 0, C.byref(utt), 1, 1, 64, C.byref(fmt), items) == ERR_ARG
    assert lib.piper_hip_voice_stream_pool_item_samples(None, 0, 0, C.byref(samples)) == ERR_ARG
    assert lib.piper_hip_voice_stream_pool_joins_pending(None, 0) == ERR_ARG
    assert b"null" in lib.piper_hip_last_error()


def test_abi_version_and_signature_table():
    lib = ph.load_library()  # binds every entry of the signature table: raises if one is missing
    assert lib.piper_hip_abi_version() == 3
    for name, nargs in zip(NEW, (8, 4, 2)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert len(fn.argtypes) == nargs, name
    for name in ("join_bounded", "item_samples", "joins_pending"):
        assert callable(getattr(ph.StreamPool, name, None)), name
