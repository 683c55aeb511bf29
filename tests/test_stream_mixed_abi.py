"""CPU: the mixed-format entry points (include/piper_hip.h "Mixed formats") exist, the format record has the layout the header states,
null-voice calls are argument errors, and the Python side refuses the formats the library refuses, with the same exceptions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import piper_hip as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["piper_hip_voice_stream_set_mixed", "piper_hip_voice_stream_item_formats", "piper_hip_voice_stream_pool_join_formats",
       "piper_hip_voice_stream_next_batch_mixed", "piper_hip_voice_stream_step_capacity_bytes", "piper_hip_voice_stream_item_format"]
ERR_ARG = -7


def header():
    return open(os.path.join(ROOT, "include", "piper_hip.h")).read()


def test_symbols_are_exported_and_declared():
    lib, src = ph.load_library(), re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/piper_hip.h"
        assert name in ph.exported_symbols()
    assert lib.piper_hip_abi_version() == 3  # the ABI version stays


def test_format_record_layout_and_constants():
    assert C.sizeof(ph.StreamFormat) == 12
    assert [(n, getattr(ph.StreamFormat, n).offset) for n, _ in ph.StreamFormat._fields_] == [("out_rate", 0), ("encoding", 4), ("gain", 8)]
    src = header()
    for name, value in (("S16", 0), ("MULAW", 1), ("ALAW", 2), ("F32", 3)):
        assert re.search(r"#define\s+PIPER_HIP_ENC_%s\s+%d\b" % (name, value), src), name
        assert getattr(ph, "ENC_" + name) == value
    assert (ph.ENC_MULAW, ph.ENC_ALAW) == (ph.G711_MULAW, ph.G711_ALAW)
    zero = ph.StreamFormat()
    assert (zero.out_rate, zero.encoding, zero.gain) == (0, ph.ENC_S16, 0.0)  # all zero = s16 at the voice's rate, gain 1


def test_null_voice_is_an_argument_error():
    lib = ph.load_library()
    fmt, n, off, item = ph.StreamFormat(), (C.c_int64 * 1)(), (C.c_int64 * 1)(), (C.c_int * 1)()
    buf = (C.c_uint8 * 16)()
    utt = ph.Utterance()
    assert lib.piper_hip_voice_stream_set_mixed(None, 0) == ERR_ARG
    assert lib.piper_hip_voice_stream_item_formats(None, 0, C.byref(fmt), 1) == ERR_ARG
    assert lib.piper_hip_voice_stream_pool_join_formats(None, 0, C.byref(utt), 1, 1, C.byref(fmt), item, n) == ERR_ARG
    assert lib.piper_hip_voice_stream_next_batch_mixed(None, 0, buf, 16, n, off) == ERR_ARG
    assert lib.piper_hip_voice_stream_step_capacity_bytes(None, 0) == ERR_ARG
    assert lib.piper_hip_voice_stream_item_format(None, 0, 0, C.byref(fmt)) == ERR_ARG


def test_python_side_format_validation():
    f = ph.stream_format(rate=8000, encoding="mulaw", gain=0.5)
    assert (f.out_rate, f.encoding, f.gain, f.dtype) == (8000, ph.ENC_MULAW, 0.5, np.uint8)
    d = ph.stream_format()
    assert (d.out_rate, d.encoding, d.gain, d.dtype) == (0, ph.ENC_S16, 1.0, np.int16)
    assert ph.stream_format(48000, "f32").dtype == np.float32 and ph.stream_format(encoding="alaw").encoding == ph.ENC_ALAW
    assert ph.stream_format(encoding=ph.ENC_F32, gain=0).gain == 0.0
    for bad in (dict(encoding="opus"), dict(encoding=4), dict(encoding=-1), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")),
                dict(encoding="f32", gain=0.5)):
        with pytest.raises(ph.InvalidArgument):
            ph.stream_format(**bad)
    with pytest.raises(ph.UnsupportedOp):
        ph.stream_format(rate=12345)
    arr = ph._formats([None, dict(rate=16000), f])
    assert [(a.out_rate, a.encoding) for a in arr] == [(0, ph.ENC_S16), (16000, ph.ENC_S16), (8000, ph.ENC_MULAW)]
