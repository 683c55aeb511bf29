"""CPU: the fp16 precision at the ABI — the header declares it, the built library exports it, the Python twin names it."""
import os
import re

import pytest

import piper_hip as ph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piper_hip.h")
OPS = ("piper_hip_conv1d_f16", "piper_hip_convtranspose1d_f16")


def test_header_declares_the_precision_and_both_ops():
    text = open(HEADER, encoding="utf-8").read()
    assert re.search(r"^#define PIPER_HIP_PRECISION_F16 3$", text, re.M)
    for name in OPS:
        assert re.search(r"^int %s\(piper_hip_ctx\* ctx," % name, text, re.M), name


@pytest.mark.parametrize("name", OPS)
def test_library_exports_the_op_and_it_refuses_a_null_context(name):
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    assert name in ph.exported_symbols()
    assert getattr(lib, name)(None, None, None, None, None, None, None, None, None, None) == ph.InvalidArgument.code


def test_set_precision_parses_f16():
    class Lib:
        def piper_hip_voice_set_precision(self, voice, code):
            self.code = code
            return 0
    rt = ph.HipRuntime.__new__(ph.HipRuntime)
    rt.lib, rt.voice, rt._keep = Lib(), None, {}
    for name in ("f16", "fp16"):
        rt.set_precision(name)
        assert rt.lib.code == 3
    assert all(hasattr(ph.HipBackend, m) for m in ("conv1dF16", "convTranspose1dF16"))
