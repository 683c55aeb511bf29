"""CPU: the fp16 MRF-stage op at the ABI — the header declares it, the built library exports it, the Python twin names it."""
import os
import re

import piper_hip as ph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piper_hip.h")
OP = "piper_hip_hifigan_mrf_f16"


def test_header_declares_the_op():
    assert re.search(r"^int %s\(piper_hip_ctx\* ctx, int type," % OP, open(HEADER, encoding="utf-8").read(), re.M)


def test_library_exports_the_op_and_it_refuses_a_null_context():
    lib = ph.load_library()
    assert getattr(lib, OP)(None, 2, None, 1, 32, 4, 3, None, None, 2, None, None, 0.1, None, None) == ph.InvalidArgument.code


def test_backend_has_the_method():
    assert callable(getattr(ph.HipBackend, "hifiganMrfF16", None))
