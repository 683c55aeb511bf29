"""CPU: the fp16 ResBlock op at the ABI — the header declares it, the built library exports it, the Python twin names it."""
import os
import re

import piper_hip as ph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piper_hip.h")
OP = "piper_hip_hifigan_resblock_f16"


def test_header_declares_the_op():
    assert re.search(r"^int %s\(piper_hip_ctx\* ctx, int type," % OP, open(HEADER, encoding="utf-8").read(), re.M)


def test_library_exports_the_op_and_it_refuses_a_null_context():
    lib = ph.load_library()
    assert lib.piper_hip_abi_version() == 3
    assert getattr(lib, OP)(None, 1, None, 1, 32, 4, 3, None, 1, None, None, 0.1, None, None) == ph.InvalidArgument.code


def test_backend_has_the_method():
    assert callable(getattr(ph.HipBackend, "hifiganResblockF16", None))
