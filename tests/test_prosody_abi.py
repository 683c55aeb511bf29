"""CPU: the prosody entry points (include/piper_hip.h "Per-phoneme prosody") — declared with the header's signatures, exported and bound,
ABI 3 kept, the record's layout, the host-side checks naming the offending field, and piper_hip_prosody_frames held to tests/prosody_ref.py
(integer equality). The header still compiles as C99."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import piper_hip as ph
import prosody_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "piper_hip.h")

SIGNATURES = {
    "piper_hip_prosody_check": "int piper_hip_prosody_check(const piper_hip_prosody* p);",
    "piper_hip_prosody_frames": "int piper_hip_prosody_frames(const piper_hip_prosody* p, const float* w0, int32_t t, int64_t cap, int32_t* frames_out, "
                                "int64_t* wanted);",
    "piper_hip_voice_slot_prosody": "int piper_hip_voice_slot_prosody(piper_hip_voice* v, int slot, const piper_hip_prosody* items, int n);",
    "piper_hip_voice_prosody_report": "int piper_hip_voice_prosody_report(const piper_hip_voice* v, int slot, int64_t* wanted_frames, int32_t* fitted, "
                                      "int max_items);",
}


def header_code():
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))


def test_the_four_symbols_are_declared_exported_and_bound():
    lib, src = ph.load_library(), header_code()
    for name, sig in SIGNATURES.items():
        assert re.sub(r"\s+", " ", sig) in src, name + ": not declared with this signature"
        assert hasattr(lib, name), name + " is not exported"
        assert name in ph.exported_symbols(), name + " is not bound by the Python shim"
    assert lib.piper_hip_abi_version() == 3 and "#define PIPER_HIP_ABI_VERSION 3" in open(HEADER).read()
    for attr in ("slot_prosody", "prosody_report"):
        assert hasattr(ph.HipRuntime, attr)
    assert callable(ph.prosody_check) and callable(ph.prosody_frames)


def test_the_record_is_40_bytes_with_the_headers_fields():
    assert C.sizeof(ph.Prosody) == 40
    assert [f[0] for f in ph.Prosody._fields_] == ["length", "min_frames", "max_frames", "noise", "t", "fit"]
    assert (ph.Prosody.t.offset, ph.Prosody.fit.offset) == (32, 36)
    m = re.search(r"typedef struct \{([^}]*)\} piper_hip_prosody;", header_code())
    assert m and [w.split()[-1].lstrip("*") for w in m.group(1).split(";") if w.strip()] == ["length", "min_frames", "max_frames", "noise", "t", "fit"]


@pytest.mark.parametrize("bad,field", [
    (dict(length=[1.0, np.nan, 1.0]), "length[1]"),
    (dict(length=[1.0, 1.0, 1000.5]), "length[2]"),
    (dict(length=[-0.1, 1.0, 1.0]), "length[0]"),
    (dict(noise=[1.0, np.inf, 1.0]), "noise[1]"),
    (dict(noise=[1.0, 1.0, -1.0]), "noise[2]"),
    (dict(min_frames=[0, -1, 0]), "min_frames[1]"),
    (dict(min_frames=[0, 0, 1000001]), "min_frames[2]"),
    (dict(max_frames=[-3, 0, 0]), "max_frames[0]"),
    (dict(max_frames=[0, 1000001, 0]), "max_frames[1]"),
    (dict(min_frames=[0, 5, 0], max_frames=[0, 4, 0]), "min_frames[1]"),
    (dict(t=0), "t = 0"),
])
def test_check_refuses_each_bad_field_and_names_it(bad, field):
    lib = ph.load_library()
    rec, _keep = ph._prosody(bad)
    assert lib.piper_hip_prosody_check(C.byref(rec)) == -7  # PIPER_HIP_ERR_ARG
    assert field in lib.piper_hip_last_error().decode()
    with pytest.raises(ph.InvalidArgument, match=re.escape(field)):
        ph.prosody_check(bad)


def test_check_accepts_the_edges_and_a_null_record_is_an_argument_error():
    ph.prosody_check(dict(length=[0.0, 1000.0], noise=[0.0, 1000.0], min_frames=[0, 1000000], max_frames=[0, 1000000]))
    ph.prosody_check(dict(min_frames=[7, 3], max_frames=[0, 3]))  # a ceiling of 0 is none
    ph.prosody_check(dict(t=5))  # every array NULL: neutral
    assert ph.load_library().piper_hip_prosody_check(None) == -7


def test_frames_equals_the_reference_on_random_inputs():
    rng = np.random.default_rng(314)
    for k in range(200):
        t = int(rng.integers(1, 120))
        w0 = (rng.random(t) * float(rng.choice([3, 12, 400]))).astype(np.float32)
        if k % 5 == 0:
            w0[rng.integers(0, t)] = np.nan
        if k % 7 == 0:
            w0[rng.integers(0, t)] = np.float32(rng.choice([1e6, 1000000.5, 3e6, 1e30, np.inf]))
        p = {}
        if k % 2:
            p["length"] = (rng.random(t) * 2.2).astype(np.float32)
        if k % 3:
            p["min_frames"] = rng.integers(0, 5, t).astype(np.int32)
            p["max_frames"] = np.where(rng.random(t) < 0.4, p["min_frames"] + rng.integers(0, 6, t), 0).astype(np.int32)
        p["fit"] = int(k % 4 != 0)
        cap = int(rng.integers(1, 4 * t + 2))
        got, wanted = ph.prosody_frames(p, w0, cap)
        ref, ref_wanted = pr.frames(w0, p, cap)
        assert np.array_equal(got, ref) and wanted == ref_wanted, k
        if p["fit"] and wanted > cap:
            assert int(got.astype(np.int64).sum()) <= cap
    got, wanted = ph.prosody_frames(None, [2.5, np.nan, 0.0, 2e6], 0)  # no record: neutral
    assert got.tolist() == [3, 0, 0, 1000000] and wanted == 1000003


def test_frames_fits_in_64_bit_integers():
    """d · cap passes 2^31 (and a float32 product would round): the quotient is the integer floor."""
    w0 = np.array([900000.0, 800000.0, 700000.0, 3.0], np.float32)
    cap = 70001
    got, wanted = ph.prosody_frames(dict(fit=1), w0, cap)
    d = [900000, 800000, 700000, 3]
    assert wanted == sum(d) and max(d) * cap > 2 ** 31
    assert got.tolist() == [x * cap // wanted for x in d] and int(got.sum()) <= cap
    assert np.array_equal(got, pr.frames(w0, dict(fit=1), cap)[0])
    same, _ = ph.prosody_frames(dict(fit=0), w0, cap)  # without fit nothing is compressed
    assert same.tolist() == d


def test_frames_refuses_a_length_mismatch_and_null_arguments():
    lib = ph.load_library()
    rec, _keep = ph._prosody(dict(length=[1.0, 1.0]))
    w0 = np.ones(3, np.float32)
    out = np.empty(3, np.int32)
    assert lib.piper_hip_prosody_frames(C.byref(rec), w0.ctypes.data_as(ph.c_f32p), 3, 0, out.ctypes.data_as(ph.c_i32p), None) == -1  # ERR_SHAPE
    assert lib.piper_hip_prosody_frames(None, None, 3, 0, out.ctypes.data_as(ph.c_i32p), None) == -7
    assert lib.piper_hip_voice_slot_prosody(None, 0, None, 0) == -7
    assert lib.piper_hip_voice_prosody_report(None, 0, None, None, 0) == -7


def test_the_header_with_the_prosody_section_is_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = ("#include \"piper_hip.h\"\n"
           "int probe(piper_hip_voice* v) {\n"
           "  float len[2] = {1.0f, 0.5f}; int32_t mn[2] = {0, 12};\n"
           "  piper_hip_prosody p = {len, mn, 0, 0, 2, 1};\n"
           "  int64_t wanted; int32_t fitted;\n"
           "  if (sizeof(piper_hip_prosody) != 40) return -1;\n"
           "  if (piper_hip_prosody_check(&p)) return -2;\n"
           "  if (piper_hip_voice_slot_prosody(v, 0, &p, 1)) return -3;\n"
           "  return piper_hip_voice_prosody_report(v, 0, &wanted, &fitted, 1);\n"
           "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src.encode(), check=True)
