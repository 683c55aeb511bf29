"""GPU: piper_hip_rel_attention_f32 on every route of csrc/attention.hip against the float64 reference of tests/att_ref.py under the rule
WITHOUT the floor, |Δ| ≤ OP_TOL · ‖ref‖∞ per batch item (att_ref's docstring says why), on att_ref.GPU_CASES:

  staged-tile kernel (lds), unsplit and key-split in 2 … 6 parts + merge      d 48 / 96, 4 ≤ T ≤ 1024, T % 4 == 0
  register-fragment kernel, 16 query rows per block (mfma16)                   T < 4, T % 4 ≠ 0, 1024 < T ≤ 2048
  register-fragment kernel, 8 query rows per block (mfma8)                     2048 < T ≤ 4096
  scalar kernel, strips of 4 and of 8 rows                                     d 32 / 64 / 80, and d 96 with a window of 8

with windows 0, 1, 4 and 7, one to three heads, one and three items, diffuse inputs everywhere and peaked ones on a quarter of the cases.
tests/test_att_ref.py asserts on the CPU which route each case takes on 256 CUs, that fp32 numpy stays below a tenth of the bound on these
very inputs and that each planted one-row defect is at least five times beyond it. Eight key parts need 456 CUs; that launch is run in a
child process through the tuning switch PIPER_HIP_ATT_SPLIT=8. One `ATTEXACT {json}` line per case: max|Δ| / bound
(profiles/attention_exact.md keeps the measured figures). The true-length cases are in tests/test_gpu_attention_lengths.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process of test_eight_parts_in_a_child_process: no conftest has set the path up
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.join(os.path.dirname(_here), "piper-swift_amd", "python")]

import att_ref as ar
import piper_hip as ph

pytestmark = pytest.mark.gpu


def cu_count(backend):
    """The device's CU count through the HIP runtime the library is bound to (hipDeviceAttributeMultiprocessorCount = 63), None if it
    does not answer plausibly."""
    try:
        fn = backend.lib.hipDeviceGetAttribute
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int]
        v = C.c_int(0)
        return int(v.value) if fn(C.byref(v), 63, 0) == 0 and 1 <= v.value <= 4096 else None
    except (AttributeError, OSError):
        return None


def run_case(backend, c, cus, forced_parts=None):
    """One launch against the float64 reference. → the ATTEXACT record (ok, ratio, …)."""
    d, T, w, H, N = (c[x] for x in ("d", "T", "w", "H", "N"))
    x = ar.inputs(c["kind"], d, T, w, H, N)
    ref = ar.rel_attention(*x, H, d, T, w)
    bufs = [backend.uploadFloat32(a) for a in x]
    out, shp = backend.relAttentionF32(*bufs, N, H, d, T, w)
    assert shp == [N, H * d, T]
    got = backend.downloadFloat32(out, N * H * d * T).reshape(shp)
    for b in bufs + [out]:
        b.free()
    r = ar.floorless(got, ref)
    route, parts = ("lds_split", forced_parts) if forced_parts else ar.route_of(d, T, w, H, N, cus or 256)
    rec = dict(case=ar.case_id(c), route=route, parts=parts, cus=cus, ratio=round(r["ratio"], 5), err=float(f"{r['err']:.3e}"),
               bound=float(f"{r['bound']:.3e}"), ok=bool(r["ok"]) and bool(np.all(np.isfinite(got))))
    print("ATTEXACT " + json.dumps(rec))
    return rec


@pytest.fixture(scope="module")
def cus(backend):
    return cu_count(backend)


@pytest.mark.parametrize("c", ar.GPU_CASES, ids=ar.case_id)
def test_rel_attention_float64(c, backend, cus):
    try:
        rec = run_case(backend, c, cus)
    except ph.ExecutionError as e:  # a launch or a copy that failed on the device is a finding, not a case to go on from
        if isinstance(e, (ph.UnsupportedOp, ph.ShapeMismatch, ph.InvalidArgument)):  # (the library refused the shape: this case fails)
            raise
        pytest.exit(f"{ar.case_id(c)}: {type(e).__name__}: {e}; nothing more is started on the GPU", returncode=3)
    if cus == 256:  # the routes tests/test_att_ref.py asserts are the ones this device takes
        assert (rec["route"], rec["parts"]) == ar.route_of(c["d"], c["T"], c["w"], c["H"], c["N"])
        if c["T"] == 1100 and (c["d"] not in (48, 96) or c["w"] > 7):
            assert rec["route"] == "scalar8"
    assert rec["ok"], f"{rec['case']} ({rec['route']}, {rec['parts']} parts): max|Δ| {rec['err']:.3e} is {rec['ratio']:.2f} × OP_TOL · ‖ref‖∞"


def test_eight_parts_in_a_child_process():
    """PIPER_HIP_ATT_SPLIT=8 (read once per process, needs PIPER_HIP_TUNING=1): eight key parts of one tile each and the merge over all of
    them at T = 1024 and 900 (the last part 4 keys long), d 96 and 48 — the part count a device of 456 CUs or more chooses by itself."""
    env = dict(os.environ, PIPER_HIP_TUNING="1", PIPER_HIP_ATT_SPLIT="8")
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.exit("forced 8 parts: the child hung on the GPU; nothing more is started on it", returncode=3)
    print(out.stdout[-10000:])
    if out.returncode < 0 or out.returncode in (134, 139):  # died on a signal: a GPU fault or an abort — a finding, not a test to go on from
        pytest.exit(f"forced 8 parts: the child died with status {out.returncode}; nothing more is started on the GPU\n" + out.stderr[-3000:], returncode=3)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "child ok" in out.stdout


def _child():
    backend = ph.HipBackend(0)
    try:
        bad = []
        for c in ar.FORCED_PARTS_CASES:
            rec = run_case(backend, c, None, ar.FORCED_PARTS)
            if not rec["ok"]:
                bad.append(rec)
        assert "PIPER_HIP_ATT_SPLIT=8" in ph.config_string(), ph.config_string()
        assert not bad, bad
    finally:
        backend.close()
    print("child ok")


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    _child()
