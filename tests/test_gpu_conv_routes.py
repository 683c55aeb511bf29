"""GPU: every conv variant the op API reaches, at its tile edges, against float64 — and asserted to be the variant that ran.

Which kernel a conv takes is decided at launch time by host heuristics over (Cout, Lout, N, CU count); the library reports the choice per
launch (HipBackend.arm_routes / last_routes). Each case of tests/conv_route_cases.py first asserts that the variant it is there for ran, on
256 CUs (on another CU count the heuristics may choose differently: the case then skips with what ran), and then holds the output to
|Δ| ≤ OP_TOL · max(1, ‖ref‖∞) against the float64 reference of tests/conv_ref.py — for the bf16 ops on operands rounded to bf16 first.
Per case the run prints `CONVROUTE {json}`: the variant, max|Δ|, the bound and their ratio."""
import json

import numpy as np
import pytest

import conv_ref as cr
import conv_route_cases as cc
import piper_hip as ph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def armed():
    """A backend of this module's own with the route records armed: the session's shared backend stays disarmed."""
    b = ph.HipBackend(0)
    b.arm_routes(True)
    yield b
    b.arm_routes(False)
    b.close()


def up(b, a):
    return b.uploadFloat32(np.ascontiguousarray(a, np.float32))


def run_case(b, c, x, w, bias):
    """The case through its op entry point → (output [N, C, Lout] fp32, route records of the call)."""
    N, L = c["N"], c["L"]
    if c["op"] == "rb":
        out = b.hifiganResblockF32(c["type"], up(b, x), N, c["cin"], L, c["K"], c["dils"], [up(b, a) for a in w], [up(b, a) for a in bias], 0.1)
        routes = b.last_routes()
        return b.downloadFloat32(out).reshape(N, c["cin"], L), routes
    xd, wd, bd = up(b, x), up(b, w), None if bias is None else up(b, bias)
    if c["op"] == "conv":
        out, shp = b.conv1dF32(xd, list(x.shape), wd, list(w.shape), bd, stride=c["stride"], dilation=c["dil"], padL=c["pl"], padR=c["pr"], groups=c["groups"])
    elif c["op"] == "convt":
        out, shp = b.convTranspose1dF32(xd, list(x.shape), wd, list(w.shape), bd, stride=c["stride"], dilation=c["dil"], padL=c["pl"], padR=c["pr"],
                                        outputPadding=c["out_pad"], groups=c["groups"])
    elif c["op"] == "conv_bf16":
        out, shp = b.conv1dBF16(xd, list(x.shape), wd, list(w.shape), bd, dilation=c["dil"], padL=c["pl"], padR=c["pr"])
    else:
        out, shp = b.convTranspose1dBF16(xd, list(x.shape), wd, list(w.shape), bd, stride=c["stride"], padL=c["pl"], padR=c["pr"])
    routes = b.last_routes()
    y = b.downloadFloat32(out, int(np.prod(shp))).reshape(shp)
    for d in (xd, wd, out) + (() if bd is None else (bd,)):
        d.free()
    return y, routes


def assert_variant(routes, want, what):
    """Every launch of the call took the variant `want` (a prefix of the record's variant part). Skips on a CU count other than 256."""
    assert routes, f"{what}: the armed backend reported no route"
    got = cr.variants(routes)
    if all(v.startswith(want) for v in got):
        return got
    if cr.cus_of(routes) != 256:
        pytest.skip(f"{what}: {cr.cus_of(routes)} CUs choose {got}, the case is built for '{want}' on 256")
    raise AssertionError(f"{what}: wanted '{want}', ran {routes}")


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=cc.IDS)
def test_variant_at_its_tile_edges(i, armed):
    c = cc.CASES[i]
    x, w, bias = cc.inputs(i)
    y, routes = run_case(armed, c, x, w, bias)
    got = assert_variant(routes, c["want"], c["id"])
    ref = cc.reference(i, x=x, w=w, b=bias)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    r = cr.judge(y, ref)
    print("CONVROUTE " + json.dumps(dict(case=c["id"], variants=got, err=r["err"], bound=r["bound"], ratio=round(r["ratio"], 4))))
    assert r["ok"], f"{c['id']} on {got}: max|Δ| {r['err']:.3e} is {r['ratio']:.2f} × the bound {r['bound']:.3e}"


def test_disarmed_backend_reports_nothing(backend):
    """Off by default: the shared backend has never been armed, and arming / disarming forgets the records."""
    x, w, bias = cc.inputs(0)
    c = cc.CASES[0]
    backend.conv1dF32(up(backend, x), list(x.shape), up(backend, w), list(w.shape), up(backend, bias), padL=c["pl"], padR=c["pr"])
    assert backend.last_routes() == []
    b = ph.HipBackend(0)
    try:
        b.arm_routes(True)
        b.conv1dF32(up(b, x), list(x.shape), up(b, w), list(w.shape), up(b, bias), padL=c["pl"], padR=c["pr"])
        first = b.last_routes()
        assert len(first) == 1 and cr.variant_of(first[0]).startswith("stream ") and cr.parse_record(first[0])[1]["Lout"] == c["L"]
        b.leakyReluF32(up(b, x), x.size, 0.1)  # an op without a launcher that reports: the last conv's records stay
        assert b.last_routes() == first
        b.arm_routes(False)
        assert b.last_routes() == []
        b.conv1dF32(up(b, x), list(x.shape), up(b, w), list(w.shape), up(b, bias), padL=c["pl"], padR=c["pr"])
        assert b.last_routes() == []
    finally:
        b.close()
