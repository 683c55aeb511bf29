"""The op-level C ABI (csrc/ops_basic.hip, the WaveNet-layer and ResBlock entry points of csrc/ops_conv.cpp) against float64 at every
dispatch branch and tile edge: the kernels and guards that the known-answer cases of tests/test_gpu_ops.py, which sit at Piper's own
shapes, never execute. References, rules, case tables and inputs: tests/ops_ref.py (checked on the CPU by tests/test_ops_ref.py).
Per case one `OPSEDGE {json}` line: the op, the shape, the worst ratio to its bound."""
import json
import math

import numpy as np
import pytest

import conv_ref as cr
import ops_ref as opr
import piper_hip as ph
from conftest import OP_TOL, assert_close
from test_gpu_ops import dl, routes_armed, up

pytestmark = pytest.mark.gpu

GUARD = np.float32(-77.25)  # what the floats around a caller-provided output hold before and after the op


def report(op, shape, ratio, **extra):
    print("OPSEDGE " + json.dumps(dict(op=op, shape=shape, ratio=round(ratio, 5) if math.isfinite(ratio) else str(ratio), **extra)))


def check_tol(op, shape, got, ref, tol, **extra):
    """assert_close's rule, reported as a ratio first."""
    report(op, shape, opr.judge_tol(got, ref, tol)["ratio"] if np.size(ref) else 0.0, **extra)
    assert_close(got, ref, tol, f"{op} {shape}")


def check_exact(op, shape, got, ref, **extra):
    r = opr.judge_exact(got, ref)
    report(op, shape, r["ratio"], **extra)
    assert r["ok"], f"{op} {shape}: differs from numpy at flat index {r['at']}"


def check_elem(op, shape, got, ref, bound, **extra):
    r = opr.judge_elem(got, ref, bound)
    report(op, shape, r["ratio"], **extra)
    assert r["ok"], f"{op} {shape}: element {r['at']} is {r['ratio']:.3f} × its bound"


def off_by_one_float(b, a):
    """`a` on the device at a 16-byte aligned address + 4: unary_f32 / binary_broadcast_f32 take their scalar loop (vec_ok == 0). Returns
    (the view, the buffer that owns it) as tests/test_gpu_eq.py builds one."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = up(b, np.concatenate([np.zeros(1, np.float32), a, np.zeros(3, np.float32)]))
    assert buf.ptr % 16 == 0
    return ph.DeviceBuffer(b, buf.ptr + 4, a.size, owned=False), buf


def guarded_out(b, n):
    """A caller-provided output of n floats one float off 16-byte alignment, GUARD on both sides. → (address, owning buffer)."""
    buf = up(b, np.full(n + 8, GUARD, np.float32))
    assert buf.ptr % 16 == 0
    return buf.ptr + 4, buf


def read_guarded(b, buf, n, what):
    whole = b.downloadFloat32(buf, n + 8)
    assert np.all(whole[:1] == GUARD) and np.all(whole[n + 1:] == GUARD), f"{what}: wrote outside the caller's output"
    return whole[1:n + 1]


# ------------------------------------------------------------------------------------------------ add_layernorm
@pytest.mark.parametrize("idx", range(len(opr.LN_CASES)), ids=[f"C{c[0]}_T{c[1]}_N{c[2]}_{'y' if c[3] else 'noy'}{'_offset' if c[4] else ''}" for c in opr.LN_CASES])
def test_add_layernorm(idx, backend):
    """add_layernorm_kernel<12> / <32> / add_layernorm_big_kernel: the C thresholds 192 | 193 and 512 | 513, `c < C` inside a register slot,
    `t < T` inside a block, batch strides, the y == NULL branch, a common-mode offset per kernel (ops_ref.LN_CASES says which case is which)."""
    C, T, N, with_y, offset = opr.LN_CASES[idx]
    x, y, g, be = opr.ln_inputs(idx)
    b = backend
    out, shp = b.addLayerNormF32(up(b, x), None if y is None else up(b, y), up(b, g), up(b, be), N, C, T, opr.LN_EPS)
    assert shp == [N, C, T]
    check_tol("add_layernorm", [N, C, T], dl(b, out, shp), opr.add_layernorm(x, y, g, be, opr.LN_EPS), OP_TOL, kernel=opr.ln_kernel(C), y=with_y, offset=offset)


# ------------------------------------------------------------------------------------------------ matmul
@pytest.mark.parametrize("idx", range(len(opr.MATMUL_CASES)), ids=["x".join("_".join(map(str, s)) for s in c) for c in opr.MATMUL_CASES])
def test_matmul(idx, backend):
    """matmul_kernel: the M-edge guard in blockIdx.y > 0, K below / at / past a 16-deep stage, ragged N tiles, both lead-dim strides in the
    host loop and in blockIdx.z, an empty result."""
    sa, sb = opr.MATMUL_CASES[idx]
    a, bm = opr.matmul_inputs(idx)
    ref, bound = opr.matmul(a, bm)
    b = backend
    dummy = np.zeros(1, np.float32)
    out, shp = b.matmulF32(up(b, a if a.size else dummy), list(sa), up(b, bm if bm.size else dummy), list(sb))
    assert shp == list(ref.shape)
    if not ref.size:
        assert out.ptr
        report("matmul", [list(sa), list(sb)], 0.0, empty=True)
        return
    check_elem("matmul", [list(sa), list(sb)], dl(b, out, shp), ref, bound)


# ------------------------------------------------------------------------------------------------ softmax, reduce_mean
@pytest.mark.parametrize("idx", range(len(opr.SOFTMAX_CASES)), ids=[f"{r}x{c}{'_masked' if m else ''}" for r, c, m in opr.SOFTMAX_CASES])
def test_softmax(idx, backend):
    """softmax_wave_kernel | softmax_block_kernel at 2048 | 2049 columns, the 64-lane edge, the row-stride loop of either, −1e4 mask fill."""
    rows, cols, masked = opr.SOFTMAX_CASES[idx]
    x = opr.softmax_input(idx)
    out, shp = backend.softmaxLastDimF32(up(backend, x), [rows, cols])
    got = dl(backend, out, shp)
    check_tol("softmax", [rows, cols], got, opr.softmax(x), opr.SOFTMAX_TOL, kernel="wave" if cols <= 2048 else "block", masked=masked)
    if masked:
        assert np.all(got[x == opr.MASK_FILL] == 0.0), "a masked key kept weight"


@pytest.mark.parametrize("idx", range(len(opr.REDUCE_CASES)), ids=[f"{r}x{c}" for r, c in opr.REDUCE_CASES])
def test_reduce_mean(idx, backend):
    """reduce_mean_lastdim_kernel: fewer columns than lanes, the 64-lane edge, many strides per lane, the row-stride loop."""
    rows, cols = opr.REDUCE_CASES[idx]
    x = opr.reduce_input(idx)
    ref, bound = opr.reduce_mean(x)
    out, shp = backend.reduceMeanLastDimF32(up(backend, x), [rows, cols])
    assert shp == [rows]
    check_elem("reduce_mean", [rows, cols], dl(backend, out, shp), ref, bound)


def test_reduce_mean_rank3(backend):
    """The rows are the product of every leading dim."""
    x = opr.gather_input((3, 5, 7), 2)
    ref, bound = opr.reduce_mean(x)
    out, shp = backend.reduceMeanLastDimF32(up(backend, x), [3, 5, 7])
    assert shp == [3, 5]
    check_elem("reduce_mean", [3, 5, 7], dl(backend, out, shp), ref, bound)


# ------------------------------------------------------------------------------------------------ the gather family
@pytest.mark.parametrize("shape", opr.GATHER_SHAPES, ids=lambda s: "rank%d" % len(s))
def test_pad_every_axis_both_sides(shape, backend):
    """gather4_kernel through pad: `d < rank` for ranks 1 to 4, `inside` on both sides of every axis, a fill that is not zero."""
    x = opr.gather_input(shape)
    pads = opr.pads_for(shape)
    ref = opr.pad(x, pads, opr.PAD_VALUE)
    out, shp = backend.padConstantF32(up(backend, x), list(shape), pads, opr.PAD_VALUE)
    assert shp == list(ref.shape)
    check_exact("pad", list(shape), dl(backend, out, shp), ref, value=opr.PAD_VALUE)


def test_pad_past_the_grid_cap(backend):
    """3·2²⁰ + 5 outputs: more than 8·CUs blocks of 1024, so every thread of gather4_kernel runs its stride loop more than once."""
    shape, pads = opr.BIG_PAD
    x = opr.gather_input(shape)
    ref = opr.pad(x, pads, opr.PAD_VALUE)
    assert ref.size == opr.BIG
    out, shp = backend.padConstantF32(up(backend, x), list(shape), pads, opr.PAD_VALUE)
    assert shp == list(ref.shape)
    check_exact("pad", list(shape), dl(backend, out, shp), ref, outputs=opr.BIG)
    out.free()


def test_transpose_every_permutation(backend):
    """All 24 orders of a (3, 5, 2, 7) tensor, every order of ranks 1 to 3."""
    import itertools
    for shape in opr.GATHER_SHAPES[:3] + [opr.PERM_SHAPE]:
        x = opr.gather_input(shape)
        xd = up(backend, x)
        worst = 0.0
        for perm in itertools.permutations(range(len(shape))):
            out, shp = backend.transposeF32(xd, list(shape), list(perm))
            ref = opr.transpose(x, perm)
            assert shp == list(ref.shape)
            r = opr.judge_exact(dl(backend, out, shp), ref)
            assert r["ok"], f"transpose {shape} perm {perm}: differs at flat index {r['at']}"
            worst = max(worst, r["ratio"])
        report("transpose", list(shape), worst, perms=math.factorial(len(shape)))


@pytest.mark.parametrize("shape,axis", opr.SLICE_SHAPES, ids=lambda v: "rank%d" % len(v) if isinstance(v, tuple) else None)
def test_slice_ranges(shape, axis, backend):
    """An empty range, steps that do not divide the range, negative steps (the count and the last index come from the host's rounding)."""
    x = opr.gather_input(shape, 3)
    xd = up(backend, x)
    for start, end, step in opr.SLICES:
        ref = opr.slice_(x, axis, start, end, step)
        out, shp = backend.sliceF32(xd, list(shape), axis, start, end, step)
        assert shp == list(ref.shape), (start, end, step)
        if ref.size == 0:
            assert out.ptr  # an empty tensor still has a buffer and a shape
            continue
        r = opr.judge_exact(dl(backend, out, shp), ref)
        assert r["ok"], f"slice {shape} axis {axis} [{start}:{end}:{step}]: differs at flat index {r['at']}"
    report("slice", list(shape), 0.0, axis=axis, ranges=len(opr.SLICES))


def test_expand(backend):
    """Stride-0 axes: two at once, a leading one, every one."""
    for ins, outs in opr.EXPANDS:
        e = opr.gather_input(ins, 1)
        out = backend.expandF32(up(backend, e), list(ins), list(outs))
        check_exact("expand", [list(ins), list(outs)], dl(backend, out, list(outs)), opr.expand(e, outs))


def test_concat_split_odd_sizes(backend):
    """The strided copies of concat2 / split2 with odd channel counts, an odd row length and three items; a split at 0 and at C."""
    b = backend
    a, c = opr.gather_input((3, 5, 7), 4), opr.gather_input((3, 2, 7), 5)
    out, shp = b.concat2Axis1F32(up(b, a), [3, 5, 7], up(b, c), [3, 2, 7])
    ref = opr.concat2_axis1(a, c)
    assert shp == [3, 7, 7]
    check_exact("concat", [[3, 5, 7], [3, 2, 7]], dl(b, out, shp), ref)
    for c0 in (5, 0, 7, 3):
        (o0, s0), (o1, s1) = b.split2Axis1F32(out, shp, c0)
        r0, r1 = opr.split2_axis1(ref, c0)
        assert s0 == list(r0.shape) and s1 == list(r1.shape)
        for o, s, r in ((o0, s0, r0), (o1, s1, r1)):
            if r.size:
                check_exact("split", [3, 7, 7], dl(b, o, s), r, c0=c0)


# ------------------------------------------------------------------------------------------------ unary
def check_unary(op, got, x, shape, **extra):
    ref = opr.unary(op, x, opr.UNARY_ALPHA.get(op, 0.0))
    if op in opr.UNARY_EXACT:
        check_exact(opr.UNARY_NAMES[op], shape, got, ref, **extra)
    else:
        check_tol(opr.UNARY_NAMES[op], shape, got, ref, opr.UNARY_TOL[op], **extra)


@pytest.mark.parametrize("op", opr.UNARY_OPS, ids=[opr.UNARY_NAMES[o] for o in opr.UNARY_OPS])
def test_unary_off_alignment(op, backend):
    """unary_kernel's scalar loop (vec_ok == 0): source and caller-provided output one float off 16-byte alignment, then each alone; and
    the aligned float4 body with its tail on the same values. alpha reaches both branches; ±0 and the finite extremes are in."""
    b = backend
    x = opr.unary_input(op)
    n, alpha = x.size, opr.UNARY_ALPHA.get(op, 0.0)
    xa = up(b, x)
    xm, keep = off_by_one_float(b, x)
    for src, out_off, what in ((xm, True, "src+4 out+4"), (xm, False, "src+4"), (xa, True, "out+4")):
        if out_off:
            addr, obuf = guarded_out(b, n)
            res = b.unaryF32(op, src, n, alpha, out=addr)
            assert res.ptr == addr and not res.owned
            got = read_guarded(b, obuf, n, f"{opr.UNARY_NAMES[op]} {what}")
        else:
            got = b.downloadFloat32(b.unaryF32(op, src, n, alpha))
        check_unary(op, got, x, [n], path=what)
    check_unary(op, b.downloadFloat32(b.unaryF32(op, xa, n, alpha)), x, [n], path="aligned")


def test_unary_past_the_grid_cap(backend):
    """3·2²⁰ + 5 elements: unary_kernel's grid stops at 8·CUs blocks, the float4 loop strides, one element is left for the tail."""
    x = opr.unary_input(ph.LEAKYRELU, opr.BIG)
    out = backend.unaryF32(ph.LEAKYRELU, up(backend, x), x.size, opr.UNARY_ALPHA[ph.LEAKYRELU])
    check_unary(ph.LEAKYRELU, backend.downloadFloat32(out), x, [x.size], path="aligned")
    out.free()


# ------------------------------------------------------------------------------------------------ binary
def check_binary(op, got, a, bm, shape, **extra):
    ref = opr.binary(op, a, bm)
    if op in opr.BINARY_EXACT:
        check_exact(opr.BINARY_NAMES[op], shape, np.asarray(got).reshape(ref.shape), ref, **extra)
    else:
        check_tol(opr.BINARY_NAMES[op], shape, got, ref, opr.BINARY_TOL[op], **extra)


@pytest.mark.parametrize("op", [ph.ADD, ph.DIV, ph.POW], ids=["add", "div", "pow"])
def test_binary_off_alignment(op, backend):
    """binary_flat_kernel's scalar loop (vec_ok == 0): a, b and the caller-provided output one float off alignment; then only b off (its
    alignment counts unless b is the scalar); then the scalar-b path with a off."""
    b = backend
    n = opr.BINARY_N
    a, bm = opr.binary_inputs((n,), (n,), op, 90)
    am, keep_a = off_by_one_float(b, a)
    bmis, keep_b = off_by_one_float(b, bm)
    addr, obuf = guarded_out(b, n)
    res, shp = b.binaryBroadcastF32(op, am, [n], bmis, [n], out=addr)
    assert shp == [n] and res.ptr == addr and not res.owned
    check_binary(op, read_guarded(b, obuf, n, opr.BINARY_NAMES[op]), a, bm, [n], path="a+4 b+4 out+4")
    out, shp = b.binaryBroadcastF32(op, up(b, a), [n], bmis, [n])
    check_binary(op, dl(b, out, shp), a, bm, [n], path="b+4")
    a1, s1 = opr.binary_inputs((n,), (1,), op, 91)
    a1m, keep_1 = off_by_one_float(b, a1)
    out, shp = b.binaryBroadcastF32(op, a1m, [n], up(b, s1), [1])
    check_binary(op, dl(b, out, shp), a1, s1, [n], path="a+4 scalar b")


@pytest.mark.parametrize("idx", range(len(opr.BINARY_TAIL_CASES)), ids=["x".join("_".join(map(str, s)) for s in c) for c in opr.BINARY_TAIL_CASES])
def test_binary_flat_tail(idx, backend):
    """binary_flat_kernel on aligned pointers with 4k + 1, + 2, + 3 elements: the scalar tail behind the float4 body, same-shape and scalar b."""
    sa, sb = opr.BINARY_TAIL_CASES[idx]
    for op in (ph.ADD, ph.SUB, ph.MUL, ph.DIV, ph.POW):
        a, bm = opr.binary_inputs(sa, sb, op, idx)
        out, shp = backend.binaryBroadcastF32(op, up(backend, a), list(sa), up(backend, bm), list(sb))
        assert shp == list(np.broadcast_shapes(sa, sb))
        check_binary(op, dl(backend, out, shp), a, bm, [list(sa), list(sb)])


@pytest.mark.parametrize("idx", range(len(opr.BINARY_BCAST_CASES)), ids=["x".join("_".join(map(str, s)) for s in c) for c in opr.BINARY_BCAST_CASES])
def test_binary_broadcast_div_pow(idx, backend):
    """The operand order matters for DIV and POW: the scalar-b path, a-side broadcasts (zero A strides in binary_bcast_kernel), rank mixing."""
    sa, sb = opr.BINARY_BCAST_CASES[idx]
    for op in (ph.SUB, ph.DIV, ph.POW):
        a, bm = opr.binary_inputs(sa, sb, op, 20 + idx)
        out, shp = backend.binaryBroadcastF32(op, up(backend, a), list(sa), up(backend, bm), list(sb))
        assert shp == list(np.broadcast_shapes(sa, sb))
        check_binary(op, dl(backend, out, shp), a, bm, [list(sa), list(sb)])


def test_binary_past_the_grid_cap(backend):
    """3·2²⁰ + 5 elements through binary_flat_kernel (same shape) and binary_bcast_kernel (a row broadcast down 23 rows)."""
    b = backend
    a, bm = opr.binary_inputs((opr.BIG,), (opr.BIG,), ph.DIV, 95)
    ad = up(b, a)
    out, shp = b.binaryBroadcastF32(ph.DIV, ad, [opr.BIG], up(b, bm), [opr.BIG])
    check_binary(ph.DIV, dl(b, out, shp), a, bm, [opr.BIG], path="flat")
    out.free()
    rows, cols = 23, opr.BIG // 23
    row = bm[:cols]
    out, shp = b.binaryBroadcastF32(ph.DIV, ad, [rows, cols], up(b, row), [1, cols])
    check_binary(ph.DIV, dl(b, out, shp), a.reshape(rows, cols), row.reshape(1, cols), [[rows, cols], [1, cols]], path="bcast")
    out.free()


# ------------------------------------------------------------------------------------------------ wavenet_layer
@pytest.fixture(scope="module")
def wn_runs(backend):
    """Every case of ops_ref.WN_CASES run once with routes armed: [(x_out or None, skip_out, route records)]."""
    b = backend
    runs = []
    for idx, (C, T, K, dil, N, last, with_skip) in enumerate(opr.WN_CASES):
        i = opr.wn_inputs(idx)
        with routes_armed(b):
            xo, so = b.wavenetLayerF32(up(b, i["x"]), None if i["sk"] is None else up(b, i["sk"]), up(b, i["w_in"]), up(b, i["b_in"]), up(b, i["w_rs"]),
                                       up(b, i["b_rs"]), N, C, T, K, dil, last)
            recs = b.last_routes()
        runs.append((None if xo is None else dl(b, xo, [N, C, T]), dl(b, so, [N, C, T]), recs))
    return runs


@pytest.mark.parametrize("idx", range(len(opr.WN_CASES)), ids=[f"C{c[0]}_T{c[1]}_K{c[2]}_d{c[3]}_N{c[4]}{'_last' if c[5] else ''}{'' if c[6] else '_noskip'}" for c in opr.WN_CASES])
def test_wavenet_layer(idx, wn_runs):
    """piper_hip_wavenet_layer_f32's own glue: the weight packing conv_pick_tile chooses for either conv, the gate-interleaved image, the
    batch strides, C res/skip rows on the last layer, skip_in == NULL on a layer that is not the last."""
    C, T, K, dil, N, last, with_skip = opr.WN_CASES[idx]
    i = opr.wn_inputs(idx)
    xo, so, recs = wn_runs[idx]
    assert len(recs) == 2, recs  # the gated in-conv, then the 1 x 1 res/skip conv
    image = opr.image_of_record(recs[0])
    assert image in opr.WN_IMAGES and opr.image_of_record(recs[1]) is None, recs
    rx, rs = opr.wavenet_layer(i["x"], i["sk"], i["w_in"], i["b_in"], i["w_rs"], i["b_rs"], K, dil, last)
    routes = [cr.family_of(cr.variant_of(r)) for r in recs]
    if last:
        assert xo is None
    else:
        check_tol("wavenet_layer.x", [N, C, T], xo, rx, OP_TOL, K=K, dilation=dil, image=image, routes=routes)
    check_tol("wavenet_layer.skip", [N, C, T], so, rs, OP_TOL, K=K, dilation=dil, image=image, routes=routes, last=last, skip_in=with_skip)


def test_wavenet_layer_cases_take_every_weight_image(wn_runs):
    """On 256 CUs the cases together read the gate-interleaved 16-wide image, the plain 16-wide one and the 32-wide one (another CU count may
    choose otherwise: nothing is asserted there)."""
    images = [opr.image_of_record(recs[0]) for _, _, recs in wn_runs]
    report("wavenet_layer.images", [list(c[:5]) for c in opr.WN_CASES], 0.0, images=images)
    if {cr.cus_of(recs) for _, _, recs in wn_runs} != {256}:
        return
    assert set(images) == set(opr.WN_IMAGES), images
    assert images[1] == "plain16" and images[3] == "gate16" and images[-1] == "wide32", images


# ------------------------------------------------------------------------------------------------ hifigan_resblock
@pytest.mark.parametrize("idx", range(len(opr.RB_CASES)), ids=[f"rb{c[0]}_C{c[1]}_T{c[2]}_K{c[3]}_slope{c[6]}" for c in opr.RB_CASES])
def test_hifigan_resblock_fallbacks(idx, backend):
    """Slope 1.5 on a geometry the fused pair kernel covers: every conv on its own through launch_conv_mfma. C = 6, which
    conv_mfma_eligible refuses: launch_conv_direct with the LeakyReLU prologue and the residual. Two items, both types."""
    type_, C, T, K, dils, N, slope = opr.RB_CASES[idx]
    x, ws, bs = opr.rb_inputs(idx)
    b = backend
    with routes_armed(b):
        out = b.hifiganResblockF32(type_, up(b, x), N, C, T, K, dils, [up(b, w) for w in ws], [up(b, v) for v in bs], slope)
        recs = b.last_routes()
    fams = [cr.family_of(cr.variant_of(r)) for r in recs]
    assert len(recs) == len(ws) and "rb_pair" not in fams, recs  # one launch per conv on any CU count
    for r in recs:
        p = cr.params_of(cr.variant_of(r))
        assert p["pro"] == "lrelu" and p["kind"] == "conv", r
    if C < 8:
        assert set(fams) == {"direct"}, recs
    assert sum(cr.params_of(cr.variant_of(r))["res"] == "1" for r in recs) == len(dils), recs
    check_tol("hifigan_resblock", [N, C, T], dl(b, out, [N, C, T]), opr.hifigan_resblock(type_, x, K, dils, ws, bs, slope), OP_TOL, type=type_, K=K,
              slope=slope, routes=sorted(set(fams)))
