"""CPU checks of tests/ops_ref.py: every formula against tests/oracle.py on the katdata cases at its own rule, the conditions the GPU cases of
tests/test_gpu_ops_edges.py rely on (from the inputs alone), and that the value defects a guard-free kernel could carry break the rules."""
import numpy as np
import pytest

import katdata as kd
import ops_ref as opr
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, assert_close
from test_oracle_golden import rb_inputs, wn_inputs


# ------------------------------------------------------------------------------------------------ the formulas against the oracle
@pytest.mark.parametrize("idx", range(len(kd.MATMUL_CASES)), ids=[c[0] for c in kd.MATMUL_CASES])
def test_matmul_formula_vs_oracle(idx):
    a, b = kd.matmul_inputs(idx)
    ref, bound = opr.matmul(a, b)
    assert np.all(bound > 0)
    r = opr.judge_elem(orc.matmul(a, b), ref, bound)
    assert r["ok"], r


@pytest.mark.parametrize("idx", range(len(kd.SOFTMAX_CASES)), ids=[c[0] for c in kd.SOFTMAX_CASES])
def test_softmax_formula_vs_oracle(idx):
    x = kd.softmax_input(idx)
    assert_close(orc.softmax(x), opr.softmax(x), opr.SOFTMAX_TOL)
    assert np.allclose(opr.softmax(x).sum(-1), 1.0, rtol=0, atol=1e-12)


def test_reduce_mean_formula_vs_oracle():
    x = kd.sym(5, (2, 3, 4, 5))
    ref, bound = opr.reduce_mean(x)
    r = opr.judge_elem(orc.reduce_mean_lastdim(x), ref, bound)
    assert r["ok"], r


def test_unary_formulas_vs_oracle():
    x = kd.unary_input()
    for op in opr.UNARY_OPS:
        xi = np.minimum(x, 80) if op == ph.EXP else np.abs(x) if op == ph.SQRT else x
        alpha = opr.UNARY_ALPHA.get(op, 0.0)
        got, ref = orc.unary(op, xi, alpha), opr.unary(op, xi, alpha)
        if op in opr.UNARY_EXACT:
            assert ref.dtype == np.float32 and opr.judge_exact(got, ref)["ok"], opr.UNARY_NAMES[op]
        else:
            assert ref.dtype == np.float64
            assert_close(got, ref, opr.UNARY_TOL[op], opr.UNARY_NAMES[op])
    assert set(opr.UNARY_EXACT) | set(opr.UNARY_TOL) == set(opr.UNARY_OPS) == set(opr.UNARY_NAMES)


@pytest.mark.parametrize("idx", range(len(kd.BINARY_CASES)), ids=[c[0] for c in kd.BINARY_CASES])
def test_binary_formulas_vs_oracle(idx):
    a, b = kd.binary_inputs(idx)
    for op in opr.BINARY_EXACT:
        assert opr.judge_exact(orc.binary(op, a, b), opr.binary(op, a, b))["ok"], opr.BINARY_NAMES[op]
    b2, a2 = np.abs(b) + np.float32(0.5), np.abs(a) + np.float32(0.1)
    assert_close(orc.binary(ph.DIV, a, b2), opr.binary(ph.DIV, a, b2), opr.BINARY_TOL[ph.DIV], "div")
    assert_close(orc.binary(ph.POW, a2, b), opr.binary(ph.POW, a2, b), opr.BINARY_TOL[ph.POW], "pow")


def test_layout_formulas_vs_oracle():
    x = kd.sym(5, (2, 3, 4, 5))
    pads = [0, 1, 0, 2, 1, 0, 3, 0]
    assert opr.judge_exact(orc.pad(x, pads, 2.5), opr.pad(x, pads, 2.5))["ok"]
    for shape in opr.GATHER_SHAPES:
        g = opr.gather_input(shape)
        assert opr.judge_exact(orc.pad(g, opr.pads_for(shape), opr.PAD_VALUE), opr.pad(g, opr.pads_for(shape), opr.PAD_VALUE))["ok"], shape
    for axis, start, end, step in ((3, 1, 4, 1), (1, 2, -1, -1), (2, 0, 4, 2), (2, 3, 0, -2), (3, 0, 5, 3)):
        assert opr.judge_exact(orc.slice_(x, axis, start, end, step), opr.slice_(x, axis, start, end, step))["ok"], (axis, start, end, step)
    assert opr.slice_(x, 1, 2, -1, -1).shape == x.shape and np.array_equal(opr.slice_(x, 1, 2, -1, -1), x[:, ::-1])  # VITS Flip
    p = opr.gather_input(opr.PERM_SHAPE)
    for perm in opr.PERMS4:
        assert opr.judge_exact(orc.transpose(p, perm), opr.transpose(p, perm))["ok"], perm
    for ins, outs in opr.EXPANDS:
        e = opr.gather_input(ins, 1)
        assert opr.judge_exact(orc.expand(e, list(outs)), opr.expand(e, outs))["ok"], (ins, outs)
    a, b = kd.sym(7, (2, 3, 6)), kd.sym(8, (2, 5, 6))
    c = opr.concat2_axis1(a, b)
    assert opr.judge_exact(orc.concat2_axis1(a, b), c)["ok"]
    for got, ref in zip(orc.split2_axis1(c, 3), opr.split2_axis1(c, 3)):
        assert opr.judge_exact(got, ref)["ok"]


def test_add_layernorm_formula_vs_oracle():
    sd = kd.case_seed("mod", 0)
    x, y = kd.sym(sd + 20, (1, 192, 14), 2.0), kd.sym(sd + 21, (1, 192, 14), 2.0)
    g, be = 1 + kd.sym(sd + 22, (192,), 0.1), kd.sym(sd + 23, (192,), 0.1)
    assert_close(orc.add_layernorm(x, y, g, be), opr.add_layernorm(x, y, g, be), OP_TOL)
    assert_close(orc.add_layernorm(x, None, g, be), opr.add_layernorm(x, None, g, be), OP_TOL)
    for idx in (1, 6):  # a small C, and the common-mode offset
        xi, yi, gi, bi = opr.ln_inputs(idx)
        ref = opr.add_layernorm(xi, yi, gi, bi)
        for n in range(xi.shape[0]):
            assert_close(orc.add_layernorm(xi[n:n + 1], None if yi is None else yi[n:n + 1], gi, bi), ref[n:n + 1], OP_TOL, f"case {idx} item {n}")


def test_wavenet_layer_formula_vs_oracle():
    i = wn_inputs()
    C, K = i["C"], i["K"]
    ox, os_ = orc.wavenet_layer(i["x"], i["sk"], i["w_in"], i["b_in"], i["w_rs"], i["b_rs"], K, 1, False)
    rx, rs = opr.wavenet_layer(i["x"], i["sk"], i["w_in"], i["b_in"], i["w_rs"], i["b_rs"], K, 1, False)
    assert_close(ox, rx, OP_TOL, "x")
    assert_close(os_, rs, OP_TOL, "skip")
    _, os_ = orc.wavenet_layer(i["x"], None, i["w_in"], i["b_in"], i["w_rs"][:C], i["b_rs"][:C], K, 1, True)
    rx, rs = opr.wavenet_layer(i["x"], None, i["w_in"], i["b_in"], i["w_rs"][:C], i["b_rs"][:C], K, 1, True)
    assert rx is None
    assert_close(os_, rs, OP_TOL, "last skip")
    j = opr.wn_inputs(1)  # dilation 2, one item
    C, T, K, dil, N, last, _ = opr.WN_CASES[1]
    ox, os_ = orc.wavenet_layer(j["x"], j["sk"], j["w_in"], j["b_in"], j["w_rs"], j["b_rs"], K, dil, last)
    rx, rs = opr.wavenet_layer(j["x"], j["sk"], j["w_in"], j["b_in"], j["w_rs"], j["b_rs"], K, dil, last)
    assert_close(ox, rx, OP_TOL, "x, dilation 2")
    assert_close(os_, rs, OP_TOL, "skip, dilation 2")


@pytest.mark.parametrize("type_", [1, 2])
def test_resblock_formula_vs_oracle(type_):
    x, K, dils, ws, bs = rb_inputs(type_)
    assert_close(orc.hifigan_resblock(type_, x, K, dils, ws, bs), opr.hifigan_resblock(type_, x, K, dils, ws, bs), OP_TOL)
    assert_close(orc.hifigan_resblock(type_, x, K, dils, ws, bs, 1.5), opr.hifigan_resblock(type_, x, K, dils, ws, bs, 1.5), OP_TOL, "slope 1.5")


# ------------------------------------------------------------------------------------------------ what the GPU cases rely on
def test_softmax_cases_have_no_fully_masked_row_and_reach_both_kernels():
    for idx, (rows, cols, masked) in enumerate(opr.SOFTMAX_CASES):
        x = opr.softmax_input(idx)
        real = x > opr.MASK_FILL / 2
        assert real.any(-1).all(), (rows, cols)
        assert (~real).any() == masked
        if masked:
            assert (real.sum(-1) == 1).any() and np.all(x[~real] == opr.MASK_FILL)
        assert np.all(np.isfinite(x)) and np.abs(x[real]).max() <= 8.0
    assert {c for _, c, _ in opr.SOFTMAX_CASES} >= {63, 64, 65, 2047, 2048, 2049}
    assert any(r > 4 * 8 * 256 for r, c, _ in opr.SOFTMAX_CASES if c <= 2048) and any(r > 8 * 256 for r, c, _ in opr.SOFTMAX_CASES if c > 2048)
    assert any(m and c <= 2048 for _, c, m in opr.SOFTMAX_CASES) and any(m and c > 2048 for _, c, m in opr.SOFTMAX_CASES)


def test_matmul_and_reduce_bounds_are_positive():
    for idx, (sa, sb) in enumerate(opr.MATMUL_CASES):
        ref, bound = opr.matmul(*opr.matmul_inputs(idx))
        assert ref.shape == tuple(np.broadcast_shapes(sa[:-2], sb[:-2])) + (sa[-2], sb[-1])
        assert np.all(bound > 0) and np.all(bound < 1e-3), (sa, sb)
    assert sum(1 for sa, _ in opr.MATMUL_CASES if 0 in sa) == 1
    assert any(sa[-2] > 128 for sa, _ in opr.MATMUL_CASES)  # blockIdx.y reaches 2
    for idx in range(len(opr.REDUCE_CASES)):
        ref, bound = opr.reduce_mean(opr.reduce_input(idx))
        assert np.all(bound > 0)
    assert {c for _, c in opr.REDUCE_CASES} >= {1, 63, 64, 65, 1000} and any(r > 4 * 8 * 256 for r, _ in opr.REDUCE_CASES)


def test_exp_pow_sqrt_inputs_stay_finite():
    for op in opr.UNARY_OPS:
        for n in (opr.UNARY_N, 4099):
            x = opr.unary_input(op, n)
            assert np.all(np.isfinite(x))
            assert not np.any((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)), "denormal input"
            with np.errstate(all="raise"):
                ref = opr.unary(op, x, opr.UNARY_ALPHA.get(op, 0.0))
            assert np.all(np.isfinite(np.asarray(ref, np.float32))), opr.UNARY_NAMES[op]
            if op == ph.SQRT:
                assert np.all(x >= 0)
            for v in (0.0,) + opr.SPECIALS.get(op, ()):
                assert v in x
            assert np.signbit(x[1]) or op == ph.SQRT  # −0 is in
    for salt, (sa, sb) in enumerate(opr.BINARY_TAIL_CASES + opr.BINARY_BCAST_CASES):
        for op in (ph.DIV, ph.POW):
            a, b = opr.binary_inputs(sa, sb, op, salt)
            assert np.all(a > 0) if op == ph.POW else np.all(b >= 0.5)
            with np.errstate(all="raise"):
                ref = opr.binary(op, a, b)
            assert np.all(np.isfinite(np.asarray(ref, np.float32))) and np.abs(ref).max() < 1e3
    assert sorted(int(np.prod(sa)) % 4 for sa, sb in opr.BINARY_TAIL_CASES if sa == sb)[:3] == [1, 2, 3]
    assert opr.UNARY_N % 4 == 3 and opr.BINARY_N % 4 == 3 and opr.BIG % 4 == 1 and opr.BIG > 8 * 256 * 1024


def test_layernorm_cases_cover_each_kernel_with_variances_far_above_eps():
    seen = {}
    for idx, (C, T, N, with_y, offset) in enumerate(opr.LN_CASES):
        x, y, g, b = opr.ln_inputs(idx)
        assert (y is not None) == with_y
        mean, var = opr.layernorm_stats(x, y)
        if C == 1:  # degenerate on purpose: the deviation is exactly zero in any arithmetic and the output is beta
            assert np.all(var == 0)
            assert np.array_equal(opr.add_layernorm(x, y, g, b), np.broadcast_to(b.astype(np.float64)[None, :, None], x.shape))
        else:
            assert var.min() > 1e3 * opr.LN_EPS, (C, T, var.min())
        if offset:
            assert np.abs(mean).min() / np.sqrt(var).max() > 20  # mean / sigma of tests/test_gpu_voice.py's offset case
        seen.setdefault(opr.ln_kernel(C), set()).add((N, with_y, bool(offset)))
    assert {c[0] for c in opr.LN_CASES} == {1, 5, 16, 96, 100, 192, 193, 208, 500, 512, 513, 768}
    assert {c[1] for c in opr.LN_CASES} == {1, 15, 16, 17, 45}
    for k in ("ln12", "ln32", "big"):
        assert {n for n, _, _ in seen[k]} == {1, 3} and {y for _, y, _ in seen[k]} == {True, False} and any(o for _, _, o in seen[k]), k


def test_gather_cases():
    assert [len(s) for s in opr.GATHER_SHAPES] == [1, 2, 3, 4] and all(d % 2 or d == 2 for s in opr.GATHER_SHAPES for d in s)
    assert len(opr.PERMS4) == 24
    for shape in opr.GATHER_SHAPES:
        assert all(p > 0 for p in opr.pads_for(shape))
    counts = [len(range(s, e, st)) for s, e, st in opr.SLICES]
    assert 0 in counts and (0, 10, 3) in opr.SLICES and any(st == -2 for _, _, st in opr.SLICES)
    for (s, e, st), cnt in zip(opr.SLICES, counts):  # the ABI refuses a range that leaves the axis
        assert cnt == 0 or (0 <= s < 10 and 0 <= s + (cnt - 1) * st < 10)
    assert any(sum(1 for i, o in zip(ins, outs) if i != o) == 2 for ins, outs in opr.EXPANDS)
    shape, pads = opr.BIG_PAD
    assert opr.pad(np.zeros(shape, np.float32), pads).size == opr.BIG


def test_wavenet_and_resblock_cases():
    # conv_pick_tile on 256 CUs: WN_T32 is the first length with 32-wide tiles at C = 32, N = 2; every other case stays 16-wide
    assert opr.wn_tile(256, 32, opr.WN_T32, 2) == 32 and opr.wn_tile(256, 32, opr.WN_T32 - 1, 2) == 16
    assert [opr.wn_tile(256, C, T, N) for C, T, K, d, N, last, sk in opr.WN_CASES] == [16, 16, 16, 16, 32]
    assert {(96, 17, 3, 1, 2, False), (32, 700, 5, 2, 1, False), (64, 2000, 1, 1, 1, True), (192, 300, 5, 1, 3, False)} <= {c[:6] for c in opr.WN_CASES}
    assert not opr.WN_CASES[3][6] and not opr.WN_CASES[3][5]  # skip_in = NULL with !last
    assert opr.image_of_record("lean_gate K=5 NQ=6 gate=1 pro=none epi=store res=0 conv | Cout=384 Cin=192 Lout=300 N=3 CUs=256") == "gate16"
    assert opr.image_of_record("stream K=3 TM=16 NT=1 KS=2 BT=256 gate=1 pro=none epi=store res=0 conv | Cout=192 Cin=96 Lout=17 N=2 CUs=256") == "plain16"
    assert opr.image_of_record("stream K=3 TM=32 NT=2 KS=1 BT=256 gate=1 pro=none epi=store res=0 conv | Cout=64 Cin=32 Lout=9 N=2 CUs=256") == "wide32"
    assert opr.image_of_record("lean_k1 K=1 NQ=6 gate=0 pro=none epi=wn_res_skip res=1 conv | Cout=384 Cin=192 Lout=300 N=3 CUs=256") is None
    for type_, C, T, K, dils, N, slope in opr.RB_CASES:
        assert N == 2 and K % 2 == 1
        assert (C in (32, 64) and T % 4 == 0 and not 0 < slope < 1) or (C < 8 and 0 < slope < 1)  # pair-eligible but for the slope / below the MFMA path
    assert {c[0] for c in opr.RB_CASES if c[1] == 32} == {1, 2} == {c[0] for c in opr.RB_CASES if c[1] < 8}


# ------------------------------------------------------------------------------------------------ value defects break the rules
def test_value_defects_break_the_rules():
    """What the new GPU cases must be able to see, on the reference itself: a variance over C − 1 in the big LayerNorm, a mean over cols + 1,
    a softmax normalised by 1 / (s + 1e-3) in the block kernel's cases, a zero pad fill, a LeakyReLU that lost its slope."""
    for idx, (C, T, N, with_y, offset) in enumerate(opr.LN_CASES):
        if opr.ln_kernel(C) != "big":
            continue
        x, y, g, b = opr.ln_inputs(idx)
        ref = opr.add_layernorm(x, y, g, b)
        _, var = opr.layernorm_stats(x, y)
        bad = (ref - b.astype(np.float64)[None, :, None]) * np.sqrt((var + opr.LN_EPS) / (var * C / (C - 1) + opr.LN_EPS))[:, None, :] + b.astype(np.float64)[None, :, None]
        assert opr.judge_tol(bad, ref, OP_TOL)["ratio"] > 2, (C, T)
    for idx, (rows, cols) in enumerate(opr.REDUCE_CASES):
        ref, bound = opr.reduce_mean(opr.reduce_input(idx))
        assert opr.judge_elem(ref * cols / (cols + 1), ref, bound)["ratio"] > 5, (rows, cols)
    caught = 0
    for idx, (rows, cols, masked) in enumerate(opr.SOFTMAX_CASES):
        if cols > 2048:
            x = opr.softmax_input(idx).astype(np.float64)
            e = np.exp(x - x.max(-1, keepdims=True))
            s = e.sum(-1, keepdims=True)
            caught += opr.judge_tol(e / (s + 1e-3), e / s, opr.SOFTMAX_TOL)["ratio"] > 5
    assert caught >= 1
    x = opr.unary_input(ph.LEAKYRELU)
    assert opr.judge_tol(opr.unary(ph.LEAKYRELU, x, 0.0), opr.unary(ph.LEAKYRELU, x, 0.1), opr.UNARY_TOL[ph.LEAKYRELU])["ratio"] > 1e4
    g = opr.gather_input(opr.GATHER_SHAPES[0])
    assert not opr.judge_exact(opr.pad(g, [1, 2], 0.0), opr.pad(g, [1, 2], opr.PAD_VALUE))["ok"]
