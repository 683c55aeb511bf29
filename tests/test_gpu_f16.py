"""GPU: the fp16 precision (PIPER_HIP_PRECISION_F16, csrc/conv_f16.hip): the two ops against float64, the voice against the oracle.

The host rule restates the header's contract: x' = fp16_rne(clamp(x, ±65504)); per output channel e = 14 − ⌊log₂ max|w|⌋,
w' = fp16_rne(w·2^e), the accumulator scaled back by 2^−e. Every case is judged twice, per element:
  1. against the float64 conv of the ROUNDED operands (w'·2^−e, x') — products of fp16 values are exact in fp32, so the GPU differs by fp32
     summation order alone: |got − ref| ≤ (n + 2)·u·(Σ|w'2^−e||x'| + |b|), u = 2⁻²⁴, n = C_in·K + 1 (convT: C_in·K/stride + 1) — the form
     tests/ops_ref.py holds matmul to;
  2. against the float64 conv of the UNROUNDED operands: (2·2⁻¹¹ + 2⁻²²)·Σ|w||x| plus that accumulation bound. A bf16 result sits near
     2⁻⁸·Σ|w||x| and fails it: this is the check that fp16 operands ran, and (scaled rows) that the scale is per channel.
Activations with 0 < |x| < 2⁻¹⁰ are moved to ±2⁻¹⁰: what the hardware does with fp16 subnormals cannot decide a case."""
import numpy as np
import pytest

import conv_ref as cr
import katdata as kd
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, assert_close
from ops_ref import U, judge_elem
from test_gpu_ops import dl, up
from test_gpu_voice import snr_db

pytestmark = pytest.mark.gpu
SD = kd.case_seed("cfg", 70) + 57

# (Cin, Cout, K, dil, padL, padR, L, N, bias) → the weight path that must run
CONV_CASES = [
    ((32, 32, 1, 1, 0, 0, 1, 1, False), "lds"),         # one column, 2 weight steps: fewer than any ring depth
    ((32, 40, 3, 1, 0, 2, 77, 1, False), "lds"),        # partial row tile, partial column tile, asymmetric pads
    ((32, 32, 5, 2, 4, 4, 5, 1, True), "lds"),          # a row shorter than the reach
    ((96, 64, 1, 1, 0, 0, 130, 3, True), "lds"),        # batch 3, a step count that is no multiple of the ring depth
    ((128, 128, 7, 12, 36, 36, 200, 1, True), "lds"),   # the widest reach
    ((256, 256, 11, 5, 25, 25, 150, 1, True), "lds"),   # the largest window that still keeps the LDS ring
    ((512, 128, 7, 12, 36, 36, 40, 1, True), "l2"),     # C_in = 512 at the widest reach: no room for the ring, weights per wave from L2
]
# (Cin, Cout, K, stride, L, N)
CONVT_CASES = [(64, 32, 4, 2, 33, 2), (128, 64, 8, 4, 65, 1), (256, 128, 16, 8, 20, 1), (512, 256, 16, 8, 9, 1)]
# 512-block launches keep the wide tiles (the launcher's rule is the split-bf16 one: test_gpu_bf16x3.WIDE_CASES): two row tiles per wave
# with 8 tiles per ring step, and all four waves along the columns sharing one tile's ring. (Cin, Cout, K, L, N) → <MTW, NTW, WM>
WIDE_CASES = [((32, 256, 3, 130, 256), (2, 4, 4)), ((32, 32, 5, 514, 256), (1, 4, 1))]


def data(sd, xshape, wshape, fan_in, Cout, has_b=True):
    x, w = kd.sym(sd, xshape), kd.weight(sd + 1, wshape, fan_in)
    tiny = (x != 0) & (np.abs(x) < 2.0 ** -10)
    x[tiny] = np.copysign(np.float32(2.0 ** -10), x[tiny])
    return x, w, (kd.sym(sd + 2, (Cout,), 0.1) if has_b else None)


def f16_operands(x, w, co_axis):
    """(x', w'·2^−e) as float64; co_axis = the weight's output-channel axis (conv 0, ConvTranspose 1)."""
    xr = np.clip(x, -65504.0, 65504.0).astype(np.float16).astype(np.float64)
    m = np.max(np.abs(w), axis=tuple(a for a in range(3) if a != co_axis), keepdims=True)
    e = np.where(m > 0, 15 - np.frexp(m)[1], 0).astype(np.float64)  # m = f·2^ex, f ∈ [0.5, 1): ⌊log₂ m⌋ = ex − 1
    wr = (w.astype(np.float64) * 2.0 ** e).astype(np.float16)
    return xr, wr.astype(np.float64) * 2.0 ** -e


def check_f16(got, conv, x, w, b, co_axis, n_terms, what, unrounded=True):
    """conv(x, w, bias) → float64 result of the op under test's geometry."""
    xr, wr = f16_operands(x, w, co_axis)
    ab = None if b is None else np.abs(b)
    acc = (n_terms + 2) * U * conv(np.abs(xr), np.abs(wr), ab)
    j = judge_elem(got, conv(xr, wr, b), acc)
    print(f"{what}: vs rounded-operand float64 {j['ratio']:.3f} of the accumulation bound")
    assert np.all(np.isfinite(got)) and j["ok"], (what, j)
    if unrounded:
        full = judge_elem(got, conv(x, w, b), (2 * 2.0 ** -11 + 2.0 ** -22) * conv(np.abs(x), np.abs(w), None) + acc)
        print(f"{what}: vs unrounded float64 {full['ratio']:.3f} of the fp16 bound")
        assert full["ok"], (what, full)


def routed(backend, call):
    """call() with route records armed → (result, the parameters of its one conv_f16 launch)."""
    backend.arm_routes(True)
    try:
        res = call()
        prm = [cr.params_of(cr.variant_of(r)) for r in backend.last_routes() if r.startswith("f16 ")]
    finally:
        backend.arm_routes(False)
    assert len(prm) == 1, backend.last_routes()
    return res, prm[0]


def run_conv(backend, case, x, w, b):
    Cin, Cout, K, d, pl, pr, L, N, _ = case
    (out, shp), prm = routed(backend, lambda: backend.conv1dF16(up(backend, x), list(x.shape), up(backend, w), list(w.shape),
                                                               None if b is None else up(backend, b), dilation=d, padL=pl, padR=pr))
    assert shp == [N, Cout, L + pl + pr - d * (K - 1)]
    return dl(backend, out, shp), prm, lambda x_, w_, b_: cr.conv1d(x_, w_, b_, 1, d, pl, pr)


@pytest.mark.parametrize("case,wsrc", CONV_CASES, ids=lambda c: "-".join(str(int(v)) for v in c) if isinstance(c, tuple) else c)
def test_conv1d_f16(case, wsrc, backend):
    Cin, Cout, K, _, _, _, L, N, has_b = case
    x, w, b = data(SD + 10 * [c for c, _ in CONV_CASES].index(case), (N, Cin, L), (Cout, Cin, K), Cin * K, Cout, has_b)
    got, prm, conv = run_conv(backend, case, x, w, b)
    assert prm["wsrc"] == wsrc and prm["kind"] == "conv", prm
    check_f16(got, conv, x, w, b, 0, Cin * K + 1, f"conv1d_f16 {case}")


@pytest.mark.parametrize("variant", ["row_scale", "saturation"])
def test_conv1d_f16_contract_edges(variant, backend):
    """row_scale: odd output channels' weights × 2⁻²⁰ (subnormal in fp16 without a scale of their own), even ones × 2¹⁰ — both judgements
    hold unchanged. saturation: one activation at 1e6, one at −1e6 — finite output, judgement 1 with x' = ±65504."""
    case = (96, 64, 1, 1, 0, 0, 130, 3, True)
    Cin, Cout, K, _, _, _, L, N, _ = case
    x, w, b = data(SD + 200, (N, Cin, L), (Cout, Cin, K), Cin * K, Cout)
    if variant == "row_scale":
        w = w * np.where(np.arange(Cout) % 2, np.float32(2.0 ** -20), np.float32(2.0 ** 10)).astype(np.float32)[:, None, None]
        b = b * np.float32(2.0 ** -20)  # (a bias of the odd rows' magnitude: it must not widen their bounds)
    else:
        x[1, 5, 17], x[2, 40, 129] = 1e6, -1e6
    got, _, conv = run_conv(backend, case, x, w, b)
    check_f16(got, conv, x, w, b, 0, Cin * K + 1, f"conv1d_f16 {variant}", unrounded=variant == "row_scale")


@pytest.mark.parametrize("case,inst", WIDE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv1d_f16_wide_tiles(case, inst, backend):
    Cin, Cout, K, L, N = case
    pad = (K - 1) // 2
    x, w, b = data(SD + 300 + 10 * [c for c, _ in WIDE_CASES].index(case), (N, Cin, L), (Cout, Cin, K), Cin * K, Cout)
    got, prm, conv = run_conv(backend, (Cin, Cout, K, 1, pad, pad, L, N, True), x, w, b)
    assert tuple(int(prm[k]) for k in ("MTW", "NTW", "WM")) == inst and prm["wsrc"] == "lds", prm
    check_f16(got, conv, x, w, b, 0, Cin * K + 1, f"conv1d_f16 {case} {inst}")


@pytest.mark.parametrize("case", CONVT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_convtranspose1d_f16(case, backend):
    Cin, Cout, K, s, L, N = case
    pad = (K - s) // 2
    x, w, b = data(SD + 500 + 10 * CONVT_CASES.index(case), (N, Cin, L), (Cin, Cout, K), Cin * K // s, Cout)
    (out, shp), prm = routed(backend, lambda: backend.convTranspose1dF16(up(backend, x), list(x.shape), up(backend, w), list(w.shape), up(backend, b),
                                                                        stride=s, padL=pad, padR=pad))
    assert shp == [N, Cout, L * s] and prm["kind"] == "convT" and prm["wsrc"] == "lds", (shp, prm)
    check_f16(dl(backend, out, shp), lambda x_, w_, b_: cr.convtranspose1d(x_, w_, b_, s, 1, pad, pad), x, w, b, 1, Cin * (K // s) + 1, f"convT_f16 {case}")


def test_f16_refuses_what_bf16_refuses(backend):
    x = up(backend, np.zeros((1, 32, 16), np.float32))
    w = up(backend, np.zeros((32, 32, 3), np.float32))
    with pytest.raises(ph.UnsupportedOp):
        backend.conv1dF16(x, [1, 32, 16], w, [32, 32, 3], None, stride=2)
    with pytest.raises(ph.UnsupportedOp):
        backend.conv1dF16(up(backend, np.zeros((1, 20, 16), np.float32)), [1, 20, 16], up(backend, np.zeros((8, 20, 3), np.float32)), [8, 20, 3], None)
    with pytest.raises(ph.UnsupportedOp):
        backend.convTranspose1dF16(x, [1, 32, 16], w, [32, 32, 3], None, stride=2)  # K % stride != 0
    with pytest.raises(ph.ShapeMismatch):
        backend.conv1dF16(x, [1, 32, 16], w, [32, 16, 3], None)


def rms(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(ref, np.float64)) ** 2)))


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_f16_voice(quality, voices, backend):
    """One item, then a ragged batch of two (F and F / 2 frames: len_ptr masking is live), under f32, bf16 and f16 in one runtime.
    e(p) = RMS error of precision p's waveform against the oracle's; e(f16) ≤ max(e(bf16) / 4, 4·e(f32)): the rounding unit predicts a
    factor 8 (18 dB), the test asks for 12 dB — the floor is not pure operand rounding — or the fp32 path's own deviation."""
    cfg, blob = voices[quality]
    ids, dur = kd.FIXTURE_IDS, [3] * 14
    F = sum(dur)
    noise, noise2 = kd.sym(SD + 900, (cfg.inter, F), 1.7320508), kd.sym(SD + 901, (cfg.inter, F // 2), 1.7320508)
    batch = [(ids, dur, noise), (ids[:7], dur[:7], noise2)]
    ref1, taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
    ref2 = np.concatenate([ref1, orc.synthesize(cfg, blob, ids[:7], dur[:7], noise2, 0.667)])
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        def run(prec):
            rt.set_precision(prec)
            rt.prepare(0, ids, dur, noise, 0.667)
            rt.launch(0)
            one = rt.collect(0).copy()
            rt.prepare_batch(1, batch, 0.667)
            rt.launch(1)
            return one, rt.collect(1).copy()
        f32 = run("f32")
        bf = run("bf16")
        h = run("f16")
        assert rt.lib.piper_hip_voice_precision(rt.voice) == 3
        # encoder + flow are untouched by the precision switch: z is still the fp32 result
        assert_close(rt.tap(0, "z", cfg.inter * F), taps["z"].reshape(-1), OP_TOL, "z under f16 precision")
        for what, i, ref in (("one item", 0, ref1), ("ragged batch", 1, ref2)):
            e32, eb, eh = rms(f32[i], ref), rms(bf[i], ref), rms(h[i], ref)
            print(f"{quality} {what}: RMS error vs oracle  f32 {e32:.3e}  bf16 {eb:.3e}  f16 {eh:.3e}  (f16 is {20 * np.log10(eb / eh):.1f} dB under bf16)")
            assert np.all(np.isfinite(h[i])) and eh <= max(eb / 4, 4 * e32), (what, e32, eb, eh)
        again = run("f32")
        assert np.array_equal(again[0], f32[0]) and np.array_equal(again[1], f32[1]), "the fp32 path must be bit-identical after the switches"
    finally:
        rt.close()


def test_f16_stream_equals_whole_item(voices, backend):
    """Medium voice, one stream of four windows against the whole item at f16: the threshold of the bf16 leg of
    test_streaming_generator_matches_whole_utterance (the roundings a window split flips are 8 times smaller here)."""
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        ids = kd.FIXTURE_IDS * 4
        dur = [3] * len(ids)
        noise = kd.sym(SD + 950, (cfg.inter, sum(dur)), 1.7320508)
        rt.set_precision("f16")
        whole = rt.synthesize(ids, dur, noise, 0.667)
        chunks = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=48, slot=3))
        assert len(chunks) == 4
        streamed = np.concatenate(chunks)
        assert streamed.size == whole.size
        assert snr_db(streamed, whole) >= 40.0, snr_db(streamed, whole)
    finally:
        rt.close()
