"""GPU: the split-bf16 precision (PIPER_HIP_PRECISION_BF16X3, csrc/conv_bf16x3.hip): the two ops against float64, the voice against the oracle.

The op rule. Host split: hi = bf16_round(a), lo = bf16_round(a − hi), both exact to reproduce. The reference is the float64 conv of the three
terms w_hi·x_hi + w_hi·x_lo + w_lo·x_hi (+ bias); every product is exact in fp32, so the GPU differs from it by fp32 summation order alone:
per element |got − ref| ≤ (n + 2)·u·(Σ|w_hi||x_hi| + Σ|w_hi||x_lo| + Σ|w_lo||x_hi| + |b|), u = 2⁻²⁴, n = 3·C_in·K + 1 summed terms — the form
tests/ops_ref.py holds matmul to. And it IS a split computation: against float64 of the UNROUNDED operands, per element
|got − full| ≤ 3·2⁻¹⁶·Σ|w||x| + that accumulation bound (a single-bf16 result sits near 2⁻⁹·Σ|w||x|; a missing term near 2⁻⁹ too)."""
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
SD = kd.case_seed("cfg", 70) + 31

# (Cin, Cout, K, dil, padL, padR, L, N, bias)
CONV_CASES = [
    (32, 32, 1, 1, 0, 0, 1, 1, False),         # one column, 2 steps (fewer than any ring depth)
    (32, 40, 3, 1, 0, 2, 77, 1, False),        # partial row tile, asymmetric pads, partial column tile
    (32, 32, 5, 2, 4, 4, 5, 1, True),          # row shorter than the reach
    (96, 64, 1, 1, 0, 0, 130, 3, True),        # batch 3, three channel groups
    (64, 64, 3, 5, 5, 5, 300, 2, True),        # five column blocks per item (NTW = 1 at this size)
    (256, 256, 11, 5, 25, 25, 150, 1, True),   # widest reach × Cin: the largest window (NTW = 1 at this size; LDS would allow no more than 2)
    (128, 128, 7, 12, 36, 36, 200, 1, True),   # medium's widest reach; step count not a multiple of the ring depth
]
# (Cin, Cout, K, stride, L, N); Cin = 512 forces the smallest tile
CONVT_CASES = [(64, 32, 4, 2, 33, 2), (128, 64, 8, 4, 65, 1), (256, 128, 16, 8, 20, 1), (512, 256, 16, 8, 9, 1)]

# The wider tiles. The launcher halves NTW, then drops MTW to 1, while a launch has fewer than two blocks per CU (512 on the 256-CU
# MI355X), so every case above runs <1, 1, WM>. These are the smallest launches that keep a wider instance: 512 blocks at that tile, two
# column blocks per item (the second one ragged), and more steps than the weight ring is deep (kDA = 4 at MTW = 2, 8 at MTW = 1) but no
# multiple of it. (Cin, Cout, K, L, N) at dilation 1 and "same" padding → the <MTW, NTW, WM> that must run.
WIDE_CASES = [
    ((32, 256, 3, 130, 256), (2, 4, 4)),   # two row tiles per wave, the kDB = 2 activation ring
    ((32, 256, 3, 66, 256), (2, 2, 4)),    # 256 blocks at NTW = 4: halved once
    ((64, 128, 3, 130, 256), (1, 4, 4)),   # 4 row tiles: no second one per wave
    ((32, 64, 5, 258, 256), (1, 4, 2)),    # two waves along the columns
    ((32, 32, 5, 514, 256), (1, 4, 1)),    # all four along the columns: 512 columns per block
]
# ConvTranspose (Cin, Cout, K, stride, L, N): blocks count input columns, rows are (phase, channel); 4 steps, one whole ring group
WIDE_CONVT = ((32, 256, 4, 2, 130, 128), (2, 4, 4))


def split(a):
    hi = kd.bf16_round(a).astype(np.float32)
    return hi, kd.bf16_round(a - hi).astype(np.float32)


def check_split_result(got, conv, x, w, b, n_terms, what):
    """conv(x, w, bias) → float64 result of the op under test's geometry."""
    (xh, xl), (wh, wl) = split(x), split(w)
    ref = conv(xh, wh, b) + conv(xl, wh, None) + conv(xh, wl, None)
    ab = None if b is None else np.abs(b)
    acc = (n_terms + 2) * U * (conv(np.abs(xh), np.abs(wh), ab) + conv(np.abs(xl), np.abs(wh), None) + conv(np.abs(xh), np.abs(wl), None))
    j = judge_elem(got, ref, acc)
    full = judge_elem(got, conv(x, w, b), 3 * 2.0 ** -16 * conv(np.abs(x), np.abs(w), ab) + acc)
    print(f"{what}: vs three-term float64 {j['ratio']:.3f} of the accumulation bound; vs unrounded float64 {full['ratio']:.3f} of the split bound")
    assert np.all(np.isfinite(got)) and j["ok"], (what, j)
    assert full["ok"], (what, full)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_conv1d_bf16x3(case, backend):
    Cin, Cout, K, d, pl, pr, L, N, has_b = case
    sd = SD + 10 * CONV_CASES.index(case)
    x, w = kd.sym(sd, (N, Cin, L)), kd.weight(sd + 1, (Cout, Cin, K), Cin * K)
    b = kd.sym(sd + 2, (Cout,), 0.1) if has_b else None
    out, shp = backend.conv1dBF16x3(up(backend, x), list(x.shape), up(backend, w), list(w.shape), None if b is None else up(backend, b),
                                    dilation=d, padL=pl, padR=pr)
    assert shp == [N, Cout, L + pl + pr - d * (K - 1)]
    check_split_result(dl(backend, out, shp), lambda x_, w_, b_: cr.conv1d(x_, w_, b_, 1, d, pl, pr), x, w, b, 3 * Cin * K + 1, f"conv1d_bf16x3 {case}")


def ran_instance(backend):
    """<MTW, NTW, WM> of the one conv_bf16x3 launch of the last op (its route record)."""
    prm = [cr.params_of(cr.variant_of(r)) for r in backend.last_routes() if r.startswith("bf16x3 ")]
    assert len(prm) == 1, backend.last_routes()
    return tuple(int(prm[0][k]) for k in ("MTW", "NTW", "WM"))


@pytest.mark.parametrize("case,inst", WIDE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv1d_bf16x3_wide_tiles(case, inst, backend):
    Cin, Cout, K, L, N = case
    pad = (K - 1) // 2
    sd = SD + 300 + 10 * [c for c, _ in WIDE_CASES].index(case)
    x, w, b = kd.sym(sd, (N, Cin, L)), kd.weight(sd + 1, (Cout, Cin, K), Cin * K), kd.sym(sd + 2, (Cout,), 0.1)
    backend.arm_routes(True)
    try:
        out, shp = backend.conv1dBF16x3(up(backend, x), list(x.shape), up(backend, w), list(w.shape), up(backend, b), padL=pad, padR=pad)
        assert ran_instance(backend) == inst
    finally:
        backend.arm_routes(False)
    assert shp == [N, Cout, L]
    check_split_result(dl(backend, out, shp), lambda x_, w_, b_: cr.conv1d(x_, w_, b_, 1, 1, pad, pad), x, w, b, 3 * Cin * K + 1, f"conv1d_bf16x3 {case} {inst}")


def test_convtranspose1d_bf16x3_wide_tiles(backend):
    (Cin, Cout, K, s, L, N), inst = WIDE_CONVT
    pad = (K - s) // 2
    x, w, b = kd.sym(SD + 700, (N, Cin, L)), kd.weight(SD + 701, (Cin, Cout, K), Cin * K // s), kd.sym(SD + 702, (Cout,), 0.1)
    backend.arm_routes(True)
    try:
        out, shp = backend.convTranspose1dBF16x3(up(backend, x), list(x.shape), up(backend, w), list(w.shape), up(backend, b), stride=s, padL=pad, padR=pad)
        assert ran_instance(backend) == inst
    finally:
        backend.arm_routes(False)
    assert shp == [N, Cout, L * s]
    check_split_result(dl(backend, out, shp), lambda x_, w_, b_: cr.convtranspose1d(x_, w_, b_, s, 1, pad, pad), x, w, b, 3 * Cin * (K // s) + 1,
                       f"convT_bf16x3 {WIDE_CONVT}")


@pytest.mark.parametrize("case", CONVT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_convtranspose1d_bf16x3(case, backend):
    Cin, Cout, K, s, L, N = case
    pad = (K - s) // 2
    sd = SD + 500 + 10 * CONVT_CASES.index(case)
    x, w, b = kd.sym(sd, (N, Cin, L)), kd.weight(sd + 1, (Cin, Cout, K), Cin * K // s), kd.sym(sd + 2, (Cout,), 0.1)
    out, shp = backend.convTranspose1dBF16x3(up(backend, x), list(x.shape), up(backend, w), list(w.shape), up(backend, b), stride=s, padL=pad, padR=pad)
    assert shp == [N, Cout, L * s]
    check_split_result(dl(backend, out, shp), lambda x_, w_, b_: cr.convtranspose1d(x_, w_, b_, s, 1, pad, pad), x, w, b, 3 * Cin * (K // s) + 1,
                       f"convT_bf16x3 {case}")


def test_bf16x3_refuses_what_bf16_refuses(backend):
    x = up(backend, np.zeros((1, 32, 16), np.float32))
    w = up(backend, np.zeros((32, 32, 3), np.float32))
    with pytest.raises(ph.UnsupportedOp):
        backend.conv1dBF16x3(x, [1, 32, 16], w, [32, 32, 3], None, stride=2)
    with pytest.raises(ph.UnsupportedOp):
        backend.conv1dBF16x3(up(backend, np.zeros((1, 20, 16), np.float32)), [1, 20, 16], up(backend, np.zeros((8, 20, 3), np.float32)), [8, 20, 3], None)
    with pytest.raises(ph.UnsupportedOp):
        backend.convTranspose1dBF16x3(x, [1, 32, 16], w, [32, 32, 3], None, stride=2)  # K % stride != 0
    with pytest.raises(ph.ShapeMismatch):
        backend.conv1dBF16x3(x, [1, 32, 16], w, [32, 16, 3], None)


def rms(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(ref, np.float64)) ** 2)))


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_bf16x3_voice(quality, voices, backend):
    """One item, then a ragged batch of two (F and F / 2 frames: len_ptr masking of both planes is live), under f32, bf16 and bf16x3 in one
    runtime. e(p) = RMS error of precision p's waveform against the oracle's; e(bf16x3) ≤ max(e(bf16) / 31.6, 4 · e(f32)): 30 dB better than
    single bf16 (derived worst case 44 dB), or within 12 dB of the fp32 path's own deviation, the floor no operand split can beat."""
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
        x3 = run("bf16x3")
        assert rt.lib.piper_hip_voice_precision(rt.voice) == 2
        # encoder + flow are untouched by the precision switch: z is still the fp32 result
        assert_close(rt.tap(0, "z", cfg.inter * F), taps["z"].reshape(-1), OP_TOL, "z under bf16x3 precision")
        for what, i, ref in (("one item", 0, ref1), ("ragged batch", 1, ref2)):
            e32, eb, ex = rms(f32[i], ref), rms(bf[i], ref), rms(x3[i], ref)
            print(f"{quality} {what}: RMS error vs oracle  f32 {e32:.3e}  bf16 {eb:.3e}  bf16x3 {ex:.3e}  (bf16x3 is {20 * np.log10(eb / ex):.1f} dB under bf16)")
            assert np.all(np.isfinite(x3[i])) and ex <= max(eb / 31.6, 4 * e32), (what, e32, eb, ex)
        again = run("f32")
        assert np.array_equal(again[0], f32[0]) and np.array_equal(again[1], f32[1]), "the fp32 path must be bit-identical after the switches"
    finally:
        rt.close()


def test_bf16x3_stream_equals_whole_item(voices, backend):
    """Medium voice, one stream of four windows against the whole item of the same precision: what differs is the window split (fp32
    summation order and the roundings it flips), as in test_streaming_generator_matches_whole_utterance's bf16 leg."""
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        ids = kd.FIXTURE_IDS * 4
        dur = [3] * len(ids)
        noise = kd.sym(SD + 950, (cfg.inter, sum(dur)), 1.7320508)
        rt.set_precision("bf16x3")
        whole = rt.synthesize(ids, dur, noise, 0.667)
        chunks = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=48, slot=3))
        assert len(chunks) == 4
        streamed = np.concatenate(chunks)
        assert streamed.size == whole.size
        assert snr_db(streamed, whole) >= 40.0, snr_db(streamed, whole)
    finally:
        rt.close()
