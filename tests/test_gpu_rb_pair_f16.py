"""GPU: the fp16 ResBlock1 pair kernel (csrc/rb_pair_f16.hip) through piper_hip_hifigan_resblock_f16 and the f16 voice.

The op rule: float64 ResBlock of the UNROUNDED operands, per-element a-priori bound walked along the reference with float64 convs of absolute
values. Per conv (2·2⁻¹¹ + 2⁻²²)·conv(|lrelu in|, |w|) for the two fp16 roundings, (C·K + 3)·2⁻²⁴·(conv(|lrelu in|, |w|) + |bias| + |residual|)
for the fp32 accumulation, and the error of its input carried through as conv(E, |w|) (LeakyReLU and the clamp are 1-Lipschitz). The bound is
a worst case: random data sits far inside it. It catches seams, taps, scales, biases and residuals; the operand type is the voice test's.
Inputs with 0 < |x| < 2⁻¹⁰ are moved to ±2⁻¹⁰ (test_gpu_f16.data). Tiles are 256 intermediate columns = 256 − 2·pb output columns.

The walk applies the contract's clamp (±65504) to every activation. Without an outlier that is the identity and the walked reference is
ops_ref.hifigan_resblock's. The row_scale variant needs it: rows × 2¹⁰ chained through three pairs carry the stream to about 10⁶ after the first
pair and 10¹¹ after the second (float64 reference), so from the second pair on the contract clamps, and only a reference that clamps too
can hold the bound unchanged."""
import numpy as np
import pytest

import conv_ref as cr
import katdata as kd
import oracle as orc
import piper_hip as ph
from ops_ref import U, hifigan_resblock, judge_elem
from test_gpu_f16 import data, rms
from test_gpu_ops import routes_armed, up

pytestmark = pytest.mark.gpu
SD = kd.case_seed("cfg", 72) + 57
FAMILY = "rb_pair_f16"
SLOPE = np.float64(np.float32(0.1))

# (type, C, K, dilations, T, N, fused pair launches)
CASES = [
    (1, 32, 3, (1,), 4, 1, 1),            # row shorter than both reaches
    (1, 32, 11, (1, 3, 5), 260, 1, 3),    # widest reach pa = 25, Wo = 246: a second tile of 14 columns, three chained pairs
    (1, 64, 3, (1, 3, 5), 252, 3, 3),     # the last multiple of 4 under Wo = 254: exactly one tile, batch 3
    (1, 64, 7, (1, 3, 5), 504, 1, 3),     # Wo = 250: a third tile of 4 columns
    (1, 128, 11, (5,), 248, 2, 1),        # two row tiles per wave at the largest LDS footprint, a last tile of 2 columns, batch 2
    (1, 256, 3, (1, 3), 64, 1, 0),        # not eligible: per-conv fallback under the same bound
    (1, 32, 3, (1, 3), 130, 1, 0),        # T % 4 != 0: fallback
    (2, 32, 3, (1, 2), 128, 1, 0),        # ResBlock2: single convs, same bound
]
EDGE = CASES[2]


def resblock_walk(type_, x, K, dils, ws, bs):
    """(float64 ResBlock with the contract's clamp on every activation, its per-element error bound)."""
    C = x.shape[1]
    act = lambda v: np.clip(np.where(v >= 0, v, v * SLOPE), -65504.0, 65504.0)

    def conv(a, w, b, d):
        return cr.conv1d(a, w, b, 1, d, (K - 1) * d // 2, (K - 1) * d // 2)

    def conv_err(a, w, b, res_abs, d, e_in):
        s = conv(np.abs(a), np.abs(w), None, d)
        return (2 * 2.0 ** -11 + 2.0 ** -22) * s + (C * K + 3) * U * (s + np.abs(b)[None, :, None] + res_abs) + conv(e_in, np.abs(w), None, d)

    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)
    for i, d in enumerate(dils):
        a = act(x)
        if type_ == 1:
            t = act(conv(a, ws[2 * i], bs[2 * i], d))
            e_t = conv_err(a, ws[2 * i], bs[2 * i], 0.0, d, e)
            e = e + conv_err(t, ws[2 * i + 1], bs[2 * i + 1], np.abs(x), 1, e_t)
            x = x + conv(t, ws[2 * i + 1], bs[2 * i + 1], 1)
        else:
            e = e + conv_err(a, ws[i], bs[i], np.abs(x), d, e)
            x = x + conv(a, ws[i], bs[i], d)
    return x, e


def operands(case, sd):
    type_, C, K, dils, T, N, _ = case
    nconv = len(dils) * (2 if type_ == 1 else 1)
    x = data(sd, (N, C, T), (C, C, K), C * K, C)[0]
    return x, [kd.weight(sd + 1 + i, (C, C, K), C * K) for i in range(nconv)], [kd.sym(sd + 40 + i, (C,), 0.1) for i in range(nconv)]


def run(b, case, x, ws, bs):
    type_, C, K, dils, T, N, npairs = case
    with routes_armed(b):
        out = b.hifiganResblockF16(type_, up(b, x), N, C, T, K, list(dils), [up(b, w) for w in ws], [up(b, v) for v in bs], 0.1)
        recs = [cr.variant_of(r) for r in b.last_routes()]
    fam = [cr.family_of(v) for v in recs]
    assert fam.count(FAMILY) == npairs and set(fam) <= {FAMILY, "f16"}, fam
    assert all(cr.params_of(v)["multi"] == "1" and cr.params_of(v)["wsrc"] == "l2" for v in recs if cr.family_of(v) == FAMILY), recs
    return b.downloadFloat32(out).reshape(N, C, T)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"rb{c[0]}_C{c[1]}_K{c[2]}_d{'-'.join(map(str, c[3]))}_T{c[4]}_n{c[5]}")
def test_hifigan_resblock_f16(case, backend):
    type_, _, K, dils = case[:4]
    x, ws, bs = operands(case, SD + 100 * CASES.index(case))
    got = run(backend, case, x, ws, bs)
    j = judge_elem(got, hifigan_resblock(type_, x, K, dils, ws, bs), resblock_walk(type_, x, K, dils, ws, bs)[1])
    print(f"hifigan_resblock_f16 {case}: worst error {j['ratio']:.3f} of the bound")
    assert np.all(np.isfinite(got)) and j["ok"], (case, j)


@pytest.mark.parametrize("variant", ["row_scale", "saturation"])
def test_rb_pair_f16_contract_edges(variant, backend):
    """row_scale: odd output channels of every weight × 2⁻²⁰, even ones × 2¹⁰, biases at the odd rows' magnitude — the bound holds unchanged
    (against the clamped walk: see the module docstring). saturation: two inputs at ±1e6 — finite everywhere, and every column beyond the
    chained reach Σ(pa + pb) of a planted one meets the bound against the plain reference."""
    type_, C, K, dils, T, N, _ = EDGE
    x, ws, bs = operands(EDGE, SD + 2000)
    planted = ((1, 5, 17), (2, 40, 240))
    if variant == "row_scale":
        rows = np.where(np.arange(C) % 2, np.float32(2.0 ** -20), np.float32(2.0 ** 10)).astype(np.float32)[:, None, None]
        ws, bs = [w * rows for w in ws], [v * np.float32(2.0 ** -20) for v in bs]
    else:
        x[planted[0]], x[planted[1]] = 1e6, -1e6
    got = run(backend, EDGE, x, ws, bs)
    ref, bound = resblock_walk(type_, x, K, dils, ws, bs)
    judged = np.ones((N, 1, T), bool)
    if variant == "saturation":
        ref = hifigan_resblock(type_, x, K, dils, ws, bs)
        reach = sum((K - 1) * d // 2 + (K - 1) // 2 for d in dils)
        for n, _, col in planted:
            judged[n, 0, max(col - reach, 0):col + reach + 1] = False
    j = judge_elem(np.where(judged, got, ref), ref, bound)
    print(f"rb_pair_f16 {variant}: worst error {j['ratio']:.3f} of the bound")
    assert np.all(np.isfinite(got)) and j["ok"], (variant, j)


def test_f16_voice_runs_pairs(voices, backend):
    """High voice, F = 42, one item and the ragged batch of two: every ResBlock step of the 128-, 64- and 32-channel stages runs the pair
    kernel (three pairs per launch), no step of the 256-channel stage or of another kind does, and the waveform meets test_f16_voice's
    criterion against the oracle — the check that fp16 operands, not bf16 ones, ran in the fused path."""
    cfg, blob = voices["high"]
    stages = ("dec.s1.", "dec.s2.", "dec.s3.")
    ids, dur = kd.FIXTURE_IDS, [3] * 14
    F = sum(dur)
    noise, noise2 = kd.sym(SD + 900, (cfg.inter, F), 1.7320508), kd.sym(SD + 901, (cfg.inter, F // 2), 1.7320508)
    ref1 = orc.synthesize(cfg, blob, ids, dur, noise, 0.667)
    ref2 = np.concatenate([ref1, orc.synthesize(cfg, blob, ids[:7], dur[:7], noise2, 0.667)])
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        e = {}
        for prec in ("f32", "bf16", "f16"):
            rt.set_precision(prec)
            with routes_armed(backend):
                rt.prepare(0, ids, dur, noise, 0.667)
                rt.launch(0)
                one = rt.collect(0).copy()
                rt.prepare_batch(1, [(ids, dur, noise), (ids[:7], dur[:7], noise2)], 0.667)
                rt.launch(1)
                two = rt.collect(1).copy()
                scheds = (rt.routes(0), rt.routes(1))
            assert np.all(np.isfinite(one)) and np.all(np.isfinite(two))
            e[prec] = (rms(one, ref1), rms(two, ref2))
        for sched in scheds:  # the f16 plans
            paired = {name for name, recs in sched if any(cr.family_of(cr.variant_of(r)) == FAMILY for r in recs)}
            assert all(cr.params_of(cr.variant_of(r))["multi"] == "3" for name, recs in sched if name in paired for r in recs), sched
            assert paired and all(name.startswith(stages) and ".rb" in name for name in paired), paired
            assert {name[:7] for name in paired} == set(stages), paired
            singles = [name for name, recs in sched if name.startswith(stages) and ".rb" in name and name not in paired]
            assert not singles, singles
        print(f"high: RMS error vs oracle (one item, ragged batch) {e}")
        for i in range(2):
            assert e["f16"][i] <= max(e["bf16"][i] / 4, 4 * e["f32"][i]), e
    finally:
        rt.close()
