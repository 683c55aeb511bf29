"""GPU: the split-bf16 ResBlock pair kernel (csrc/rb_pair_bf16x3.hip) through piper_hip_hifigan_resblock_bf16x3 and the bf16x3 voice.

The op rule: float64 ResBlock of the UNROUNDED operands, per-element a-priori bound built with float64 convs of absolute values. Per conv
3·2⁻¹⁶·conv(|lrelu in|, |w|) for the split, (3·C·K + 3)·2⁻²⁴·(conv(|lrelu in|, |w|) + |bias| + |residual|) for the fp32 accumulation, and the
error of its input carried through as conv(E, |w|) (LeakyReLU is 1-Lipschitz); ResBlock2 adds the input's error directly as well. A dropped
term sits near 2⁻⁹·Σ|w||x|, far outside. Tiles are 256 intermediate columns = 256 − 2·pb output columns (pb = conv b's reach each side)."""
import numpy as np
import pytest

import conv_ref as cr
import katdata as kd
import oracle as orc
import piper_hip as ph
from ops_ref import U, hifigan_resblock, judge_elem
from test_gpu_bf16x3 import rms
from test_gpu_ops import routes_armed, up

pytestmark = pytest.mark.gpu
SD = kd.case_seed("cfg", 71) + 57
FAMILY = "rb_pair_bf16x3"

# (type, C, K, dilations, T, N, fused pair launches)
CASES = [
    (2, 32, 3, (1, 2), 4, 1, 1),         # row shorter than both reaches
    (2, 32, 7, (3, 12), 372, 2, 1),      # widest reach (184 outputs per tile): seams between tiles, 4 columns in a third tile, batch
    (2, 64, 7, (3, 12), 368, 1, 1),      # the largest LDS footprint; exactly two tiles
    (2, 64, 5, (2, 6), 468, 1, 1),       # 232 outputs per tile: a last tile of 4 columns
    (2, 32, 3, (1, 2, 4), 128, 1, 1),    # odd step count: pair + single conv
    (1, 32, 11, (1, 3, 5), 260, 1, 3),   # three chained ResBlock1 pairs, pa = 25
    (1, 64, 3, (1, 3, 5), 252, 3, 3),    # 254 outputs per tile: the last multiple of 4 below one tile
    (2, 128, 7, (3, 12), 200, 1, 0),     # not eligible: per-conv fallback under the same bound
    (2, 32, 3, (1, 2), 130, 1, 0),       # T % 4 != 0: fallback
]


def resblock_bound(type_, x, K, dils, ws, bs, slope=0.1):
    """Per-element error bound of the split-bf16 ResBlock, walked along the float64 reference."""
    C = x.shape[1]
    lrelu = lambda v: np.where(v >= 0, v, v * slope)

    def conv_err(inp, w, b, res_abs, d, e_in):
        p = (K - 1) * d // 2
        s = cr.conv1d(np.abs(lrelu(inp)), np.abs(w), None, 1, d, p, p)
        return 3 * 2.0 ** -16 * s + (3 * C * K + 3) * U * (s + np.abs(b)[None, :, None] + res_abs) + cr.conv1d(e_in, np.abs(w), None, 1, d, p, p)

    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)
    for i, d in enumerate(dils):
        if type_ == 1:
            t = cr.conv1d(x, ws[2 * i], bs[2 * i], 1, d, (K - 1) * d // 2, (K - 1) * d // 2, lrelu=slope)
            e_t = conv_err(x, ws[2 * i], bs[2 * i], 0.0, d, e)
            e = e + conv_err(t, ws[2 * i + 1], bs[2 * i + 1], np.abs(x), 1, e_t)
            x = x + cr.conv1d(t, ws[2 * i + 1], bs[2 * i + 1], 1, 1, (K - 1) // 2, (K - 1) // 2, lrelu=slope)
        else:
            e = e + conv_err(x, ws[i], bs[i], np.abs(x), d, e)
            x = x + cr.conv1d(x, ws[i], bs[i], 1, d, (K - 1) * d // 2, (K - 1) * d // 2, lrelu=slope)
    return e


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"rb{c[0]}_C{c[1]}_K{c[2]}_d{'-'.join(map(str, c[3]))}_T{c[4]}_n{c[5]}")
def test_hifigan_resblock_bf16x3(case, backend):
    type_, C, K, dils, T, N, npairs = case
    sd = SD + 100 * CASES.index(case)
    nconv = len(dils) * (2 if type_ == 1 else 1)
    x = kd.sym(sd, (N, C, T))
    ws = [kd.weight(sd + 1 + i, (C, C, K), C * K) for i in range(nconv)]
    bs = [kd.sym(sd + 40 + i, (C,), 0.1) for i in range(nconv)]
    b = backend
    with routes_armed(b):
        out = b.hifiganResblockBF16x3(type_, up(b, x), N, C, T, K, list(dils), [up(b, w) for w in ws], [up(b, v) for v in bs], 0.1)
        fam = [cr.family_of(cr.variant_of(r)) for r in b.last_routes()]
    assert fam.count(FAMILY) == npairs and set(fam) <= {FAMILY, "bf16x3"}, fam
    got = b.downloadFloat32(out).reshape(N, C, T)
    j = judge_elem(got, hifigan_resblock(type_, x, K, dils, ws, bs), resblock_bound(type_, x, K, dils, ws, bs))
    print(f"hifigan_resblock_bf16x3 {case}: worst error {j['ratio']:.3f} of the bound, routes {fam}")
    assert np.all(np.isfinite(got)) and j["ok"], (case, j)


@pytest.mark.parametrize("quality,stages", [("medium", ("dec.s1.", "dec.s2.")), ("high", ("dec.s2.", "dec.s3."))])
def test_bf16x3_voice_runs_pairs(quality, stages, voices, backend):
    """F = 42: the 32- / 64-channel stages' ResBlock steps run the pair kernel, no other step does, and the waveform meets
    test_bf16x3_voice's criterion against the oracle."""
    cfg, blob = voices[quality]
    ids, dur = kd.FIXTURE_IDS, [3] * 14
    noise = kd.sym(SD + 900, (cfg.inter, sum(dur)), 1.7320508)
    ref = orc.synthesize(cfg, blob, ids, dur, noise, 0.667)
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        e = {}
        for prec in ("f32", "bf16", "bf16x3"):
            rt.set_precision(prec)
            with routes_armed(backend):
                rt.prepare(0, ids, dur, noise, 0.667)
                rt.launch(0)
                wave = rt.collect(0).copy()
                routes = rt.routes(0)
            assert np.all(np.isfinite(wave))
            e[prec] = rms(wave, ref)
        # 37 copies of the item: more than 1536 frames in the batch, so the per-conv schedule (one pair launch per ResBlock on its lane)
        with routes_armed(backend):
            rt.prepare_batch(1, [(ids, dur, noise)] * 37, 0.667)
            rt.launch(1)
            many = rt.collect(1).copy()
            routes_many = rt.routes(1)
        e["bf16x3 x37"] = rms(many, np.tile(ref, 37))
        for sched, multi in ((routes, "multi=3"), (routes_many, "multi=1")):
            paired = {name for name, recs in sched if any(cr.family_of(cr.variant_of(r)) == FAMILY and multi in r for r in recs)}
            assert paired and all(name.startswith(stages) and ".rb" in name for name in paired), paired
            assert {name[:7] for name in paired} == set(stages), paired
            singles = [name for name, recs in sched if name.startswith(stages) and ".rb" in name and name not in paired]
            assert not singles, singles
        print(f"{quality}: RMS error vs oracle {e}")
        assert np.all(np.isfinite(many)) and max(e["bf16x3"], e["bf16x3 x37"]) <= max(e["bf16"] / 31.6, 4 * e["f32"]), e
    finally:
        rt.close()
