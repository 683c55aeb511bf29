"""GPU: ResBlock2 steps (i, i+1) in one launch on the fp16 pipe (csrc/rb_pair_f16.hip, form 2) through piper_hip_hifigan_mrf_f16 and the f16
medium voice. The op rule: the float64 mean of the three blocks of the UNROUNDED operands; per element (E_0 + E_1 + E_2)/3 +
2⁻²³·(|r_0| + |r_1| + |r_2|), E_j test_gpu_rb_pair_f16.resblock_walk's bound for block j (x1 stays fp32 between the two convs, as in the
walk), the second term the mean's two fp32 adds and its division at twice their worst case."""
import numpy as np
import pytest

import conv_ref as cr
import katdata as kd
import oracle as orc
import piper_hip as ph
from ops_ref import hifigan_resblock, judge_elem
from test_gpu_f16 import rms
from test_gpu_ops import routes_armed, up
from test_gpu_rb_pair_f16 import FAMILY, operands, resblock_walk

pytestmark = pytest.mark.gpu
SD = kd.case_seed("cfg", 73) + 57
MEDIUM = ((1, 2), (2, 6), (3, 12))  # the medium voice's dilations beside kernels (3, 5, 7): Wo = 252 / 232 / 184

# (type, C, kernels, dilations per block, T, N, fused pair records)
CASES = [
    (2, 32, (3, 5, 7), MEDIUM, 4, 1, 3),               # row shorter than every reach
    (2, 32, (3, 5, 7), MEDIUM, 380, 1, 3),             # grid of 3 tiles of 184; K = 3: 252 + 128, its third block leaves; K = 5: 232 + 148
    (2, 64, (3, 5, 7), MEDIUM, 368, 3, 3),             # exactly two tiles of the narrowest pair, batch 3
    (2, 128, (11, 11, 11), ((5, 3),) * 3, 232, 2, 0),  # 128 channels stay on the two-launch path (x1 fits neither LDS nor registers): single convs
    (2, 32, (3, 3, 3), ((1, 3, 5),) * 3, 64, 1, 3),    # steps (0, 1) fused, the odd third step as single convs
    (1, 64, (3, 7, 11), ((1, 3),) * 3, 252, 1, 6),     # ResBlock1: form-1 launches of three pairs
    (2, 256, (3, 3, 3), ((1, 2),) * 3, 64, 1, 0),      # channel count not covered: fallback under the same bound
    (2, 32, (3, 5, 7), MEDIUM, 130, 1, 0),             # T % 4 != 0: fallback
]


def run_and_judge(b, case, sd, row_scale=False):
    type_, C, Ks, dils, T, N, npairs = case
    per = [operands((type_, C, K, d, T, N, 0), sd + 100 * j) for j, (K, d) in enumerate(zip(Ks, dils))]
    x, ws, bs = per[0][0], [p[1] for p in per], [p[2] for p in per]
    if row_scale:
        rows = np.where(np.arange(C) % 2, np.float32(2.0 ** -20), np.float32(2.0 ** 10)).astype(np.float32)[:, None, None]
        ws, bs = [[w * rows for w in wj] for wj in ws], [[v * np.float32(2.0 ** -20) for v in bj] for bj in bs]
    with routes_armed(b):
        out = b.hifiganMrfF16(type_, up(b, x), N, C, T, list(Ks), [list(d) for d in dils], [up(b, w) for wj in ws for w in wj],
                              [up(b, v) for bj in bs for v in bj], 0.1)
        recs = [cr.variant_of(r) for r in b.last_routes()]
    fam = [cr.family_of(v) for v in recs]
    assert fam.count(FAMILY) == npairs and set(fam) <= {FAMILY, "f16"}, fam
    for prm in (cr.params_of(v) for v in recs if cr.family_of(v) == FAMILY):
        assert prm.get("form", "1") == str(type_) and prm["multi"] == "3" and prm["wsrc"] == "l2", recs
    got = b.downloadFloat32(out).reshape(N, C, T)
    walks = [resblock_walk(type_, x, K, d, w, v) for K, d, w, v in zip(Ks, dils, ws, bs)]
    # row_scale is judged against the clamped walk (test_gpu_rb_pair_f16's module docstring); without outliers the two references agree
    rs = [wk[0] for wk in walks] if row_scale else [hifigan_resblock(type_, x, K, d, w, v) for K, d, w, v in zip(Ks, dils, ws, bs)]
    j = judge_elem(got, ((rs[0] + rs[1]) + rs[2]) / 3, sum(wk[1] for wk in walks) / 3 + 2.0 ** -23 * sum(np.abs(r) for r in rs))
    print(f"hifigan_mrf_f16 {case} row_scale={row_scale}: worst error {j['ratio']:.3f} of the bound")
    return np.all(np.isfinite(got)) and j["ok"], j


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"rb{c[0]}_C{c[1]}_K{'-'.join(map(str, c[2]))}_d{'-'.join(map(str, c[3][0]))}_T{c[4]}_n{c[5]}")
def test_hifigan_mrf_f16(case, backend):
    ok, j = run_and_judge(backend, case, SD + 1000 * CASES.index(case))
    assert ok, (case, j)


def test_rb2_pair_f16_row_scale(backend):
    """Odd output rows × 2⁻²⁰, even rows × 2¹⁰, biases × 2⁻²⁰: both scales act per channel, before the bias and the fp32 x1 add."""
    ok, j = run_and_judge(backend, CASES[2], SD + 9000, row_scale=True)
    assert ok, j


def test_f16_medium_voice_runs_rb2_pairs(voices, backend):
    """F = 42, one item and the ragged batch of two (merged schedule): every ResBlock step of the 64- / 32-channel stages carries form-2
    records of three pairs, none runs single convs (dec.s0., 128 channels, is not eligible); test_f16_voice's criterion against the oracle.
    F = 1540 (per-ResBlock schedule): one pair per launch, the closing step folds the MRF mean; rms(f16 − f32) ≤ rms(bf16 − f32)/4."""
    cfg, blob = voices["medium"]
    stages = ("dec.s1.", "dec.s2.")
    ids, dur, long_dur = kd.FIXTURE_IDS, [3] * 14, [110] * 14
    noise, noise2, long_noise = (kd.sym(SD + 900 + i, (cfg.inter, f), 1.7320508) for i, f in enumerate((42, 21, 1540)))
    ref1 = orc.synthesize(cfg, blob, ids, dur, noise, 0.667)
    ref2 = np.concatenate([ref1, orc.synthesize(cfg, blob, ids[:7], dur[:7], noise2, 0.667)])

    def paired_steps(sched, multi):
        prm = {name: [cr.params_of(cr.variant_of(r)) for r in recs if cr.family_of(cr.variant_of(r)) == FAMILY] for name, recs in sched}
        paired = {name for name, p in prm.items() if p}
        assert all(q["form"] == "2" and q["multi"] == multi for name in paired for q in prm[name]), prm
        assert all(name.startswith(stages) and ".rb" in name for name in paired) and {name[:7] for name in paired} == set(stages), paired
        singles = [name for name, _ in sched if name.startswith(stages) and ".rb" in name and name not in paired]
        assert not singles, singles
        return paired

    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        e, long_wave = {}, {}
        for prec in ("f32", "bf16", "f16"):
            rt.set_precision(prec)
            with routes_armed(backend):
                rt.prepare(0, ids, dur, noise, 0.667)
                rt.prepare_batch(1, [(ids, dur, noise), (ids[:7], dur[:7], noise2)], 0.667)
                rt.prepare(2, ids, long_dur, long_noise, 0.667)
                waves = []
                for slot in range(3):
                    rt.launch(slot)
                    waves.append(rt.collect(slot).copy())
                scheds = [rt.routes(slot) for slot in range(3)]
            assert all(np.all(np.isfinite(w)) for w in waves)
            e[prec], long_wave[prec] = (rms(waves[0], ref1), rms(waves[1], ref2)), waves[2]
        paired_steps(scheds[0], "3"), paired_steps(scheds[1], "3")  # the f16 plans
        closing = [name for name in paired_steps(scheds[2], "1") if name.endswith("_mrfmean")]
        assert sorted(name[:7] for name in closing) == sorted(stages), closing
        d16, db = rms(long_wave["f16"], long_wave["f32"]), rms(long_wave["bf16"], long_wave["f32"])
        print(f"medium: RMS error vs oracle (one item, ragged batch) {e}; F = 1540 vs the f32 waveform: f16 {d16:.3e} bf16 {db:.3e}")
        assert all(e["f16"][i] <= max(e["bf16"][i] / 4, 4 * e["f32"][i]) for i in range(2)), e
        assert d16 <= db / 4, (d16, db)
    finally:
        rt.close()
