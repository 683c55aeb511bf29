"""GPU: every step in front of the generator against a float64 reference (tests/front_ref.py), teacher-forced from the GPU's own buffers.

Per case one prepare / launch / collect; z of every item is checked against the fp32 oracle as before, then front_ref.verify walks the
slot's step list: per step it reads what the step reads with "<tensor>@<previous step>", what it writes with "<tensor>@<this step>"
(piper_hip_voice_tap's step selector) and compares with the float64 formula under the plain rule |Δ| ≤ OP_TOL · max(1, ‖ref‖∞) — no
allowance. No step is skipped; a step name the walker does not know fails the test. Per case one `FRONTEXACT {json}` line: the worst
max|Δ| / bound per kind of step and the reference's wall time (profiles/front_exact_units.md keeps the measured figures).

Which kernel a step takes is decided by tile counts against the CU count (csrc/conv_lean.hip try_launch_conv_lean, csrc/conv_short.hip,
csrc/conv.hip launch_conv_mfma, csrc/voice.hip build_encoder / build_flow, csrc/attention.hip rel_attention_split_parts). A plan is built
for the BUCKET: Tb = ⌈T / 16⌉ · 16, Fb = ⌈F / 16⌉ · 16 (⌈F / 64⌉ · 64 above 1024 frames). One utterance, 256 CUs, medium voice:

  LayerNorm folded into its consumers      Tb · NB ≤ 640; `ln_self` (consumer computes the statistics: o_add / ffn2_add) where the lean kernels
                                           take qkv, ffn1 and proj of a whole-utterance plan, else `stats_out` (o_add_stats / ffn2_add_stats:
                                           the predictor plan, PIPER_HIP_NO_LN_SELF); above 640: add_ln1 / add_ln2 kernels, plain convs
  attention                                key-split in 2 parts + merge from Tb = 144, 3 parts at 656, unsplit again above 1024
  FFN conv 2                               the 8-row kernel while 24 · ⌈Tb / 16⌉ tiles ≤ 2 · CUs (Tb ≤ 336)
  blocks walk several 16-column chunks     gated conv from Fb > 672, folded tail from Fb > 896, k = 1 convs from Fb > 1360
  flow tail                                folded (…res_skip_post_sub_flip_preN) by default; seam / post_sub + pre through the switches

Where the step list tells the path the cases assert it."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process of test_fallback_schedules_in_child_processes: no conftest has set the path up
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.join(os.path.dirname(_here), "piper-swift_amd", "python")]

import front_ref as fr
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, assert_close

pytestmark = pytest.mark.gpu


def _ids(T, seed):
    return list(np.random.RandomState(seed).randint(1, 130, size=T))


# (label, [(ids, dp_noise)], noise_w): tests/test_front_ref.py checks on the CPU that these seeds keep ≤ 1 % of the ids within 1e-4 of an
# integer duration
PREDICT_CASES = [
    ("predict T=14", [(_ids(14, 1), fr.dp_noise(14, 1))], 0.8),
    ("predict T=130", [(_ids(130, 2), fr.dp_noise(130, 2))], 0.8),
    ("predict ragged 40/7/1", [(_ids(40, 3), fr.dp_noise(40, 3)), (_ids(7, 4), fr.dp_noise(7, 4)), (_ids(1, 5), fr.dp_noise(1, 5))], 0.8),
    ("predict T=14 noise_w=0", [(_ids(14, 6), fr.dp_noise(14, 6))], 0.0),
]


def report_line(label, rows, ref_s, **extra):
    print("FRONTEXACT " + json.dumps(dict(case=label, worst={k: round(v, 5) for k, v in fr.worst_by_kind(rows).items()}, ref_s=round(ref_s, 2), **extra)))


def run_and_verify(rt, blob, slot, utts, label, check_z=True, z_max_ids=None, att_floorless=False):
    """prepare + launch + collect, z of every item against the oracle (z_max_ids: only of the items with at most that many ids — the CPU
    oracle's flow is the slow part of a long item, which the steps cover one by one), then every front step of every item (att_floorless:
    front_ref.verify's keyword). → (audio, rows, step names)."""
    cfg = rt.cfg
    if len(utts) == 1:
        rt.prepare(slot, *utts[0], fr.NOISE_SCALE)
    else:
        rt.prepare_batch(slot, utts, fr.NOISE_SCALE)
    rt.launch(slot)
    audio = rt.collect(slot).copy()
    lensT, lensF = [len(u[0]) for u in utts], [int(np.sum(u[1])) for u in utts]
    if check_z:
        z = rt.tap(slot, "z")
        offs = np.concatenate([[0], np.cumsum(lensF)]) * cfg.inter
        for b, u in enumerate(utts):
            if z_max_ids is not None and len(u[0]) > z_max_ids:
                continue
            _, taps = orc.synthesize(cfg, blob, u[0], u[1], u[2], fr.NOISE_SCALE, taps=True)
            assert_close(z[offs[b]:offs[b + 1]], taps["z"].reshape(-1), OP_TOL, f"{label}[{b}]: z vs oracle")
    dev = fr.GpuDevice(rt, slot, lensT, lensF)
    rows, ref_s = fr.verify(dev, cfg, blob, [fr.Inputs(*u) for u in utts], label, att_floorless=att_floorless)
    # the tensor "z" the generator reads is the buffer the last flow step left the latent in
    report_line(label, rows, ref_s, T=lensT, F=lensF)
    return audio, rows, [n for n in dev.steps() if fr.is_front_step(n)]


@pytest.fixture(scope="module")
def rts(backend, voices):
    out = {q: ph.HipRuntime(backend, *voices[q]) for q in ("medium", "high")}
    yield out
    for rt in out.values():
        rt.close()


def single(rts, voices, quality, T, F, slot, durations=None):
    cfg, blob = voices[quality]
    rt = rts[quality]
    _, rows, steps = run_and_verify(rt, blob, slot, [fr.utterance(cfg, T, F, 1000 + T + F, durations)], f"{quality} T={T} F={F}")
    info = rt.plan_info(slot)
    assert info["bucket_t"] == -(-T // 16) * 16
    return cfg, rows, steps


def assert_default_path(cfg, steps, ln="self", fold=True):
    sfx = {"self": "", "stats": "_stats"}.get(ln)
    for l in range(cfg.n_layers):
        if ln == "plain":
            assert {f"enc{l}.o", f"enc{l}.add_ln1", f"enc{l}.ffn1_relu", f"enc{l}.ffn2", f"enc{l}.add_ln2", f"enc{l}.qkv"} <= set(steps), steps
        else:
            assert {f"enc{l}.o_add{sfx}", f"enc{l}.ln1_ffn1_relu", f"enc{l}.ffn2_add{sfx}"} <= set(steps), steps
    assert ("enc.proj" if ln == "plain" else "enc.ln2_proj") in steps
    folded = [s for s in steps if "res_skip_post_sub" in s]
    assert len(folded) == (cfg.n_flows if fold else 0), steps


@pytest.mark.parametrize("quality", ["medium", "high"])
@pytest.mark.parametrize("T,F,dur", [(1, 1, None), (14, 42, None), (3, 7, [4, 0, 3])])
def test_short_utterances(quality, T, F, dur, rts, voices):
    """T = 1 / F = 1: one column in a 16-column bucket, every halo is padding. T = 14 / F = 42: factor 1. T = 3 with a zero duration in the
    middle: an id without a frame."""
    cfg, rows, steps = single(rts, voices, quality, T, F, 0, dur)
    assert_default_path(cfg, steps)


def test_key_split_attention_and_partial_chunk(rts, voices):
    """T = 130 (bucket 144): key-split attention in two parts plus merge, ln_self, FFN conv 2 on the 8-row kernel (24 · 9 = 216 tiles ≤ 512),
    the last 16-column chunk partial (130 = 8 · 16 + 2; F = 390 = 24 · 16 + 6)."""
    cfg, rows, steps = single(rts, voices, "medium", 130, 390, 1)
    assert_default_path(cfg, steps)


def test_long_utterance_multi_chunk_blocks(rts, voices):
    """T = 340 (bucket 352), F = 1400 (bucket 1408): FFN conv 2 leaves the 8-row kernel (24 · 22 = 528 tiles > 2 · CUs), ln_self still on; blocks
    walk several chunks in the gated conv (F > 672), the folded tail (F > 896) and the k = 1 convs (F > 1360); the last chunk is partial."""
    cfg, rows, steps = single(rts, voices, "medium", 340, 1400, 2)
    assert_default_path(cfg, steps)


def test_unfused_layernorm_above_640_columns(rts, voices):
    """T = 650 (bucket 656 > 640), durations of 1: the add_layernorm kernels, plain qkv / FFN / proj convs, the FFN's plain k = 3 conv on the
    streaming kernel, three attention key parts."""
    cfg, rows, steps = single(rts, voices, "medium", 650, 650, 3)
    assert_default_path(cfg, steps, ln="plain")


def test_unsplit_attention_above_1024(rts, voices):
    """T = 1040, durations of 1: attention rows above 1024 run unsplit."""
    cfg, rows, steps = single(rts, voices, "medium", 1040, 1040, 4)
    assert_default_path(cfg, steps, ln="plain")


def test_ragged_batch_every_item(rts, voices, quality="medium"):
    cfg, blob = voices[quality]
    utts = [fr.utterance(cfg, T, 3 * T, 300 + T) for T in (130, 5, 61, 1)]
    _, rows, steps = run_and_verify(rts[quality], blob, 5, utts, f"{quality} ragged 130/5/61/1")
    assert {r[2] for r in rows} == {0, 1, 2, 3}
    assert_default_path(cfg, steps)


def test_batch_of_twenty_takes_the_unfused_schedule(rts, voices):
    """20 × T = 40 (bucket 48: Tb · NB = 960 > 640): the unfused LayerNorm schedule in a batch."""
    cfg, blob = voices["medium"]
    utts = [fr.utterance(cfg, 40, 40, 100 + b) for b in range(20)]
    _, rows, steps = run_and_verify(rts["medium"], blob, 6, utts, "medium 20x40")
    assert_default_path(cfg, steps, ln="plain")


@pytest.mark.parametrize("F_short", [339, 371])
def test_plan_reuse_with_a_shorter_utterance(F_short, rts, voices):
    """T = 126 / F = 378, then T = 113 on the same slot. F = 371 lands on the same plan (128 ids, 384 frames): columns past the true length
    still hold the longer utterance's values in every reused buffer, encoder and flow. F = 339 falls into the 352-frame bucket: its plan
    is another one, taken from the cache onto the same slot id."""
    cfg, blob = voices["medium"]
    rt = rts["medium"]
    run_and_verify(rt, blob, 7, [fr.utterance(cfg, 126, 378, 400)], "medium long")
    info = rt.plan_info(7)
    run_and_verify(rt, blob, 7, [fr.utterance(cfg, 113, F_short, 401)], f"medium short (F={F_short}) after long")
    after = rt.plan_info(7)
    assert after["bucket_t"] == info["bucket_t"] == 128
    assert (after["bucket_f"] == info["bucket_f"]) == (F_short == 371), "F = 371 must land on the same plan"


def prepare_predicted(rt, slot, utts, noise_w):
    """prepare_batch with durations = NULL: (ids, dp_noise) per item, the flow's noise injected as zeros."""
    n = len(utts)
    arr = (ph.Utterance * n)()
    keep = []
    for i, (ids, dpn) in enumerate(utts):
        u, k = rt._utt(ids, None, None, fr.NOISE_SCALE, noise_w=noise_w, dp_noise=dpn)
        arr[i] = u
        keep.append(k)
    rc = rt.lib.piper_hip_voice_prepare_batch(rt.voice, arr, n, slot)
    assert rc >= 0, rc
    tot = C.c_int64()
    assert rt.lib.piper_hip_voice_prepared_samples(rt.voice, slot, None, 0, C.byref(tot)) == 0
    rt._keep[slot] = (keep, int(tot.value))


@pytest.mark.parametrize("case", range(len(PREDICT_CASES)))
@pytest.mark.parametrize("quality", ["medium", "high"])
def test_predictor_plan(quality, case, rts, voices):
    """prepare(durations = NULL): the cached encoder + predictor plan through the "predict:" selector — the stats_out encoder, enc.ln2_final,
    every dp.* step, logw and the integer durations — then the slot's own plan (it continues from the copied projection: expansion and flow)
    with the predicted durations."""
    label, utts, nw = PREDICT_CASES[case]
    cfg, blob = voices[quality]
    rt = rts[quality]
    prepare_predicted(rt, 8, utts, nw)
    rt.launch(8)
    rt.collect(8)
    lensT = [len(u[0]) for u in utts]
    dur = rt.durations(8)
    offs = np.concatenate([[0], np.cumsum(lensT)])
    durs = [dur[offs[b]:offs[b + 1]] for b in range(len(utts))]
    pdev = fr.GpuDevice(rt, 8, lensT, [0] * len(utts), predict=True)
    rows, ref_s = fr.verify(pdev, cfg, blob, [fr.Inputs(ids, dp_noise=dpn, noise_w=nw) for ids, dpn in utts], f"{quality} {label}")
    steps = pdev.steps()
    assert "enc.ln2_final" in steps and "dp.affine_exp_ceil" in steps and any(s.endswith("o_add_stats") for s in steps), steps
    report_line(f"{quality} {label}", rows, ref_s)
    # the durations the slot uses are the ones the predictor plan left (Piper: at least one frame per utterance)
    got = pdev.read("dp.dur", "dp.affine_exp_ceil")
    for b in range(len(utts)):
        want = got[b].reshape(-1).astype(np.int64)
        if want.sum() < 1:
            want[0] = 1
        assert np.array_equal(want, durs[b])
    lensF = [int(d.sum()) for d in durs]
    dev = fr.GpuDevice(rt, 8, lensT, lensF)
    assert dev.steps()[0] == "expand_noise"
    inputs = [fr.Inputs(ids, durs[b], np.zeros((cfg.inter, lensF[b]), np.float32)) for b, (ids, _) in enumerate(utts)]
    rows2, ref_s2 = fr.verify(dev, cfg, blob, inputs, f"{quality} {label} flow")
    report_line(f"{quality} {label} flow", rows2, ref_s2, F=lensF)


def test_selector_leaves_the_slot_as_a_full_run(rts, voices):
    """Reading with "@" leaves collect's audio and the plain taps of a following read bit-identical to a run without it; an unknown step name
    is PIPER_HIP_ERR_ARG."""
    cfg, blob = voices["medium"]
    rt = rts["medium"]
    utt = fr.utterance(cfg, 14, 42, 77)
    rt.prepare(9, *utt, fr.NOISE_SCALE)
    rt.launch(9)
    audio = rt.collect(9).copy()
    plain = {n: rt.tap(9, n).copy() for n in ("enc_out", "m_p", "logs_p", "z_p", "z", "dec_pre")}
    steps = rt.steps(9)
    assert steps == [s["name"] for s in rt.profile(9, iters=1) if not s["name"].startswith("(") and not s["name"].endswith((".fork", ".join"))]
    for name in ("front.h@flow2.wn1.in_gate", "front.x@embed", "front.zp@expand_noise", "z@" + steps[-1]):
        rt.tap(9, name)
    for n, v in plain.items():
        assert np.array_equal(rt.tap(9, n), v), n
    assert np.array_equal(rt.collect(9), audio)
    rt.launch(9)
    assert np.array_equal(rt.collect(9), audio)
    with pytest.raises(ph.InvalidArgument):
        rt.tap(9, "front.h@flow2.no_such_step")
    with pytest.raises(ph.InvalidArgument):
        rt.tap(9, "front.nothing@embed")


SWITCH_SETS = {
    "no_lean": {"PIPER_HIP_NO_LEAN": "1"},
    "no_lean_no_short": {"PIPER_HIP_NO_LEAN": "1", "PIPER_HIP_NO_SHORT": "1"},
    "no_lean_no_short_tm32": {"PIPER_HIP_NO_LEAN": "1", "PIPER_HIP_NO_SHORT": "1", "PIPER_HIP_TM16_BELOW": "0"},
    "no_flow_fold": {"PIPER_HIP_NO_FLOW_FOLD": "1"},
    "no_flow_fold_no_seam": {"PIPER_HIP_NO_FLOW_FOLD": "1", "PIPER_HIP_NO_FLOW_SEAM": "1"},
    "no_ln_self": {"PIPER_HIP_NO_LN_SELF": "1"},
    "no_ln_fuse": {"PIPER_HIP_NO_LN_FUSE": "1"},
    "att_block": {"PIPER_HIP_ATT_BLOCK": "1"},
}


@pytest.mark.parametrize("switches", list(SWITCH_SETS))
def test_fallback_schedules_in_child_processes(switches):
    """The production paths of large batches, reached at small shapes through the A/B switches (read once per process, need
    PIPER_HIP_TUNING=1): one child per switch set; medium T = 14 / F = 42 and T = 130 / F = 390, high T = 14 / F = 42 in each.
    NO_LEAN: conv_short for the gated and the LayerNorm-behind k = 3 convs, the streaming k = 1 convs, flow_seam.hip; + NO_SHORT: the
    streaming kernel everywhere, 16-wide tiles with K-split; + TM16_BELOW=0: 32-wide tiles; NO_FLOW_FOLD: seam + the lean EPI_WN_SKIP_LAST
    conv; + NO_FLOW_SEAM: post_sub with the reversed output map and a separate pre with the reversed input map; NO_LN_SELF: the statistics
    path on a whole-utterance plan; NO_LN_FUSE: the unfused LayerNorm schedule; ATT_BLOCK: the attention + conv_o + LayerNorm launch."""
    env = dict(os.environ, PIPER_HIP_TUNING="1", **SWITCH_SETS[switches])
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", switches], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{switches}: the child hung on the GPU; nothing more is started on it", returncode=3)
    print(out.stdout[-30000:])
    if out.returncode < 0 or out.returncode in (134, 139):  # died on a signal: a GPU fault or an abort — a finding, not a test to go on from
        pytest.exit(f"{switches}: the child died with status {out.returncode}; nothing more is started on the GPU\n" + out.stderr[-3000:], returncode=3)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "child ok" in out.stdout


def _child(switches):
    backend = ph.HipBackend(0)
    try:
        for quality, T, F in (("medium", 14, 42), ("medium", 130, 390), ("high", 14, 42)):
            cfg = ph.voice_config(quality)
            blob = ph.synthetic_blob(cfg, 1234)
            rt = ph.HipRuntime(backend, cfg, blob)
            try:
                _, rows, steps = run_and_verify(rt, blob, 0, [fr.utterance(cfg, T, F, 500 + T)], f"{switches} {quality} T={T} F={F}")
                if switches == "no_flow_fold":
                    assert not [s for s in steps if "res_skip_post_sub" in s] and sum("post_sub_flip_pre" in s for s in steps) == cfg.n_flows - 1, steps
                elif switches == "no_flow_fold_no_seam":
                    assert sum(s.endswith(".post_sub") for s in steps) == cfg.n_flows and sum(s.endswith(".pre") for s in steps) == cfg.n_flows, steps
                elif switches == "no_ln_self":
                    assert_default_path(cfg, steps, ln="stats")
                elif switches == "no_ln_fuse":
                    assert_default_path(cfg, steps, ln="plain")
                elif switches == "att_block":
                    assert sum(s.endswith("attention_o_add_ln1") for s in steps) == cfg.n_layers, steps
            finally:
                rt.close()
        cs = ph.config_string()
        for k in SWITCH_SETS[switches]:
            assert k in cs, (k, cs)
    finally:
        backend.close()
    print("child ok")


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    _child(sys.argv[2])
