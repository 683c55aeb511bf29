"""GPU: the folded tail of the flow couplings (conv_k1_tail_kernel behind fold_flow_tail) against the oracle.

Each coupling's last res_skip conv, post, x1 − m, Flip and the next coupling's pre run as ONE k = 1 launch over a matrix multiplied
out when the voice is created. The cases are the sizes at which that launch takes another path: less than one 16-column chunk, a
partial last chunk, a ragged batch whose shortest item ends inside the first chunk, rows long enough that a block walks several
chunks, a cached plan serving a shorter utterance, and the bounded predicted-durations plan. z at OP_TOL, the waveform at WAVE_TOL."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import katdata as kd
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, ROOT, WAVE_TOL, assert_close

pytestmark = pytest.mark.gpu

SD = kd.case_seed("mod", 0) + 7000
QUALITIES = ["medium", "high"]


@pytest.fixture(scope="module")
def rts(backend, voices):
    out = {q: ph.HipRuntime(backend, *voices[q]) for q in QUALITIES}
    yield out
    for rt in out.values():
        rt.close()


def utterance(F, seed, inter=192):
    """T ids whose durations sum to F exactly (3 frames per id, the first ids shortened or dropped to fit)."""
    T = max(1, -(-F // 3))
    ids = (kd.FIXTURE_IDS * (T // len(kd.FIXTURE_IDS) + 1))[:T]
    dur = [3] * T
    for i in range(3 * T - F):
        dur[i % T] -= 1
    assert sum(dur) == F and min(dur) >= 0
    return ids, dur, kd.sym(seed, (inter, F), 1.7320508)


def check_single(rt, cfg, blob, ids, dur, noise, what, slot=0):
    F = int(np.sum(dur))
    rt.prepare(slot, ids, dur, noise, 0.667)
    rt.launch(slot)
    audio = rt.collect(slot)
    z = rt.tap(slot, "z", cfg.inter * F)
    ref_audio, ref_taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
    assert_close(z, ref_taps["z"], OP_TOL, what + ": z")
    assert_close(audio, ref_audio, WAVE_TOL, what + ": audio")
    assert_close(rt.tap(slot, "z_p", cfg.inter * F), ref_taps["z_p"], OP_TOL, what + ": z_p (the pristine copy)")


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("F", [7, 37, 1037])
def test_single_utterance(quality, F, rts, voices):
    """F = 7: less than one chunk; 37: a partial last chunk; 1037: 65 chunks × 18 row tiles pass four blocks per CU, so every block
    walks several chunks (alternating exchange buffer) and the last one is partial."""
    cfg, blob = voices[quality]
    ids, dur, noise = utterance(F, SD + F, cfg.inter)
    check_single(rts[quality], cfg, blob, ids, dur, noise, f"{quality} F={F}")


@pytest.mark.parametrize("quality", QUALITIES)
def test_ragged_batch_shortest_item_inside_the_first_chunk(quality, rts, voices):
    cfg, blob = voices[quality]
    rt = rts[quality]
    utts = [utterance(F, SD + 100 + F, cfg.inter) for F in (37, 5, 50)]
    rt.prepare_batch(2, utts, 0.667)
    assert rt.plan_info(2)["bucket_f"] >= 50
    rt.launch(2)
    audio = rt.collect(2)
    z = rt.tap(2, "z", sum(cfg.inter * int(np.sum(u[1])) for u in utts))
    off = zoff = 0
    for b, (ids, dur, noise) in enumerate(utts):
        F = int(np.sum(dur))
        ref, taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
        assert_close(z[zoff:zoff + cfg.inter * F], taps["z"], OP_TOL, f"{quality} ragged item {b}: z")
        assert_close(audio[off:off + F * cfg.hop], ref, WAVE_TOL, f"{quality} ragged item {b}: audio")
        off += F * cfg.hop
        zoff += cfg.inter * F
    assert off == audio.size


@pytest.mark.parametrize("quality", QUALITIES)
def test_plan_reused_by_a_shorter_utterance(quality, rts, voices):
    """The second utterance runs on the first one's plan: columns past its end still hold the longer one's values in both z buffers."""
    cfg, blob = voices[quality]
    rt = rts[quality]
    ids, dur, noise = utterance(45, SD + 200, cfg.inter)
    check_single(rt, cfg, blob, ids, dur, noise, f"{quality} F=45", slot=3)
    info = rt.plan_info(3)
    ids, dur, noise = utterance(35, SD + 201, cfg.inter)
    check_single(rt, cfg, blob, ids, dur, noise, f"{quality} F=35 on the plan of F=45", slot=3)
    after = rt.plan_info(3)
    assert after["cached_plans"] == info["cached_plans"] and after["bucket_f"] == info["bucket_f"]


@pytest.mark.parametrize("quality", QUALITIES)
def test_bounded_predicted_durations(quality, rts, voices):
    cfg, blob = voices[quality]
    rt = rts[quality]
    ids = kd.FIXTURE_IDS * 2
    nz = kd.sym(SD + 300, (2, len(ids)), 1.7320508)
    kw = dict(length_scale=1.1, noise_w=0.8, dp_noise=nz, noise_mode="device", seed=91)
    rt.prepare(1, ids, None, None, 0.667, **kw)  # the two-step path decides the durations the bounded plan must reproduce
    rt.launch(1)
    rt.collect(1)
    dur = rt.durations(1).copy()
    F = int(dur.sum())
    rt.prepare(4, ids, None, None, 0.667, max_frames=F + 21, **kw)
    rt.launch(4)
    audio = rt.collect(4)
    assert audio.size == F * cfg.hop and np.array_equal(rt.durations(4), dur)
    noise = orc.random_normal_like(cfg.inter * F, 91).reshape(cfg.inter, F)
    ref, taps = orc.synthesize(cfg, blob, ids, dur.tolist(), noise, 0.667, taps=True)
    assert_close(rt.tap(4, "z", cfg.inter * F), taps["z"], OP_TOL, f"{quality}: bounded, z")
    assert_close(audio, ref, WAVE_TOL, f"{quality}: bounded, audio")


def step_names(rt, slot):
    return [e["name"] for e in rt.profile(slot, iters=1) if not e["name"].startswith("(")]  # (without the event-floor pseudo-entry)


def factor8(cfg):
    ids = kd.FIXTURE_IDS * 8
    return ids, [3] * len(ids), kd.sym(SD + 400, (cfg.inter, 3 * len(ids)), 1.7320508)


@pytest.mark.parametrize("quality", QUALITIES)
def test_step_list_has_one_tail_launch_per_coupling(quality, rts, voices):
    cfg, _ = voices[quality]
    rt = rts[quality]
    ids, dur, noise = factor8(cfg)
    rt.prepare(5, ids, dur, noise, 0.667)
    rt.launch(5)
    rt.collect(5)
    names = step_names(rt, 5)
    last = cfg.wn_layers - 1
    want = [f"flow{f}.wn{last}.res_skip_post_sub_flip_pre{f - 1}" for f in range(cfg.n_flows - 1, 0, -1)] + [f"flow0.wn{last}.res_skip_post_sub"]
    assert [n for n in names if "post_sub" in n] == want, names
    assert not any("flow_seam" in n or n.endswith(f".wn{last}.res_skip") or ".post_sub_flip_pre" in n for n in names), names
    if quality == "medium":
        assert len(names) == 75, (len(names), names)


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[3]]
import katdata as kd
import piper_hip as ph
backend = ph.HipBackend(0)
out = {}
for q in ("medium", "high"):
    cfg = ph.voice_config(q)
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    ids = kd.FIXTURE_IDS * 8
    dur = [3] * len(ids)
    rt.prepare(0, ids, dur, kd.sym(int(sys.argv[4]), (cfg.inter, 3 * len(ids)), 1.7320508), 0.667)
    rt.launch(0)
    rt.collect(0)
    out[q + "_z"] = rt.tap(0, "z", cfg.inter * 3 * len(ids))
    out[q + "_names"] = np.array([e["name"] for e in rt.profile(0, iters=1) if not e["name"].startswith("(")])
    rt.close()
out["config"] = np.array(ph.config_string())
backend.close()
np.savez(sys.argv[1], **out)
"""


def test_switch_restores_the_unfolded_schedule(rts, voices):
    """One fresh child process with PIPER_HIP_NO_FLOW_FOLD=1 (honoured under PIPER_HIP_TUNING=1): the seam schedule's step list, and a z
    that agrees with the folded one at OP_TOL."""
    env = dict(os.environ, PIPER_HIP_TUNING="1", PIPER_HIP_NO_FLOW_FOLD="1")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "unfolded.npz")
        subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "tests"), os.path.join(ROOT, "piper-swift_amd", "python"), str(SD + 400)],
                       env=env, check=True, timeout=300)
        got = dict(np.load(path))
    assert "PIPER_HIP_NO_FLOW_FOLD" in str(got["config"])
    for q in QUALITIES:
        cfg, _ = voices[q]
        names = [str(n) for n in got[q + "_names"]]
        last = cfg.wn_layers - 1
        want = [f"flow{f}.post_sub_flip_pre{f - 1}" for f in range(cfg.n_flows - 1, 0, -1)] + ["flow0.post_sub"]
        assert [n for n in names if "post_sub" in n] == want, names
        assert sum(n.endswith(f".wn{last}.res_skip") for n in names) == cfg.n_flows
        if q == "medium":
            assert len(names) == 79, (len(names), names)
        ids, dur, noise = factor8(cfg)
        rts[q].prepare(6, ids, dur, noise, 0.667)
        rts[q].launch(6)
        rts[q].collect(6)
        assert_close(rts[q].tap(6, "z", cfg.inter * sum(dur)), got[q + "_z"], OP_TOL, f"{q}: folded z vs the unfolded schedule")
