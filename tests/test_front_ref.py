"""CPU: tests/front_ref.py proves itself before tests/test_gpu_front_exact.py relies on it.

  * free running in float64 it agrees with the C oracle's taps (enc_out, m_p, logs_p, z_p, z, logw) and with tests/golden at OP_TOL —
    for the folded-LayerNorm + folded-tail schedule, for the seam schedule and for the add_layernorm schedule (one walker, three step lists);
  * the verifier passes over a stand-in for the device (front_ref.SimDevice: the same steps in float32, channels and taps summed in the
    reverse order), which records how far honest fp32 sits inside the bound (`FRONTEXACT` lines, profiles/front_exact_units.md);
  * each defect planted into that stand-in is caught, at the step it sits in;
  * a step name the walker does not know fails."""
import json
import os

import numpy as np
import pytest

import front_ref as fr
import katdata as kd
import oracle as orc
from conftest import OP_TOL, assert_close

SD = kd.case_seed("dp", 0)
QUIET = lambda *_: None


def sim(cfg, blob, names, inputs, defect=None, dtype=np.float32):
    return fr.SimDevice(cfg, fr.FrontRef(cfg, blob, dtype, reverse=dtype == np.float32), names, inputs, defect)


@pytest.fixture(scope="module")
def medium(voices):
    cfg, blob = voices["medium"]
    return cfg, blob, fr.FrontRef(cfg, blob)


@pytest.fixture(scope="module")
def case14(medium):
    """T = 14, F = 42 with ragged durations (one zero): whole-utterance inputs and the honest stand-in on the default schedule."""
    cfg, blob, _ = medium
    dur = [3, 5, 1, 2, 0, 4, 3, 1, 2, 6, 4, 5, 3, 3]
    ids, dur, noise = fr.utterance(cfg, 14, 42, 7, durations=dur)
    inp = fr.Inputs(ids, dur, noise)
    return inp, fr.default_steps(cfg), sim(cfg, blob, fr.default_steps(cfg), [inp])


@pytest.mark.parametrize("fold,ln", [(True, "self"), (False, "stats"), (False, "plain")])
def test_free_running_float64_vs_oracle_and_golden(fold, ln, medium, golden_mods):
    cfg, blob, _ = medium
    ids, dur = kd.FIXTURE_IDS, [3] * 14
    noise = kd.sym(kd.case_seed("mod", 0) + 80, (192, 42), 1.7320508)  # the inputs of golden "synth_f1" (tests/test_gpu_voice.py)
    names = fr.default_steps(cfg, fold=fold, ln=ln)
    dev = sim(cfg, blob, names, [fr.Inputs(ids, dur, noise)], dtype=np.float64)
    _, taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
    last = dev.snap[(names[-1], 0)]
    zbuf = "front.zp"  # an even number of couplings ends where it began
    got = dict(enc_out=last["front.x"], m_p=last["front.stats"][:cfg.inter], logs_p=last["front.stats"][cfg.inter:], z_p=last["z_p"], z=last[zbuf])
    for k, v in got.items():
        assert_close(v, taps[k], OP_TOL, k + " vs oracle")
        assert_close(v, golden_mods["synth_f1." + k], OP_TOL, k + " vs golden")


@pytest.mark.parametrize("quality", ["medium", "high"])
@pytest.mark.parametrize("nw", [0.8, 0.0])
def test_free_running_predictor_vs_oracle_and_golden(quality, nw, voices):
    cfg, blob = voices[quality]
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "dp.npz"))
    ids = kd.FIXTURE_IDS
    dpn = kd.sym(SD + 1, (2, 14), 1.7320508)
    names = fr.default_steps(cfg, predict=True)
    dev = sim(cfg, blob, names, [fr.Inputs(ids, dp_noise=dpn, noise_w=nw)], dtype=np.float64)
    last = dev.snap[(names[-1], 0)]
    enc, _ = orc.text_encoder(cfg, blob, ids)
    assert_close(last["front.x"], enc, OP_TOL, "enc_out vs oracle")
    lw = orc.duration_logw(cfg, blob, enc, dpn, nw)
    assert np.abs(last["dp.logw"].reshape(-1) - lw).max() <= 2e-4  # the oracle is fp32: test_duration_predictor.LOGW_TOL
    ref = g[f"{quality}.f1.nw{nw}.logw"]
    assert np.abs(last["dp.logw"].reshape(-1) - ref).max() <= 2e-4
    w = np.exp(np.asarray(ref, np.float64))
    safe = np.abs(w - np.round(w)) > 2e-3
    assert np.array_equal(last["dp.dur"].reshape(-1)[safe], g[f"{quality}.f1.nw{nw}.dur"][safe])


def test_verifier_passes_on_honest_fp32(medium, case14):
    cfg, blob, R = medium
    inp, names, dev = case14
    rows, ref_s = fr.verify(dev, cfg, blob, [inp], "sim 14/42", report=QUIET, R=R)
    assert len({r[0] for r in rows}) == len(names)  # no step skipped
    worst = fr.worst_by_kind(rows)
    print("FRONTEXACT " + json.dumps(dict(case="cpu stand-in medium T=14 F=42", worst={k: round(v, 5) for k, v in worst.items()}, ref_s=round(ref_s, 2))))
    assert max(worst.values()) < 0.5, worst  # honest fp32 sits well inside the bound


@pytest.mark.parametrize("schedule", ["seam_stats", "plain", "predict"])
def test_verifier_passes_on_the_other_schedules(schedule, medium):
    cfg, blob, R = medium
    ids, dur, noise = fr.utterance(cfg, 5, 17, 11)
    inp = fr.Inputs(ids, dur, noise, dp_noise=fr.dp_noise(5, 3))
    names = dict(seam_stats=fr.default_steps(cfg, fold=False, ln="stats"), plain=fr.default_steps(cfg, fold=False, ln="plain"),
                 predict=fr.default_steps(cfg, predict=True))[schedule]
    rows, ref_s = fr.verify(sim(cfg, blob, names, [inp]), cfg, blob, [inp], schedule, report=QUIET, R=R)
    print("FRONTEXACT " + json.dumps(dict(case=f"cpu stand-in medium T=5 F=17 {schedule}", worst={k: round(v, 5) for k, v in fr.worst_by_kind(rows).items()},
                                          ref_s=round(ref_s, 2))))


def test_unknown_step_name_fails(medium, case14):
    cfg, blob, R = medium
    inp, names, dev = case14
    dev2 = fr.SimDevice.__new__(fr.SimDevice)
    dev2.names, dev2.snap, dev2.n = names[:3] + ["enc0.brand_new_kernel"], dev.snap, 1
    with pytest.raises(fr.UnknownStep):
        fr.verify(dev2, cfg, blob, [inp], report=QUIET, R=R)


# ---- planted defects: (step the defect sits in, function that alters what that step writes)
def _gate_tail_unmasked(cfg):
    """the last ⌊K/2⌋ columns of one gated conv computed from unmasked input: the buffer holds a longer utterance's values past the true length"""
    step = "flow2.wn1.in_gate"

    def defect(name, R, b, inp, out):
        if name == step:
            K = cfg.wn_kernel
            h = np.asarray(b["front.h"], np.float32)
            stale = kd.sym(5, (h.shape[0], K // 2), 1.0)
            full = R.in_gate(2, 1, np.concatenate([h, stale], 1))
            return {"front.acts": full[:, :h.shape[1]]}
    return step, defect


def _flip_dropped(cfg):
    step = "flow1.wn3.res_skip_post_sub_flip_pre0"

    def defect(name, R, b, inp, out):
        if name == step:  # the next pre reads x1new in the channel order of a latent that was not flipped
            o = dict(out)
            zout = [k for k in out if k != "front.h"][0]
            o["front.h"] = R.flow_pre(0, np.asarray(out[zout][0], np.float32)[::-1])
            return o
    return step, defect


def _ln_eps(cfg):
    step = "enc3.ln1_ffn1_relu"

    def defect(name, R, b, inp, out):
        if name == step:
            x1 = R.ln_enc(b["front.y"], 1, 3, eps=1e-3)
            return {"front.x1": x1, "front.ff": R.ffn1(x1, 3)}
    return step, defect


def _tail_bias(cfg):
    step = "flow3.wn3.res_skip_post_sub_flip_pre2"

    def defect(name, R, b, inp, out):
        if name == step:  # the post bias left out of the folded matrix's bias vector: x1 − m is off by it, and so is the pre behind it
            o = dict(out)
            zout = [k for k in out if k != "front.h"][0]
            arr, sl = out[zout]
            pb = R.W("flow.flows.6.post.bias")[:, None]
            pb = pb[::-1] if sl.start == 0 else pb  # (physical order of a flipped half)
            o[zout] = (arr + pb, sl)
            return o
    return step, defect


def _halo_wrong_side(cfg):
    step = "flow0.wn2.in_gate"

    def defect(name, R, b, inp, out):
        if name == step:  # the chunk that starts at column 16 takes its left halo from the columns to its right
            h = np.asarray(b["front.h"], np.float32).copy()
            K = cfg.wn_kernel
            acts = np.array(out["front.acts"], np.float32)
            h2 = h.copy()
            h2[:, 16 - K // 2:16] = h[:, 32:32 + K // 2]
            acts[:, 16:16 + K // 2] = R.in_gate(0, 2, h2)[:, 16:16 + K // 2]
            return {"front.acts": acts}
    return step, defect


def _spline_bin(cfg):
    step = "dp.flow5.spline_flip"

    def defect(name, R, b, inp, out):
        if name == step:
            z = np.asarray(b["dp.z"], np.float32)
            return {"dp.z": np.stack([R.spline_inverse(z[1], b["dp.hsp"], bin_shift=1), z[0]], 0)}
    return step, defect


@pytest.mark.parametrize("plant", [_gate_tail_unmasked, _flip_dropped, _ln_eps, _tail_bias, _halo_wrong_side])
def test_planted_defect_is_caught_at_its_step(plant, medium, case14):
    cfg, blob, R = medium
    inp, names, _ = case14
    step, defect = plant(cfg)
    assert step in names
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify(sim(cfg, blob, names, [inp], defect), cfg, blob, [inp], plant.__name__, report=QUIET, R=R)
    assert e.value.step == step, (e.value.step, str(e.value))
    print(f"  {plant.__name__}: caught at {e.value.step} → {e.value.tensor}, |Δ|/bound {e.value.result['ratio']:.1f}")


def test_planted_spline_bin_off_by_one(medium):
    cfg, blob, R = medium
    inp = fr.Inputs(fr.utterance(cfg, 14, 14, 3)[0], dp_noise=fr.dp_noise(14, 5))
    names = fr.default_steps(cfg, predict=True)
    step, defect = _spline_bin(cfg)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify(sim(cfg, blob, names, [inp], defect), cfg, blob, [inp], "spline", report=QUIET, R=R)
    assert e.value.step == step


def test_planted_attention_ignores_the_true_length(medium):
    """A ragged item: the device's rows are the bucket's, the columns past the item's true length hold another utterance's q ; k ; v.
    Attention that does not exclude those keys is caught at the attention step."""
    cfg, blob, R = medium
    ids, dur, noise = fr.utterance(cfg, 5, 15, 21)
    inp = fr.Inputs(ids, dur, noise)
    names = fr.default_steps(cfg)
    step = "enc1.rel_attention"

    def defect(name, R_, b, i_, out):
        if name == step:
            qkv = np.asarray(b["front.qkv"], np.float32)
            wide = np.concatenate([qkv, kd.sym(9, (qkv.shape[0], 11), 1.0)], 1)  # the bucket's 16 columns
            return {"front.att": R_.attention(wide, 1)[:, :qkv.shape[1]]}

    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify(sim(cfg, blob, names, [inp], defect), cfg, blob, [inp], "ragged attention", report=QUIET, R=R)
    assert e.value.step == step
    # and the masked form of the same wide evaluation is what the reference computes
    q = kd.sym(10, (3 * cfg.hidden, 16), 1.0)
    assert np.abs(R.attention(q, 1, length=5)[:, :5] - R.attention(q[:, :5], 1)).max() < 1e-12


def test_duration_seeds_stay_clear_of_integers(voices):
    """The GPU cases' predictor seeds: in float64, free running, at most 1 % of the ids lie within 1e-4 (relative) of an integer duration."""
    import test_gpu_front_exact as tg
    cfg, blob = voices["medium"]
    R = fr.FrontRef(cfg, blob)
    for label, utts, nw in tg.PREDICT_CASES:
        inputs = [fr.Inputs(ids, dp_noise=dpn, noise_w=nw) for ids, dpn in utts]
        names = fr.default_steps(cfg, predict=True)
        near = total = 0
        dev = fr.SimDevice(cfg, R, names, inputs)
        for b in range(len(inputs)):
            w = np.exp(np.asarray(dev.snap[(names[-1], b)]["dp.logw"], np.float64).reshape(-1))
            near += int((np.abs(w - np.rint(w)) <= fr.DUR_REL * w).sum())
            total += w.size
        assert near <= fr.DUR_SHARE * total, (label, near, total)
