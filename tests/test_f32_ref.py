"""CPU: the float64 reference of the fp32 generator and its chained check (tests/f32_ref.py) validated on their own, before they judge a kernel.

* free running, the reference gives the C oracle's `generator` on the same z within OP_TOL (it is tied to torch_ref by test_bf16_ref.py);
* two honest fp32 implementations (torch's accumulation order, and the channels reversed) pass the teacher-forced check under the plain
  OP_TOL rule with the taps of every schedule; the largest |Δ| / bound seen is printed: it shows how much room OP_TOL leaves
  (measured: ≤ 0.0094 on the contractions of both voices — a kernel may be a hundred times worse than torch's fp32 before the rule
  trips — and 0.075 on the waveform, where the fp32 rounding of a saturated sample alone is an eighth of the floor);
* planted defects fail the check at the unit where they are planted: one element off by 2 × bound at a tile edge, a consumer that read a
  producer's non-zero tail past the true length, the mean's 1/3 replaced by 1/3 + 1e-3, an error in front of tanh in saturation — the
  last one invisible to a plain OP_TOL comparison of the waveform;
* the inputs of the GPU cases meet the saturation condition of the waveform link (floor-dominated samples ≤ 10 %)."""
import numpy as np
import pytest

import f32_ref as fr
import katdata as kd
import oracle as orc
from conftest import OP_TOL, assert_close

F = 37  # frames: every stage but conv_pre / stage 0 spans more than one 256-column tile, none ends on one before the last
QUIET = dict(report=lambda s: None)


def voice_z(cfg, blob):
    """z of a whole-voice utterance as the GPU cases make it (encoder and flow of the C oracle): it drives tanh into saturation, a plain
    random z (max |v| ≈ 0.9) does not."""
    ids, dur, noise = fr.utterance(cfg, F, 61)
    return orc.synthesize(cfg, blob, ids, dur, noise, fr.NOISE_SCALE, taps=True)[1]["z"]


@pytest.fixture(scope="module")
def chains(voices):
    out = {}
    for q in ("medium", "high"):
        cfg, blob = voices[q]
        z = voice_z(cfg, blob)
        out[q] = {acc: fr.F32Ref(cfg, blob, acc=acc).generator(z) for acc in ("f64", "f32", "f32r")}
    return out


@pytest.mark.parametrize("quality,frames", [("medium", 42), ("medium", 131), ("high", 42), ("high", 37)])
def test_free_running_reference_matches_the_c_oracle(quality, frames, voices):
    cfg, blob = voices[quality]
    z = kd.sym(kd.case_seed("cfg", 62) + frames, (cfg.inter, frames), 1.0)
    got = fr.F32Ref(cfg, blob).generator(z)["audio"]
    ref = orc.generator(cfg, blob, z)
    print(f"{quality} F={frames}: float64 reference vs C oracle max|Δ| {np.max(np.abs(got - ref)):.3e}")
    assert_close(got, ref, OP_TOL, f"{quality} F={frames}: float64 reference vs C oracle")


@pytest.mark.parametrize("schedule", ["all", "merged", "pair", "per_conv"])
@pytest.mark.parametrize("acc", ["f32", "f32r"])
@pytest.mark.parametrize("quality", ["medium", "high"])
def test_honest_fp32_implementations_pass_the_plain_rule(quality, acc, schedule, voices, chains):
    cfg, blob = voices[quality]
    G = chains[quality][acc]
    T = fr.schedule_view(cfg, G, schedule)
    rows = fr.verify_item(fr.F32Ref(cfg, blob), T, G["audio"], f"{quality}/{acc}/{schedule}")
    n_steps = sum(1 for n in T if ".rb" in n)
    assert len(rows) == 2 + cfg.n_ups + n_steps + (cfg.n_ups if schedule == "per_conv" else 0)
    kinds = fr.worst_by_kind(rows)
    print(f"{quality}/{acc}/{schedule}: worst |Δ|/bound per kind {({k: round(v, 4) for k, v in kinds.items()})}")
    assert ("rb_composed" in kinds) == (schedule == "pair" or (schedule == "merged" and cfg.rb_n_dil > 2))
    assert max(v for k, v in kinds.items() if k != "waveform") < 0.1, "torch's own fp32 order uses a hundredth of OP_TOL: a tenth means the reference is off"
    assert kinds["waveform"] < 0.5  # half an ulp below 1.0 is 2⁻²⁵ = 0.125 of the floor, plus numpy's tanh


def planted(cfg, G, schedule="pair"):
    return {k: np.array(v, np.float32) for k, v in fr.schedule_view(cfg, G, schedule).items()}


@pytest.mark.parametrize("col", [255, 256])
@pytest.mark.parametrize("quality,name", [("medium", "dec.s1.rb1.c1"), ("high", "dec.s2.rb2.c2"), ("medium", "dec.s2.up")])
def test_one_element_off_at_a_tile_edge_fails_at_its_unit(quality, name, col, voices, chains):
    cfg, blob = voices[quality]
    G = chains[quality]["f32"]
    T = planted(cfg, G)
    bound = fr.base_tol(chains[quality]["f64"][name])
    T[name][3, col] += 2.0 * bound
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(fr.F32Ref(cfg, blob), T, G["audio"], **QUIET)
    assert e.value.unit == name and e.value.columns.tolist() == [col] and e.value.result["n_over"] == 1
    assert 1.9 < e.value.result["ratio"] < 2.1


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_a_consumer_that_read_a_stale_tail_fails_in_its_last_reach_columns(quality, voices, chains):
    """The fp32 streams are not zeroed past the true length: a kernel that ignores len_ptr convolves the previous utterance's tail in.
    Emulated by running the consumer on its producer's tensor extended by 64 non-zero columns and cutting the result to the true length."""
    cfg, blob = voices[quality]
    G = chains[quality]["f32"]
    R32, R = fr.F32Ref(cfg, blob, acc="f32"), fr.F32Ref(cfg, blob)
    stale = lambda x: np.concatenate([x, 0.5 * np.ones((x.shape[0], 64), np.float32)], axis=1)
    # (a) a ResBlock launch: the pair plan's composed steps of ResBlock 1 of stage 1, fed `up` with a tail
    u, j = 1, 1
    d1 = cfg.rb_n_dil - 1 if cfg.resblock_type == 2 else 1
    name, L = f"dec.s{u}.rb{j}.c{d1}", G[f"dec.s{u}.up"].shape[1]
    T = planted(cfg, G)
    T[name] = R32._chain(u, j, 0, d1, stale(G[f"dec.s{u}.up"]))[:, :L].astype(np.float32)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(R, T, G["audio"], **QUIET)
    reach = sum(R.reach(j, d) for d in range(d1 + 1))
    cols = e.value.columns
    assert e.value.unit == name and cols.max() == L - 1 and cols.min() >= L - reach, (e.value.unit, cols.min(), L - reach)
    # (b) the ConvTranspose of stage 1 with the average-of-three prologue, fed stage 0's ResBlock outputs with tails
    last = cfg.rb_n_dil - 1
    rs = [stale(G[f"dec.s0.rb{jj}.c{last}"]) for jj in range(3)]
    Lo = G["dec.s1.up"].shape[1]
    T = planted(cfg, G)
    T["dec.s1.up"] = R32.up(1, rs).ref[:, :Lo].astype(np.float32)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(R, T, G["audio"], **QUIET)
    s, k = cfg.up_rates[1], cfg.up_kernels[1]
    assert e.value.unit == "dec.s1.up" and e.value.columns.max() == Lo - 1 and e.value.columns.min() >= Lo - (k // s) * s


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_a_wrong_third_in_the_mean_fails_at_its_consumer(quality, voices):
    """(r0 + r1 + r2) · (1/3 + 1e-3): in the merged schedule the mean lives in the next ConvTranspose's prologue, in the per-conv schedule in
    the stored lrelu(mean). Against the waveform at WAVE_TOL the same generator still passes on this input (printed)."""
    cfg, blob = voices[quality]
    z = voice_z(cfg, blob)
    G = fr.F32Ref(cfg, blob, acc="f32").generator(z, third=1.0 / 3.0 + 1e-3)
    R = fr.F32Ref(cfg, blob)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(R, planted(cfg, G, "pair"), G["audio"], **QUIET)
    assert e.value.unit == "dec.s1.up"
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(R, planted(cfg, G, "per_conv"), G["audio"], **QUIET)
    assert e.value.unit == "dec.s0.mean_lrelu"
    clean = R.generator(z)["audio"]
    print(f"{quality}: waveform of the defective generator vs the clean one: max|Δ| {np.max(np.abs(G['audio'] - clean)):.2e}")


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_an_error_in_front_of_tanh_in_saturation_is_seen_by_the_slope_weighted_bound_only(quality, voices, chains):
    cfg, blob = voices[quality]
    G, G64 = chains[quality]["f32"], chains[quality]["f64"]
    v = G64["v"]
    cand = np.nonzero((np.abs(v) > 3.0) & (np.abs(v) < 4.0))[0]
    assert cand.size, f"the input has no sample with 3 < |v| < 4 (max |v| {np.abs(v).max():.2f})"
    i = int(cand[0])
    e_v = 10.0 * fr.base_tol(v)
    audio = G["audio"].copy()
    audio[i] = np.float32(np.tanh(v[i] + e_v))
    # the plain post-tanh comparison at OP_TOL (what assert_close does) does not see it …
    assert_close(audio, np.tanh(v), OP_TOL, "plain OP_TOL on the waveform")
    # … the slope-weighted bound does, at the sample where it was planted
    R = fr.F32Ref(cfg, blob)
    fr.verify_item(R, planted(cfg, G), G["audio"], **QUIET)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify_item(R, planted(cfg, G), audio, **QUIET)
    assert e.value.unit == "audio" and e.value.columns.tolist() == [i]
    print(f"{quality}: |v| {abs(v[i]):.2f}, slope {1 - np.tanh(v[i]) ** 2:.2e}: error {e_v:.1e} in front of tanh → {abs(audio[i] - np.tanh(v[i])):.2e} "
          f"behind it (OP_TOL bound 1e-4), |Δ|/bound {e.value.result['ratio']:.1f}")


@pytest.mark.parametrize("quality,frames", [("medium", 42), ("medium", 131), ("high", 42), ("high", 35)])
def test_gpu_case_inputs_meet_the_saturation_condition(quality, frames, voices):
    """The whole voice (encoder, flow at noise_scale NOISE_SCALE) in front of the generator, as the GPU cases run it: the share of samples
    where the floor exceeds the slope term, from the reference alone. verify_item asserts the same for every waveform it checks on the GPU."""
    cfg, blob = voices[quality]
    ids, dur, noise = fr.utterance(cfg, frames, frames)  # the seed of the single-utterance GPU cases
    _, taps = orc.synthesize(cfg, blob, ids, dur, noise, fr.NOISE_SCALE, taps=True)
    w = fr.Waveform(fr.F32Ref(cfg, blob).generator(taps["z"])["v"])
    print(f"{quality} F={frames}: max |v| {np.abs(w.v).max():.2f}, floor-dominated samples {100 * w.floor_share:.2f} %, |tanh| > 0.999 on "
          f"{100 * np.mean(np.abs(w.ref) > 0.999):.1f} %")
    assert w.floor_share <= fr.FLOOR_SHARE_MAX
