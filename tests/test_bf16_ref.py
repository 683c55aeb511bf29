"""CPU: the rounding-exact bf16 reference (tests/bf16_ref.py) validated on its own, before it judges a kernel.

* with rounding switched off it is the plain fp32 generator (torch_ref.Ref.generator) to 1e-5;
* a generator that accumulates in fp32 (torch's order, and a second order with the channels reversed that took no part in measuring κ) is
  accepted by the fp64 reference at every unit, teacher-forced, within `tol` — with every tensor tapped and with the last ResBlock's closing
  step folded into the mean (the schedules that never store it), at both voices' channel counts;
* the median per-element tol of every unit stays ≤ 2 · OP_TOL · max(1, ‖ref‖∞) (asserted inside verify_item);
* sensitivity: a defect planted in the REFERENCE (one column at a tile edge taken from its neighbour; the MRF mean's third operand taken from
  r1) is caught by the exact check, while the waveform of a generator with the same defect still clears the old 35 dB bar where noted."""
import numpy as np
import pytest
import torch

import bf16_ref as br
import katdata as kd
import torch_ref

F = 37  # frames: 37 · 256 = 9 472 samples; every stage longer than one 128-column tile except conv_pre / stage 0


def snr_db(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return 10.0 * np.log10((ref ** 2).sum() / max(((x - ref) ** 2).sum(), 1e-300))


@pytest.fixture(scope="module")
def chains(voices):
    out = {}
    for q in ("medium", "high"):
        cfg, blob = voices[q]
        z = kd.sym(kd.case_seed("cfg", 40), (cfg.inter, F), 1.0)
        out[q] = {acc: br.Bf16Ref(cfg, blob, acc=acc).generator(z) for acc in ("f64", "f32", "f32r")}
    return out


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_rounding_off_is_the_fp32_generator(quality, voices):
    cfg, blob = voices[quality]
    z = kd.sym(kd.case_seed("cfg", 41), (cfg.inter, 20), 1.0)
    got = br.Bf16Ref(cfg, blob, rounding=False).generator(z)["audio"]
    with torch.no_grad():
        ref = torch_ref.Ref(cfg, blob).generator(torch_ref.t(z)[None]).numpy().reshape(-1)
    assert np.max(np.abs(got - ref)) <= 1e-5, np.max(np.abs(got - ref))
    with_rounding = br.Bf16Ref(cfg, blob).generator(z)["audio"]
    assert 30.0 < snr_db(with_rounding, ref) < 70.0  # the roundings are really there (≈ 45 dB)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("acc", ["f32", "f32r"])
@pytest.mark.parametrize("quality", ["medium", "high"])
def test_fp32_accumulation_is_accepted_by_the_fp64_reference(quality, acc, fold, voices, chains):
    cfg, blob = voices[quality]
    T = dict(chains[quality][acc])
    if fold:
        for u in range(cfg.n_ups):
            T.pop(f"dec.s{u}.rb{cfg.n_rb - 1}.c{cfg.rb_n_dil - 1}")
    rows = br.verify_item(br.Bf16Ref(cfg, blob), T, T["audio"], f"{quality}/{acc}/fold={fold}")
    assert len(rows) == 2 + cfg.n_ups * (2 + cfg.n_rb * cfg.rb_n_dil) - 1 - (cfg.n_ups if fold else 0) + 1
    if quality == "high":  # the expected order of one flip: 2⁻⁸ · |v| · |w| ≈ 2e-5 — the allowance is a few of them, not hundreds
        allow = [r["bound"] - r["base"] for n, r in rows if ".rb" in n]
        assert 0 < max(allow) < 1e-3, max(allow)


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_free_running_orders_drift_apart(quality, chains):
    """Why the check is teacher-forced: the same reference in two accumulation orders, run end to end, agrees far worse than one unit does."""
    a, b = chains[quality]["f64"]["audio"], chains[quality]["f32r"]["audio"]
    print(f"{quality}: free-running fp64 vs fp32 accumulation: SNR {snr_db(b, a):.1f} dB, max|Δ| {np.abs(a - b).max():.2e}")
    assert snr_db(b, a) > 45.0


def test_planted_defects_fail_the_exact_check_and_pass_the_snr_bar(voices, chains):
    cfg, blob = voices["medium"]
    G = chains["medium"]["f32r"]
    R = br.Bf16Ref(cfg, blob)
    br.verify_item(R, G, G["audio"], "clean", report=lambda s: None)

    def wrong_column(unit):  # column 128 (first of the second tile) takes its neighbour's taps
        ref = unit.ref.copy()
        ref[:, 128] = unit.ref[:, 127]
        return br.Unit(ref, unit.allow, unit.eps)
    with pytest.raises(AssertionError, match="dec.s1.rb0.c0"):
        br.verify_item(R, G, G["audio"], "defect A", report=lambda s: None, hooks={"dec.s1.rb0.c0": wrong_column})

    def third_from_r1(unit):
        u = cfg.n_ups - 1
        r0, r1 = G[f"dec.s{u}.rb0.c{cfg.rb_n_dil - 1}"], G[f"dec.s{u}.rb1.c{cfg.rb_n_dil - 1}"]
        return br.Unit(br.Bf16Ref.mean32(r0, r1, r1))
    with pytest.raises(AssertionError, match="dec.mean"):
        br.verify_item(R, G, G["audio"], "defect B", report=lambda s: None, hooks={"dec.mean": third_from_r1})

    # the same defects in a generator's waveform against the clean one: what a whole-voice SNR sees of them
    class ColumnDefect(br.Bf16Ref):
        def rb_step(self, u, j, d, x):
            unit = super().rb_step(u, j, d, x)
            return wrong_column(unit) if (u, j, d) == (1, 0, 0) else unit
    z = G["z"]
    clean = chains["medium"]["f64"]["audio"]
    a = ColumnDefect(cfg, blob).generator(z)["audio"]
    print(f"defect A (one column): waveform SNR vs clean {snr_db(a, clean):.1f} dB, max|Δ| {np.abs(a - clean).max():.2e}")
    assert snr_db(a, clean) >= 35.0  # invisible to the old assertion

    class MeanDefect(br.Bf16Ref):
        stage = 0

        def rb_step(self, u, j, d, x):
            MeanDefect.stage = u
            return super().rb_step(u, j, d, x)

        @staticmethod
        def mean32(r0, r1, r2):
            return br.Bf16Ref.mean32(r0, r1, r1 if MeanDefect.stage == cfg.n_ups - 1 else r2)
    b = MeanDefect(cfg, blob).generator(z)["audio"]
    print(f"defect B (mean's third operand = r1, last stage): waveform SNR vs clean {snr_db(b, clean):.1f} dB")


def test_a_mean_that_cancels_to_zero_keeps_its_error_bound(voices):
    """Regression (profiles/conv_routes.md, Finding): three ResBlock outputs that cancel to exactly 0.0 in the reference's fp32 order — the
    device, summing the last conv in another order, lands a few 1e-9 beside it. A zero has no binade, so round_amb gave it no allowance and
    the image had to be 0 bit for bit. Its true value is known to ±err like every other element's: a value within err passes, nothing else."""
    cfg, blob = voices["high"]
    R = br.Bf16Ref(cfg, blob)
    h32 = np.array([[0.0, 0.0, 0.5, 0.0]], np.float32)
    err = np.array([[1e-5, 0.0, 1e-5, 1e-5]])
    hb, cost = R.round_amb(h32, err)
    assert np.array_equal(hb, h32)
    assert 1e-5 <= cost[0, 0] <= 1.01e-5 + 2.0 ** -24 and cost[0, 1] == 0 and cost[0, 2] == 0 and cost[0, 3] == cost[0, 0]
    unit = br.Unit(hb, cost, base=0.0)
    assert unit.compare(np.array([[-3.987e-9, 0.0, 0.5, 9e-6]], np.float32))["ok"]       # what the device gave at the element found
    assert not unit.compare(np.array([[0.0, 1e-9, 0.5, 0.0]], np.float32))["ok"]          # an exact zero (no error) stays exact
    assert not unit.compare(np.array([[3.2e-5, 0.0, 0.5, 0.0]], np.float32))["ok"]        # and the allowance is err, not a bf16 ulp of the tensor
    assert not unit.compare(np.array([[0.0, 0.0, 0.50390625, 0.0]], np.float32))["ok"]    # an unambiguous element one bf16 ulp off
