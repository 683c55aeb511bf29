"""GPU: the production ledger of conv kernel variants, and one float64-checked witness plan per variant.

test_production_ledger re-enumerates the workloads of tests/conv_route_plans.py on an armed backend and holds the set of variants each voice
launches — shapes dropped — to tests/conv_routes_table.py, on 256 CUs (another CU count: it prints what differs and asserts nothing about
it). A dispatcher change, a new threshold or a new default that moves a production shape onto another variant fails here until
tools/probe/conv_routes.py has rewritten the table — and with it the witnesses below.

test_witness_plan runs every witness plan of the table once: the routes must hold every variant the plan is witness for; then the existing
per-unit checks run unchanged under their own bounds — front_ref.verify on every encoder / flow / predictor step, f32_ref.verify_slot or
bf16_ref.verify_slot on the generator (OP_TOL · max(1, ‖ref‖∞), the bf16 rounding-exact rule) — and the units that carry the witnessed
variants, joined to the routes by step name, must be among the rows that passed. Batched plans check their first and last item.
Most plans take under a second; the cheapest plans that reach some variants are long ones (high bf16 20 × 400: about 30 s, 3 × 400 and 4 × 400
about 20 s, medium F = 2688 13 s — profiles/conv_routes.md)."""
import json

import numpy as np
import pytest

import bf16_ref as br
import conv_route_plans as rp
import conv_routes_table as tb
import f32_ref as fr
import front_ref as ff
import piper_hip as ph
from test_gpu_front_exact import prepare_predicted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def armed():
    b = ph.HipBackend(0)
    b.arm_routes(True)
    yield b
    b.arm_routes(False)
    b.close()


_voices = {}


def voice(quality):
    if quality not in _voices:
        cfg = ph.voice_config(quality)
        _voices[quality] = (cfg, ph.synthetic_blob(cfg, 1234))
    return _voices[quality]


def runtime(backend, quality, prec):
    rt = ph.HipRuntime(backend, *voice(quality))
    if prec == "bf16":
        rt.set_precision("bf16")
    return rt


@pytest.mark.parametrize("quality,prec", rp.VOICES, ids=[rp.voice_key(*v) for v in rp.VOICES])
def test_production_ledger(quality, prec, armed):
    key = rp.voice_key(quality, prec)
    uses = {}
    for name in rp.WORKLOADS:
        rt = runtime(armed, quality, prec)  # a fresh runtime: every plan is enqueued with the switch on
        try:
            for var in rp.run_workload(rt, name):
                uses.setdefault(var, []).append(name)
        finally:
            rt.close()
    want = {v: sorted(ws) for v, ws in tb.TABLE[key].items()}
    got = {v: sorted(ws) for v, ws in uses.items()}
    new, gone = sorted(set(got) - set(want)), sorted(set(want) - set(got))
    moved = {v: (want[v], got[v]) for v in set(got) & set(want) if got[v] != want[v]}
    print("CONVLEDGER " + json.dumps(dict(voice=key, cus=rp.SEEN_CUS, variants=len(got), new=new, gone=gone, moved=sorted(moved))))
    if rp.SEEN_CUS != tb.NUM_CUS:
        return  # the table is the 256-CU part's: reported above, not asserted
    assert not new and not gone and not moved, (f"{key}: production moved — variants with no entry (and no float64 witness) {new}; entries no workload "
                                                f"reaches any more {gone}; other workloads {moved}. Rewrite the table with tools/probe/conv_routes.py")


def witness_plans():
    """[(voice key, witness, [variants])] — one entry per distinct plan."""
    plans = {}
    for key, ws in tb.WITNESS.items():
        for var, w in ws.items():
            plans.setdefault((key, tuple(w)), []).append(var)
    return [(k, w, sorted(v)) for (k, w), v in sorted(plans.items(), key=lambda kv: (kv[0][0], str(kv[0][1])))]


PLANS = witness_plans()


def plan_id(p):
    key, w, _ = p
    return f"{key}-" + (f"{w[2]}x{w[1]}" if w[0] == "ladder" else w[1])


def units_of_step(step, front_rows, gen_rows):
    """The verified rows that answer for schedule step `step`: a front step by its own name; a generator step by its stage and kind."""
    if not step.startswith("dec."):
        return [r[4] for r in front_rows if r[0] == step]
    if "conv_post" in step:
        return [r for n, r in gen_rows if n == "audio"]
    if step.startswith("dec.conv_pre") or step == "dec.pre":
        return [r for n, r in gen_rows if n in ("dec_pre", "dec.conv_pre")]
    stage = ".".join(step.split(".")[:2]) + "."
    if step.endswith("convT"):  # "dec.s0.lrelu_convT", "dec.s1.mrfmean_lrelu_convT": the stage's upsampler
        return [r for n, r in gen_rows if n == stage + "up"]
    return [r for n, r in gen_rows if n.startswith(stage + "rb") or n == stage + "mean_lrelu"]


@pytest.mark.parametrize("plan", PLANS, ids=[plan_id(p) for p in PLANS])
def test_witness_plan(plan, armed):
    key, w, variants = plan
    quality, prec = key.split("/")
    cfg, blob = voice(quality)
    rt = runtime(armed, quality, prec)
    label = plan_id(plan)
    try:
        if w == ("production", "predictor"):  # the cached encoder + predictor plan of 112 ids, its noise injected so that the reference knows it
            ids = rp.utterance(cfg, 336, 21)[0]
            prepare_predicted(rt, 0, [(ids, ff.dp_noise(len(ids), 21))], 0.8)
            rt.launch(0)
            rt.collect(0)
            routes = rt.routes(0, predict=True)
            dev = ff.GpuDevice(rt, 0, [len(ids)], [0], predict=True)
            front_rows, _ = ff.verify(dev, cfg, blob, [ff.Inputs(ids, dp_noise=ff.dp_noise(len(ids), 21), noise_w=0.8)], label, report=lambda s: None)
            gen_rows = []
        else:
            if w[0] == "ladder":
                utts = [rp.utterance(cfg, w[1], 700 + 31 * b + w[1]) for b in range(w[2])]
            else:
                assert w[1].startswith("single_f"), f"no recipe for the production witness {w}"
                F = {"1": 42, "8": 336, "64": 2688}[w[1][8:]]
                utts = [rp.utterance(cfg, F, 11 + F)]
            if len(utts) == 1:
                rt.prepare(0, *utts[0], fr.NOISE_SCALE)
            else:
                rt.prepare_batch(0, utts, fr.NOISE_SCALE)
            rt.launch(0)
            audio = rt.collect(0).copy()
            routes = rt.routes(0)
            items = sorted({0, len(utts) - 1})
            lensT, lensF = [len(u[0]) for u in utts], [int(np.sum(u[1])) for u in utts]
            dev = ff.GpuDevice(rt, 0, lensT, lensF)
            front_rows, _ = ff.verify(dev, cfg, blob, [ff.Inputs(*u) for u in utts], label, items=items, report=lambda s: None)
            if prec == "bf16":
                gen_rows = br.verify_slot(rt, blob, 0, lensF, audio, label, items, report=lambda s: None)
            else:
                gen_rows, _, _ = fr.verify_slot(rt, blob, 0, lensF, audio, label, items, report=lambda s: None)
        by_variant = {}
        assert rp.merge(by_variant, routes) > 0, f"{label}: the plan reports no routes (armed before the prepare?)"
        if rp.SEEN_CUS != tb.NUM_CUS and not set(variants) <= set(by_variant):
            pytest.skip(f"{label}: {rp.SEEN_CUS} CUs route this plan differently; the witnesses are the {tb.NUM_CUS}-CU part's")
        worst = {}
        for var in variants:
            assert var in by_variant, f"{label} no longer runs '{var}' (it runs {sorted(by_variant)}): rewrite the table and its witnesses"
            for step in by_variant[var]:
                units = units_of_step(step, front_rows, gen_rows)
                assert units, f"{label}: no verified unit answers for step {step}, which carries '{var}'"
                assert all(r["ok"] for r in units), f"{label}: a unit of step {step} ('{var}') is beyond its bound"
                # (|Δ| over the bound where the unit has one per tensor; a bf16 unit's per-element tolerance: over its largest)
                worst[var] = max([worst.get(var, 0.0)] + [r["ratio"] if "ratio" in r else r["err"] / r["bound"] if r["bound"] else 0.0 for r in units])
        print("CONVWITNESS " + json.dumps(dict(plan=label, worst={v: round(x, 4) for v, x in worst.items()})))
    finally:
        rt.close()
