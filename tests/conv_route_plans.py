"""The production workloads and the witness ladder whose kernel variants tests/conv_routes_table.py lists — TEST INFRASTRUCTURE, run on the
GPU by tools/probe/conv_routes.py (which writes the table) and tests/test_gpu_conv_routes_table.py (which holds the library to it).

A workload arms nothing itself: the caller hands a runtime made on an armed backend (HipBackend.arm_routes before the first prepare). It
prepares and launches once and returns {variant: [step names]} over every plan it touched — the slot's plan, the predictor plan and the
generator window plans of a stream — with the shapes dropped (conv_ref.variant_of). A step with no record is an error: the plan was
enqueued while the switch was off, or a launcher does not report."""
import conv_ref as cr
import f32_ref as fr

VOICES = (("medium", "f32"), ("high", "f32"), ("x_low", "f32"), ("high", "bf16"))
WORKLOADS = ("single_f1", "single_f8", "single_f64", "batch_4x336", "batch_8x336", "batch_20x84", "ragged_84_5_61_1", "bounded", "predictor",
             "stream_chunk20", "pool_16", "pool_64")
LADDER_F = (1, 2, 35, 42, 61, 84, 112, 127, 128, 129, 131, 200, 336, 400)
LADDER_N = (1, 3, 4, 20)
SEEN_CUS = None  # the CU count of the records merged so far


def voice_key(quality, prec):
    return f"{quality}/{prec}"


def utterance(cfg, F, seed):
    """F frames over ⌈F / 3⌉ ids: 14 / 112 / 896 ids at factor 1 / 8 / 64."""
    return fr.utterance(cfg, F, seed)


def merge(into, routes):
    """routes [(step, [records])] → into {variant: sorted step names}. → number of steps that left records."""
    global SEEN_CUS
    n = 0
    for step, recs in routes:
        n += bool(recs)
        for r in recs:
            SEEN_CUS = cr.parse_record(r)[1]["CUs"]
            steps = into.setdefault(cr.variant_of(r), [])
            if step not in steps:
                steps.append(step)
    return n


def _slot_routes(rt, slot, out, what, predict=False, window=False):
    routes = rt.routes(slot, predict=predict, window=window)
    assert merge(out, routes) > 0, f"{what}: no step of the plan left a route record (was the backend armed before the prepare?)"
    return routes


def run_batch(rt, slot, utts, out, what):
    if len(utts) == 1:
        rt.prepare(slot, *utts[0], fr.NOISE_SCALE)
    else:
        rt.prepare_batch(slot, utts, fr.NOISE_SCALE)
    rt.launch(slot)
    rt.collect(slot)
    return _slot_routes(rt, slot, out, what)


def run_workload(rt, name, slot=0):
    """{variant: [step names]} of workload `name` on runtime `rt`."""
    cfg = rt.cfg
    out = {}
    if name.startswith("single_f"):
        F = {"1": 42, "8": 336, "64": 2688}[name[8:]]
        run_batch(rt, slot, [utterance(cfg, F, 11 + F)], out, name)
    elif name.startswith("batch_"):
        n, F = (int(t) for t in name[6:].split("x"))
        run_batch(rt, slot, [utterance(cfg, F, 100 + b) for b in range(n)], out, name)
    elif name == "ragged_84_5_61_1":
        run_batch(rt, slot, [utterance(cfg, F, 300 + F) for F in (84, 5, 61, 1)], out, name)
    elif name in ("bounded", "predictor"):
        ids = utterance(cfg, 336, 21)[0]
        rt.prepare(slot, ids, None, None, fr.NOISE_SCALE, noise_mode="device", max_frames=1024)
        rt.launch(slot)
        rt.collect(slot)
        _slot_routes(rt, slot, out, name, predict=(name == "predictor"))
    elif name == "stream_chunk20":
        ids, dur, noise = utterance(cfg, 336, 31)
        for _ in rt.synthesize_stream(ids, dur, noise, fr.NOISE_SCALE, chunkFrames=20, slot=slot):
            _slot_routes(rt, slot, out, name, window=True)
        _slot_routes(rt, slot, out, name)
    elif name.startswith("pool_"):
        rows = int(name[5:])
        pool = rt.stream_pool(slot, rows, chunkFrames=20)
        try:
            pool.join([utterance(cfg, 84, 400 + b) for b in range(rows)], fr.NOISE_SCALE)
            while pool.step():
                _slot_routes(rt, slot, out, name, window=True)
        finally:
            pool.close()
    else:
        raise ValueError(name)
    return {v: sorted(s) for v, s in out.items()}


def run_ladder_plan(rt, F, N, slot=0):
    """{variant: [step names]} of the ladder plan N × F frames."""
    out = {}
    run_batch(rt, slot, [utterance(rt.cfg, F, 700 + 31 * b + F) for b in range(N)], out, f"ladder {N}x{F}")
    return {v: sorted(s) for v, s in out.items()}
