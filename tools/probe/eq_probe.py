"""The equaliser on the device: what filtering the items through a biquad cascade (include/piper_hip.h "Equaliser") adds to a whole-item
collect, against the same call without an EQ and against the host route it replaces, on one voice, in one process.

Medium voice (22 050 Hz), the fixture utterance tiled by `factor` (F = 42 · factor frames, 3 frames per id, device noise), `batch` such
items in one ragged batch. Timed from the launch to the samples on the host (pageable buffers), the routes interleaved:

  f32, f32+eq1, f32+eq4        piper_hip_voice_collect without an EQ, with one section, with four (every launch is filtered again)
  s16, s16+eq1, s16+eq4        piper_hip_voice_collect_pcm16 at the voice's rate, the same three
  host4                        the host route the EQ replaces: the raw floats down (collect), piper_hip_eq_from_f32 per item with the
                               four sections, then int16 on the host (numpy: ×32767, rounded, clipped)

  --pool-rows 16,64,256: one step of a pool of that many rows (chunks of 64 frames, int16 at the voice's rate, every row a factor-8 item),
  without an EQ and with eq4 on every row: the median of the steps in which every row delivers, `--runs` pools each. With --lib-root the
  package and library of another tree are used (the parent commit's), for the pool legs without an EQ only.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per route, and the whole leg `--runs` times: the spread of a route is
max − min of its medians over the runs. Needs the GPU: there is no fallback.

Writes <out>/eq.json and the table of <out>/eq.md (everything from a "## Notes" heading on is kept); with --lib-root only <out>/<tag>.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EQ1 = [(2, 80.0, 0.707)]
EQ4 = [(2, 40.0, 0.707), (5, 3000.0, 1.0, 6.0), (7, 6000.0, 0.707, -3.0), (1, 7000.0, 0.707)]
ROUTES = ("f32", "f32+eq1", "f32+eq4", "s16", "s16+eq1", "s16+eq4", "host4")


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def leg(ph, kd, rt, factor, batch, warmup, reps):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(batch)]
    slots = {"": 0, "eq1": 2, "eq4": 4}
    for s in slots.values():
        rt.prepare_batch(s, utts, 0.667)
    rt.slot_eq(0, None)
    rt.slot_eq(2, EQ1)
    rt.slot_eq(4, EQ4)
    per, n = rt.prepared_samples(0)
    pcm, f32 = np.empty(n, np.int16), np.empty(n, np.float32)
    times = {k: [] for k in ROUTES}
    for k in range(warmup + reps):
        for name in ROUTES:
            slot = 0 if name == "host4" else slots[name.partition("+")[2]]
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_launch(v, slot))
            if name.startswith("s16"):
                ph._check(lib.piper_hip_voice_collect_pcm16(v, slot, None, pcm.ctypes.data_as(ph.c_i16p), n))
            else:
                ph._check(lib.piper_hip_voice_collect(v, slot, f32.ctypes.data_as(ph.c_f32p), n))
            if name == "host4":
                at = 0
                for p in per:
                    y = ph.eq_from_f32(f32[at:at + p], EQ4, rt.cfg.sample_rate)
                    pcm[at:at + p] = np.clip(np.rint(y * np.float32(32767.0)), -32768, 32767).astype(np.int16)
                    at += p
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
    res = {k: med(t) for k, t in times.items()}
    res["samples"] = int(n)
    for s in slots.values():
        rt.slot_eq(s, None)
    return res


def pool_leg(kd, rt, rows, eq=None):
    """ms of the steps of a pool of `rows` rows in which every row delivers a full chunk (the first step, which builds its plan, left out)"""
    ids = kd.FIXTURE_IDS * 8  # 336 frames: five full steps of 64 frames, then a short one
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(rows)]
    pool = rt.stream_pool(10, rows, chunkFrames=64, work_slot=11, **({"eq": eq} if eq else {}))
    times = []
    try:
        pool.join(utts, 0.667)
        for k in range(5):
            t0 = time.perf_counter()
            out = pool.step(pcm=True)
            t1 = time.perf_counter()
            assert len(out) == rows and all(c.size == 64 * rt.cfg.hop for c in out.values())
            if k:
                times.append((t1 - t0) * 1e3)
    finally:
        pool.close()
    return med(times)


def summarise(runs):
    out = {"runs": runs}
    for k in ROUTES:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="1x1,1x8,8x1,8x8,64x1,64x8", help="factor x batch, comma-separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pool-rows", default="16,64,256")
    ap.add_argument("--lib-root", default=None, help="another tree whose package and library to use (pool legs only)")
    ap.add_argument("--tag", default="eq")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    root = args.lib_root or ROOT
    sys.path.insert(0, os.path.join(root, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import katdata as kd
    import piper_hip as ph
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "eq", "voice": "medium", "eq1": EQ1, "eq4": EQ4, "warmup": args.warmup, "reps": args.reps, "runs": args.runs,
           "legs": [], "pool": []}
    if not args.lib_root:
        for spec in [x for x in args.legs.split(",") if x]:
            f, b = (int(x) for x in spec.split("x"))
            r = summarise([leg(ph, kd, rt, f, b, args.warmup, args.reps) for _ in range(args.runs)])
            r["factor"], r["batch"] = f, b
            out["legs"].append(r)
            print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    for rows in [int(x) for x in args.pool_rows.split(",") if x]:
        pool_leg(kd, rt, rows)  # (untimed: the pool's plans exist before it is timed)
        t = [pool_leg(kd, rt, rows) for _ in range(args.runs)]
        q = {"rows": rows, "ms_runs": t, "ms": med(t), "min": min(t), "max": max(t)}
        if not args.lib_root:
            te = [pool_leg(kd, rt, rows, EQ4) for _ in range(args.runs)]
            q.update({"eq4_ms_runs": te, "eq4_ms": med(te), "eq4_min": min(te), "eq4_max": max(te)})
        out["pool"].append(q)
        print(json.dumps(q), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + ".json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if args.lib_root:
        return
    lines = ["# The equaliser on the device", "",
             f"Medium voice (22 050 Hz), one launch → samples on the host, median ms over {args.reps} interleaved repetitions after "
             f"{args.warmup} untimed ones; ± = max − min of the medians of {args.runs} runs of the leg (`tools/probe/eq_probe.py`; raw "
             f"figures in `eq.json`). eq1 = {EQ1}, eq4 = {EQ4} (type, f0, q, gain_db). host4: floats down, `piper_hip_eq_from_f32` with "
             "eq4, int16 on the host.", "",
             "| factor | batch | samples | collect | +eq1 | +eq4 | collect_pcm16 | +eq1 | +eq4 | host4 |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    for r in out["legs"]:
        lines.append(f"| {r['factor']} | {r['batch']} | {r['runs'][0]['samples']} | " + " | ".join(cell(r, k) for k in ROUTES) + " |")
    if out["pool"]:
        lines += ["", "One step of a pool, chunks of 64 frames, int16 on the host, median ms of four full steps, min … max over "
                  f"{args.runs} pools, without an EQ and with eq4 on every row:", "",
                  "| rows | pool step | min … max | with eq4 | min … max |", "|---|---|---|---|---|"]
        lines += [f"| {q['rows']} | {q['ms']} | {q['min']} … {q['max']} | {q['eq4_ms']} | {q['eq4_min']} … {q['eq4_max']} |" for q in out["pool"]]
    md = os.path.join(args.out, "eq.md")
    notes = ""
    if os.path.exists(md):
        old = open(md).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    with open(md, "w") as fh:
        fh.write("\n".join(lines) + "\n" + notes)


if __name__ == "__main__":
    main()
