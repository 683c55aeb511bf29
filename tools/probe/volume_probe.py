"""Per-phoneme volume on the device: what shaping the items under a gain envelope (include/piper_hip.h "Per-phoneme volume") adds to a
whole-item collect, on one voice, in one process.

Medium voice (22 050 Hz), the fixture utterance tiled by `factor` (F = 42 · factor frames, 3 frames per id, device noise), `batch` such
items in one ragged batch, 16-bit PCM at the voice's own rate; the gains cycle through (1, 0.25, 1, 2, 0, 1.5) per id. Timed from the launch
to the int16 samples on the host (pageable buffers), the two routes interleaved:

  plain    piper_hip_voice_collect_pcm16 on a slot whose staging carried no volume
  vol      the same call on a slot whose staging carried one (every launch is shaped again: one launch of volume.hip per collect)

  --pool-rows N (256): one step of an N-row streaming pool (chunks of 64 frames, int16 at the voice's rate, every row a factor-8 item),
  every row joined without a volume against every row joined with one: the median of the steps in which all rows deliver, the two pools
  run one after the other, `--runs` times each.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per route, and the whole leg `--runs` times: the spread of a route is
max − min of its medians over the runs. Needs the GPU: there is no fallback.

Writes <out>/volume.json and the table of <out>/volume.md (everything from a "## Notes" heading on is kept)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "piper-swift_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import katdata as kd  # noqa: E402
import piper_hip as ph  # noqa: E402

CYCLE = (1.0, 0.25, 1.0, 2.0, 0.0, 1.5)
KEYS = ("plain_ms", "vol_ms")


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def leg(rt, factor, batch, warmup, reps):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(batch)]
    gains = np.resize(np.array(CYCLE, np.float32), len(ids))
    slots = {"plain_ms": 0, "vol_ms": 2}
    rt.prepare_batch(0, utts, 0.667)
    rt.prepare_batch(2, utts, 0.667, volume=[gains] * batch)
    per, n = rt.prepared_samples(0)
    pcm = np.empty(n, np.int16)
    times = {k: [] for k in KEYS}
    for k in range(warmup + reps):
        for name in KEYS:
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_launch(v, slots[name]))
            ph._check(lib.piper_hip_voice_collect_pcm16(v, slots[name], None, pcm.ctypes.data_as(ph.c_i16p), n))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
    res = {k: med(t) for k, t in times.items()}
    res["samples"] = int(n)
    return res


def pool_leg(rt, rows, with_volume):
    """ms of the steps of a pool of `rows` rows in which every row delivers a full chunk (the first step, which builds its plan, left out)"""
    ids = kd.FIXTURE_IDS * 8  # 336 frames: five full steps of 64 frames, then a short one
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(rows)]
    gains = np.resize(np.array(CYCLE, np.float32), len(ids))
    pool = rt.stream_pool(10, rows, chunkFrames=64, work_slot=11)
    times = []
    try:
        pool.join(utts, 0.667, volume=[gains] * rows if with_volume else None)
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
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in KEYS:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    out["vol_minus_plain_ms"] = round(out["vol_ms"] - out["plain_ms"], 4)
    out["vol_slower_beyond_spread"] = bool(out["vol_ms"] - out["plain_ms"] > out["plain_ms_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="8x1,64x8", help="factor x batch, comma-separated")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pool-rows", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "volume", "voice": "medium", "gains": list(CYCLE), "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "legs": []}
    for spec in [x for x in args.legs.split(",") if x]:
        f, b = (int(x) for x in spec.split("x"))
        r = summarise([leg(rt, f, b, args.warmup, args.reps) for _ in range(args.runs)])
        r["factor"], r["batch"] = f, b
        out["legs"].append(r)
        print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    if args.pool_rows:
        for wv in (False, True):  # (untimed: the plans of both pools exist before either is timed)
            pool_leg(rt, args.pool_rows, wv)
        plain = [pool_leg(rt, args.pool_rows, False) for _ in range(args.runs)]
        vol = [pool_leg(rt, args.pool_rows, True) for _ in range(args.runs)]
        out["pool"] = {"rows": args.pool_rows, "chunk_frames": 64, "samples_per_step": args.pool_rows * 64 * cfg.hop, "plain_ms_runs": plain,
                       "vol_ms_runs": vol, "plain_ms": med(plain), "vol_ms": med(vol), "plain_ms_spread": round(max(plain) - min(plain), 4),
                       "vol_ms_spread": round(max(vol) - min(vol), 4), "vol_minus_plain_ms": round(med(vol) - med(plain), 4)}
        print(json.dumps(out["pool"]), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "volume.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    lines = ["# Per-phoneme volume on the device", "",
             f"Medium voice (22 050 Hz), int16 at the voice's rate, gains cycling through {CYCLE} per id (`tools/probe/volume_probe.py`; raw "
             f"figures in `volume.json`). One launch → int16 on the host, median ms over {args.reps} interleaved repetitions after {args.warmup} "
             f"untimed ones; ± = max − min of the medians of {args.runs} runs of the leg.", "",
             "| factor | batch | samples | collect_pcm16 | collect_pcm16 with a volume | volume − plain |",
             "|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    for r in out["legs"]:
        tail = f"{r['vol_minus_plain_ms']}{' (slower beyond the spread)' if r['vol_slower_beyond_spread'] else ''}"
        lines.append(f"| {r['factor']} | {r['batch']} | {r['runs'][0]['samples']} | {cell(r, 'plain_ms')} | {cell(r, 'vol_ms')} | {tail} |")
    if "pool" in out:
        q = out["pool"]
        lines += ["", f"One step of a {q['rows']}-row pool, chunks of {q['chunk_frames']} frames ({q['samples_per_step']} samples a step), int16 on the host, "
                  f"median ms of four full steps, ± over {args.runs} pools:", "",
                  "| rows | pool step | pool step, a volume on every row | volume − plain |", "|---|---|---|---|",
                  f"| {q['rows']} | {q['plain_ms']} ± {q['plain_ms_spread']} | {q['vol_ms']} ± {q['vol_ms_spread']} | {q['vol_minus_plain_ms']} |"]
    md = os.path.join(args.out, "volume.md")
    notes = ""
    if os.path.exists(md):
        old = open(md).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    with open(md, "w") as fh:
        fh.write("\n".join(lines) + "\n" + notes)
    print(json.dumps({k: w for k, w in out.items() if k != "legs"}))


if __name__ == "__main__":
    main()
