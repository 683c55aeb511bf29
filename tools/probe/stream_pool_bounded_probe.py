"""Streaming pool: what a join with PREDICTED durations costs the host thread that drives the pool, with and without the host round trip.

Medium voice, sessions of factors 1 … 8 cycled (14 · factor ids, durations predicted, device noise), chunk 64, a 16-row and a 64-row pool
kept full. After every step each free row is filled by a join of ONE session — the serving pattern: requests arrive one at a time.

  --mode predicted   stream_pool_join with durations == NULL: the join uploads, runs encoder + predictor and waits for the frame counts
                     before it enqueues the flow and the adopt. Uses nothing newer than the pool itself, so it runs on an older build
                     (--root <tree of that build>).
  --mode bounded     stream_pool_join_bounded with max_frames = --frames-per-id · ids: nothing in the join waits for the GPU.

Per pool size, over `--reps` timed steps after `--warmup` untimed ones, the whole leg `--runs` times:
  join_ms_median / join_ms_p95   host wall time inside one join call;
  first_audio_ms                 from the start of the last join before a step to the return of that step, which delivers the joined
                                 session's first chunk (median);
  step_ms                        wall time of one stream_next_batch (median). In bounded mode the step is where the host waits for the
                                 joins made before it, so the join's GPU time shows here if the host arrives early.
  over_bound                     joins the predictor pushed over max_frames (bounded mode; their rows are free again).
--work-slots K rotates the joins through K work slot ids (default 1: every join reuses one, and so first waits for the previous join's
work on that slot's stream — the wait every prepare makes before it rewrites a slot's staging).
The spread of a figure is max − min of its per-run values. Needs the GPU: there is no fallback.

Writes <out>/<name>.json; each call adds or replaces its own section "<mode>@<label>" and keeps the others.

    timeout -k 10 300 python tools/probe/stream_pool_bounded_probe.py --mode bounded --label this
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def p95(x):
    return round(float(np.percentile(np.asarray(x, np.float64), 95)), 4)


def leg(ph, kd, rt, mode, rows, chunk, warmup, reps, frames_per_id, work_slots):
    pool = rt.stream_pool(0, rows, chunkFrames=chunk, work_slot=1)
    state = {"next": 0, "over": 0}

    def join_one():
        i = state["next"]
        state["next"] += 1
        f = 1 + i % 8
        utt = (kd.FIXTURE_IDS * f, None, None, {"noise_mode": "device", "seed": 1000 + i})
        pool.work_slot = 1 + i % work_slots
        t0 = time.perf_counter()
        if mode == "bounded":
            (item,) = pool.join_bounded([utt], frames_per_id * 14 * f, 0.667)
        else:
            ((item, _samples),) = pool.join([utt], 0.667)
        return t0, time.perf_counter(), item

    joins, first, steps = [], [], []
    for k in range(warmup + reps):
        last, new = None, []
        for _ in range(pool.free_rows):
            last = join_one()
            new.append(last[2])
            if k >= warmup:
                joins.append((last[1] - last[0]) * 1e3)
        t0 = time.perf_counter()
        pool.step()
        t1 = time.perf_counter()
        if k >= warmup:
            steps.append((t1 - t0) * 1e3)
            if last is not None:
                first.append((t1 - last[0]) * 1e3)
        if mode == "bounded":  # (untimed) an item over its bound never ran: its row is free again
            for item in new:
                try:
                    pool.item_samples(item)
                except ph.ShapeMismatch:
                    state["over"] += 1
    pool.close()
    return {"join_ms_median": med(joins), "join_ms_p95": p95(joins), "first_audio_ms": med(first), "step_ms": med(steps), "joins": len(joins),
            "over_bound": state["over"]}


def summarise(runs):
    out = {"runs": runs}
    for k in runs[0]:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("predicted", "bounded"), required=True)
    ap.add_argument("--label", default="this", help="which build the section belongs to, e.g. parent / this")
    ap.add_argument("--root", default=HERE, help="the tree whose library and Python package are measured")
    ap.add_argument("--pools", default="16,64")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=96)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames-per-id", type=int, default=6)
    ap.add_argument("--work-slots", type=int, default=1, help="work slot ids the joins rotate through (1: every join reuses one)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles"))
    ap.add_argument("--name", default="stream_pool_bounded")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, os.path.join(root, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(root, "tests"))
    import katdata as kd
    import piper_hip as ph
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    section = {"mode": args.mode, "label": args.label, "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled",
               "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "work_slots": args.work_slots}
    if args.mode == "bounded":
        section["max_frames"] = "%d per id" % args.frames_per_id
    for rows in [int(x) for x in args.pools.split(",") if x]:
        section["rows_%d" % rows] = summarise([leg(ph, kd, rt, args.mode, rows, args.chunk, args.warmup, args.reps, args.frames_per_id, args.work_slots)
                                               for _ in range(args.runs)])
        print(json.dumps({k: w for k, w in section["rows_%d" % rows].items() if k != "runs"}), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    out = json.load(open(path)) if os.path.exists(path) else {"probe": "stream_pool_bounded"}
    out["%s@%s" % (args.mode, args.label)] = section
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in section.items() if not k.startswith("rows_")}))


if __name__ == "__main__":
    main()
