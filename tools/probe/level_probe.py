"""Level control on the device: what the look-ahead limiter (include/piper_hip.h "Level control") adds to a stream step and to a
whole-item collect, on one voice, in one process.

Medium voice (22 050 Hz), 16-bit PCM at the voice's own rate, sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id,
device noise), chunk 64, level {drive 2, ceiling 0.5, release 50 ms}.

  pool     two streaming pools of n rows (16 / 64 / 256), each kept full with the same sessions (refilled, untimed, before its step), taking
           turns step by step so that the variants are interleaved: plain = piper_hip_voice_stream_next_batch_pcm16 on a pool without a
           level, level = the same call on a pool with piper_hip_voice_stream_set_level.
  single   one utterance of factor 1 / 8 / 64 prepared on two slot ids, one of them with piper_hip_voice_slot_level; timed from the launch to
           the int16 samples on the host (pageable buffer), interleaved.
  chain    --chain N: nothing is timed here — piper_hip_level_f32 runs N times on a factor-64 waveform (688 128 samples, 21 504 blocks), for
           a kernel-trace run of a profiler around this script, which tells the three phases apart (level_gain_kernel is the serial chain).

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per variant, and the whole leg `--runs` times: the spread of a variant
is max − min of its medians over the runs; the baseline is the un-levelled variant. Needs the GPU: there is no fallback.

Writes <out>/level.json and the table of <out>/level.md (everything from a "## Notes" heading on is kept). Legs already in the JSON that
this call does not measure stay in it, so every leg can be a process of its own, each under its own time limit:

    timeout -k 10 200 python tools/probe/level_probe.py --sizes 16,64 --factors "" && \
    timeout -k 10 300 python tools/probe/level_probe.py --sizes 256 --factors "" && \
    timeout -k 10 200 python tools/probe/level_probe.py --sizes "" --factors 1,8,64
"""
import argparse
import ctypes as C
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

LEVEL = (2.0, 0.5, 50.0)
KEYS = ("plain_ms", "level_ms")


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def pool_leg(rt, n, chunk, warmup, reps):
    lib, v = rt.lib, rt.voice
    slots = {"plain_ms": 8, "level_ms": 10}
    pools = {k: rt.stream_pool(s, n, chunkFrames=chunk, work_slot=s + 1, level=LEVEL if k == "level_ms" else None) for k, s in slots.items()}
    cap = rt.stream_step_capacity(10)
    pcm = np.empty(cap, np.int16)
    nxt = {k: 0 for k in KEYS}
    times, samples = {k: [] for k in KEYS}, []
    got = (C.c_int64 * n)()
    for k in range(warmup + reps):
        for name in KEYS:
            free = pools[name].free_rows
            if free:
                pools[name].join([session(nxt[name] + j) for j in range(free)], 0.667)
                nxt[name] += free
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(v, slots[name], None, pcm.ctypes.data_as(ph.c_i16p), cap, got))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
                if name == "plain_ms":
                    samples.append(sum(int(x) for x in got))
    for p in pools.values():
        p.close()
    res = {k: med(t) for k, t in times.items()}
    res["samples"] = int(np.median(samples))
    return res


def single_leg(rt, factor, warmup, reps):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    slots = {"plain_ms": 0, "level_ms": 2}
    for s in slots.values():
        rt.prepare(s, ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234)
    rt.slot_level(0, None)
    rt.slot_level(2, LEVEL)
    n = rt._keep[0][1]
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
    rt.slot_level(2, None)
    res = {k: med(t) for k, t in times.items()}
    res["samples"] = int(n)
    return res


def summarise(runs):
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in KEYS:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    out["level_minus_plain_ms"] = round(out["level_ms"] - out["plain_ms"], 4)
    out["level_slower_beyond_spread"] = bool(out["level_ms"] - out["plain_ms"] > out["plain_ms_spread"])
    return out


def chain(backend, n):
    x = kd.sym(77, (14 * 64 * 3 * 256,), 0.9)
    buf = backend.uploadFloat32(x)
    out = backend.level_f32(buf, 22050, LEVEL)
    for _ in range(n):
        backend.level_f32(buf, 22050, LEVEL, out=out)
    assert np.array_equal(backend.downloadFloat32(out, x.size).view(np.uint32), ph.level_from_f32(x, LEVEL, 22050).view(np.uint32))
    print(json.dumps({"chain_runs": n, "samples": int(x.size), "blocks": int(x.size // 32)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--factors", default="1,8,64")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chain", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--fresh", action="store_true", help="drop the legs an earlier call left in the JSON")
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    if args.chain:
        chain(backend, args.chain)
        backend.close()
        return
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "level", "voice": "medium", "level": list(LEVEL), "chunk_frames": args.chunk, "factors": "1..8 cycled",
           "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "pool": [], "single": []}
    path = os.path.join(args.out, "level.json")
    if not args.fresh and os.path.exists(path):  # legs measured by earlier calls with the same settings stay
        old = json.load(open(path))
        if all(old.get(k) == out[k] for k in ("chunk_frames", "warmup", "reps", "runs")):
            out["pool"], out["single"] = old.get("pool", []), old.get("single", [])
    for n in [int(x) for x in args.sizes.split(",") if x]:
        r = summarise([pool_leg(rt, n, args.chunk, args.warmup, args.reps) for _ in range(args.runs)])
        r["rows"] = n
        out["pool"] = sorted([o for o in out["pool"] if o["rows"] != n] + [r], key=lambda o: o["rows"])
        print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    for f in [int(x) for x in args.factors.split(",") if x]:
        r = summarise([single_leg(rt, f, args.warmup, args.reps) for _ in range(args.runs)])
        r["factor"] = f
        out["single"] = sorted([o for o in out["single"] if o["factor"] != f] + [r], key=lambda o: o["factor"])
        print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    lines = ["# Level control on the device", "",
             f"Medium voice (22 050 Hz), int16 at the voice's rate, level {LEVEL}, chunk {args.chunk}, factors 1 … 8 cycled "
             f"(`tools/probe/level_probe.py`; raw figures in `level.json`). Median ms over {args.reps} interleaved repetitions after "
             f"{args.warmup} untimed ones; ± = max − min of the medians of {args.runs} runs of the leg.", "",
             "| leg | samples | without a level | with a level | level − plain |", "|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    tail = lambda r: f"{r['level_minus_plain_ms']}{' (slower beyond the spread)' if r['level_slower_beyond_spread'] else ''}"  # noqa: E731
    for r in out["pool"]:
        lines.append(f"| pool kept full, {r['rows']} rows, step | {r['runs'][0]['samples']} | {cell(r, 'plain_ms')} | {cell(r, 'level_ms')} | {tail(r)} |")
    for r in out["single"]:
        lines.append(f"| one utterance, factor {r['factor']}, launch → int16 | {r['runs'][0]['samples']} | {cell(r, 'plain_ms')} | {cell(r, 'level_ms')} | {tail(r)} |")
    md = os.path.join(args.out, "level.md")
    notes = ""
    if os.path.exists(md):
        old = open(md).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    with open(md, "w") as fh:
        fh.write("\n".join(lines) + "\n" + notes)
    print(json.dumps({k: w for k, w in out.items() if k not in ("pool", "single")}))


if __name__ == "__main__":
    main()
