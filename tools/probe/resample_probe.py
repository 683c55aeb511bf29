"""The output rate on the device: what resampling to 8, 16 or 48 kHz costs a PCM step and a PCM collect, on one voice, in one process.

Medium voice (22 050 Hz), sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id, device noise), chunk 64.

  pool     one streaming pool of n rows (16 / 64 / 256) per rate — the voice's own (the baseline: the un-resampled PCM step) and 8 000,
           16 000, 48 000 — each kept full with the same sessions (refilled, untimed, before its step). The pools take turns step by step,
           so the variants are interleaved; timed is piper_hip_voice_stream_next_batch_pcm16.
  single   one utterance of factor 1 / 8 / 64, prepared once; timed from the launch to the samples on the host (pageable buffer):
           collect_pcm16 against collect_pcm16_rate at each rate, interleaved.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per variant, and the whole leg `--runs` times: the spread of a variant
is max − min of its medians over the runs. Needs the GPU: there is no fallback.

Writes <out>/resample.json and the table of <out>/resample.md (everything from a "## Notes" heading on is kept). Legs already in the JSON
that this call does not measure stay in it, so every leg can be a process of its own, each under its own time limit, chained so that a
failure stops the rest:

    timeout -k 10 240 python tools/probe/resample_probe.py --sizes 16 --factors "" && \
    timeout -k 10 300 python tools/probe/resample_probe.py --sizes 64 --factors "" && \
    timeout -k 10 600 python tools/probe/resample_probe.py --sizes 256 --factors "" && \
    timeout -k 10 240 python tools/probe/resample_probe.py --sizes "" --factors 1,8,64
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

RATES = (0, 8000, 16000, 48000)  # 0: the voice's own rate
c_i16p = C.POINTER(C.c_int16)


def key(rate):
    return "native_ms" if rate == 0 else "r%d_ms" % rate


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def pool_leg(rt, n, chunk, warmup, reps):
    lib, v = rt.lib, rt.voice
    pools, bufs, nxt, times, samples = [], [], [], {key(r): [] for r in RATES}, {key(r): [] for r in RATES}
    for i, rate in enumerate(RATES):
        pools.append(rt.stream_pool(8 + 2 * i, n, chunkFrames=chunk, work_slot=9 + 2 * i, rate=rate or None))
        bufs.append(np.empty(rt.stream_step_capacity(8 + 2 * i), np.int16))
        nxt.append(0)
    got = (C.c_int64 * n)()
    for k in range(warmup + reps):
        for i, rate in enumerate(RATES):
            free = pools[i].free_rows
            if free:
                pools[i].join([session(nxt[i] + j) for j in range(free)], 0.667)
                nxt[i] += free
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(v, 8 + 2 * i, None, bufs[i].ctypes.data_as(c_i16p), bufs[i].size, got))
            t1 = time.perf_counter()
            if k >= warmup:
                times[key(rate)].append((t1 - t0) * 1e3)
                samples[key(rate)].append(sum(int(x) for x in got))
    for p in pools:
        p.close()
    out = {k: med(t) for k, t in times.items()}
    out.update({k.replace("_ms", "_samples"): int(np.median(s)) for k, s in samples.items()})
    return out


def single_leg(rt, factor, warmup, reps):
    lib, v, src = rt.lib, rt.voice, rt.cfg.sample_rate
    ids = kd.FIXTURE_IDS * factor
    rt.prepare(0, ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234)
    n = rt._keep[0][1]
    bufs = [np.empty(ph.resample_count(src, r or src, n), np.int16) for r in RATES]
    times = {key(r): [] for r in RATES}
    for k in range(warmup + reps):
        for i, rate in enumerate(RATES):
            p = bufs[i].ctypes.data_as(c_i16p)
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_launch(v, 0))
            if rate:
                ph._check(lib.piper_hip_voice_collect_pcm16_rate(v, 0, None, rate, p, bufs[i].size))
            else:
                ph._check(lib.piper_hip_voice_collect_pcm16(v, 0, None, p, bufs[i].size))
            t1 = time.perf_counter()
            if k >= warmup:
                times[key(rate)].append((t1 - t0) * 1e3)
    out = {k: med(t) for k, t in times.items()}
    out["samples"] = int(n)
    return out


def summarise(runs):
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in [key(r) for r in RATES]:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--factors", default="1,8,64")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--fresh", action="store_true", help="drop the legs an earlier call left in the JSON")
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "resample", "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled", "warmup": args.warmup, "reps": args.reps,
           "runs": args.runs, "pool": [], "single": []}
    path = os.path.join(args.out, "resample.json")
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
    cols = " | ".join("native" if r == 0 else "%d Hz" % r for r in RATES)
    lines = ["# Output rate on the device", "",
             f"Medium voice (22 050 Hz), chunk {args.chunk}, factors 1 … 8 cycled (`tools/probe/resample_probe.py`; raw figures in `resample.json`). Median "
             f"ms over {args.reps} interleaved repetitions after {args.warmup} untimed ones; ± = max − min of the medians of {args.runs} runs of the leg.", "",
             f"| leg | input samples | {cols} |", "|---|---|" + "---|" * len(RATES)]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    for r in out["pool"]:
        lines.append(f"| pool kept full, {r['rows']} rows, PCM step | {r['runs'][0]['native_samples']} | " + " | ".join(cell(r, key(x)) for x in RATES) + " |")
    for r in out["single"]:
        lines.append(f"| one utterance, factor {r['factor']}, launch → samples | {r['runs'][0]['samples']} | " + " | ".join(cell(r, key(x)) for x in RATES) + " |")
    md = os.path.join(args.out, "resample.md")
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
