"""G.711 on the device: what companding in the kernels saves a telephony host over companding the int16 samples on one core, on one
voice, in one process.

Medium voice (22 050 Hz) delivering at 8 000 Hz, sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id, device noise),
chunk 64, μ-law.

  pool     two streaming pools of n rows (16 / 64 / 256) at 8 000 Hz, each kept full with the same sessions (refilled, untimed, before its
           step), taking turns step by step so that the variants are interleaved:
             host     piper_hip_voice_stream_next_batch_pcm16, then piper_hip_g711_from_pcm16 over the step's samples (its share of the
                      time is reported as host_share_ms);
             device   piper_hip_voice_stream_next_batch_g711.
  single   one utterance of factor 1 / 8 / 64, prepared once; timed from the launch to the bytes on the host (pageable buffer):
           collect_pcm16_rate + piper_hip_g711_from_pcm16 against collect_g711, interleaved.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per variant, and the whole leg `--runs` times: the spread of a variant
is max − min of its medians over the runs; the baseline is the host route. Needs the GPU: there is no fallback.

Writes <out>/g711.json and the table of <out>/g711.md (everything from a "## Notes" heading on is kept). Legs already in the JSON that this
call does not measure stay in it, so every leg can be a process of its own, each under its own time limit, chained so that a failure stops
the rest:

    timeout -k 10 200 python tools/probe/g711_probe.py --sizes 16,64 --factors "" && \
    timeout -k 10 300 python tools/probe/g711_probe.py --sizes 256 --factors "" && \
    timeout -k 10 200 python tools/probe/g711_probe.py --sizes "" --factors 1,8,64
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

RATE, LAW = 8000, ph.G711_MULAW
KEYS = ("host_ms", "device_ms")


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def pool_leg(rt, n, chunk, warmup, reps):
    lib, v = rt.lib, rt.voice
    slots = {"host_ms": 8, "device_ms": 10}
    pools = {k: rt.stream_pool(s, n, chunkFrames=chunk, work_slot=s + 1, rate=RATE) for k, s in slots.items()}
    cap = rt.stream_step_capacity(8)
    pcm, out = np.empty(cap, np.int16), np.empty(cap, np.uint8)
    nxt = {k: 0 for k in KEYS}
    times, share, samples = {k: [] for k in KEYS}, [], []
    got = (C.c_int64 * n)()
    for k in range(warmup + reps):
        for name in KEYS:
            free = pools[name].free_rows
            if free:
                pools[name].join([session(nxt[name] + j) for j in range(free)], 0.667)
                nxt[name] += free
            t0 = time.perf_counter()
            if name == "host_ms":
                ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(v, slots[name], None, pcm.ctypes.data_as(ph.c_i16p), cap, got))
                tm = time.perf_counter()
                total = sum(int(x) for x in got)
                ph._check(lib.piper_hip_g711_from_pcm16(LAW, pcm.ctypes.data_as(ph.c_i16p), total, out.ctypes.data_as(ph.c_u8p)))
            else:
                ph._check(lib.piper_hip_voice_stream_next_batch_g711(v, slots[name], None, LAW, out.ctypes.data_as(ph.c_u8p), cap, got))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
                if name == "host_ms":
                    share.append((t1 - tm) * 1e3)
                    samples.append(total)
    for p in pools.values():
        p.close()
    res = {k: med(t) for k, t in times.items()}
    res["host_share_ms"] = med(share)
    res["samples"] = int(np.median(samples))
    return res


def single_leg(rt, factor, warmup, reps):
    lib, v, src = rt.lib, rt.voice, rt.cfg.sample_rate
    ids = kd.FIXTURE_IDS * factor
    rt.prepare(0, ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234)
    n = ph.resample_count(src, RATE, rt._keep[0][1])
    pcm, out = np.empty(n, np.int16), np.empty(n, np.uint8)
    times, share = {k: [] for k in KEYS}, []
    for k in range(warmup + reps):
        for name in KEYS:
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_launch(v, 0))
            if name == "host_ms":
                ph._check(lib.piper_hip_voice_collect_pcm16_rate(v, 0, None, RATE, pcm.ctypes.data_as(ph.c_i16p), n))
                tm = time.perf_counter()
                ph._check(lib.piper_hip_g711_from_pcm16(LAW, pcm.ctypes.data_as(ph.c_i16p), n, out.ctypes.data_as(ph.c_u8p)))
            else:
                ph._check(lib.piper_hip_voice_collect_g711(v, 0, None, LAW, RATE, out.ctypes.data_as(ph.c_u8p), n))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
                if name == "host_ms":
                    share.append((t1 - tm) * 1e3)
    res = {k: med(t) for k, t in times.items()}
    res["host_share_ms"] = med(share)
    res["samples"] = int(n)
    return res


def summarise(runs):
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in KEYS + ("host_share_ms",):
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    out["device_minus_host_ms"] = round(out["device_ms"] - out["host_ms"], 4)
    out["device_slower_beyond_spread"] = bool(out["device_ms"] - out["host_ms"] > out["host_ms_spread"])
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
    out = {"probe": "g711", "voice": "medium", "rate": RATE, "law": "mulaw", "chunk_frames": args.chunk, "factors": "1..8 cycled",
           "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "pool": [], "single": []}
    path = os.path.join(args.out, "g711.json")
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
    lines = ["# G.711 on the device", "",
             f"Medium voice (22 050 Hz) at {RATE} Hz, μ-law, chunk {args.chunk}, factors 1 … 8 cycled (`tools/probe/g711_probe.py`; raw figures in "
             f"`g711.json`). Median ms over {args.reps} interleaved repetitions after {args.warmup} untimed ones; ± = max − min of the medians of "
             f"{args.runs} runs of the leg. host = the int16 call + `piper_hip_g711_from_pcm16` on one core (its share in the third column); "
             "device = the G.711 call.", "",
             "| leg | samples | host route | of which companding | device route | device − host |", "|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    for r in out["pool"]:
        lines.append(f"| pool kept full, {r['rows']} rows, step | {r['runs'][0]['samples']} | {cell(r, 'host_ms')} | {cell(r, 'host_share_ms')} | "
                     f"{cell(r, 'device_ms')} | {r['device_minus_host_ms']}{' (slower beyond the spread)' if r['device_slower_beyond_spread'] else ''} |")
    for r in out["single"]:
        lines.append(f"| one utterance, factor {r['factor']}, launch → bytes | {r['runs'][0]['samples']} | {cell(r, 'host_ms')} | "
                     f"{cell(r, 'host_share_ms')} | {cell(r, 'device_ms')} | "
                     f"{r['device_minus_host_ms']}{' (slower beyond the spread)' if r['device_slower_beyond_spread'] else ''} |")
    md = os.path.join(args.out, "g711.md")
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
