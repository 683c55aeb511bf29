"""16-bit PCM from the device against fp32 + conversion on the host, on one voice, in one process.

Medium voice, sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id, device noise), chunk 64.

  pool     a streaming pool of n rows (16 / 64 / 256) kept full: every row that frees is refilled (untimed) before the next step. The two
           variants alternate step by step on the same pool:
             float+host   piper_hip_voice_stream_next_batch, then piper_hip_pcm16_from_f32 over the step's samples (what a host that
                          ends in PCM did before the PCM entry points existed); the conversion's share is reported separately;
             pcm          piper_hip_voice_stream_next_batch_pcm16.
  single   one utterance of factor 1 / 8 / 64, prepared once; timed from the launch to the samples on the host (pageable buffer):
             float+host   launch, collect, piper_hip_pcm16_from_f32;
             pcm          launch, collect_pcm16;
             pcm_norm     launch, collect_pcm16 with normalize = 1 (peak pass + pack).

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per variant, interleaved, and the whole leg `--runs` times: the
spread of a variant is max − min of its medians over the runs. In a pool leg the two variants take turns on ONE pool, so a float step and
the PCM step after it are different steps of the same sessions (even and odd ones); with the pool kept full and 30 of each per run the
two medians see the same mix of rows. Needs the GPU: there is no fallback.

Writes <out>/pcm16_probe.json and the table of <out>/pcm16.md (everything from a "## Notes" heading on is kept). Legs already in the JSON
that this call does not measure stay in it, so every leg can be a process of its own, each under its own time limit, chained so that a
failure stops the rest:

    timeout -k 10 240 python tools/probe/pcm16_probe.py --sizes 16 --factors "" && \
    timeout -k 10 240 python tools/probe/pcm16_probe.py --sizes 64 --factors "" && \
    timeout -k 10 420 python tools/probe/pcm16_probe.py --sizes 256 --factors "" && \
    timeout -k 10 240 python tools/probe/pcm16_probe.py --sizes "" --factors 1,8,64

(`--fresh` forgets the legs of an earlier file.)
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

POOL_SLOT, WORK_SLOT = 14, 15
c_i16p = C.POINTER(C.c_int16)


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def pool_leg(rt, n, chunk, warmup, reps):
    lib, v, hop = rt.lib, rt.voice, rt.cfg.hop
    pool = rt.stream_pool(POOL_SLOT, n, chunkFrames=chunk, work_slot=WORK_SLOT)
    cap = n * chunk * hop
    fbuf, pbuf, hbuf = np.empty(cap, np.float32), np.empty(cap, np.int16), np.empty(cap, np.int16)
    got = (C.c_int64 * n)()
    fp, pp, hp = fbuf.ctypes.data_as(ph.c_f32p), pbuf.ctypes.data_as(c_i16p), hbuf.ctypes.data_as(c_i16p)
    t_float, t_host, t_pcm, samples = [], [], [], []
    nxt = 0
    for k in range(2 * (warmup + reps)):
        free = pool.free_rows
        if free:
            pool.join([session(nxt + j) for j in range(free)], 0.667)
            nxt += free
        timed = k >= 2 * warmup
        if k % 2 == 0:
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_stream_next_batch(v, POOL_SLOT, fp, cap, got))
            t1 = time.perf_counter()
            total = sum(int(x) for x in got)
            t2 = time.perf_counter()
            ph._check(lib.piper_hip_pcm16_from_f32(fp, total, hp))
            t3 = time.perf_counter()
            if timed:
                t_float.append((t1 - t0 + t3 - t2) * 1e3)
                t_host.append((t3 - t2) * 1e3)
                samples.append(total)
        else:
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(v, POOL_SLOT, None, pp, cap, got))
            t1 = time.perf_counter()
            if timed:
                t_pcm.append((t1 - t0) * 1e3)
    pool.close()
    return {"float_host_ms": med(t_float), "host_conversion_ms": med(t_host), "pcm_ms": med(t_pcm), "samples_per_step": int(np.median(samples))}


def single_leg(rt, factor, warmup, reps):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    rt.prepare(0, ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234)
    n = rt._keep[0][1]
    fbuf, pbuf, hbuf = np.empty(n, np.float32), np.empty(n, np.int16), np.empty(n, np.int16)
    fp, pp, hp = fbuf.ctypes.data_as(ph.c_f32p), pbuf.ctypes.data_as(c_i16p), hbuf.ctypes.data_as(c_i16p)
    plain, norm = ph.PcmParams(1.0, 0), ph.PcmParams(1.0, 1)
    t_float, t_host, t_pcm, t_norm = [], [], [], []
    for k in range(warmup + reps):
        timed = k >= warmup
        t0 = time.perf_counter()
        ph._check(lib.piper_hip_voice_launch(v, 0))
        ph._check(lib.piper_hip_voice_collect(v, 0, fp, n))
        t1 = time.perf_counter()
        ph._check(lib.piper_hip_pcm16_from_f32(fp, n, hp))
        t2 = time.perf_counter()
        ph._check(lib.piper_hip_voice_launch(v, 0))
        ph._check(lib.piper_hip_voice_collect_pcm16(v, 0, C.byref(plain), pp, n))
        t3 = time.perf_counter()
        ph._check(lib.piper_hip_voice_launch(v, 0))
        ph._check(lib.piper_hip_voice_collect_pcm16(v, 0, C.byref(norm), pp, n))
        t4 = time.perf_counter()
        if timed:
            t_float.append((t2 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
            t_pcm.append((t3 - t2) * 1e3)
            t_norm.append((t4 - t3) * 1e3)
    assert np.array_equal(ph.pcm16(fbuf), hbuf)
    return {"float_host_ms": med(t_float), "host_conversion_ms": med(t_host), "pcm_ms": med(t_pcm), "pcm_norm_ms": med(t_norm), "samples": int(n)}


def summarise(runs, keys):
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in keys:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    out["gain_ms"] = round(out["float_host_ms"] - out["pcm_ms"], 4)
    out["gain_exceeds_float_spread"] = bool(out["gain_ms"] > out["float_host_ms_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--factors", default="1,8,64")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--fresh", action="store_true", help="drop the legs an earlier call left in the JSON")
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "pcm16", "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled", "warmup": args.warmup, "reps": args.reps,
           "runs": args.runs, "pool": [], "single": []}
    path = os.path.join(args.out, "pcm16_probe.json")
    if not args.fresh and os.path.exists(path):  # legs measured by earlier calls with the same settings stay
        old = json.load(open(path))
        if all(old.get(k) == out[k] for k in ("chunk_frames", "warmup", "reps", "runs")):
            out["pool"], out["single"] = old.get("pool", []), old.get("single", [])
    for n in [int(x) for x in args.sizes.split(",") if x]:
        r = summarise([pool_leg(rt, n, args.chunk, args.warmup, args.reps) for _ in range(args.runs)], ("float_host_ms", "host_conversion_ms", "pcm_ms"))
        r["rows"] = n
        out["pool"] = sorted([o for o in out["pool"] if o["rows"] != n] + [r], key=lambda o: o["rows"])
        print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    for f in [int(x) for x in args.factors.split(",") if x]:
        r = summarise([single_leg(rt, f, args.warmup, args.reps) for _ in range(args.runs)], ("float_host_ms", "host_conversion_ms", "pcm_ms", "pcm_norm_ms"))
        r["factor"] = f
        out["single"] = sorted([o for o in out["single"] if o["factor"] != f] + [r], key=lambda o: o["factor"])
        print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    lines = ["# 16-bit PCM from the device", "",
             f"Medium voice, chunk {args.chunk}, factors 1 … 8 cycled (`tools/probe/pcm16_probe.py`; raw figures in `pcm16_probe.json`). Median ms over "
             f"{args.reps} interleaved repetitions after {args.warmup} untimed ones; ± = max − min of the medians of {args.runs} runs of the leg.", "",
             "| leg | samples | fp32 + host conversion | of which host conversion | PCM from the device | gain | gain > ± of fp32 | PCM, normalize = 1 |", "|---|---|---|---|---|---|---|---|"]
    for r in out["pool"]:
        lines.append(f"| pool kept full, {r['rows']} rows, per step | {r['runs'][0]['samples_per_step']} | {r['float_host_ms']} ± {r['float_host_ms_spread']} | "
                     f"{r['host_conversion_ms']} | {r['pcm_ms']} ± {r['pcm_ms_spread']} | {r['gain_ms']} | {'yes' if r['gain_exceeds_float_spread'] else 'NO'} | – |")
    for r in out["single"]:
        lines.append(f"| one utterance, factor {r['factor']}, launch → samples | {r['runs'][0]['samples']} | {r['float_host_ms']} ± {r['float_host_ms_spread']} | "
                     f"{r['host_conversion_ms']} | {r['pcm_ms']} ± {r['pcm_ms_spread']} | {r['gain_ms']} | {'yes' if r['gain_exceeds_float_spread'] else 'NO'} | {r['pcm_norm_ms']} ± {r['pcm_norm_ms_spread']} |")
    md = os.path.join(args.out, "pcm16.md")
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
