"""Loudness on the device: what measuring BS.1770 integrated loudness and applying its gain (include/piper_hip.h "Loudness") adds to a
whole-item collect, and what the round trip it replaces costs, on one voice, in one process.

Medium voice (22 050 Hz), the fixture utterance tiled by `factor` (F = 42 · factor frames, 3 frames per id, device noise), `batch` such
items in one ragged batch, 16-bit PCM at the voice's own rate, target −16 LUFS. Timed from the launch to the int16 samples on the host
(pageable buffers), the three routes interleaved:

  plain    piper_hip_voice_collect_pcm16 on a slot id without a loudness
  loud     the same call on a slot id with piper_hip_voice_slot_loudness
  host     what a host does without it: piper_hip_voice_collect (floats), then per item piper_hip_loudness_from_f32, the gain in numpy
           and piper_hip_pcm16_from_f32, all on the CPU

  --kernels N: nothing is timed here — piper_hip_loudness_f32 runs N times on a factor-64 waveform (688 128 samples), for a kernel-trace
  run of a profiler around this script, which tells the measuring kernel from the gate.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per route, and the whole leg `--runs` times: the spread of a route is
max − min of its medians over the runs. Needs the GPU: there is no fallback.

Writes <out>/loudness.json and the table of <out>/loudness.md (everything from a "## Notes" heading on is kept)."""
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

TARGET = (-16.0, 0.0)
KEYS = ("plain_ms", "loud_ms", "host_ms")


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def leg(rt, factor, batch, warmup, reps):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(batch)]
    slots = {"plain_ms": 0, "loud_ms": 2, "host_ms": 4}
    for s in slots.values():
        rt.prepare_batch(s, utts, 0.667)
        rt.slot_loudness(s, None)
    rt.slot_loudness(2, TARGET)
    per, n = rt.prepared_samples(0)
    pcm, wave = np.empty(n, np.int16), np.empty(n, np.float32)
    edges = np.concatenate([[0], np.cumsum(per)])
    times = {k: [] for k in KEYS}
    rate = rt.cfg.sample_rate
    for k in range(warmup + reps):
        for name in KEYS:
            t0 = time.perf_counter()
            ph._check(lib.piper_hip_voice_launch(v, slots[name]))
            if name == "host_ms":
                ph._check(lib.piper_hip_voice_collect(v, 4, wave.ctypes.data_as(ph.c_f32p), n))
                for b in range(batch):
                    x = wave[edges[b]:edges[b + 1]]
                    g = ph.loudness_gain(TARGET, ph.loudness_from_f32(x, rate))
                    pcm[edges[b]:edges[b + 1]] = ph.pcm16(x * g)
            else:
                ph._check(lib.piper_hip_voice_collect_pcm16(v, slots[name], None, pcm.ctypes.data_as(ph.c_i16p), n))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
    lufs, gain = rt.loudness(2)
    host = [float(ph.loudness_from_f32(wave[edges[b]:edges[b + 1]], rate)) for b in range(batch)]
    rt.slot_loudness(2, None)
    res = {k: med(t) for k, t in times.items()}
    res["samples"] = int(n)
    res["lufs_item0"] = round(float(lufs[0]), 4)
    res["max_abs_device_minus_host_lu"] = float(max(abs(float(a) - b) for a, b in zip(lufs, host)))
    return res


def summarise(runs):
    """medians over the runs and the run-to-run spread (max − min of the runs' medians) of every timed key"""
    out = {"runs": runs}
    for k in KEYS:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    out["loud_minus_plain_ms"] = round(out["loud_ms"] - out["plain_ms"], 4)
    out["loud_slower_beyond_spread"] = bool(out["loud_ms"] - out["plain_ms"] > out["plain_ms_spread"])
    out["host_minus_loud_ms"] = round(out["host_ms"] - out["loud_ms"], 4)
    return out


def kernels(backend, n):
    x = kd.sym(77, (14 * 64 * 3 * 256,), 0.9)
    buf = backend.uploadFloat32(x)
    got = [float(backend.loudness_f32(buf, 22050)) for _ in range(n + 1)]
    assert len(set(got)) == 1 and abs(got[0] - float(ph.loudness_from_f32(x, 22050))) < 0.002, got[:2]
    print(json.dumps({"kernel_runs": n + 1, "samples": int(x.size), "lufs": got[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="8,64")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    if args.kernels:
        kernels(backend, args.kernels)
        backend.close()
        return
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    out = {"probe": "loudness", "voice": "medium", "target": list(TARGET), "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "legs": []}
    for f in [int(x) for x in args.factors.split(",") if x]:
        for b in [int(x) for x in args.batches.split(",") if x]:
            r = summarise([leg(rt, f, b, args.warmup, args.reps) for _ in range(args.runs)])
            r["factor"], r["batch"] = f, b
            out["legs"].append(r)
            print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "loudness.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    lines = ["# Loudness on the device", "",
             f"Medium voice (22 050 Hz), int16 at the voice's rate, target {TARGET[0]} LUFS (`tools/probe/loudness_probe.py`; raw figures in "
             f"`loudness.json`). One launch → int16 on the host, median ms over {args.reps} interleaved repetitions after {args.warmup} untimed "
             f"ones; ± = max − min of the medians of {args.runs} runs of the leg.", "",
             "| factor | batch | samples | collect_pcm16 | collect_pcm16 with a loudness | collect, then loudness and PCM on the host | loudness − plain |",
             "|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
    for r in out["legs"]:
        tail = f"{r['loud_minus_plain_ms']}{' (slower beyond the spread)' if r['loud_slower_beyond_spread'] else ''}"
        lines.append(f"| {r['factor']} | {r['batch']} | {r['runs'][0]['samples']} | {cell(r, 'plain_ms')} | {cell(r, 'loud_ms')} | {cell(r, 'host_ms')} | {tail} |")
    md = os.path.join(args.out, "loudness.md")
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
