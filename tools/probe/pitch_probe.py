"""The pitch on the device: what shifting the items of a request (include/piper_hip.h "Pitch") costs from the launch to int16 on the
host, against the same collect without a pitch and against the host route it replaces, on one voice, in one process.

Medium voice (22 050 Hz), the fixture utterance tiled by --factor (8: F = 336 frames, 64: F = 2688; 3 frames per id, device noise),
--batch such items in one batch. Timed from the launch to the samples in a pageable host buffer, the routes interleaved:

  s16         piper_hip_voice_collect_pcm16 without a pitch (what the parent commit runs)
  s16+pitch   the same on a slot staged with a pitch of +3 semitones on every item (varispeed: the durations are supplied)
  s16-pitch   the same at −5 semitones: longer items, 48 taps
  host        the route the stage replaces: the floats down (collect), piper_hip_pitch_from_f32 per item at +3 semitones on one core,
              then int16 with numpy

With --lib-root the package and library of another tree are used (the parent commit's), for the `s16` route only; --plain-only runs
this tree the same way (the `s16` route alone, back to back), which is the leg to hold against the parent's.

Every leg runs --warmup untimed rounds, then --reps timed ones per route, and the whole leg --runs times: the spread of a route is
max − min of its medians over the runs. Needs the GPU: there is no fallback. Prints one JSON object; --out writes it to that file too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
UP, DOWN = (3.0, 0), (-5.0, 0)


def leg(ph, kd, rt, factor, batch, warmup, reps, parent):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * factor
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(batch)]
    rt.prepare_batch(0, utts, 0.667)
    per, n = rt.prepared_samples(0)
    pcm, f32 = np.empty(n, np.int16), np.empty(n, np.float32)
    routes, out = ["s16"], {}
    if not parent:
        for slot, name, shift in ((2, "s16+pitch", UP), (3, "s16-pitch", DOWN)):
            rt.prepare_batch(slot, utts, 0.667, pitch=shift)
            out[name] = np.empty(rt.pitch_samples(slot)[1], np.int16)
        routes += ["s16+pitch", "s16-pitch", "host"]
    times = {k: [] for k in routes}
    for k in range(warmup + reps):
        for name in routes:
            t0 = time.perf_counter()
            if name == "s16":
                ph._check(lib.piper_hip_voice_launch(v, 0))
                ph._check(lib.piper_hip_voice_collect_pcm16(v, 0, None, pcm.ctypes.data_as(ph.c_i16p), n))
            elif name == "host":
                ph._check(lib.piper_hip_voice_launch(v, 0))
                ph._check(lib.piper_hip_voice_collect(v, 0, f32.ctypes.data_as(ph.c_f32p), n))
                y = np.concatenate([ph.pitch_from_f32(x, UP[0]) for x in np.split(f32, np.cumsum(per)[:-1])])
                (np.clip(y, -1.0, 1.0).astype(np.float64) * 32767.0).astype(np.int16)
            else:
                slot = 2 if name == "s16+pitch" else 3
                ph._check(lib.piper_hip_voice_launch(v, slot))
                ph._check(lib.piper_hip_voice_collect_pcm16(v, slot, None, out[name].ctypes.data_as(ph.c_i16p), out[name].size))
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
    res = {k: round(float(np.median(t)), 4) for k, t in times.items()}
    res["samples"] = int(n)
    for name, buf in out.items():
        res[name + " samples"] = int(buf.size)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factor", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lib-root", default=None, help="another tree (the parent commit's): its package and library, the s16 route only")
    ap.add_argument("--plain-only", action="store_true", help="this tree, the s16 route alone: the twin of a --lib-root run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = a.lib_root or ROOT
    sys.path.insert(0, os.path.join(root, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import katdata as kd
    import piper_hip as ph
    backend = ph.HipBackend(0)
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    runs = [leg(ph, kd, rt, a.factor, a.batch, a.warmup, a.reps, a.lib_root is not None or a.plain_only) for _ in range(a.runs)]
    out = {"tree": "parent" if a.lib_root else "this, s16 alone" if a.plain_only else "this", "factor": a.factor, "batch": a.batch,
           "warmup": a.warmup, "reps": a.reps, "runs": runs, "routes": {}}
    for k in runs[0]:
        if k.endswith("samples"):
            out[k] = runs[0][k]
            continue
        m = [r[k] for r in runs]
        out["routes"][k] = {"median_ms": round(float(np.median(m)), 4), "spread_ms": round(max(m) - min(m), 4)}
    rt.close()
    backend.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
