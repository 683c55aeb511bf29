"""The join on the device: what assembling a batch into one programme (include/piper_hip.h "Join") costs from the launch to int16 on
the host, against the same collect without a join and against the host route it replaces, on one voice, in one process.

Medium voice (22 050 Hz), the fixture utterance tiled by 8 (F = 336 frames, 3 frames per id, device noise), 8 such items in one ragged
batch. Timed from the launch to the samples in a pageable host buffer, the routes interleaved:

  s16         piper_hip_voice_collect_pcm16 without a join: the items back to back (what the parent commit runs)
  s16+join    the same with a join on the slot: gap 200 ms, trim on (threshold 0.01, pad 5 ms, fade 3 ms)
  host        the route the join replaces: the floats down (collect), then numpy finds each item's edges, fades, concatenates with the
              silences (tests/join_ref.py's arithmetic, vectorised) and converts to int16

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
JOIN = dict(gap_ms=200.0, trim=1, trim_threshold=0.01, trim_pad_ms=5.0, fade_ms=3.0)


def host_join(items, rate):
    """trim / fade / gap / int16 on the host, with numpy"""
    gap = np.zeros(int(np.floor(JOIN["gap_ms"] * rate / 1000.0 + 0.5)), np.float32)
    P = int(np.floor(JOIN["trim_pad_ms"] * rate / 1000.0 + 0.5))
    Fd = int(np.floor(JOIN["fade_ms"] * rate / 1000.0 + 0.5))
    parts = []
    for i, x in enumerate(items):
        idx = np.flatnonzero(np.abs(x) > np.float32(JOIN["trim_threshold"]))
        if idx.size:
            s, t = max(0, int(idx[0]) - P), min(x.size, int(idx[-1]) + 1 + P)
            y = x[s:t].copy()
            m = min(Fd, y.size)
            g = ((np.arange(m) + 1.0) / (Fd + 1.0)).astype(np.float32)
            if s > 0:
                y[:m] *= g
            if t < x.size:
                y[y.size - m:] *= g[::-1]
            parts.append(y)
        if i + 1 < len(items):
            parts.append(gap)
    y = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return (np.clip(y, -1.0, 1.0).astype(np.float64) * 32767.0).astype(np.int16)


def leg(ph, kd, rt, warmup, reps, parent):
    lib, v = rt.lib, rt.voice
    ids = kd.FIXTURE_IDS * 8
    utts = [(ids, [3] * len(ids), None, {"noise_mode": "device", "seed": 1234 + i}) for i in range(8)]
    rt.prepare_batch(0, utts, 0.667)
    routes = ["s16"]
    if not parent:
        rt.prepare_batch(2, utts, 0.667)
        rt.slot_join(2, JOIN)
        routes += ["s16+join", "host"]
        cap = rt.join_capacity(2)
        joined = np.empty(cap, np.int16)
    per, n = rt.prepared_samples(0)
    pcm, f32 = np.empty(n, np.int16), np.empty(n, np.float32)
    times = {k: [] for k in routes}
    for k in range(warmup + reps):
        for name in routes:
            t0 = time.perf_counter()
            if name == "s16":
                ph._check(lib.piper_hip_voice_launch(v, 0))
                ph._check(lib.piper_hip_voice_collect_pcm16(v, 0, None, pcm.ctypes.data_as(ph.c_i16p), n))
            elif name == "s16+join":
                ph._check(lib.piper_hip_voice_launch(v, 2))
                ph._check(lib.piper_hip_voice_collect_pcm16(v, 2, None, joined.ctypes.data_as(ph.c_i16p), cap))
            else:
                ph._check(lib.piper_hip_voice_launch(v, 0))
                ph._check(lib.piper_hip_voice_collect(v, 0, f32.ctypes.data_as(ph.c_f32p), n))
                host_join(np.split(f32, np.cumsum(per)[:-1]), rt.cfg.sample_rate)
            t1 = time.perf_counter()
            if k >= warmup:
                times[name].append((t1 - t0) * 1e3)
    res = {k: round(float(np.median(t)), 4) for k, t in times.items()}
    res["samples"] = int(n)
    if not parent:
        res["programme_samples"] = int(rt.join_report(2)[2])
        rt.slot_join(2, None)
    return res


def main():
    ap = argparse.ArgumentParser()
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
    runs = [leg(ph, kd, rt, a.warmup, a.reps, a.lib_root is not None or a.plain_only) for _ in range(a.runs)]
    out = {"tree": "parent" if a.lib_root else "this, s16 alone" if a.plain_only else "this", "warmup": a.warmup, "reps": a.reps, "runs": runs, "routes": {}}
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
