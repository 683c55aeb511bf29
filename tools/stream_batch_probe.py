"""Batched streaming vs single-slot streams on one voice: prints ONE JSON line.

Medium voice, chunk 64, mixed-length utterances (factors 1 … 8 of the 14-id fixture, 3 frames per id, device noise). For each group size
n in {1, 4, 16, 64, 256}: time to first chunk (stream_begin_batch + the first stream_next_batch), per-step wall ms (median, p95) and
aggregate audio seconds per wall second over the whole group. For n <= 16 the same sessions also run as n single-slot streams
(stream_begin / stream_next on slots 0 … n-1, driven round robin). Every configuration runs once untimed first (plan builds, graph
captures), then once timed. Needs the GPU: there is no fallback.

    python tools/stream_batch_probe.py [--sizes 1,4,16,64,256] [--chunk 64]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piper-swift_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import katdata as kd  # noqa: E402
import piper_hip as ph  # noqa: E402


def sessions(n):
    """n utterances of factors 1 … 8 in turn (F = 42 · factor frames)."""
    return [(kd.FIXTURE_IDS * (1 + i % 8), [3] * (14 * (1 + i % 8)), None, {"noise_mode": "device", "seed": 1000 + i}) for i in range(n)]


def batched(rt, group, chunk):
    t0 = time.perf_counter()
    marks = []
    samples = 0
    for chunks in rt.synthesize_stream_batch(group, 0.667, chunkFrames=chunk, slot=0):
        marks.append(time.perf_counter())
        samples += sum(c.size for c in chunks)
    return t0, marks, samples


def singles(rt, group, chunk):
    """n single-slot streams driven round robin: one stream_next per live session per round."""
    lib, v, hop = rt.lib, rt.voice, rt.cfg.hop
    buf = np.empty(chunk * hop, np.float32)
    got = C.c_int64()
    keep = []
    t0 = time.perf_counter()
    for s, (ids, dur, noise, kw) in enumerate(group):
        u, k = rt._utt(ids, dur, noise, 0.667, **kw)
        keep.append(k)
        rc = lib.piper_hip_voice_stream_begin(v, C.byref(u), s, chunk)
        if rc < 0:
            ph._check(rc)
    live = list(range(len(group)))
    marks, samples, first = [], 0, None
    while live:
        nxt = []
        for s in live:
            ph._check(lib.piper_hip_voice_stream_next(v, s, buf.ctypes.data_as(ph.c_f32p), buf.size, C.byref(got)))
            if got.value:
                samples += got.value
                nxt.append(s)
                if first is None:
                    first = time.perf_counter()
        live = nxt
        marks.append(time.perf_counter())
    return t0, first, marks, samples


def stats(t0, marks, samples, hop_rate, first=None):
    steps = np.diff([t0] + marks) * 1e3
    wall = marks[-1] - t0
    return {"first_chunk_ms": round(((first or marks[0]) - t0) * 1e3, 3), "steps": len(marks),
            "step_ms_median": round(float(np.median(steps)), 3), "step_ms_p95": round(float(np.percentile(steps, 95)), 3),
            "wall_ms": round(wall * 1e3, 3), "audio_s_per_wall_s": round(samples / hop_rate / wall, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4,16,64,256")
    ap.add_argument("--chunk", type=int, default=64)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    # a group of 256 at factor 8 holds an encoder + flow plan of ≈ 32 GB (its full schedule's arena): keep the generator plans cached
    rt.set_plan_cache(128, 96 << 30)
    rate = float(cfg.sample_rate)
    out = {"probe": "stream_batch", "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled", "sample_rate": rate,
           "receptive_field_frames": int(rt.lib.piper_hip_voice_receptive_field(rt.voice)), "results": []}
    for n in sizes:
        group = sessions(n)
        batched(rt, group, args.chunk)  # untimed: builds and captures
        t0, marks, samples = batched(rt, group, args.chunk)
        r = {"n": n, "audio_s": round(samples / rate, 3), "batched": stats(t0, marks, samples, rate), "plans": rt.plan_info(0)["cached_plans"]}
        if n <= 16:
            singles(rt, group, args.chunk)
            t0, first, marks, samples_s = singles(rt, group, args.chunk)
            assert samples_s == samples
            r["single_round_robin"] = stats(t0, marks, samples_s, rate, first)
        out["results"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
