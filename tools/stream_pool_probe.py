"""The streaming pool against a fixed group and against single-slot streams, on one voice.

Medium voice, chunk 64, sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id, device noise). For each session count
n in {16, 64}, all from one run:

  pool_staggered   a pool of n rows; the sessions arrive over time (seeded: a random number of arrivals before every step, joined in
                   one join). First audio after join per session (from the join call to the end of the step that delivers its first
                   chunk): median and p95. Aggregate audio seconds per wall second, joins included.
  pool_full        the pool kept full: every row that frees is refilled before the next step. ms per step (the step call alone) and ms
                   per join.
  pool_quarter     the same with n / 4 rows kept occupied in the pool of n rows: what low occupancy costs at the fixed generator batch.
  pool_at_once     the n sessions joined into an empty pool in one join, then steps until idle: the group's work step for step.
  group            the same n sessions as ONE stream_begin_batch group, all present at once — the upper bound. Three times, to show the
                   run-to-run spread.
  single           the same n sessions as single-slot streams driven round robin, 16 at a time (the voice has 16 slot ids).

Every leg runs once untimed first (plan builds, graph captures), then timed. Writes <out>/stream_pool_probe.json and a table in
<out>/stream_pool.md. Needs the GPU: there is no fallback.

    python tools/stream_pool_probe.py [--sizes 16,64] [--chunk 64] [--out profiles]
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

POOL_SLOT, WORK_SLOT = 14, 15
KEEP_STEPS = 48  # steps of the kept-occupied legs


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def pct(x, q):
    return round(float(np.percentile(np.asarray(x, np.float64), q)), 3)


def pool_staggered(rt, n, chunk, seed):
    rng = np.random.default_rng(seed)
    pool = rt.stream_pool(POOL_SLOT, n, chunkFrames=chunk, work_slot=WORK_SLOT)
    joined_at, first, step_ms, join_ms = {}, [], [], []
    nxt, samples = 0, 0
    t0 = time.perf_counter()
    while True:
        k = min(int(rng.integers(0, max(3, n // 8 + 1))), n - nxt, pool.free_rows)
        if k:
            t = time.perf_counter()
            for item, _ in pool.join([session(nxt + j) for j in range(k)], 0.667):
                joined_at[item] = t
            join_ms.append((time.perf_counter() - t) * 1e3)
            nxt += k
        t = time.perf_counter()
        out = pool.step()
        now = time.perf_counter()
        if not out:
            if nxt >= n:
                break
            continue  # an idle step while nobody has arrived yet
        step_ms.append((now - t) * 1e3)
        for item, c in out.items():
            samples += c.size
            if item in joined_at:
                first.append((now - joined_at.pop(item)) * 1e3)
    wall = now - t0
    pool.close()
    return {"sessions": n, "steps": len(step_ms), "joins": len(join_ms), "first_audio_ms_median": pct(first, 50), "first_audio_ms_p95": pct(first, 95),
            "step_ms_median": pct(step_ms, 50), "join_ms_median": pct(join_ms, 50), "wall_ms": round(wall * 1e3, 3), "samples": samples}


def pool_kept(rt, n, occupied, chunk):
    """`occupied` rows of a pool of n kept busy for KEEP_STEPS steps: freed rows are refilled before the next step."""
    pool = rt.stream_pool(POOL_SLOT, n, chunkFrames=chunk, work_slot=WORK_SLOT)
    step_ms, join_ms, active = [], [], []
    nxt, samples = 0, 0
    t0 = time.perf_counter()
    for _ in range(KEEP_STEPS):
        k = occupied - (n - pool.free_rows)
        if k > 0:
            t = time.perf_counter()
            pool.join([session(nxt + j) for j in range(k)], 0.667)
            join_ms.append((time.perf_counter() - t) * 1e3)
            nxt += k
        t = time.perf_counter()
        out = pool.step()
        step_ms.append((time.perf_counter() - t) * 1e3)
        active.append(len(out))
        samples += sum(c.size for c in out.values())
    wall = time.perf_counter() - t0
    pool.close()
    assert min(active) == occupied
    return {"rows": n, "occupied": occupied, "steps": KEEP_STEPS, "step_ms_median": pct(step_ms, 50), "step_ms_p95": pct(step_ms, 95),
            "join_ms_median": pct(join_ms, 50), "joins": len(join_ms), "samples_per_step": samples // KEEP_STEPS, "wall_ms": round(wall * 1e3, 3),
            "samples": samples}


def pool_at_once(rt, n, chunk):
    """The group's sessions joined into an empty pool in ONE join, then steps until idle: step for step the group's work (the same rows
    active, the same windows), through the pool's row stores. As in `group`, the first step holds encoder + flow."""
    pool = rt.stream_pool(POOL_SLOT, n, chunkFrames=chunk, work_slot=WORK_SLOT)
    t0 = time.perf_counter()
    pool.join([session(i) for i in range(n)], 0.667)
    marks, samples = [], 0
    while True:
        out = pool.step()
        if not out:
            break
        marks.append(time.perf_counter())
        samples += sum(c.size for c in out.values())
    pool.close()
    steps = np.diff([t0] + marks) * 1e3
    return {"steps": len(marks), "first_chunk_ms": round(float(steps[0]), 3), "step_ms_median": pct(steps, 50), "step_ms_p95": pct(steps, 95),
            "step2_ms": round(float(steps[1]), 3) if len(steps) > 1 else None, "samples_per_step": samples // len(marks), "wall_ms": round((marks[-1] - t0) * 1e3, 3),
            "samples": samples}


def group(rt, n, chunk):
    t0 = time.perf_counter()
    marks, samples = [], 0
    for chunks in rt.synthesize_stream_batch([session(i) for i in range(n)], 0.667, chunkFrames=chunk, slot=0):
        marks.append(time.perf_counter())
        samples += sum(c.size for c in chunks)
    # the first one holds stream_begin_batch (encoder + flow of the whole group); step2_ms: every item longer than one chunk is still active
    steps = np.diff([t0] + marks) * 1e3
    return {"steps": len(marks), "first_chunk_ms": round(float(steps[0]), 3), "step_ms_median": pct(steps, 50), "step_ms_p95": pct(steps, 95),
            "step2_ms": round(float(steps[1]), 3) if len(steps) > 1 else None, "samples_per_step": samples // len(marks), "wall_ms": round((marks[-1] - t0) * 1e3, 3),
            "samples": samples}


def single(rt, n, chunk):
    """n single-slot streams round robin on 16 slot ids: a slot whose stream has ended begins the next session."""
    lib, v, hop = rt.lib, rt.voice, rt.cfg.hop
    buf = np.empty(chunk * hop, np.float32)
    got = C.c_int64()
    keep, begun_at, first = {}, {}, []
    nxt, samples = 0, 0
    live = {}
    t0 = time.perf_counter()
    while True:
        for s in range(16):
            if s not in live and nxt < n:
                ids, dur, noise, kw = session(nxt)
                u, keep[s] = rt._utt(ids, dur, noise, 0.667, **kw)
                begun_at[s] = time.perf_counter()
                rc = lib.piper_hip_voice_stream_begin(v, C.byref(u), s, chunk)
                if rc < 0:
                    ph._check(rc)
                live[s] = nxt
                nxt += 1
        if not live:
            break
        for s in list(live):
            ph._check(lib.piper_hip_voice_stream_next(v, s, buf.ctypes.data_as(ph.c_f32p), buf.size, C.byref(got)))
            if got.value:
                samples += got.value
                if s in begun_at:
                    first.append((time.perf_counter() - begun_at.pop(s)) * 1e3)
            else:
                del live[s]
    wall = time.perf_counter() - t0
    return {"first_audio_ms_median": pct(first, 50), "first_audio_ms_p95": pct(first, 95), "wall_ms": round(wall * 1e3, 3), "samples": samples}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)  # the joins' encoder + flow plans (one per bucket and join size) next to the generator plans
    rate = float(cfg.sample_rate)
    out = {"probe": "stream_pool", "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled", "sample_rate": rate,
           "arrival_seed": args.seed, "receptive_field_frames": int(rt.lib.piper_hip_voice_receptive_field(rt.voice)), "results": []}

    def rated(r):
        r["audio_s_per_wall_s"] = round(r["samples"] / rate / (r["wall_ms"] * 1e-3), 2)
        return r

    for n in [int(x) for x in args.sizes.split(",")]:
        r = {"n": n}
        for name, leg in (("pool_staggered", lambda: pool_staggered(rt, n, args.chunk, args.seed)),
                          ("pool_full", lambda: pool_kept(rt, n, n, args.chunk)),
                          ("pool_quarter", lambda: pool_kept(rt, n, max(n // 4, 1), args.chunk)),
                          ("pool_at_once", lambda: pool_at_once(rt, n, args.chunk)),
                          ("single", lambda: single(rt, n, args.chunk))):
            leg()  # untimed: builds and captures
            r[name] = rated(leg())
        group(rt, n, args.chunk)
        r["group"] = [rated(group(rt, n, args.chunk)) for _ in range(3)]
        med = [g["step_ms_median"] for g in r["group"]]
        r["group_step_ms_median_spread"] = round(max(med) - min(med), 3)
        r["full_minus_group_step_ms"] = round(r["pool_full"]["step_ms_median"] - float(np.median(med)), 3)
        r["at_once_minus_group_step_ms"] = round(r["pool_at_once"]["step_ms_median"] - float(np.median(med)), 3)
        r["plans"] = rt.plan_info(0)["cached_plans"]
        out["results"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "stream_pool_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    lines = ["# Streaming pool probe", "",
             f"Medium voice, chunk {args.chunk}, factors 1 … 8 cycled, arrival seed {args.seed} (`tools/stream_pool_probe.py`; raw figures in "
             "`stream_pool_probe.json`). Times in ms; audio-s / wall-s over the whole leg.", "",
             "| n | leg | first audio median / p95 | step median / p95 | samples per step | audio-s / wall-s |", "|---|---|---|---|---|---|"]
    for r in out["results"]:
        s, f, q, g1 = r["pool_staggered"], r["pool_full"], r["pool_quarter"], r["single"]
        lines.append(f"| {r['n']} | pool, staggered arrivals | {s['first_audio_ms_median']} / {s['first_audio_ms_p95']} | {s['step_ms_median']} / – | {s['samples'] // s['steps']} | {s['audio_s_per_wall_s']} |")
        lines.append(f"| {r['n']} | pool kept full | – | {f['step_ms_median']} / {f['step_ms_p95']} | {f['samples_per_step']} | {f['audio_s_per_wall_s']} |")
        lines.append(f"| {r['n']} | pool at a quarter | – | {q['step_ms_median']} / {q['step_ms_p95']} | {q['samples_per_step']} | {q['audio_s_per_wall_s']} |")
        a = r["pool_at_once"]
        lines.append(f"| {r['n']} | pool, all joined at once | {a['first_chunk_ms']} / – | {a['step_ms_median']} / {a['step_ms_p95']} | {a['samples_per_step']} | {a['audio_s_per_wall_s']} |")
        for k, g in enumerate(r["group"]):
            lines.append(f"| {r['n']} | group, run {k + 1} | {g['first_chunk_ms']} / – | {g['step_ms_median']} / {g['step_ms_p95']} | {g['samples_per_step']} | {g['audio_s_per_wall_s']} |")
        lines.append(f"| {r['n']} | single-slot round robin | {g1['first_audio_ms_median']} / {g1['first_audio_ms_p95']} | – | – | {g1['audio_s_per_wall_s']} |")
    with open(os.path.join(args.out, "stream_pool.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
