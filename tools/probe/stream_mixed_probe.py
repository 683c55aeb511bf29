"""Mixed-format streaming: what one pool for every output format costs against one pool per format, on one voice, in one process.

Medium voice (22 050 Hz), sessions of factors 1 … 8 cycled (F = 42 · factor frames, 3 frames per id, device noise), chunk 64 — the session
mix of profiles/stream_pool_probe.json. Every pool is kept full (refilled, untimed, before its step).

  mix      (a) one mixed 64-row pool with 16 rows each of (8 000 μ-law), (16 000 s16), (48 000 s16) and (the voice's rate, s16) against four
           uniform 16-row pools of those formats stepped round robin. A round is one step of the mixed pool, or one step of each of the
           four; the two arrangements alternate round by round.
  uniform  (b) a mixed 64-row pool whose rows all carry (8 000 μ-law) against the uniform pool of that format (stream_set_rate(8000) +
           stream_next_batch_g711), alternating step by step: the cost of the per-row dispatch.
  pcm      the 64-row uniform PCM pool step at the voice's rate (stream_next_batch_pcm16) alone: the figure compared between two builds.
           It uses nothing of the mixed interface, so it runs on a build without it.

Every leg runs `--warmup` untimed rounds, then `--reps` timed ones per arrangement, and the whole leg `--runs` times: the spread of an
arrangement is max − min of its medians over the runs. Needs the GPU: there is no fallback.

Writes <out>/<name>.json (default stream_mixed.json); legs already in the file that this call does not measure stay in it.

    timeout -k 10 300 python tools/probe/stream_mixed_probe.py --legs mix,uniform,pcm
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

MIX = [(8000, "mulaw"), (16000, "s16"), (48000, "s16"), (0, "s16")]


def session(i):
    f = 1 + i % 8
    return (kd.FIXTURE_IDS * f, [3] * (14 * f), None, {"noise_mode": "device", "seed": 1000 + i})


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


class Filler:
    """keeps a pool full with the session sequence; formats(row count) → the formats of a join, or None"""

    def __init__(self, pool, formats=None):
        self.pool, self.formats, self.nxt = pool, formats, 0

    def fill(self):
        free = self.pool.free_rows
        if free:
            sess = [session(self.nxt + j) for j in range(free)]
            self.pool.join(sess, 0.667, **({"formats": self.formats(self.nxt, free)} if self.formats else {}))
            self.nxt += free


def uniform_step(rt, slot, enc, buf, got):
    """the matching step call of a uniform pool"""
    lib, v = rt.lib, rt.voice
    if enc == "s16":
        ph._check(lib.piper_hip_voice_stream_next_batch_pcm16(v, slot, None, buf.ctypes.data_as(ph.c_i16p), buf.size // 2, got))
    else:
        ph._check(lib.piper_hip_voice_stream_next_batch_g711(v, slot, None, ph._law(enc), buf.ctypes.data_as(ph.c_u8p), buf.size, got))


def mixed_step(rt, slot, buf, got, off):
    ph._check(rt.lib.piper_hip_voice_stream_next_batch_mixed(rt.voice, slot, buf.ctypes.data_as(ph.c_vp), buf.size, got, off))


def step_bytes(rt, rate, enc, rows, chunk):
    n = chunk * rt.cfg.hop if not rate else ph.resample_step_bound(rt.cfg.sample_rate, rate, chunk * rt.cfg.hop)
    return rows * ((n * (1 if enc != "s16" else 2) + 3) & ~3)


def mix_leg(rt, chunk, warmup, reps):
    """(a): rows 16k … 16k + 15 of the mixed pool carry MIX[k]; uniform pool k holds the same sessions' share of the sequence"""
    fmts = [ph.stream_format(rate=r, encoding=e) for r, e in MIX]
    mixed = Filler(rt.stream_pool(0, 64, chunkFrames=chunk, work_slot=1, mixed=True))
    # a free row keeps its place in the pool, so a join's formats follow the rows it takes: row r carries MIX[r // 16]
    mixed.formats = lambda nxt, free: [fmts[r // 16] for r in free_rows(mixed.pool)][:free]
    uni = [Filler(rt.stream_pool(2 + 2 * k, 16, chunkFrames=chunk, work_slot=3 + 2 * k, rate=r or None)) for k, (r, e) in enumerate(MIX)]
    mbuf = np.empty(sum(step_bytes(rt, r, e, 16, chunk) for r, e in MIX), np.uint8)
    ubuf = [np.empty(step_bytes(rt, r, e, 16, chunk), np.uint8) for r, e in MIX]
    got64, off64, got16 = (C.c_int64 * 64)(), (C.c_int64 * 64)(), (C.c_int64 * 16)()
    times = {"mixed_ms": [], "four_pools_ms": []}
    for k in range(warmup + reps):
        mixed.fill()
        t0 = time.perf_counter()
        mixed_step(rt, 0, mbuf, got64, off64)
        t1 = time.perf_counter()
        for f in uni:
            f.fill()
        t2 = time.perf_counter()
        for j, (r, e) in enumerate(MIX):
            uniform_step(rt, 2 + 2 * j, e, ubuf[j], got16)
        t3 = time.perf_counter()
        if k >= warmup:
            times["mixed_ms"].append((t1 - t0) * 1e3)
            times["four_pools_ms"].append((t3 - t2) * 1e3)
    for f in [mixed] + uni:
        f.pool.close()
    return {k: med(t) for k, t in times.items()}


def free_rows(pool):
    """the rows the next join takes, lowest first (a row is free when stream_item_format refuses it)"""
    fmt = ph.StreamFormat()
    return [r for r in range(pool.capacity)
            if pool.rt.lib.piper_hip_voice_stream_item_format(pool.rt.voice, pool.slot, r, C.byref(fmt)) != 0]


def uniform_leg(rt, chunk, warmup, reps):
    """(b): the same format in every row, mixed pool against uniform pool"""
    f = ph.stream_format(rate=8000, encoding="mulaw")
    mixed = Filler(rt.stream_pool(0, 64, chunkFrames=chunk, work_slot=1, mixed=True), lambda nxt, free: [f] * free)
    uni = Filler(rt.stream_pool(2, 64, chunkFrames=chunk, work_slot=3, rate=8000))
    buf = np.empty(step_bytes(rt, 8000, "mulaw", 64, chunk), np.uint8)
    got, off = (C.c_int64 * 64)(), (C.c_int64 * 64)()
    times = {"mixed_ms": [], "uniform_ms": []}
    for k in range(warmup + reps):
        mixed.fill()
        t0 = time.perf_counter()
        mixed_step(rt, 0, buf, got, off)
        t1 = time.perf_counter()
        uni.fill()
        t2 = time.perf_counter()
        uniform_step(rt, 2, "mulaw", buf, got)
        t3 = time.perf_counter()
        if k >= warmup:
            times["mixed_ms"].append((t1 - t0) * 1e3)
            times["uniform_ms"].append((t3 - t2) * 1e3)
    mixed.pool.close()
    uni.pool.close()
    return {k: med(t) for k, t in times.items()}


def pcm_leg(rt, chunk, warmup, reps):
    pool = Filler(rt.stream_pool(2, 64, chunkFrames=chunk, work_slot=3))
    buf, got, times = np.empty(64 * chunk * rt.cfg.hop * 2, np.uint8), (C.c_int64 * 64)(), []
    for k in range(warmup + reps):
        pool.fill()
        t0 = time.perf_counter()
        uniform_step(rt, 2, "s16", buf, got)
        t1 = time.perf_counter()
        if k >= warmup:
            times.append((t1 - t0) * 1e3)
    pool.pool.close()
    return {"pcm_pool_ms": med(times)}


def summarise(runs):
    out = {"runs": runs}
    for k in runs[0]:
        vals = [r[k] for r in runs]
        out[k] = med(vals)
        out[k + "_spread"] = round(max(vals) - min(vals), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="mix,uniform,pcm")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--name", default="stream_mixed")
    args = ap.parse_args()
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    rt.set_plan_cache(256, 96 << 30)
    path = os.path.join(args.out, args.name + ".json")
    out = {"probe": "stream_mixed", "voice": "medium", "chunk_frames": args.chunk, "factors": "1..8 cycled", "warmup": args.warmup,
           "reps": args.reps, "runs": args.runs, "mix_formats": ["%d %s" % (r or cfg.sample_rate, e) for r, e in MIX]}
    if os.path.exists(path):
        old = json.load(open(path))
        if all(old.get(k) == out[k] for k in ("chunk_frames", "warmup", "reps", "runs")):
            out.update({k: old[k] for k in ("mix", "uniform", "pcm") if k in old})
    legs = {"mix": mix_leg, "uniform": uniform_leg, "pcm": pcm_leg}
    for name in [x for x in args.legs.split(",") if x]:
        out[name] = summarise([legs[name](rt, args.chunk, args.warmup, args.reps) for _ in range(args.runs)])
        print(json.dumps({k: w for k, w in out[name].items() if k != "runs"}), file=sys.stderr, flush=True)
    if "mix" in out:
        m = out["mix"]
        m["four_minus_mixed_ms"] = round(m["four_pools_ms"] - m["mixed_ms"], 4)
        m["gain_beyond_spread"] = bool(m["four_minus_mixed_ms"] > m["four_pools_ms_spread"])
    if "uniform" in out:
        u = out["uniform"]
        u["mixed_over_uniform"] = round(u["mixed_ms"] / u["uniform_ms"], 4)
    rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: ({a: b for a, b in w.items() if a != "runs"} if isinstance(w, dict) else w) for k, w in out.items()}))


if __name__ == "__main__":
    main()
