"""The three generator precisions side by side: launch → samples on the host for f32, bf16 and bf16x3 (split bf16, include/piper_hip.h
PIPER_HIP_PRECISION_BF16X3) on the same utterance, in one process.

Per voice (medium, high) three runtimes on one backend, one per precision; per factor (8, 64) the fixture utterance tiled by `factor`
(F = 42 · factor frames, 3 frames per id, injected noise) is prepared once on each and then replayed: launch, collect into a pageable buffer,
host clock around both (collect waits for the slot's stream). The precisions are interleaved replay by replay, `--warmup` untimed rounds, then
`--reps` timed ones, and the whole leg `--runs` times: a cell is the median of the runs' medians, its spread max − min of them. The waveform
RMS error of each precision against the fp32 result of the same process is printed next to the times (the oracle comparison is the test's,
tests/test_gpu_bf16x3.py). Needs the GPU: there is no fallback.

`--precisions` picks the list that runs interleaved (f32 first: the rms baseline) and `--name` the files: `--precisions f32,bf16,bf16x3,f16
--name f16` is profiles/f16.md, the fp16 precision (PIPER_HIP_PRECISION_F16) beside the other three in one process.

Writes <out>/<name>.json and the table of <out>/<name>.md (everything from a "## Notes" heading on is kept)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PRECISIONS = ("f32", "bf16", "bf16x3")


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def leg(ph, rts, n, warmup, reps):
    PRECISIONS = tuple(rts)
    """median ms per precision of launch → collect on slot 0 (prepared by the caller), interleaved"""
    buf = np.empty(n, np.float32)
    times = {p: [] for p in PRECISIONS}
    for k in range(warmup + reps):
        for p in PRECISIONS:
            rt = rts[p]
            t0 = time.perf_counter()
            ph._check(rt.lib.piper_hip_voice_launch(rt.voice, 0))
            ph._check(rt.lib.piper_hip_voice_collect(rt.voice, 0, buf.ctypes.data_as(ph.c_f32p), n))
            t1 = time.perf_counter()
            if k >= warmup:
                times[p].append((t1 - t0) * 1e3)
    return {p: med(t) for p, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", default="medium,high")
    ap.add_argument("--factors", default="8,64")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--precisions", default=",".join(PRECISIONS))
    ap.add_argument("--name", default="bf16x3")
    args = ap.parse_args()
    precisions = tuple(p for p in args.precisions.split(",") if p)
    if precisions[0] != "f32":
        ap.error("--precisions starts with f32 (the rms baseline)")
    last = precisions[-1]
    sys.path.insert(0, os.path.join(ROOT, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import katdata as kd
    import piper_hip as ph
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    out = {"probe": args.name, "precisions": list(precisions), "warmup": args.warmup, "reps": args.reps, "runs": args.runs, "legs": []}
    for quality in [q for q in args.voices.split(",") if q]:
        cfg = ph.voice_config(quality)
        blob = ph.synthetic_blob(cfg, 1234)
        rts = {}
        for p in precisions:
            rts[p] = ph.HipRuntime(backend, cfg, blob)
            rts[p].set_precision(p)
        for factor in [int(f) for f in args.factors.split(",") if f]:
            ids = kd.FIXTURE_IDS * factor
            dur = [3] * len(ids)
            noise = kd.sym(4321 + factor, (cfg.inter, sum(dur)), 1.7320508)
            wave = {}
            for p in precisions:
                rts[p].prepare(0, ids, dur, noise, 0.667)
                rts[p].launch(0)
                wave[p] = rts[p].collect(0).astype(np.float64)
            n = wave["f32"].size
            runs = [leg(ph, rts, n, args.warmup, args.reps) for _ in range(args.runs)]
            r = {"voice": quality, "factor": factor, "samples": int(n), "runs": runs}
            for p in precisions:
                vals = [x[p] for x in runs]
                r[p] = med(vals)
                r[p + "_spread"] = round(max(vals) - min(vals), 4)
                r[p + "_rms_vs_f32"] = float(np.sqrt(np.mean((wave[p] - wave["f32"]) ** 2)))
            out["legs"].append(r)
            print(json.dumps({k: w for k, w in r.items() if k != "runs"}), file=sys.stderr, flush=True)
        for rt in rts.values():
            rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.name + ".json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    title = "# Split bf16 (PIPER_HIP_PRECISION_BF16X3) against f32 and bf16" if last == "bf16x3" else f"# {last} against " + ", ".join(precisions[:-1])
    lines = [title, "",
             f"One launch → samples on the host (pageable), median ms over {args.reps} replays per precision, the {len(precisions)} interleaved, after "
             f"{args.warmup} untimed rounds; ± = max − min of the medians of {args.runs} runs of the leg (`tools/probe/bf16x3_probe.py`; raw figures "
             f"in `{args.name}.json`). rms = RMS difference of the waveform from the f32 waveform of the same process.", "",
             "| voice | factor | samples | " + " | ".join(p + " ms" for p in precisions) + f" | {last} / f32 | " + " | ".join(p + " rms" for p in precisions[1:]) + " |",
             "|" + "---|" * (4 + 2 * len(precisions) - 1)]
    for r in out["legs"]:
        cell = lambda k: f"{r[k]} ± {r[k + '_spread']}"  # noqa: E731
        lines.append(f"| {r['voice']} | {r['factor']} | {r['samples']} | " + " | ".join(cell(p) for p in precisions) + f" | {r[last] / r['f32']:.3f} | " +
                     " | ".join(f"{r[p + '_rms_vs_f32']:.3e}" for p in precisions[1:]) + " |")
    md = os.path.join(args.out, args.name + ".md")
    notes = ""
    if os.path.exists(md):
        old = open(md).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    with open(md, "w") as fh:
        fh.write("\n".join(lines) + "\n" + notes)


if __name__ == "__main__":
    main()
