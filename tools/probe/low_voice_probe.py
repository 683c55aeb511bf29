"""x_low against medium on the same ids, in one process: ms per utterance and the per-step table.

Both voices are synthetic (seed 1234). The utterance is the bench's: the 14 fixture ids tiled `factor` times, 3 frames per id, device
noise. Per factor (1 and 8) both voices are prepared once on their own runtime; then, interleaved repetition by repetition (medium,
x_low, medium, …), launch → collect into a pageable buffer is timed on the host. `--warmup` untimed rounds, `--reps` timed ones, the leg
`--runs` times: a figure is the median of the runs' medians, its spread max − min of them. x_low does strictly less encoder and flow
work and the same generator work, so the expectation is  x_low ≤ medium + spread of medium;  the JSON says whether it held.

The per-step table comes from piper_hip_voice_profile (median of `--profile-runs` calls of `--profile-iters` replays each) on the same
prepared slots: step name, the kernel the dispatch rules give it at these shapes (kernel_of), µs for x_low, and the medium step that
does the same work with its kernel and µs. Generator steps are summed into one row per stage (the same kernels on the same shapes for
both voices).

Writes <out>/x_low.json and the tables of <out>/x_low.md (everything from a "## Notes" heading on is kept; --render-only rewrites the
tables from the JSON). Needs the GPU: there is no fallback.

    timeout -k 10 300 python tools/probe/low_voice_probe.py
"""
import argparse
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

VOICES = ("medium", "x_low")


def med(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def timed_leg(rts, bufs, slot, warmup, reps):
    t = {q: [] for q in VOICES}
    for k in range(warmup + reps):
        for q in VOICES:
            rt, buf = rts[q], bufs[q]
            t0 = time.perf_counter()
            ph._check(rt.lib.piper_hip_voice_launch(rt.voice, slot))
            ph._check(rt.lib.piper_hip_voice_collect(rt.voice, slot, buf.ctypes.data_as(ph.c_f32p), buf.size))
            t1 = time.perf_counter()
            if k >= warmup:
                t[q].append((t1 - t0) * 1e3)
    return {q: med(v) for q, v in t.items()}


def step_table(rt, slot, iters, runs):
    """[(step, µs)] in schedule order; generator steps ("dec.…") folded into one row per stage prefix."""
    per = {}
    order = []
    for _ in range(runs):
        for s in rt.profile(slot, iters=iters, max_entries=1024):
            name = s["name"]
            if name.startswith("("):
                continue
            if name.startswith("dec."):
                parts = name.split(".")
                name = ".".join(parts[:2]) + (".*" if len(parts) > 2 else "")
            if name not in per:
                per[name] = []
                order.append(name)
            per[name].append(s["avg_us"])
    out = []
    for name in order:
        v = np.asarray(per[name], np.float64)
        n = len(v) // runs  # folded rows: launches per run
        out.append((name, round(float(np.median(v.reshape(runs, n).sum(axis=1))), 2)))
    return out


def kernel_of(step, hidden):
    """The kernel a front step takes at the probe's shapes (one utterance of at most 112 ids / 336 frames: every launch is "few tiles"),
    restated from the dispatch rules of csrc/conv.hip launch_conv_mfma, conv_lean.hip, conv_short.hip, attention.hip and voice.hip.
    hidden = 192: LayerNorm statistics in the consumer (ln_self), folded coupling tails, 8-row FFN conv; hidden = 96: none of the three."""
    wide = hidden == 192
    last = step.rsplit(".", 1)[-1]
    if step.startswith("dec."):
        return "generator (same kernels for both voices)"
    if last == "rel_attention":
        return f"rel_attention_lds_kernel<{hidden // 2}>"
    if "res_skip_post_sub" in step:
        return "conv_k1_tail_kernel (folded tail)"
    if "post_sub_flip_pre" in step:
        return "flow_seam_kernel"
    if last == "in_gate":
        return "conv_gate_kernel<5, 6>" if wide else "conv_short_kernel (gated k 5)"
    if last in ("qkv", "res_skip", "post_sub", "o_add") or (last == "pre" and wide):
        return f"conv_k1_kernel<{hidden // 32}>"
    if last == "pre":
        return "conv_stream_kernel<1> (48 input channels)"
    if last in ("ln2_qkv", "ln2_proj"):
        return "conv_k1_ln_kernel<6>" if wide else "conv_stream_kernel<1, PRO_LN>"
    if last == "ln1_ffn1_relu":
        return "conv_k3_ln_kernel<6>" if wide else "conv_short_kernel (k 3, PRO_LN)"
    if last == "ffn2_add":
        return "conv_k3_r8_kernel<24>"
    if last in ("o_add_stats", "ffn2_add_stats"):
        return "conv_stream_kernel (stats_out)"
    return {"embed": "embed_kernel", "expand_noise": "expand_noise_kernel"}.get(last, "")


def counterpart(step, medium):
    """The medium step that does an x_low step's work: the statistics variants map to the ln_self ones, a coupling's last res_skip conv
    to the folded tail that contains it (its seam / post_sub row then shows "↑": the same medium launch)."""
    if step in medium:
        return step
    if step.endswith("_stats") and step[:-6] in medium:
        return step[:-6]
    if step.endswith(".res_skip"):
        hit = [m for m in medium if m.startswith(step + "_")]
        return hit[0] if hit else None
    if ".post_sub" in step:
        return "↑"
    return None


def render(out, out_dir):
    lines = ["# x_low against medium", "",
             f"Synthetic voices, the 14 fixture ids tiled, 3 frames per id, device noise (`tools/probe/low_voice_probe.py`; raw figures in "
             f"`x_low.json`). ms per utterance = launch → collect on the host, the two voices interleaved in one process: median of {out['runs']} runs "
             f"of {out['reps']} repetitions after {out['warmup']} untimed ones, ± = max − min of the runs' medians.", "",
             "| factor | ids | frames | medium ms | x_low ms | x_low − medium | x_low ≤ medium + ± of medium |", "|---|---|---|---|---|---|---|"]
    for r in out["factors"]:
        lines.append(f"| {r['factor']} | {r['ids']} | {r['frames']} | {r['medium_ms']} ± {r['medium_ms_spread']} | {r['x_low_ms']} ± {r['x_low_ms_spread']} | "
                     f"{r['x_low_minus_medium_ms']} | {'yes' if r['x_low_within_expectation'] else 'NO'} |")
    for r in out["factors"]:
        med_steps = {s["step"]: s for s in r["steps"]["medium"]}
        lines += ["", f"## Steps at factor {r['factor']}", "",
                  f"piper_hip_voice_profile, median of {out['profile_runs']} calls of {out['profile_iters']} replays, in x_low's schedule order; the generator's "
                  "launches are summed per stage. Beside each x_low step the medium step that does the same work: `o_add` / `ffn2_add` for the "
                  "`_stats` variants, and the folded tail of a coupling for its last `res_skip` conv — the seam (or the last `post_sub`) in the row "
                  "below is part of that same medium launch (↑).", "",
                  "| step | x_low kernel | x_low µs | medium step | medium kernel | medium µs |", "|---|---|---|---|---|---|"]
        for s in r["steps"]["x_low"]:
            c = counterpart(s["step"], med_steps)
            m = med_steps.get(c)
            lines.append(f"| {s['step']} | {s['kernel']} | {s['us']} | {'' if c is None else 'same' if c == s['step'] else c} | {m['kernel'] if m else ''} | {m['us'] if m else ''} |")
        lines.append(f"| **sum of the steps** | | {r['step_sum_us']['x_low']} | | | {r['step_sum_us']['medium']} |")
    md = os.path.join(out_dir, "x_low.md")
    notes = ""
    if os.path.exists(md):
        old = open(md).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    with open(md, "w") as fh:
        fh.write("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="1,8")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--profile-iters", type=int, default=20)
    ap.add_argument("--profile-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--render-only", action="store_true", help="rewrite x_low.md from the x_low.json already in --out (no GPU needed)")
    args = ap.parse_args()
    if args.render_only:
        render(json.load(open(os.path.join(args.out, "x_low.json"))), args.out)
        return
    backend = ph.HipBackend(0)  # DeviceUnavailable without the library or the GPU: no fallback
    rts = {}
    for q in VOICES:
        cfg = ph.voice_config(q)
        rts[q] = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    out = {"probe": "low_voice", "voices": list(VOICES), "warmup": args.warmup, "reps": args.reps, "runs": args.runs,
           "profile_iters": args.profile_iters, "profile_runs": args.profile_runs, "factors": []}
    tables = {}
    for slot, f in enumerate(int(x) for x in args.factors.split(",") if x):
        ids = kd.FIXTURE_IDS * f
        bufs = {}
        for q in VOICES:
            rts[q].prepare(slot, ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234)
            bufs[q] = np.empty(rts[q]._keep[slot][1], np.float32)
        runs = [timed_leg(rts, bufs, slot, args.warmup, args.reps) for _ in range(args.runs)]
        r = {"factor": f, "ids": len(ids), "frames": 3 * len(ids), "runs": runs}
        for q in VOICES:
            vals = [x[q] for x in runs]
            r[q + "_ms"] = med(vals)
            r[q + "_ms_spread"] = round(max(vals) - min(vals), 4)
        r["x_low_minus_medium_ms"] = round(r["x_low_ms"] - r["medium_ms"], 4)
        r["x_low_within_expectation"] = bool(r["x_low_ms"] <= r["medium_ms"] + r["medium_ms_spread"])
        steps = {q: step_table(rts[q], slot, args.profile_iters, args.profile_runs) for q in VOICES}
        r["steps"] = {q: [{"step": n, "kernel": kernel_of(n, rts[q].cfg.hidden), "us": us} for n, us in steps[q]] for q in VOICES}
        r["step_sum_us"] = {q: round(sum(us for _, us in steps[q]), 1) for q in VOICES}
        tables[f] = steps
        out["factors"].append(r)
        print(json.dumps({k: w for k, w in r.items() if k not in ("runs", "steps")}), file=sys.stderr, flush=True)
    for rt in rts.values():
        rt.close()
    backend.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "x_low.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    render(out, args.out)
    print(json.dumps({k: w for k, w in out.items() if k != "factors"}))


if __name__ == "__main__":
    main()
