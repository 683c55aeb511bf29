#!/usr/bin/env python3
"""The production ledger of conv kernel variants (profiles/conv_routes.md).

  conv_routes.py run [--out conv_routes.json] [--voices medium/f32,…]   on the MI355X: per voice, every workload of
      tests/conv_route_plans.py on a fresh runtime of an ARMED backend (prepare + launch once: milliseconds, no reference), then the
      witness ladder F × N. Writes {voice: {"workloads": {name: {variant: [steps]}}, "ladder": {"F,N": {variant: [steps]}}}, "cus": n}.
  conv_routes.py table conv_routes.json                                  anywhere: writes tests/conv_routes_table.py from it — per voice
      variant → workloads, and per variant its witness: the cheapest ladder plan (N · F, then N) whose routes hold it, else the cheapest
      workload (marked as a production shape).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "piper-swift_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

# cheapest first: what a production-shape witness costs to check
WORKLOAD_COST = ("single_f1", "predictor", "ragged_84_5_61_1", "stream_chunk20", "single_f8", "bounded", "pool_16", "batch_20x84", "batch_4x336",
                 "batch_8x336", "pool_64", "single_f64")


def run(out_path, only):
    import conv_route_plans as rp
    import piper_hip as ph
    res = {"voices": {}, "cus": None, "errors": []}
    backend = ph.HipBackend(0)
    backend.arm_routes(True)
    try:
        for quality, prec in rp.VOICES:
            key = rp.voice_key(quality, prec)
            if only and key not in only:
                continue
            cfg = ph.voice_config(quality)
            blob = ph.synthetic_blob(cfg, 1234)
            v = res["voices"][key] = {"workloads": {}, "ladder": {}}

            def fresh():
                rt = ph.HipRuntime(backend, cfg, blob)
                if prec == "bf16":
                    rt.set_precision("bf16")
                return rt

            for name in rp.WORKLOADS:
                rt = fresh()
                t0 = time.time()
                try:
                    v["workloads"][name] = rp.run_workload(rt, name)
                    res["cus"] = rp.SEEN_CUS
                except (ph.ExecutionError, AssertionError) as e:  # reported, not hidden: the table is not written from a run with errors
                    res["errors"].append(f"{key} {name}: {type(e).__name__}: {e}")
                finally:
                    rt.close()
                print(f"{key} {name}: {len(v['workloads'].get(name, {}))} variants, {time.time() - t0:.2f} s", flush=True)
            rt = fresh()
            try:
                for N in rp.LADDER_N:
                    for F in rp.LADDER_F:
                        try:
                            v["ladder"][f"{F},{N}"] = rp.run_ladder_plan(rt, F, N)
                        except (ph.ExecutionError, AssertionError) as e:
                            res["errors"].append(f"{key} ladder {N}x{F}: {type(e).__name__}: {e}")
            finally:
                rt.close()
            print(f"{key} ladder: {len(v['ladder'])} plans", flush=True)
            with open(out_path, "w") as f:  # after every voice: a later failure keeps what was measured
                json.dump(res, f, indent=1, sort_keys=True)
    finally:
        backend.close()
    for e in res["errors"]:
        print("ERROR " + e)
    return 1 if res["errors"] else 0


def table(json_path):
    res = json.load(open(json_path))
    assert not res["errors"], res["errors"]
    lines = ['"""Production ledger of conv kernel variants — WRITTEN BY tools/probe/conv_routes.py (run, then table); do not edit by hand.',
             "", "TABLE[voice][variant] = the workloads of tests/conv_route_plans.py whose plans launch the variant (shapes dropped), on NUM_CUS CUs.",
             'WITNESS[voice][variant] = ("ladder", F, N): the cheapest plan of the witness ladder whose routes hold the variant, or',
             '("production", workload): no ladder plan reaches it, its cheapest production shape stands in. profiles/conv_routes.md has the prose."""',
             f"NUM_CUS = {res['cus']}", "", "TABLE = {"]
    wit_lines = ["WITNESS = {"]
    for key in sorted(res["voices"]):
        v = res["voices"][key]
        uses = {}
        for name, vs in v["workloads"].items():
            for var in vs:
                uses.setdefault(var, []).append(name)
        lines.append(f"    {key!r}: {{")
        wit_lines.append(f"    {key!r}: {{")
        plans = sorted(((int(k.split(",")[1]) * int(k.split(",")[0]), int(k.split(",")[1]), int(k.split(",")[0])) for k in v["ladder"]))
        for var in sorted(uses):
            ws = sorted(uses[var], key=WORKLOAD_COST.index)
            lines.append(f"        {var!r}: {ws!r},")
            w = next((("ladder", F, N) for _, N, F in plans if var in v["ladder"][f"{F},{N}"]), None) or ("production", ws[0])
            wit_lines.append(f"        {var!r}: {w!r},")
        lines.append("    },")
        wit_lines.append("    },")
    text = "\n".join(lines + ["}", ""] + wit_lines + ["}", ""])
    with open(os.path.join(ROOT, "tests", "conv_routes_table.py"), "w") as f:
        f.write(text)
    print(f"tests/conv_routes_table.py: {sum(len(v['workloads']) for v in res['voices'].values())} workloads, {text.count(chr(10))} lines")
    return 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["run"]:
        out = a[a.index("--out") + 1] if "--out" in a else "conv_routes.json"
        only = a[a.index("--voices") + 1].split(",") if "--voices" in a else None
        sys.exit(run(out, only))
    if a[:1] == ["table"] and len(a) == 2:
        sys.exit(table(a[1]))
    sys.exit(__doc__)
