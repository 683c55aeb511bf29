"""The kernels, the runtime calls and the plan bytes of a slot id's way through every staging route, for holding two builds of the library
against each other under a trace (rocprofv3 --kernel-trace --stats -- python tools/probe/staging_calls.py, and in a run of its own
rocprofv3 --hip-trace --stats -- python …): the kernel name → count maps, the HIP API name → count maps of the allocation, copy, event and
launch calls, and the cached_bytes this script prints must be equal.

The sequence is the one of tests/test_gpu_staging.py::test_one_slot_id_through_every_staging_route, run ONCE and without the fresh
runtimes it compares against: on the medium voice prepare_batch (n = 1), predict_durations, prepare_batch (n = 3, ragged, prosody, volume,
pitch), prepare_batch_bounded (fit, volume, pitch), a batched stream with a volume, prepare_batch (n = 1) again, all on one slot id; then
the middle three on a voice with a speaker table. Each whole-item step is launched and collected as the test does.

With --lib-root the package and library of another tree are used (the parent commit's). Needs the GPU: there is no fallback. Prints one
JSON object; --out writes it to that file too."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-root", default=None, help="another tree (the parent commit's): its package and library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.lib_root or ROOT, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import piper_hip as ph
    import test_gpu_staging as tg
    backend = ph.HipBackend(0)
    cfg = ph.voice_config("medium")
    voice = (cfg, ph.synthetic_blob(cfg, 1234))
    out = {"tree": "parent" if a.lib_root else "this", "steps": []}
    for speakers, route in ((False, tg.ROUTE), (True, tg.ROUTE[1:4])):
        rt = tg.make(backend, voice, speakers)
        for name, step in route:
            got = step(rt, speakers)
            sizes = {k: int(x.size) for k, x in got.items() if hasattr(x, "size")}
            out["steps"].append({"voice": "speaker-table" if speakers else "plain", "step": name, "sizes": sizes,
                                 "cached_bytes": int(rt.plan_info(tg.SLOT)["cached_bytes"])})
        rt.close()
    backend.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
