"""The kernels, the runtime calls and the bytes of one slot id's streams, for holding two builds of the library against each other under a
trace (rocprofv3 --kernel-trace --stats -- python tools/probe/stream_buffers.py, and in a run of its own rocprofv3 --hip-trace --stats --
python …): the kernel name → count maps, the HIP API name → count maps of the copy, launch, event and wait calls, and the cached_bytes
and memory_stats this script prints must be equal.

The sequence is the one of tests/test_gpu_stream_buffers.py, run ONCE and without the fresh runtimes it compares against: on the medium
voice a single stream, then a group of 3, each at 2, 5 and 2 frames a chunk with a level, an EQ and a sink per pass, on one slot id; then
a mixed pool of 3 rows opened, run and closed at 2, 5 and 5 frames a chunk on that slot id.

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
    import test_gpu_stream_buffers as tb
    backend = ph.HipBackend(0)
    cfg = ph.voice_config("medium")
    rt = tb.make(backend, (cfg, ph.synthetic_blob(cfg, 1234)))
    out = {"tree": "parent" if a.lib_root else "this", "streams": [], "pools": []}
    for run, sinks in ((tb.single_stream, tb.SINGLE_SINKS), (tb.group_stream, tb.GROUP_SINKS)):
        for chunk, sink in zip(tb.CHUNKS, sinks):
            got = run(rt, chunk, sink)
            out["streams"].append({"stream": run.__name__, "chunk": chunk, "sizes": [int(g.size) for g in got],
                                   "cached_bytes": int(rt.plan_info(tb.SLOT)["cached_bytes"])})
    for chunk in (2, 5, 5):
        got = tb.pool_cycle(rt, chunk)
        out["pools"].append({"chunk": chunk, "sizes": [int(g.size) for g in got], "memory_stats": backend.memory_stats()})
    rt.close()
    backend.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
