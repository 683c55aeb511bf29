"""The launches and the plan bytes of the whole-item output chain, for holding two builds of the library against each other under a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/probe/chain_launches.py): the kernel names and call counts of the two
traces must be equal, and so must the cached_bytes this script prints.

Medium voice, the batch of tests/test_gpu_pitch.py (3 items of 40, 14 and 23 ids at 3 frames per id) with a per-id volume and the
pitches +3, 0 and −5 semitones: ONE prepare_batch and ONE launch, then every sink (f32, s16, s16 at 8 kHz, s16 at 48 kHz with gain
0.5, μ-law at 8 kHz) collected in three phases:

  none       no stage on the slot id: the shaped, pitched items
  all        EQ, loudness target, level and join (gap and trim on)
  normalize  EQ and join only, the PCM sinks with normalize = 1 (the float sink has none)

With --lib-root the package and library of another tree are used (the parent commit's). Needs the GPU: there is no fallback. Prints one
JSON object; --out writes it to that file too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SLOT = 5
SHIFTS = [(3.0, 0), (0.0, 0), (-5.0, 0)]
EQ = [("highpass", 120.0, 0.707), ("peaking", 3000.0, 1.0, 6.0)]
JOIN = dict(lead_ms=1.5, gap_ms=20.0, tail_ms=3.0, trim=1, trim_threshold=0.01, trim_pad_ms=2.0, fade_ms=3.0)
SINKS = [("f32", None, 1.0), ("s16", None, 1.0), ("s16", 8000, 1.0), ("s16", 48000, 0.5), ("mulaw", 8000, 1.0)]


def collect_all(rt, normalize):
    sizes = []
    for enc, rate, gain in SINKS:
        if enc == "f32":
            got = rt.collect(SLOT)
        elif enc == "s16":
            got = rt.collect_pcm16(SLOT, gain=gain, rate=rate, normalize=normalize)
        else:
            got = rt.collect_g711(SLOT, enc, gain=gain, rate=rate, normalize=normalize)
        sizes.append(int(got.size))
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-root", default=None, help="another tree (the parent commit's): its package and library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.lib_root or ROOT, "piper-swift_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import katdata as kd
    import piper_hip as ph
    backend = ph.HipBackend(0)
    cfg = ph.voice_config("medium")
    rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    items = [((kd.FIXTURE_IDS * 4)[:n], [3] * n, kd.sym(900 + k, (cfg.inter, 3 * n), 1.7320508)) for k, n in enumerate((40, 14, 23))]
    vols = [np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], np.float32), len(it[0])) for it in items]
    rt.prepare_batch(SLOT, items, 0.667, volume=vols, pitch=SHIFTS)
    out = {"tree": "parent" if a.lib_root else "this", "phases": {}}
    out["phases"]["prepared"] = {"cached_bytes": int(rt.plan_info(SLOT)["cached_bytes"])}
    rt.launch(SLOT)
    phases = (("none", dict(eq=None, loudness=None, level=None, join=None), False),
              ("all", dict(eq=EQ, loudness=(-16.0, 0.0), level=(3.0, 0.5, 50.0), join=JOIN), False),
              ("normalize", dict(eq=EQ, loudness=None, level=None, join=JOIN), True))
    for name, st, normalize in phases:
        rt.slot_eq(SLOT, st["eq"])
        rt.slot_loudness(SLOT, st["loudness"])
        rt.slot_level(SLOT, st["level"])
        rt.slot_join(SLOT, st["join"])
        out["phases"][name] = {"samples": collect_all(rt, normalize), "cached_bytes": int(rt.plan_info(SLOT)["cached_bytes"])}
    rt.close()
    backend.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
