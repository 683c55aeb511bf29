"""Timing of the speaker feature: the spk.rows step at N = 1 and N = 8 (piper_hip_voice_profile) and ids-to-audio at factor 8 for a
multi-speaker medium voice next to the single-speaker one. One JSON object on stdout (and into the file given as the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "piper-swift_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import piper_hip as ph  # noqa: E402

backend = ph.HipBackend(0)
cfg = ph.voice_config("medium")
blob = ph.synthetic_blob(cfg, 1234)
S, gin = 904, 512
scfg = ph.speaker_config(S, gin)
sblob = ph.synthetic_speaker_blob(cfg, scfg, 4321)
plain = ph.HipRuntime(backend, cfg, blob)
multi = ph.HipRuntime(backend, cfg, blob)
multi.attach_speakers(scfg, sblob)
ids, dur, noise = bench.utterance(8, 1234, cfg.inter)
out = {"workload": f"medium factor 8: {len(ids)} ids, {sum(dur)} frames", "S": S, "gin": gin}


def e2e(rt, reps=60):
    for _ in range(5):
        rt.prepare(0, ids, dur, noise, 0.667)
        rt.launch(0)
        rt.collect(0)
    wall, gpu = [], []
    for _ in range(reps):
        a = time.perf_counter()
        rt.prepare(0, ids, dur, noise, 0.667)
        rt.launch(0)
        rt.collect(0)
        wall.append((time.perf_counter() - a) * 1e3)
        gpu.append(rt.last_gpu_ms(0))
    return {"ids_to_audio_ms_median": round(float(np.median(wall)), 4), "ids_to_audio_ms_p10": round(float(np.percentile(wall, 10)), 4),
            "ids_to_audio_ms_p90": round(float(np.percentile(wall, 90)), 4), "gpu_ms_median": round(float(np.median(gpu)), 4)}


multi.slot_speakers(0, [17])
# interleaved A / B / A / B so that drift shows
out["single_1"] = e2e(plain)
out["multi_1"] = e2e(multi)
out["single_2"] = e2e(plain)
out["multi_2"] = e2e(multi)

rows_main = ph.speaker_row_floats(cfg) - cfg.hidden
out["weight_bytes_main"] = rows_main * gin * 4
out["read_once_us_at_6.3TBps"] = round(rows_main * gin * 4 / 6.3e12 * 1e6, 3)
for N in (1, 8):
    items = [bench.utterance(8, 700 + b, cfg.inter) for b in range(N)]
    multi.slot_speakers(2, [(7 * b) % S for b in range(N)])
    multi.prepare_batch(2, items)
    multi.launch(2)
    multi.collect(2)
    runs = []
    for _ in range(3):
        prof = multi.profile(2, iters=20)
        runs.append([p for p in prof if p["name"] == "spk.rows"][0]["avg_us"])
    total = sum(p["avg_us"] for p in prof)
    sub = multi.time_subset(2, "spk.rows", iters=200)
    out[f"spk_rows_N{N}"] = {"profile_median_us": [round(r, 3) for r in runs], "graph_replay_us": round(sub[0], 3), "schedule_sum_us": round(total, 1),
                             "launches": len(prof)}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
plain.close()
multi.close()
backend.close()
