"""What profiles/prosody.md reports: the _prosody steps against the plain ones in one process, and ids -> audio of the
bounded route with and without a neutral prosody. Headline shape: medium voice, factor 8, one item."""
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

backend = ph.HipBackend(0)
cfg = ph.voice_config("medium")
rt = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
ids = list(kd.FIXTURE_IDS) * 8
t = len(ids)
nz = kd.sym(77, (2, t), 1.7320508)
kw = dict(dp_noise=nz, noise_mode="device", seed=1234)
neutral = dict(length=np.ones(t, np.float32), min_frames=np.zeros(t, np.int32), max_frames=np.zeros(t, np.int32), noise=np.ones(t, np.float32))
out = {}

# the two steps that have a _prosody variant, plain and with prosody: the expansion in the slot's plan, the predictor's last step in the
# predictor plan the slot's prepare ran ("predict:")
rt.prepare(1, ids, None, None, 0.667, **kw)
rt.launch(1); rt.collect(1)
F = int(rt.durations(1).sum())
rt.prepare(2, ids, None, None, 0.667, prosody=neutral, **kw)
rt.launch(2); rt.collect(2)
sub = {"expand_noise": [], "expand_noise_prosody": [], "dp.affine_exp_ceil": [], "dp.affine_exp_ceil_prosody": []}
for rep in range(7):
    sub["expand_noise"].append(rt.time_subset(1, "dp.affine_exp_ceil|expand_noise", 400)[:2])
    sub["expand_noise_prosody"].append(rt.time_subset(2, "dp.affine_exp_ceil_prosody|expand_noise_prosody", 400)[:2])
    sub["dp.affine_exp_ceil"].append(rt.time_subset(1, "predict:dp.affine_exp_ceil|expand_noise", 400)[:2])
    sub["dp.affine_exp_ceil_prosody"].append(rt.time_subset(2, "predict:dp.affine_exp_ceil_prosody|expand_noise_prosody", 400)[:2])
out["frames"] = F
out["time_subset_us"] = {k: dict(launches=v[0][1], runs=[round(x[0], 3) for x in v]) for k, v in sub.items()}

# ids -> audio, bounded route, wall clock
bound = F + 16
pairs = [(ids, nz)]


def one(prosody):
    t0 = time.perf_counter()
    rt.prepare_batch_bounded(3, pairs, bound, noise_mode="device", seed=1234, prosody=prosody)
    rt.launch(3)
    rt.collect(3)
    return (time.perf_counter() - t0) * 1e3


for p in (None, [neutral]):  # warm both sets of plans and their graphs
    for _ in range(5):
        one(p)
wall = {"plain": [], "prosody": []}
for rep in range(7):
    for name, p in (("plain", None), ("prosody", [neutral])):
        xs = sorted(one(p) for _ in range(60))
        wall[name].append(round(xs[len(xs) // 2], 4))
out["bounded_ids_to_audio_ms_median_of_60"] = wall
print(json.dumps(out))
rt.close()
backend.close()
