"""The per-phoneme prosody contract of include/piper_hip.h ("Per-phoneme prosody") restated in numpy — TEST INFRASTRUCTURE.

From w0 = fl(expf(logw) · length_scale) on, the frame rule is one correctly rounded fp32 multiplication, ceil and integers, so `durations`
and `fit` are exact: a kernel or the host function either equals them or is wrong. `frame_ids` is generate_path (frame f belongs to the
smallest t with cum[t] > f; an all-zero result still yields one frame, of id 0). `frame_ns` is the per-frame noise scale
ns[t(f)] = fl(noise_scale · noise[t(f)]), and `expand` the latent expansion in float64 from m_p / logs_p with that scale.

A prosody here is a dict with the optional keys length, min_frames, max_frames, noise (arrays of t entries) and fit."""
import numpy as np


def _field(p, key, t, neutral, dt):
    v = None if p is None else p.get(key)
    return np.full(t, neutral, dt) if v is None else np.asarray(v, dt)


def durations(w0, p=None):
    """d[t] of the rule before fitting (int32), from the fp32 w0."""
    w0 = np.asarray(w0, np.float32)
    t = w0.size
    with np.errstate(invalid="ignore", over="ignore"):
        w1 = (w0 * _field(p, "length", t, 1.0, np.float32)).astype(np.float32)  # one fp32 multiply
        c = np.ceil(w1)
        d0 = np.where(c > 0, np.where(c < np.float32(1e6), c, np.float32(1e6)), np.float32(0))  # NaN compares false: 0
    d0 = np.nan_to_num(d0, nan=0.0).astype(np.int64)
    mx = _field(p, "max_frames", t, 0, np.int64)
    mn = _field(p, "min_frames", t, 0, np.int64)
    d1 = np.where(mx > 0, np.minimum(d0, mx), d0)
    return np.maximum(d1, mn).astype(np.int32)


def fit(d, cap, want_fit=True):
    """(durations used, wanted = Σ d, fitted): ⌊d · cap / S⌋ in integers when fitting is asked for and S > cap."""
    d = np.asarray(d, np.int64)
    S = int(d.sum())
    if want_fit and cap > 0 and S > cap:
        return np.array([int(x) * int(cap) // S for x in d], np.int32), S, 1
    return d.astype(np.int32), S, 0


def frames(w0, p=None, cap=0):
    """What piper_hip_prosody_frames computes: (frames per id, wanted)."""
    used, S, _ = fit(durations(w0, p), cap, bool(p and p.get("fit")))
    return used, S


def frame_count(d):
    return max(int(np.asarray(d, np.int64).sum()), 1)


def frame_ids(d):
    """t(f) for f in [0, frame_count): the smallest t with cum[t] > f; the lone frame of an all-zero result belongs to id 0."""
    d = np.asarray(d, np.int64)
    if d.sum() < 1:
        return np.zeros(1, np.int64)
    return np.repeat(np.arange(d.size), d)


def frame_ns(d, noise_scale, p=None):
    """ns[t(f)] per frame, fp32: fl(noise_scale · noise[t(f)])."""
    ns = (np.float32(noise_scale) * _field(p, "noise", np.asarray(d).size, 1.0, np.float32)).astype(np.float32)
    return ns[frame_ids(d)]


def expand(m_p, logs_p, d, nz, noise_scale, p=None):
    """z_p [C, F] in float64 from the fp32 m_p, logs_p [C, T], the noise nz [C, F] and the per-frame scale."""
    ids = frame_ids(d)
    m, lg = np.asarray(m_p, np.float64)[:, ids], np.asarray(logs_p, np.float64)[:, ids]
    return m + (np.asarray(nz, np.float64) * np.exp(lg)) * frame_ns(d, noise_scale, p).astype(np.float64)[None, :]
