"""The per-phoneme volume contract of include/piper_hip.h "Per-phoneme volume" in numpy fp32: every operation on float32 arrays, so each
is rounded on its own, as the kernels and the host twin do it.

    gf[f]  = gain[t(f)], t(f) the smallest t with cum[t] > f; the single frame of an all-zero duration row belongs to id 0
    c      = hop div 2;  m = n − c;  k = floor(m / hop);  i = m − k·hop
    a      = gf[max(k, 0)];  b = gf[min(k + 1, F − 1)];  w = fl(i / hop)
    e(n)   = fl(a + fl(fl(b − a)·w));  v[n] = fl(x[n]·e(n))

`defect` plants one wrong reading of that text; tests/test_volume_ref.py shows that the vectors tell each of them from the contract."""
import numpy as np

F32 = np.float32

DEFECTS = ("centre_at_frame_start", "step", "no_clamp_start", "no_clamp_end", "ramp_in_f64", "w_plus_one", "zero_ids_not_skipped",
           "all_zero_row_not_id0")


def frame_gains(gain, durations, defect=None):
    """gf [F], F = max(Σ d, 1). gain None: all 1.0."""
    d = np.asarray(durations, np.int64).reshape(-1)
    g = np.ones(d.size, F32) if gain is None else np.asarray(gain, F32).reshape(-1)
    assert g.size == d.size and d.size >= 1 and (d >= 0).all()
    if d.sum() == 0:
        return g[-1:].copy() if defect == "all_zero_row_not_id0" else g[:1].copy()
    gf = np.repeat(g, d)
    if defect == "zero_ids_not_skipped":  # an id without frames still claims the frame it would have started on
        start = np.cumsum(d) - d
        for t in range(d.size):
            if d[t] == 0 and start[t] < gf.size:
                gf[start[t]] = g[t]
    return gf


def envelope(gf, hop, defect=None):
    """e [F·hop] fp32"""
    gf = np.asarray(gf, F32).reshape(-1)
    F, hop = gf.size, int(hop)
    assert F >= 1 and hop >= 1
    n = np.arange(F * hop, dtype=np.int64)
    if defect == "step":
        return gf[n // hop].copy()
    c = 0 if defect == "centre_at_frame_start" else hop // 2
    m = n - c
    k = np.floor_divide(m, hop)
    i = m - k * hop
    ka = k % F if defect == "no_clamp_start" else np.maximum(k, 0)
    a = gf[ka]
    if defect == "no_clamp_end":  # past the last frame the gain is taken to be 0
        b = np.where(k + 1 < F, gf[np.minimum(k + 1, F - 1)], F32(0.0)).astype(F32)
    else:
        b = gf[np.minimum(k + 1, F - 1)]
    if defect == "ramp_in_f64":
        return (a.astype(np.float64) + (b.astype(np.float64) - a.astype(np.float64)) * (i.astype(np.float64) / hop)).astype(F32)
    w = ((i + 1) if defect == "w_plus_one" else i).astype(F32) / F32(hop)
    d = b - a
    dw = d * w
    e = a + dw
    assert e.dtype == F32
    return e


def apply(x, gf, hop, defect=None):
    """v [F·hop] fp32"""
    x = np.asarray(x, F32).reshape(-1)
    e = envelope(gf, hop, defect)
    assert x.size == e.size, (x.size, e.size)
    with np.errstate(invalid="ignore", over="ignore"):
        return x * e


def in_ramp(gf, hop):
    """bool [F·hop]: the samples whose two gains differ (the contract's b − a ≠ 0)"""
    gf = np.asarray(gf, F32).reshape(-1)
    F = gf.size
    k = np.floor_divide(np.arange(F * hop, dtype=np.int64) - hop // 2, hop)
    return gf[np.maximum(k, 0)] != gf[np.minimum(k + 1, F - 1)]
