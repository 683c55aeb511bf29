"""The join contract of include/piper_hip.h "Join", restated in numpy: float64 for the sample counts and the ramp, float32 products,
everything else moved bit for bit. `join` takes a list of float32 items and returns (programme, start, len, total).

Planted defects (keyword arguments, all off by default) exist so that tests/test_join_ref.py can show that each of them is caught by a
named vector of VECTORS; DEFECTS maps every defect to the vector that catches it.

ramp_recip stands for "the ramp divided in fp32". A correctly rounded fp32 quotient of two integers below 2^24 equals the double quotient
rounded to fp32 (53 >= 2 * 24 + 2 bits make the double rounding innocuous), so a correctly rounded fp32 division cannot be told from the
contract. What a device's fast fp32 division does instead is multiply by a rounded reciprocal, and that is the defect planted here."""
import math

import numpy as np

F32 = np.float32
FIELDS = ("lead_ms", "gap_ms", "tail_ms", "trim", "trim_threshold", "trim_pad_ms", "fade_ms")


def params(j):
    """dict / object with the fields of piper_hip_join → a complete dict (missing fields 0)"""
    get = (lambda k: j.get(k, 0)) if isinstance(j, dict) else (lambda k: getattr(j, k, 0))
    return {k: get(k) for k in FIELDS}


def S(ms, rate, trunc_s=False):
    """S(ms) = (int64) floor((double)ms * rate / 1000.0 + 0.5), the float widened first"""
    v = float(F32(ms)) * float(rate) / 1000.0
    return int(v) if trunc_s else int(math.floor(v + 0.5))


def ramp(k, Fd, ramp_recip=False, ramp_k_over_fd=False):
    """g(k) = (float)((double)(k + 1) / (double)(Fd + 1)) for an int array k"""
    k = np.asarray(k, np.int64)
    if ramp_k_over_fd:
        return (k.astype(np.float64) / float(max(Fd, 1))).astype(F32)
    if ramp_recip:
        return (k + 1).astype(F32) * (F32(1.0) / F32(Fd + 1))
    return ((k + 1).astype(np.float64) / float(Fd + 1)).astype(F32)


def kept_range(x, p, P, ge=False, nan_loud=False, no_clamp=False):
    """[s, t) of one item"""
    n = x.size
    if not p["trim"]:
        return 0, n
    thr = F32(p["trim_threshold"])
    with np.errstate(invalid="ignore"):
        loud = (np.abs(x) >= thr) if ge else (np.abs(x) > thr)  # an fp32 compare, false for NaN
    if nan_loud:
        loud = loud | np.isnan(x)
    idx = np.flatnonzero(loud)
    if idx.size == 0:
        return 0, 0
    a, e = int(idx[0]), int(idx[-1])
    if no_clamp:
        return a - P, e + 1 + P
    return max(0, a - P), min(n, e + 1 + P)


def join(items, j, rate, gaps=None, ge=False, nan_loud=False, no_clamp=False, fade_uncut=False, ramp_recip=False, ramp_k_over_fd=False,
         tail_first=False, gap_after_last=False, drop_empty_gap=False, trunc_s=False, neg_zero=False):
    p = params(j)
    gaps = [] if gaps is None else list(gaps)
    P, Fd = S(p["trim_pad_ms"], rate, trunc_s), S(p["fade_ms"], rate, trunc_s)
    zero = F32(-0.0) if neg_zero else F32(0.0)
    parts, start, length = [np.full(S(p["lead_ms"], rate, trunc_s), zero, F32)], [], []
    at = parts[0].size
    for i, x in enumerate(items):
        x = np.ascontiguousarray(x, F32).reshape(-1)
        n = x.size
        s, t = kept_range(x, p, P, ge, nan_loud, no_clamp)
        y = np.take(x, np.arange(s, t), mode="wrap").astype(F32) if n else np.zeros(0, F32)  # (no_clamp: indices outside the item wrap)
        L = y.size
        m = min(Fd, L)
        k = np.arange(m)

        def head():
            if (s > 0 or fade_uncut) and m:
                y[:m] = y[:m] * ramp(k, Fd, ramp_recip, ramp_k_over_fd)

        def tail():
            if (t < n or fade_uncut) and m:
                y[L - 1 - k] = y[L - 1 - k] * ramp(k, Fd, ramp_recip, ramp_k_over_fd)

        for f in ((tail, head) if tail_first else (head, tail)):
            f()
        start.append(at)
        length.append(L)
        parts.append(y)
        at += L
        last = i == len(items) - 1
        if last and not gap_after_last:
            continue
        if drop_empty_gap and L == 0:
            continue
        g = S(gaps[i] if i < len(gaps) else p["gap_ms"], rate, trunc_s)
        parts.append(np.full(g, zero, F32))
        at += g
    parts.append(np.full(S(p["tail_ms"], rate, trunc_s), zero, F32))
    at += parts[-1].size
    out = np.concatenate(parts).astype(F32)
    assert out.size == at
    return out, np.array(start, np.int64), np.array(length, np.int64), at


def capacity(items_samples, j, rate, gaps=None):
    """the no-trim upper bound on total"""
    p = params(j)
    gaps = [] if gaps is None else list(gaps)
    n = len(items_samples)
    c = S(p["lead_ms"], rate) + S(p["tail_ms"], rate) + int(sum(items_samples))
    for i in range(n - 1):
        c += S(gaps[i] if i < len(gaps) else p["gap_ms"], rate)
    return c


def _noise(n, seed, amp=0.5):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(F32)


def _quiet_loud_quiet(n, lo, hi, seed, quiet=1e-3):
    """noise at `quiet` with a body of amplitude ≥ 0.3 in [lo, hi)"""
    x = _noise(n, seed, quiet)
    body = _noise(hi - lo, seed + 1, 0.5)
    x[lo:hi] = np.where(np.abs(body) < 0.3, F32(0.3), body)
    return x


def _vectors():
    v = {}
    x = np.zeros(40, F32)
    x[10], x[15], x[20] = 0.25, 0.5, -0.25
    v["threshold_exact"] = ([x, _quiet_loud_quiet(50, 10, 30, 1)], dict(trim=1, trim_threshold=0.25, gap_ms=1.0), 8000, None)
    x = _quiet_loud_quiet(64, 20, 40, 2)
    x[3], x[60] = np.nan, -np.nan
    v["nan_edge"] = ([x], dict(trim=1, trim_threshold=0.1), 8000, None)
    x = np.zeros(30, F32)
    x[1], x[28] = 0.9, -0.9
    v["pad_clamp"] = ([x, x], dict(trim=1, trim_threshold=0.1, trim_pad_ms=1.0, gap_ms=0.5), 8000, None)  # P = 8 > 1
    x = _quiet_loud_quiet(80, 0, 40, 3)  # loud from sample 0: the head is not cut, the tail is
    v["uncut_edge"] = ([x, x[::-1].copy()], dict(trim=1, trim_threshold=0.1, fade_ms=1.0, gap_ms=0.25), 8000, None)
    x = np.full(400, 0.75, F32)
    x[:150] = 1e-4
    x[-150:] = 1e-4
    v["ramp_81"] = ([x], dict(trim=1, trim_threshold=0.1, fade_ms=10.0), 8000, None)  # Fd + 1 = 81
    v["ramp_basic"] = ([_quiet_loud_quiet(100, 30, 70, 4)], dict(trim=1, trim_threshold=0.1, fade_ms=0.5), 8000, None)
    x = _noise(40, 5, 1e-3)
    # 5 kept samples under Fd = 8, both edges cut; at the first sample fl(fl(x·1/9)·5/9) != fl(fl(x·5/9)·1/9)
    x[18:23] = [0.4888507127761841, -0.5003, 0.9007, 0.3001, -0.6011]
    v["short_overlap"] = ([x], dict(trim=1, trim_threshold=0.1, fade_ms=1.0), 8000, None)
    v["last_gap"] = ([_noise(10, 6), _noise(12, 7)], dict(gap_ms=1.0), 8000, None)
    v["empty_middle"] = ([_quiet_loud_quiet(30, 5, 20, 8), _noise(25, 9, 1e-3), _quiet_loud_quiet(30, 5, 20, 10)],
                         dict(trim=1, trim_threshold=0.1, gap_ms=1.0), 8000, [2.0, 3.0])
    v["round_s"] = ([_noise(9, 11), _noise(9, 12)], dict(lead_ms=0.75, gap_ms=0.75, tail_ms=0.75), 22050, None)  # 16.5375 → 17
    v["silences"] = ([_noise(5, 13), _noise(5, 14)], dict(lead_ms=1.0, gap_ms=1.0, tail_ms=1.0), 8000, None)
    return v


VECTORS = _vectors()

# defect → the vector that catches it
DEFECTS = {
    "ge": "threshold_exact",
    "nan_loud": "nan_edge",
    "no_clamp": "pad_clamp",
    "fade_uncut": "uncut_edge",
    "ramp_recip": "ramp_81",
    "ramp_k_over_fd": "ramp_basic",
    "tail_first": "short_overlap",
    "gap_after_last": "last_gap",
    "drop_empty_gap": "empty_middle",
    "trunc_s": "round_s",
    "neg_zero": "silences",
}
