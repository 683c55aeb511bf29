"""The pitch contract of include/piper_hip.h ("Pitch") restated in numpy: the 32.32 step and the counts in Python integers, the filter
design in float64 (plain Python floats in the order the library's design loop uses, so that the rounded table can be held bit for bit),
the samples in the contract's float32 order, the padded item of a voice slot and the tempo factor. The keyword switches plant the
defects that tests/test_pitch_ref.py must each catch on a named vector."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
ONE = 1 << 32
PHASES = 128
SHIFTS = (-12.0, -5.0, -0.37, 0.0, 0.01, 3.0, 7.0, 12.0)
SIZES = (0, 1, 2, 23, 24, 47, 48, 255, 256, 257, 4097)


def step(semitones):
    """Q = floor(2^(st/12) · 2^32 + 0.5) for a finite st in [−12, 12]"""
    st = float(F32(semitones))
    if not math.isfinite(st) or not -12.0 <= st <= 12.0:
        raise ValueError("semitones %r" % (semitones,))
    rho = float(np.exp2(F64(st) / F64(12.0)))
    return int(math.floor(rho * 4294967296.0 + 0.5))


def taps(Q):
    """P = 2·ceil(24·max(Q, 2^32) / 2^32) in integer arithmetic"""
    return 2 * ((24 * max(Q, ONE) + ONE - 1) >> 32)


def count(n, Q, floor_count=False):
    """N' = ceil(N·2^32 / Q); N' = N at Q = 2^32"""
    n = int(n)
    return (n << 32) // Q if floor_count else ((n << 32) + Q - 1) // Q


def frames(n, Q, hop, floor_frames=False):
    """F' = ceil(N' / hop)"""
    c = count(n, Q)
    return c // hop if floor_frames else (c + hop - 1) // hop


def _i0(x):
    q = x * x / 4.0
    term, total = 1.0, 1.0
    for k in range(1, 500):
        term *= q / (float(k) * float(k))
        total += term
        if term < total * 1e-17:
            break
    return total


@functools.lru_cache(maxsize=None)
def design(Q, fc_fixed=False):
    """The [129][P] table in float64: Kaiser(9)-windowed sinc, cutoff 0.93·min(1, 1/ρq), every row divided by its own sum.
    fc_fixed plants the defect "fc not lowered for ρ > 1"."""
    P = taps(Q)
    rq = float(Q) / 4294967296.0
    fc = 0.93 if fc_fixed else 0.93 * min(1.0, 1.0 / rq)
    half, i0b = float(P // 2), _i0(9.0)
    out = np.empty((PHASES + 1, P), F64)
    for p in range(PHASES + 1):
        c = []
        for t in range(P):
            tau = float(t - (P // 2 - 1)) - float(p) / 128.0
            a = fc * tau
            h = fc * (1.0 if a == 0.0 else math.sin(math.pi * a) / (math.pi * a))
            r = tau / half
            w = _i0(9.0 * math.sqrt(1.0 - r * r)) / i0b if abs(tau) < half else 0.0
            c.append(h * w)
        total = 0.0
        for v in c:
            total += v
        out[p] = [v / total for v in c]
    out.setflags(write=False)
    return out


def table(Q):
    return design(Q).astype(F32)


def apply(x, semitones, nearest=False, alpha_bits=False, floor_count=False, centre=False, f64_sums=False, fc_fixed=False, clamp=False):
    """y[0 … N') of x[0 … N) in the contract's order. The switches plant: nearest phase (no y1), α from the wrong bits, floor in N', the
    window centred on P/2, sums kept in float64, fc not lowered for ρ > 1, the edge sample repeated instead of zeros."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    Q = step(semitones)
    N = x.size
    if Q == ONE:
        return x.copy()
    n_out = count(N, Q, floor_count)
    tab = design(Q, fc_fixed).astype(F32)
    P = tab.shape[1]
    j = np.arange(n_out, dtype=np.uint64)
    u = j * np.uint64(Q)
    n = (u >> np.uint64(32)).astype(np.int64)
    frac = (u & np.uint64(0xffffffff)).astype(np.int64)
    p = frac >> 25
    abits = (frac & 0xffffff) if alpha_bits else ((frac >> 1) & 0xffffff)
    alpha = (abits.astype(F32) * F32(2.0 ** -24)).astype(F32)
    base = n - (P // 2 if centre else P // 2 - 1)
    acc = F64 if f64_sums else F32
    y0, y1 = np.zeros(n_out, acc), np.zeros(n_out, acc)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(P):
            i = base + t
            inside = (i >= 0) & (i < N)
            if N == 0:
                s = np.zeros(n_out, F32)
            elif clamp:
                s = x[np.clip(i, 0, N - 1)]
            else:
                s = np.where(inside, x[np.clip(i, 0, N - 1)], F32(0.0)).astype(F32)
            if f64_sums:
                y0 = y0 + tab[p, t].astype(F64) * s.astype(F64)
                y1 = y1 + tab[p + 1, t].astype(F64) * s.astype(F64)
            else:
                y0 = (y0 + (tab[p, t] * s).astype(F32)).astype(F32)
                y1 = (y1 + (tab[p + 1, t] * s).astype(F32)).astype(F32)
        y0, y1 = y0.astype(F32), y1.astype(F32)
        if nearest:
            return y0
        d = (y1 - y0).astype(F32)
        return (y0 + (alpha * d).astype(F32)).astype(F32)


def item(x, semitones, hop, floor_frames=False, dirty_tail=False):
    """The pitched item of a voice slot: (row [F'·hop], F'), samples [N', F'·hop) are +0.0f. The switches plant F' by floor and a tail
    that is not zeroed (it keeps what a buffer held before: ones)."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    Q = step(semitones)
    y = apply(x, semitones)
    Fp = frames(x.size, Q, hop, floor_frames)
    row = np.full(Fp * hop, 1.0 if dirty_tail else 0.0, F32)
    k = min(y.size, row.size)
    row[:k] = y[:k]
    return row, Fp


def length_scale(ls, semitones, inverse=False):
    """length_scale' = fl(ls·rf) of keep_tempo = 1: rf = (float)(Q / 2^32), ls = 0 taken as 1.0. `inverse` plants the factor 1/ρ."""
    rq = float(step(semitones)) / 4294967296.0
    rf = F32(1.0 / rq) if inverse else F32(rq)
    base = F32(1.0) if float(ls) == 0.0 else F32(ls)
    return F32(base * rf)


def sine(freq, n=22050, rate=22050, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(n, dtype=F64) / rate)).astype(F32)


def noise(n, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal(n)).astype(F32)


# name → (x, semitones, hop): each is run through apply(), item() and length_scale(1.1, ·)
VECTORS = {
    "noise-up3": (noise(700, 1), 3.0, 256),
    "noise-down5": (noise(700, 2), -5.0, 256),
    "noise-octave-up": (noise(513, 3), 12.0, 256),
    "noise-octave-down": (noise(300, 4), -12.0, 64),
    "noise-fine": (noise(1000, 5), 0.01, 256),
    "sine-up7": (sine(4000.0, 2048), 7.0, 256),
    "dc-down": (np.full(40, 0.75, F32), -0.37, 16),
    "short": (noise(23, 6), 7.0, 4),
    "one": (np.array([1.0], F32), -12.0, 4),
    "neutral": (noise(300, 7), 0.0, 256),
}
DEFECTS = {
    "nearest": dict(nearest=True), "alpha_bits": dict(alpha_bits=True), "floor_count": dict(floor_count=True), "centre": dict(centre=True),
    "f64_sums": dict(f64_sums=True), "fc_fixed": dict(fc_fixed=True), "clamp": dict(clamp=True),
}
ITEM_DEFECTS = {"floor_frames": dict(floor_frames=True), "dirty_tail": dict(dirty_tail=True)}
