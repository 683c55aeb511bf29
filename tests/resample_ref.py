"""The output-rate contract of include/piper_hip.h ("Output rate") restated in numpy: the filter design in float64, the conversion in the
contract's float32 order, and the ranges a stream step emits. The CPU tests hold the library's table against design(); the GPU tests
compare the device's samples with apply(), bit for bit."""
from math import gcd

import numpy as np

F32, F64 = np.float32, np.float64
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
PAIRS = [(i, o) for i in (16000, 22050) for o in RATES if o != i]  # the 14 pairs from the voices' own rates


def ratio(in_rate, out_rate):
    """(L, M, P): out / gcd, in / gcd, taps per phase = 2·ceil(24·max(L, M) / L) in integer arithmetic"""
    g = gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    P = 2 * ((24 * max(L, M) + L - 1) // L)
    return L, M, P


def design(in_rate, out_rate):
    """The [L][P] table in float64: Kaiser(9)-windowed sinc, cutoff 0.93·min(1, L / M), every phase divided by its own sum."""
    L, M, P = ratio(in_rate, out_rate)
    fc = F64(0.93) * min(F64(1.0), F64(L) / F64(M))
    p = np.arange(L, dtype=F64)[:, None]
    t = np.arange(P, dtype=F64)[None, :]
    tau = t - F64(P // 2 - 1) - p / F64(L)
    h = fc * np.sinc(fc * tau)  # np.sinc(x) = sin(pi x) / (pi x)
    r = tau / F64(P // 2)
    inside = np.abs(tau) < P // 2
    w = np.where(inside, np.i0(F64(9.0) * np.sqrt(np.where(inside, 1.0 - r * r, 0.0))) / np.i0(F64(9.0)), 0.0)
    c = h * w
    return c / c.sum(axis=1, keepdims=True)


def count(n_in, L, M):
    """J(n_in) = ceil(n_in·L / M)"""
    return (int(n_in) * L + M - 1) // M


def step_bound(n_in, L, M, P):
    return count(n_in, L, M) + count(P // 2, L, M) + 1


def apply(x, table, L, M, j0=0, j1=None, fma=False, descending=False, phase_shift=0, swap=False):
    """y[j] for j in [j0, j1) (default: all J(N)) in the contract's order: u = j·M, n = u div L, p = u mod L,
    y[j] = sum_t c[p][t] · x[n − (P/2 − 1) + t], x = 0 outside [0, N), float32 products and float32 sums in ascending t from 0.
    The keyword switches plant the defects the self-validation test must catch: an FMA (product kept in float64 into the sum), taps summed
    in descending order, the phase off by one, M and L swapped in n."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    table = np.ascontiguousarray(table, F32)
    N, P = x.size, table.shape[1]
    if j1 is None:
        j1 = count(N, L, M)
    j = np.arange(j0, j1, dtype=np.int64)
    u = j * M
    n, p = (u // M if swap else u // L), (u % L + phase_shift) % L
    pad = P + 1
    xp = np.concatenate([np.zeros(pad, F32), x, np.zeros(pad + int(n.max(initial=0)) + P, F32)])
    base = n - (P // 2 - 1) + pad
    acc = np.zeros(j.size, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in (range(P - 1, -1, -1) if descending else range(P)):
            c, s = table[p, t], xp[np.clip(base + t, 0, xp.size - 1)]
            if fma:
                acc = (acc.astype(F64) + c.astype(F64) * s.astype(F64)).astype(F32)
            else:
                acc = (acc + (c * s).astype(F32)).astype(F32)
    return acc


def stream_ranges(n_frames, chunk_frames, hop, L, M, P):
    """[(j0, j1)] per step of a row of n_frames·hop samples decoded chunk_frames at a time: a step whose chunk ends at input sample e < N
    emits up to ceil((e − P/2)·L / M), the last step the rest."""
    N, out, j0, f = n_frames * hop, [], 0, 0
    while f < n_frames:
        f = min(n_frames, f + chunk_frames)
        e = f * hop
        j1 = count(N, L, M) if e == N else max(j0, count(max(e - P // 2, 0), L, M))
        out.append((j0, j1))
        j0 = j1
    return out


def apply_chunked(x, table, L, M, n_frames, chunk_frames, hop):
    """The stream's way: each step reads only its chunk, the P − 1 samples before it and, on the last step, zeros behind the item."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    P, parts, f = table.shape[1], [], 0
    for j0, j1 in stream_ranges(n_frames, chunk_frames, hop, L, M, P):
        s, f = f * hop, min(n_frames, f + chunk_frames)
        e = f * hop
        known = x.copy()
        known[:max(s - (P - 1), 0)] = np.nan  # what the step no longer has …
        known[e:] = np.nan                    # … and what it does not have yet: a read of either poisons the sample
        parts.append(apply(known if e < x.size else np.where(np.arange(x.size) >= max(s - (P - 1), 0), x, np.nan), table, L, M, j0, j1))
    return np.concatenate(parts) if parts else np.empty(0, F32)
