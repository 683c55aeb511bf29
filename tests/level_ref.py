"""The level contract of include/piper_hip.h ("Level control") restated in numpy: the look-ahead limiter in the contract's float32 order,
and the ranges a stream step hands downstream. The CPU tests hold the library's host twin against apply(); the GPU tests compare the
device's samples with apply() of the device's own raw audio, bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
B, W = 32, 6          # PIPER_HIP_LEVEL_BLOCK, PIPER_HIP_LEVEL_LOOKAHEAD
CARRY = B * (W + 2) - 1  # 255: what a step can deliver beyond its chunk


def params(level):
    """(drive, ceiling, release_ms) with the zeros resolved: {1, 1, 50}"""
    d, c, r = (float(v) for v in level)
    return F32(d if d else 1.0), F32(c if c else 1.0), F32(r if r else 50.0)


def rel(level, rate):
    """fp32(min(1, 32·1000 / (rate · release_ms))), computed in float64 and rounded once"""
    _, _, ms = params(level)
    return F32(min(F64(1.0), F64(B) * F64(1000.0) / (F64(rate) * F64(ms))))


def ready(e, shift=0):
    """y is final on [0, ready(e)) when samples [0, e) are known and more follow. shift plants the defect: blocks late (+) or early (−)."""
    return max(0, B * (int(e) // B - (W + 1) + shift))


def step_bound(n_in):
    return int(n_in) + CARRY


def gains(x, level, rate, lookahead=W, release_after_min=False, node_is_g=False):
    """(u, node): u = fl(x·drive) and node[0 … K], K = ceil(N / 32)"""
    drive, ceiling, _ = params(level)
    r_ = rel(level, rate)
    x = np.ascontiguousarray(x, F32).reshape(-1)
    N = x.size
    K = (N + B - 1) // B
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = (x * drive).astype(F32)
        a = np.abs(u)
        a = np.where(np.isnan(a), F32(0), a)
        p = np.zeros(K + lookahead + 2, F32)
        if N:
            p[:K] = np.maximum.reduceat(np.concatenate([a, np.zeros(K * B - N, F32)]), np.arange(0, K * B, B))
        r = np.where(p > ceiling, (ceiling / np.where(p > ceiling, p, F32(1))).astype(F32), F32(1)).astype(F32)
    node = np.empty(K + 1, F32)
    G = F32(1.0)
    for k in range(K + 1):
        m = r[k:k + lookahead + 1].min()
        if release_after_min:
            Gn = min(F32(1.0), F32(min(m, G) + r_))
        else:
            Gn = min(m, F32(G + r_))
        node[k] = Gn if node_is_g else min(G, Gn)
        G = Gn
    return u, node


def apply(x, level, rate, lo=0, hi=None, fma_g=False, fma_y=False, **defects):
    """y[lo, hi) (default: the whole item). g(n) = fl(node[k] + fl(fl(node[k+1] − node[k]) · (i / 32))), y = fl(u · g).
    The keyword switches plant the defects the self-validation test must catch: an FMA in g (the product kept exact into the sum) or in y
    (x·drive kept exact into the product), look-ahead W − 1 (lookahead=), the release added after the min (release_after_min=),
    node[k] = G[k] (node_is_g=)."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    u, node = gains(x, level, rate, **defects)
    if hi is None:
        hi = x.size
    n = np.arange(lo, hi, dtype=np.int64)
    k, i = n // B, n % B
    t = (i.astype(F32) / F32(B)).astype(F32)
    drive = params(level)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (node[k + 1] - node[k]).astype(F32)
        if fma_g:
            g = (node[k].astype(F64) + d.astype(F64) * t.astype(F64)).astype(F32)
        else:
            g = (node[k] + (d * t).astype(F32)).astype(F32)
        if fma_y:
            return (x[lo:hi].astype(F64) * F64(drive) * g.astype(F64)).astype(F32)
        return (u[lo:hi] * g).astype(F32)


def step_ranges(n_frames, chunk_frames, hop, shift=0):
    """[(lo, hi)] per step of a row of n_frames·hop samples decoded chunk_frames at a time: a step whose chunk ends at input sample e < N
    hands downstream the limited samples up to ready(e), the last step the rest."""
    N, out, lo, f = n_frames * hop, [], 0, 0
    while f < n_frames:
        f = min(n_frames, f + chunk_frames)
        e = f * hop
        hi = N if e == N else ready(e, shift)
        out.append((lo, hi))
        lo = hi
    return out


def apply_chunked(x, level, rate, n_frames, chunk_frames, hop):
    """The stream's way: each step sees only the samples [0, e) decoded so far."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    parts, f = [], 0
    for lo, hi in step_ranges(n_frames, chunk_frames, hop):
        f = min(n_frames, f + chunk_frames)
        parts.append(apply(x[:f * hop], level, rate, lo, hi))
    return np.concatenate(parts) if parts else np.empty(0, F32)
