"""The equaliser contract of include/piper_hip.h ("Equaliser") restated in numpy float64: the RBJ cookbook design, the transposed direct
form II cascade, and the absolute-anchored block tree that makes the device's parallel form exact. It loops over samples and is
vectorised over blocks; it uses no np.matmul, so every matrix product sums in the contract's order (ascending j, starting from the j = 0
product). The design uses Python's math module, which is the C library's cos, sin, pow and sqrt, as the library's host code is.

defect= plants a mistake the tests must see:
  arithmetic   "alpha_q" (α = s/Q), "a_db20" (A = 10^(g/20)), "reverse" (the blocks run the sections in reverse order while the
               transitions keep the contract's order), "swap_shelf" (low and high shelf swapped), "p_next" (P_{l+1} in place of P_l in
               the fold), "zero_start" (the middle block starts from zero state), "pass_nonfinite" (a non-finite sample is filtered as
               it is)
  order        "ascending" (the fold takes the levels lowest first: the same sum, other roundings), "reverse_all" (the whole cascade in
               reverse order: the same LTI filter, other roundings)"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
B = 64                 # PIPER_HIP_EQ_BLOCK
MAX_SECTIONS = 4       # PIPER_HIP_EQ_MAX_SECTIONS
LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAKING, LOWSHELF, HIGHSHELF = range(1, 8)
TYPES = (LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAKING, LOWSHELF, HIGHSHELF)
GAIN_TYPES = (PEAKING, LOWSHELF, HIGHSHELF)

# the two filter sets of the tests, both at 22 050 Hz
F1 = [(HIGHPASS, 40.0, 0.707, 0.0), (PEAKING, 3000.0, 1.0, 6.0), (HIGHSHELF, 6000.0, 0.707, -3.0), (LOWPASS, 7000.0, 0.707, 0.0)]
F2 = [(HIGHPASS, 10.0, 5.0, 0.0), (PEAKING, 50.0, 30.0, -30.0), (PEAKING, 100.0, 0.1, 30.0), (LOWPASS, 9900.0, 10.0, 0.0)]


def f32(v):
    """a field as the C struct holds it, widened back to a Python float"""
    return float(F32(v))


def design(eq, rate, defect=None):
    """[(b0, b1, b2, a1, a2)] per section, each normalised by its a0, all in double as written in the header"""
    out = []
    fs = float(rate)
    for sec in eq:
        typ, f0, q, g = sec[0], f32(sec[1]), f32(sec[2]), f32(sec[3] if len(sec) > 3 else 0.0)
        if defect == "swap_shelf" and typ in (LOWSHELF, HIGHSHELF):
            typ = LOWSHELF + HIGHSHELF - typ
        w0 = 2.0 * math.pi * f0 / fs
        c, s = math.cos(w0), math.sin(w0)
        alpha = s / q if defect == "alpha_q" else s / (2.0 * q)
        A = math.pow(10.0, g / 20.0) if defect == "a_db20" else math.pow(10.0, g / 40.0)
        if typ == LOWPASS:
            b0, b1, b2 = (1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0
            a0, a1, a2 = 1.0 + alpha, -2.0 * c, 1.0 - alpha
        elif typ == HIGHPASS:
            b0, b1, b2 = (1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0
            a0, a1, a2 = 1.0 + alpha, -2.0 * c, 1.0 - alpha
        elif typ == BANDPASS:
            b0, b1, b2 = alpha, 0.0, -alpha
            a0, a1, a2 = 1.0 + alpha, -2.0 * c, 1.0 - alpha
        elif typ == NOTCH:
            b0, b1, b2 = 1.0, -2.0 * c, 1.0
            a0, a1, a2 = 1.0 + alpha, -2.0 * c, 1.0 - alpha
        elif typ == PEAKING:
            b0, b1, b2 = 1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A
            a0, a1, a2 = 1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A
        elif typ == LOWSHELF:
            r = 2.0 * math.sqrt(A) * alpha
            b0 = A * ((A + 1.0) - (A - 1.0) * c + r)
            b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * c)
            b2 = A * ((A + 1.0) - (A - 1.0) * c - r)
            a0 = (A + 1.0) + (A - 1.0) * c + r
            a1 = -2.0 * ((A - 1.0) + (A + 1.0) * c)
            a2 = (A + 1.0) + (A - 1.0) * c - r
        elif typ == HIGHSHELF:
            r = 2.0 * math.sqrt(A) * alpha
            b0 = A * ((A + 1.0) + (A - 1.0) * c + r)
            b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * c)
            b2 = A * ((A + 1.0) + (A - 1.0) * c - r)
            a0 = (A + 1.0) - (A - 1.0) * c + r
            a1 = 2.0 * ((A - 1.0) - (A + 1.0) * c)
            a2 = (A + 1.0) - (A - 1.0) * c - r
        else:
            raise ValueError(typ)
        out.append((b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0))
    if defect == "reverse_all":
        out = out[::-1]
    return out


@np.errstate(invalid="ignore", over="ignore")
def _step(st, v, co):
    """one sample through the cascade; st [..., D] is updated in place, v [...] float64; returns y [...]"""
    for i, (b0, b1, b2, a1, a2) in enumerate(co):
        y = b0 * v + st[..., 2 * i]
        st[..., 2 * i] = (b1 * v - a1 * y) + st[..., 2 * i + 1]
        st[..., 2 * i + 1] = b2 * v - a2 * y
        v = y
    return v


def _read(x, defect=None):
    x = np.asarray(x, F32).astype(F64)
    if defect != "pass_nonfinite":
        x = np.where(np.isfinite(x), x, 0.0)
    return x


def transition(co):
    """A [D][D]: column j is unit state j stepped once with no input"""
    D = 2 * len(co)
    A = np.zeros((D, D), F64)
    for j in range(D):
        st = np.zeros(D, F64)
        st[j] = 1.0
        _step(st, 0.0, co)
        A[:, j] = st
    return A


def mat(a, b):
    """a·b, every sum over ascending j starting from the j = 0 product"""
    acc = a[:, 0:1] * b[0:1, :]
    for j in range(1, a.shape[1]):
        acc = acc + a[:, j:j + 1] * b[j:j + 1, :]
    return acc


def matvec(P, S):
    """P·S for S [..., D], the same order"""
    acc = P[:, 0] * S[..., 0:1]
    for j in range(1, P.shape[1]):
        acc = acc + P[:, j] * S[..., j:j + 1]
    return acc


def powers(co, levels):
    """P_0 = A^64 by six squarings, P_{l+1} = P_l·P_l"""
    P = transition(co)
    for _ in range(6):
        P = mat(P, P)
    out = [P]
    for _ in range(levels - 1):
        out.append(mat(out[-1], out[-1]))
    return out


def sequential(x, eq, rate):
    """the plain recurrence over the whole item, float64 y (no blocks)"""
    co = design(eq, rate)
    xs = _read(x)
    st = np.zeros(2 * len(co), F64)
    y = np.empty(xs.size, F64)
    for n in range(xs.size):
        y[n] = _step(st, xs[n], co)
    return y


def _levels(K):
    return max(1, int(K - 1).bit_length() + 1)


def _blocks(xs, K):
    """xs zero-padded to [K][64] and the true length of every block"""
    N = xs.size
    pad = np.zeros(K * B, F64)
    pad[:N] = xs
    return pad.reshape(K, B), np.minimum(B, N - np.arange(K) * B)


def _run(xb, cnt, start, co, out=None, defect=None):
    """every block from its start state over its true length; the states it ends in, and y where out is given"""
    if defect == "reverse":  # the blocks run the sections last first, on the contract's state layout
        return _run_reversed(xb, cnt, start, co, out)
    st = start.copy()
    for i in range(B):
        live = cnt > i
        if not live.any():
            break
        s2 = st[live]
        y = _step(s2, xb[live, i], co)
        st[live] = s2
        if out is not None:
            out[live, i] = y
    return st


def _run_reversed(xb, cnt, start, co, out):
    st = start.copy()
    for i in range(B):
        live = cnt > i
        if not live.any():
            break
        s2, v = st[live], xb[live, i]
        for j in range(len(co) - 1, -1, -1):
            b0, b1, b2, a1, a2 = co[j]
            y = b0 * v + s2[:, 2 * j]
            s2[:, 2 * j] = (b1 * v - a1 * y) + s2[:, 2 * j + 1]
            s2[:, 2 * j + 1] = b2 * v - a2 * y
            v = y
        st[live] = s2
        if out is not None:
            out[live, i] = v
    return st


def tree(E, P):
    """T_0 = E, T_{l+1}[m] = P_l·T_l[2m] + T_l[2m+1]"""
    T = [E]
    while T[-1].shape[0] > 1:
        t = T[-1]
        h = t.shape[0] // 2
        T.append(matvec(P[len(T) - 1], t[0:2 * h:2]) + t[1:2 * h:2])
    return T


def fold(K, T, P, D, defect=None):
    """S[k]: S = 0, then for every set bit l of k, highest first, S ← P_l·S + T_l[(k >> l) − 1]"""
    k = np.arange(K)
    S = np.zeros((K, D), F64)
    L = len(T)
    if defect == "ascending":  # the same sum lowest level first: S ← S + M·T_l, M ← M·P_l, M the span of the segments already taken
        M = np.broadcast_to(np.eye(D), (K, D, D)).copy()
        for l in range(L):
            m = ((k >> l) & 1) == 1
            if not m.any():
                continue
            t, Mm = T[l][(k[m] >> l) - 1], M[m]
            add = Mm[:, :, 0] * t[:, 0:1]
            for j in range(1, D):
                add = add + Mm[:, :, j] * t[:, j:j + 1]
            S[m] = S[m] + add
            Mn = Mm[:, :, 0:1] * P[l][0][None, None, :]
            for j in range(1, D):
                Mn = Mn + Mm[:, :, j:j + 1] * P[l][j][None, None, :]
            M[m] = Mn
        return S
    for l in range(L - 1, -1, -1):
        m = ((k >> l) & 1) == 1
        if not m.any():
            continue
        Pl = P[l + 1] if defect == "p_next" else P[l]
        S[m] = matvec(Pl, S[m]) + T[l][(k[m] >> l) - 1]
    return S


def apply64(x, eq, rate, defect=None):
    """the contract's y in float64 before the final rounding"""
    co = design(eq, rate, defect)
    xs = _read(x, defect)
    N, D = xs.size, 2 * len(co)
    if N == 0:
        return np.empty(0, F64)
    K = (N + B - 1) // B
    xb, cnt = _blocks(xs, K)
    P = powers(co, _levels(K) + 1)
    E = _run(xb, cnt, np.zeros((K, D), F64), co, defect=defect)
    T = tree(E, P)
    S = fold(K, T, P, D, defect)
    if defect == "zero_start":
        S[K // 2] = 0.0
    y = np.zeros((K, B), F64)
    _run(xb, cnt, S, co, y, defect)
    return y.reshape(-1)[:N]


def apply(x, eq, rate, defect=None):
    """y[n] = (float)v, the contract's output"""
    return apply64(x, eq, rate, defect).astype(F32)


def streamed(x, eq, rate, steps):
    """The stream form: the item in steps of the given sample counts (multiples of 64 but the last), a carry of one aggregate per set bit
    of the block count, merged like a binary counter. Returns the concatenated fp32 outputs."""
    co = design(eq, rate)
    xs = _read(x)
    D = 2 * len(co)
    P = powers(co, 40)
    carry = {}  # level → aggregate
    k0, out, at = 0, [], 0
    for n in steps:
        chunk = xs[at:at + n]
        at += n
        K = (n + B - 1) // B
        xb, cnt = _blocks(chunk, K)
        y = np.zeros((K, B), F64)
        for j in range(K):
            S = np.zeros((1, D), F64)
            for l in sorted(carry, reverse=True):
                S = matvec(P[l], S) + carry[l][None]
            E = _run(xb[j:j + 1], cnt[j:j + 1], np.zeros((1, D), F64), co)
            _run(xb[j:j + 1], cnt[j:j + 1], S, co, y[j:j + 1])
            c, l = E[0], 0
            while l in carry:
                c = matvec(P[l], carry.pop(l)[None])[0] + c
                l += 1
            carry[l] = c
        k0 += K
        out.append(y.reshape(-1)[:n].astype(F32))
    return np.concatenate(out) if out else np.empty(0, F32)
