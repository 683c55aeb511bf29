"""ITU-R BS.1770 / EBU R128 integrated loudness restated in numpy, float64 (include/piper_hip.h "Loudness"): the reference the host twin and
the kernels are checked against. Pure numpy and one Python loop per biquad — no scipy, so the GPU tests can import it.

`defect=` plants one deviation from the contract; the tests show that each of them moves the result by more than the tolerance the
device is held to."""
import math

import numpy as np

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
DEFECTS = ("no_relative_gate", "no_offset", "no_highpass", "no_shelf", "hop_400ms", "coeffs_48k")


def coeffs(rate):
    """(shelf_b, shelf_a, hp_b, hp_a) at `rate`, float64 [3] each."""
    K = math.tan(math.pi * 1681.974450955533 / rate)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K = math.tan(math.pi * 38.13547087602444 / rate)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    hb = np.array([1.0, -2.0, 1.0])
    ha = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return sb, sa, hb, ha


def biquad(b, a, x):
    """y[n] = b0 x[n] + b1 x[n−1] + b2 x[n−2] − a1 y[n−1] − a2 y[n−2], zero state, sequentially in float64."""
    x = np.asarray(x, np.float64)
    f = b[0] * x
    f[1:] += b[1] * x[:-1]
    f[2:] += b[2] * x[:-2]
    a1, a2 = float(a[1]), float(a[2])
    y = f.tolist()
    y1 = y2 = 0.0
    for n, fn in enumerate(y):
        v = fn - a1 * y1 - a2 * y2
        y[n] = v
        y2 = y1
        y1 = v
    return np.array(y, np.float64)


def kweight(x, rate, defect=None):
    x = np.asarray(x, np.float32).astype(np.float64)
    x = np.where(np.isfinite(x), x, 0.0)
    sb, sa, hb, ha = coeffs(48000 if defect == "coeffs_48k" else rate)
    y = x if defect == "no_shelf" else biquad(sb, sa, x)
    return y if defect == "no_highpass" else biquad(hb, ha, y)


def block_count(n, rate):
    h = rate // 10
    return (n - 4 * h) // h + 1 if n >= 4 * h else 0


def measure(x, rate, defect=None):
    """{"L": LUFS (−inf when unmeasurable), "blocks": J, "abs": |A|, "rel": |R|} of float32 samples at `rate`."""
    assert rate in RATES, rate
    x = np.asarray(x, np.float32).reshape(-1)
    h = rate // 10
    hop = 4 * h if defect == "hop_400ms" else h
    off = 0.0 if defect == "no_offset" else -0.691
    J = (x.size - 4 * h) // hop + 1 if x.size >= 4 * h else 0
    out = {"L": -math.inf, "blocks": J, "abs": 0, "rel": 0}
    if J == 0:
        return out
    y = kweight(x[:(J - 1) * hop + 4 * h], rate, defect)
    z = np.array([np.sum(np.square(y[j * hop:j * hop + 4 * h])) for j in range(J)]) / (4.0 * h)
    with np.errstate(divide="ignore"):
        l = off + 10.0 * np.log10(z)
    A = l > -70.0
    out["abs"] = int(A.sum())
    if not A.any():
        return out
    gate = off + 10.0 * math.log10(float(np.mean(z[A]))) - 10.0
    R = A if defect == "no_relative_gate" else A & (l > gate)
    out["rel"] = int(R.sum())
    out["L"] = off + 10.0 * math.log10(float(np.mean(z[R])))
    return out


def lufs(x, rate, defect=None):
    return measure(x, rate, defect)["L"]


def resolve(loudness):
    """(target, max_gain) with the defaults in place; `loudness`: (target_lufs, max_gain_db)."""
    t, m = loudness
    return (-16.0 if t == 0 else float(np.float32(t))), (20.0 if m == 0 else float(np.float32(m)))


def gain(loudness, L):
    """g for the fp32 L a measurement reported: (float)10^(min(target − L, max_gain) / 20); 1.0 for an unmeasurable item."""
    L = float(np.float32(L))
    if L == -math.inf:
        return np.float32(1.0)
    t, m = resolve(loudness)
    return np.float32(10.0 ** (min(t - L, m) / 20.0))


def apply(x, g):
    """u = fl(x·g), one fp32 multiply."""
    return (np.asarray(x, np.float32) * np.float32(g)).astype(np.float32)


# ---- the signals of the tests: Gaussian, fixed seed

def sine(rate, seconds=3.0, freq=997.0, amp=1.0):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(int(round(rate * seconds))) / rate)).astype(np.float32)


def _stretches(rate, parts, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([(s * rng.standard_normal(int(round(sec * rate)))).astype(np.float32) for sec, s in parts])


def s1(rate):
    """stationary: no block is gated"""
    return _stretches(rate, [(3.0, 0.1)], 7001)


def s2(rate):
    """a quiet middle above the absolute gate: the relative gate alone takes blocks"""
    return _stretches(rate, [(1.5, 0.1), (1.5, 0.002), (1.0, 0.1)], 7002)


def s3(rate):
    """silence and a quiet tail: both gates take blocks"""
    return _stretches(rate, [(1.0, 0.05), (1.2, 0.0), (0.9, 0.05), (0.7, 0.004)], 7003)
