"""The 16-bit PCM arithmetic contract of include/piper_hip.h ("16-bit PCM straight from the device") restated in numpy, every float32 and
float64 operation spelled out. The GPU tests compare the device's samples with these, bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64


def effective_gain(gain):
    """gain 0 is taken as 1.0"""
    g = F32(gain)
    return F32(1.0) if g == 0 else g


def pcm16_reference(x, gain=1.0):
    """normalize = 0: y = x·gain (one fp32 multiply, skipped for gain 1), then piper_hip_pcm16_from_f32: NaN → 0, clamp to [−1, 1], × 32767.0
    in double precision, truncate toward zero."""
    y = np.ascontiguousarray(x, F32).reshape(-1)
    g = effective_gain(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        if g != 1:
            y = (y * g).astype(F32)
        d = y.astype(F64)
        d = np.where(np.isnan(d), F64(0.0), np.clip(d, F64(-1.0), F64(1.0)))
        return np.trunc(d * F64(32767.0)).astype(np.int16)


def peak(x):
    """max |x| with NaN ignored; 0 for an empty item"""
    a = np.abs(np.ascontiguousarray(x, F32).reshape(-1))
    a = a[~np.isnan(a)]
    return F32(a.max()) if a.size else F32(0.0)


def normalize_scale(pk):
    """the correctly rounded fp32 quotient 32767 / max(0.01, peak): divided in double, rounded once"""
    m = max(F32(0.01), F32(pk))
    with np.errstate(divide="ignore"):
        return F32(F64(32767.0) / F64(m))


def pcm16_normalized(x, gain=1.0):
    """normalize = 1 for ONE item: Piper's audio * (32767 / max(0.01, max|audio|)), clip, astype(int16), carried out in float32."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    s, g = normalize_scale(peak(x)), effective_gain(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * s).astype(F32)
        if g != 1:
            v = (v * g).astype(F32)
        v = np.where(np.isnan(v), F32(0.0), np.clip(v, F32(-32767.0), F32(32767.0))).astype(F32)
        return np.trunc(v).astype(np.int16)


def pcm16_items(items, gain=1.0, normalize=False):
    """a slot's items back to back, as collect_pcm16 reports them"""
    f = pcm16_normalized if normalize else pcm16_reference
    return np.concatenate([f(it, gain) for it in items]) if len(items) else np.empty(0, np.int16)


def fp32_shortcut(x):
    """what the contract forbids: the multiply by 32767 in float32 (it can round up across an integer boundary)"""
    y = np.ascontiguousarray(x, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(y), F32(0.0), np.clip(y, F32(-1.0), F32(1.0))).astype(F32)
        return np.trunc((y * F32(32767.0)).astype(F32)).astype(np.int16)


def adversarial_vector():
    """For every k in −32767 … 32767 step 257 (plus both ends) the float32 nearest k/32767 and its two neighbours; then ±1, ±(1 + 2⁻²³), ±2,
    ±inf, NaN, ±0, the smallest denormal, ±0.5/32767."""
    ks = sorted(set(list(range(-32767, 32768, 257)) + [-32767, 32767]))
    mid = (np.asarray(ks, F64) / F64(32767.0)).astype(F32)
    near = np.stack([np.nextafter(mid, F32(-np.inf)), mid, np.nextafter(mid, F32(np.inf))], axis=1).reshape(-1)
    one_up = F32(1.0) + F32(2.0 ** -23)
    h = F32(F64(0.5) / F64(32767.0))
    extra = np.asarray([1.0, -1.0, one_up, -one_up, 2.0, -2.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.nextafter(F32(0), F32(1)), h, -h], F32)
    v = np.concatenate([near, extra]).astype(F32)
    v.setflags(write=False)
    return v
