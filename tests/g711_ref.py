"""The G.711 contract of include/piper_hip.h "G.711 output" in numpy, in the table-search form the header states (the kernels find the
segment from the leading-zero count, the host C functions with a loop: three derivations). encode: int16 → uint8; decode: uint8 → int16."""
import os

import numpy as np

MULAW, ALAW = 1, 2
LAWS = {"mulaw": MULAW, "alaw": ALAW}
MU_ENDS = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF], np.int32)
A_ENDS = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF], np.int32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711.npz")


def _law(law):
    law = LAWS.get(law, law)
    assert law in (MULAW, ALAW), law
    return law


def encode(pcm, law, ones_complement=False):
    """ones_complement: the planted defect — ITU-T G.191's μ-law takes the magnitude of a negative sample as ~v, not −v."""
    s = np.asarray(pcm, np.int16).astype(np.int32)
    if _law(law) == MULAW:
        v = s >> 2  # arithmetic
        neg = v < 0
        mag = np.where(neg, ~v if ones_complement else -v, v)
        m = np.minimum(mag, 8159) + 33
        seg = (MU_ENDS[None, :] < m.reshape(-1, 1)).sum(axis=1).reshape(m.shape)
        code = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
        return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)
    v = s >> 3
    neg = v < 0
    m = np.where(neg, -v - 1, v)
    seg = (A_ENDS[None, :] < m.reshape(-1, 1)).sum(axis=1).reshape(m.shape)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def decode(data, law):
    b = np.asarray(data, np.uint8).astype(np.int32)
    if _law(law) == MULAW:
        u = ~b & 0xFF
        t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
        return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)
    a = b ^ 0x55
    t = (a & 15) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def all_pcm():
    return np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


def golden():
    """{mulaw_encode, alaw_encode: uint8 [65536] for inputs −32768 … 32767; mulaw_decode, alaw_decode: int16 [256]} (tools/make_g711_golden.py)"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def table_encode(pcm, law):
    """encode through the golden table: what the GPU tests expect (no arithmetic of this file in the way)"""
    name = "mulaw_encode" if _law(law) == MULAW else "alaw_encode"
    return golden_cached()[name][np.asarray(pcm, np.int16).astype(np.int32) + 32768]


def table_decode(data, law):
    name = "mulaw_decode" if _law(law) == MULAW else "alaw_decode"
    return golden_cached()[name][np.asarray(data, np.uint8)]


_golden = None


def golden_cached():
    global _golden
    if _golden is None:
        _golden = golden()
    return _golden
