"""CPU: the numpy restatement of the per-phoneme volume contract (tests/volume_ref.py) — the header's known answer, the identities the
header states, and every planted defect told from the contract by at least one vector."""
import numpy as np
import pytest

import volume_ref as vr

F32 = np.float32
CYCLE = (1.0, 0.25, 1.0, 2.0, 0.0, 1.5)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def signal(n, seed):
    """finite samples of every size, both zeros, the largest and the smallest normal numbers"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F32)
    for at, val in enumerate((0.0, -0.0, np.finfo(F32).max, -np.finfo(F32).tiny, 1.0, -1.0)):
        if at < n:
            x[at] = val
    return x


def vectors():
    """(name, gains per id, durations, hop)"""
    rng = np.random.default_rng(7)
    out = [("known answer", [1.0, 0.5], [1, 1], 4),
           ("cycle, 3 frames per id", list(CYCLE) * 2, [3] * 12, 256),
           ("cycle, hop 6", list(CYCLE), [1, 2, 1, 3, 1, 2], 6),
           ("cycle, hop 250", list(CYCLE), [2] * 6, 250),
           ("zero-duration ids", [1.0, 0.25, 2.0, 0.5, 1.5], [2, 0, 3, 0, 1], 8),
           ("first and last id without frames", [3.0, 0.25, 2.0, 7.0], [0, 2, 2, 0], 6),
           ("all-zero row", [0.5, 2.0, 3.0], [0, 0, 0], 6),
           ("one frame", [0.75], [1], 250),
           ("random gains, hop 250", rng.uniform(0.0, 16.0, 37).astype(F32), [1] * 37, 250),
           ("random gains, hop 6", rng.uniform(0.0, 16.0, 37).astype(F32), [1] * 37, 6)]
    return out


def test_known_answer():
    v = vr.apply(np.ones(8, F32), [1.0, 0.5], 4)
    assert np.array_equal(v, np.array([1, 1, 1, 0.875, 0.75, 0.625, 0.5, 0.5], F32))
    assert np.array_equal(vr.frame_gains([1.0, 0.5], [1, 1]), np.array([1.0, 0.5], F32))


@pytest.mark.parametrize("hop", [1, 4, 6, 250, 256])
@pytest.mark.parametrize("frames", [1, 2, 37])
def test_a_neutral_volume_is_the_identity_bit_for_bit(frames, hop):
    x = signal(frames * hop, frames + hop)
    for gf in (np.ones(frames, F32), vr.frame_gains(None, [frames])):
        assert np.array_equal(bits(vr.apply(x, gf, hop)), bits(x))


@pytest.mark.parametrize("g", [0.0, 0.25, 0.3, 1.5, 16.0])
def test_a_constant_gain_is_exact(g):
    for frames, hop in ((1, 250), (5, 6), (37, 256)):
        e = vr.envelope(np.full(frames, g, F32), hop)
        assert np.array_equal(bits(e), bits(np.full(frames * hop, g, F32)))
        x = signal(frames * hop, 3)
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(vr.apply(x, np.full(frames, g, F32), hop)), bits(x * F32(g)))
    assert not vr.in_ramp(np.full(4, g, F32), 6).any()


def test_frame_gains_follow_the_frame_rule():
    assert np.array_equal(vr.frame_gains([1.0, 0.25, 2.0, 0.5, 1.5], [2, 0, 3, 0, 1]), np.array([1, 1, 2, 2, 2, 1.5], F32))
    assert np.array_equal(vr.frame_gains([3.0, 0.25, 2.0, 7.0], [0, 2, 2, 0]), np.array([0.25, 0.25, 2, 2], F32))
    assert np.array_equal(vr.frame_gains([0.5, 2.0, 3.0], [0, 0, 0]), np.array([0.5], F32))  # the single frame belongs to id 0
    assert np.array_equal(vr.frame_gains(None, [0, 4]), np.ones(4, F32))


def test_the_cycle_ramps_a_third_and_rests_at_unity_on_two_ninths():
    gf = vr.frame_gains(list(CYCLE) * 4, [3] * 24)
    ramp = vr.in_ramp(gf, 256)
    e = vr.envelope(gf, 256)
    # 23 boundaries of one hop each in 72 frames, and the ids at 1.0 keep two of their three hops each (the first id: two and a half)
    assert ramp.sum() == 23 * 256 and (e[~ramp] == 1.0).sum() == (8 * 2) * 256 + 128
    assert np.isfinite(e).all() and e.min() == 0.0 and e.max() == 2.0
    assert ramp.sum() * 4 >= e.size and (e[~ramp] == 1.0).sum() * 10 >= e.size  # what the GPU tests ask of their requests


@pytest.mark.parametrize("defect", vr.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for name, gain, dur, hop in vectors():
        gf = vr.frame_gains(gain, dur)
        x = np.ones(gf.size * hop, F32)
        bad_gf = vr.frame_gains(gain, dur, defect)
        bad = vr.apply(x, bad_gf, hop, defect) if bad_gf.size == gf.size else None
        if bad is None or not np.array_equal(bits(bad), bits(vr.apply(x, gf, hop))):
            caught.append(name)
    print(defect, "caught by", caught)
    assert caught, defect
    assert defect not in (None, "")
