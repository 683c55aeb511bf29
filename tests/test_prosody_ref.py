"""CPU: tests/prosody_ref.py, the numpy restatement of the prosody contract (include/piper_hip.h "Per-phoneme prosody"). A fixed battery of
inputs must tell the reference from five planted defects — what the GPU tests rely on when they hold the kernels to it — and the
properties the header states must hold on random inputs."""
import numpy as np
import pytest

import prosody_ref as pr


def battery():
    """(w0, prosody, cap, noise_scale) cases: fractions that ceil differently before and after the multiply, floors above ceilings' reach,
    NaN, values over 1e6, totals over the bound whose scaled parts have fractions ≥ .5 and products past 2^31."""
    rng = np.random.default_rng(20251)
    cases = []
    w0 = np.array([2.4, 0.7, 3.0, 5.5, 1.2, 0.0, 7.9], np.float32)
    p = dict(length=np.array([0.5, 1.7, 1.0, 0.3, 2.5, 1.0, 1.0], np.float32), min_frames=np.array([0, 0, 6, 0, 0, 2, 0], np.int32),
             max_frames=np.array([0, 1, 8, 0, 2, 0, 3], np.int32), noise=np.array([1.0, 0.0, 0.5, 2.0, 1.0, 0.25, 3.0], np.float32), fit=1)
    cases.append((w0, p, 11, 0.667))
    cases.append((w0, dict(p, fit=0), 11, 0.667))
    # a floor above its ceiling: the rule's order (ceiling, then floor) decides, so the floor wins. piper_hip_prosody_check refuses such a
    # record; the arithmetic is defined all the same, and only here can the two orders be told apart.
    cases.append((w0, dict(min_frames=np.array([0, 4, 0, 0, 0, 0, 0], np.int32), max_frames=np.array([0, 2, 0, 0, 0, 0, 0], np.int32)), 0, 1.0))
    cases.append((np.array([np.nan, 3e6, 1e6, 999999.5, -2.0], np.float32), dict(length=np.array([1, 1, 1, 1, 1], np.float32), fit=1), 1 << 20, 1.0))
    cases.append((np.array([9e5, 8e5, 7e5, 3.0], np.float32), dict(fit=1), 70000, 0.5))  # d · cap past 2^31
    # 749103 · 51010 / 1802866 = 21194.99997…: the fp32 quotient rounds up to 21195
    cases.append((np.array([749103, 961658, 92105], np.float32), dict(fit=1), 51010, 0.5))
    for _ in range(6):
        t = int(rng.integers(3, 40))
        w0 = (rng.random(t) * 9).astype(np.float32)
        p = dict(length=(rng.random(t) * 2).astype(np.float32), min_frames=rng.integers(0, 4, t).astype(np.int32),
                 max_frames=np.where(rng.random(t) < 0.3, rng.integers(4, 9, t), 0).astype(np.int32), noise=(rng.random(t) * 2).astype(np.float32), fit=1)
        cases.append((w0, p, int(rng.integers(5, 60)), 0.8))
    return cases


def reference(w0, p, cap, noise_scale):
    used, wanted = pr.frames(w0, p, cap)
    return used, wanted, pr.frame_ns(used, noise_scale, p)


def agrees(impl):
    for case in battery():
        a, b = impl(*case), reference(*case)
        if not (np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])):
            return False
    return True


def _rule(w0, p, floor_first=False, length_after_ceil=False):
    w0 = np.asarray(w0, np.float32)
    t = w0.size
    ln = np.asarray(p.get("length", np.ones(t)), np.float32)
    mn = np.asarray(p.get("min_frames", np.zeros(t)), np.int64)
    mx = np.asarray(p.get("max_frames", np.zeros(t)), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.ceil(np.ceil(w0) * ln) if length_after_ceil else np.ceil((w0 * ln).astype(np.float32))
        d0 = np.nan_to_num(np.where(c > 0, np.minimum(c, np.float32(1e6)), 0), nan=0.0).astype(np.int64)
    if floor_first:
        d = np.maximum(d0, mn)
        return np.where(mx > 0, np.minimum(d, mx), d).astype(np.int32)
    d1 = np.where(mx > 0, np.minimum(d0, mx), d0)
    return np.maximum(d1, mn).astype(np.int32)


def _with(durations=None, fit=None, ns=None):
    def impl(w0, p, cap, noise_scale):
        d = (durations or pr.durations)(w0, p)
        used, S, _ = (fit or pr.fit)(d, cap, bool(p.get("fit")))
        return used, S, (ns or pr.frame_ns)(used, noise_scale, p)
    return impl


def fit_rounding(d, cap, want):
    d = np.asarray(d, np.int64)
    S = int(d.sum())
    if want and S > cap:
        return np.array([(2 * int(x) * cap + S) // (2 * S) for x in d], np.int32), S, 1
    return d.astype(np.int32), S, 0


def fit_float(d, cap, want):
    d = np.asarray(d, np.int64)
    S = int(d.sum())
    if want and S > cap:
        return np.floor(d.astype(np.float32) * np.float32(cap) / np.float32(S)).astype(np.int32), S, 1
    return d.astype(np.int32), S, 0


def ns_by_frame_index(d, noise_scale, p):
    n = pr.frame_count(d)
    noise = np.asarray(p.get("noise", np.ones(len(d))), np.float32)
    return (np.float32(noise_scale) * noise[np.minimum(np.arange(n), noise.size - 1)]).astype(np.float32)


DEFECTS = {
    "floor applied before the ceiling": _with(durations=lambda w0, p: _rule(w0, p, floor_first=True)),
    "length applied after ceil": _with(durations=lambda w0, p: _rule(w0, p, length_after_ceil=True)),
    "fit rounds instead of flooring": _with(fit=fit_rounding),
    "fit computed in float": _with(fit=fit_float),
    "ns taken from id f instead of t(f)": _with(ns=ns_by_frame_index),
}


def test_the_battery_accepts_the_reference_and_an_independent_restatement():
    assert agrees(reference)
    assert agrees(_with(durations=lambda w0, p: _rule(w0, p)))  # the rule written a second time, the same order


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect_is_caught(name):
    assert not agrees(DEFECTS[name]), name


def test_fitted_total_never_exceeds_the_bound():
    rng = np.random.default_rng(7)
    for _ in range(300):
        t = int(rng.integers(1, 200))
        d = rng.integers(0, int(rng.choice([4, 50, 1000000])) + 1, t)
        cap = int(rng.integers(1, 1 << int(rng.integers(1, 30))))
        used, S, fitted = pr.fit(d, cap)
        assert S == int(d.sum()) and fitted == int(S > cap)
        assert int(used.astype(np.int64).sum()) <= max(cap, S if not fitted else 0)
        if fitted:
            assert int(used.astype(np.int64).sum()) <= cap and np.all(used <= d)
        else:
            assert np.array_equal(used, d)


def test_an_all_zero_result_still_yields_one_frame():
    d = pr.durations(np.array([0.0, -1.0, np.nan], np.float32))
    assert d.tolist() == [0, 0, 0]
    assert pr.frame_count(d) == 1 and pr.frame_ids(d).tolist() == [0]
    assert pr.frame_ns(d, 0.5, dict(noise=[3.0, 1.0, 1.0])).tolist() == [1.5]
    used, S, fitted = pr.fit(np.array([1, 1, 1]), 2)  # fitting may take everything: ⌊1 · 2 / 3⌋ = 0
    assert used.tolist() == [0, 0, 0] and (S, fitted) == (3, 1) and pr.frame_count(used) == 1


def test_neutral_prosody_is_the_identity():
    rng = np.random.default_rng(11)
    w0 = (rng.random(64) * 12).astype(np.float32)
    w0[5], w0[9] = np.nan, 4e6
    t = w0.size
    neutral = dict(length=np.ones(t, np.float32), min_frames=np.zeros(t, np.int32), max_frames=np.zeros(t, np.int32), noise=np.ones(t, np.float32))
    with np.errstate(invalid="ignore"):
        c = np.ceil(w0)
        plain = np.nan_to_num(np.where(c > 0, np.minimum(c, 1e6), 0), nan=0.0).astype(np.int32)  # the step without prosody
    for p in (None, {}, neutral):
        assert np.array_equal(pr.durations(w0, p), plain)
        assert np.array_equal(pr.frame_ns(plain, 0.667, p), np.full(pr.frame_count(plain), np.float32(0.667)))
    m, lg = rng.standard_normal((3, t)), rng.standard_normal((3, t)) * 0.1
    nz = rng.standard_normal((3, pr.frame_count(plain)))
    assert np.array_equal(pr.expand(m, lg, plain, nz, 0.667, neutral), pr.expand(m, lg, plain, nz, 0.667, None))
