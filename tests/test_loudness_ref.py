"""CPU: the numpy restatement of BS.1770 integrated loudness (tests/loudness_ref.py) against known answers, and the planted defects that
the tolerance of the device tests (0.002 LU) must be able to tell from the contract: each moves the reference by more than 0.02 LU on a
signal whose gates it exercises."""
import math

import numpy as np
import pytest

import loudness_ref as ld

RATES = (16000, 22050)


@pytest.fixture(scope="module")
def measured():
    """{(signal, rate): measure(...)} once for the module"""
    return {(name, rate): ld.measure(getattr(ld, name)(rate), rate) for name in ("s1", "s2", "s3") for rate in RATES}


def test_coefficients_at_48k_are_the_standards_table():
    sb, sa, hb, ha = ld.coeffs(48000)
    assert abs(sb[0] - 1.53512485958697) < 1e-12 and abs(sa[1] + 1.69065929318241) < 1e-12
    assert abs(sb[1] + 2.69169618940638) < 1e-12 and abs(sb[2] - 1.19839281085285) < 1e-12 and abs(sa[2] - 0.73248077421585) < 1e-12
    assert abs(ha[1] + 1.99004745483398) < 1e-12 and abs(ha[2] - 0.99007225036621) < 1e-12
    assert list(hb) == [1.0, -2.0, 1.0] and sa[0] == ha[0] == 1.0


@pytest.mark.parametrize("rate,want", [(48000, -3.010), (22050, -2.981), (16000, -2.970)])
def test_full_scale_997_hz_sine(rate, want):
    x = ld.sine(rate)
    L = ld.lufs(x, rate)
    assert abs(L - want) <= 0.005, L
    tenth = ld.lufs((0.1 * x.astype(np.float64)).astype(np.float32), rate)
    assert abs((L - tenth) - 20.0) < 1e-6  # (the fp32 rounding of 0.1·x is all that separates them from exactly 20)


def test_biquad_agrees_with_scipy():
    signal = pytest.importorskip("scipy.signal")
    x = ld.s2(22050).astype(np.float64)
    sb, sa, hb, ha = ld.coeffs(22050)
    want = signal.lfilter(hb, ha, signal.lfilter(sb, sa, x))
    assert np.max(np.abs(ld.kweight(x.astype(np.float32), 22050) - want)) < 1e-12


def test_the_signals_show_the_gates_they_are_meant_to(measured):
    for rate in RATES:
        m1, m2, m3 = (measured[(s, rate)] for s in ("s1", "s2", "s3"))
        assert m1["blocks"] == m1["abs"] == m1["rel"] == 27
        # S2: the relative gate alone takes blocks
        assert m2["blocks"] == 37 and m2["abs"] == m2["blocks"] and 4 <= m2["rel"] < m2["abs"], m2
        # S3: the absolute gate takes the silence, the relative gate the quiet tail
        assert m3["blocks"] == 35 and 4 <= m3["rel"] < m3["abs"] < m3["blocks"], m3


@pytest.mark.parametrize("defect", ld.DEFECTS)
def test_every_planted_defect_moves_the_reference(measured, defect):
    moved = {}
    for rate in RATES:
        for name in ("s2", "s3"):
            moved[(name, rate)] = ld.lufs(getattr(ld, name)(rate), rate, defect) - measured[(name, rate)]["L"]
    print(defect, {k: round(v, 4) for k, v in moved.items()})
    for rate in RATES:  # on S2 or S3, at every rate
        assert max(abs(moved[("s2", rate)]), abs(moved[("s3", rate)])) > 0.02, (defect, rate, moved)


@pytest.mark.parametrize("n,blocks", [(8819, 0), (8820, 1), (11024, 1), (11025, 2)])
def test_edges_at_22050(n, blocks):
    m = ld.measure(ld.s1(22050)[:n], 22050)
    assert m["blocks"] == blocks == ld.block_count(n, 22050)
    assert (m["L"] == -math.inf) == (blocks == 0)


def test_silence_and_non_finite_samples():
    assert ld.lufs(np.zeros(22050, np.float32), 22050) == -math.inf  # every block under the absolute gate
    assert ld.lufs(np.empty(0, np.float32), 22050) == -math.inf
    x = ld.s1(22050).copy()
    y = x.copy()
    y[[3, 30000]] = [np.nan, np.inf]
    x[[3, 30000]] = 0.0
    assert ld.lufs(y, 22050) == ld.lufs(x, 22050)


def test_gain_formula():
    assert ld.gain((0.0, 0.0), -8.64) == np.float32(10.0 ** ((-16.0 - float(np.float32(-8.64))) / 20.0))
    assert ld.gain((-3.0, 6.0), -11.07) == np.float32(10.0 ** (6.0 / 20.0))  # capped
    assert ld.gain((-3.0, 6.0), -8.0) == np.float32(10.0 ** (5.0 / 20.0))
    assert ld.gain((-70.0, 0.0), -1.0) == np.float32(10.0 ** (-69.0 / 20.0))  # attenuation is unbounded
    assert ld.gain((-16.0, 0.0), -math.inf) == np.float32(1.0)
