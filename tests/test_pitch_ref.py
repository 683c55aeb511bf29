"""CPU: the numpy restatement of the pitch contract (tests/pitch_ref.py) checked on its own — the shifted sines against the ideal sine, the
spectral peak, the hand-stated integers of the step, the taps and the counts — and every planted defect caught by a named vector."""
import numpy as np
import pytest

import pitch_ref as pr

F32, F64 = np.float32, np.float64
RATE = 22050
SINE_SHIFTS = (-12.0, -5.0, -0.37, 0.01, 3.0, 7.0, 12.0)


@pytest.fixture(scope="module")
def sines():
    """(f, st) → (y, ρq): one second of a 0.5 sine at f Hz shifted by st, computed once"""
    out = {}
    for f in (200.0, 1000.0, 4000.0):
        x = pr.sine(f, RATE, RATE)
        for st in SINE_SHIFTS:
            out[(f, st)] = (pr.apply(x, st), pr.step(st) / 2.0 ** 32)
    return out


@pytest.mark.parametrize("st", SINE_SHIFTS)
@pytest.mark.parametrize("f", (200.0, 1000.0, 4000.0))
def test_shifted_sine_is_the_ideal_sine(sines, f, st):
    """SNR ≥ 80 dB against 0.5·sin(2π·f·ρq·j / rate) over [200, N' − 200): the reference alone gives 92 … 114 dB, a phase or centre error
    of one step about 40 dB."""
    y, rq = sines[(f, st)]
    assert y.size == pr.count(RATE, pr.step(st))
    j = np.arange(y.size, dtype=F64)
    ideal = 0.5 * np.sin(2.0 * np.pi * f * rq * j / RATE)
    err = (y.astype(F64) - ideal)[200:-200]
    snr = 10.0 * np.log10(np.sum(ideal[200:-200] ** 2) / np.sum(err ** 2))
    print("f %g st %g: SNR %.1f dB, peak %.6f" % (f, st, snr, np.abs(y[200:-200]).max() / 0.5))
    assert snr >= 80.0


@pytest.mark.parametrize("st", SINE_SHIFTS)
@pytest.mark.parametrize("f", (200.0, 1000.0, 4000.0))
def test_spectral_peak_sits_at_the_shifted_frequency(sines, f, st):
    y, rq = sines[(f, st)]
    spec = np.abs(np.fft.rfft(y.astype(F64) * np.hanning(y.size)))
    assert int(np.argmax(spec)) == int(round(f * rq * y.size / RATE))


# st → (Q, P, N' of N = 1, 255, 4097, 22050), stated by hand from 2^(st/12) evaluated to 50 digits at the fp32 value of st:
# 2^(−7/12)·2^32 = 2866546759.5289, 2^(−0.37f/12)·2^32 = 4204149032.8207, 2^(1e-9f/12)·2^32 = 4294967296.2481, 2^(0.01f/12)·2^32 = 4297448882.9791,
# 2^(3/12)·2^32 = 5107605667.1072
STATED = {
    -12.0: (2147483648, 48, (2, 510, 8194, 44100)),
    -7.0: (2866546760, 48, (2, 383, 6139, 33038)),
    -0.37: (4204149033, 48, (2, 261, 4186, 22527)),
    0.0: (4294967296, 48, (1, 255, 4097, 22050)),
    1e-9: (4294967296, 48, (1, 255, 4097, 22050)),
    0.01: (4297448883, 50, (1, 255, 4095, 22038)),
    3.0: (5107605667, 58, (1, 215, 3446, 18542)),
    12.0: (8589934592, 96, (1, 128, 2049, 11025)),
}


@pytest.mark.parametrize("st", sorted(STATED))
def test_step_taps_and_counts_match_the_stated_integers(st):
    Q, P, counts = STATED[st]
    assert pr.step(st) == Q
    assert pr.taps(Q) == P
    assert tuple(pr.count(n, Q) for n in (1, 255, 4097, 22050)) == counts
    assert pr.count(0, Q) == 0
    tab = pr.design(Q)
    assert tab.shape == (129, P) and tab.size * 4 <= 49536
    eps = P * 2.0 ** -52  # P quotients and P sums in double, each rounded by at most 2^-53 of a magnitude below 2
    assert np.abs(tab.sum(axis=1) - 1.0).max() <= eps
    # row 128 is row 0 one sample later
    assert np.abs(tab[128, 1:] - tab[0, :-1]).max() <= eps and tab[128, 0] == 0.0 and tab[0, -1] == 0.0


def test_refusals_of_the_reference():
    for st in (12.5, -12.001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pr.step(st)


def test_neutral_is_the_identity_and_dc_passes():
    x = pr.noise(300, 11)
    x[[3, 100]] = [np.nan, -np.inf]
    for st in (0.0, -0.0, 1e-9):
        assert np.array_equal(pr.apply(x, st).view(np.uint32), x.view(np.uint32))
    y = pr.apply(np.full(400, 0.75, F32), -5.0)
    # P = 48 products and 48 sums, each rounded by at most 2^-25 of a magnitude below 1, and rows whose fp32 taps sum to 1 within 48·2^-25
    assert np.abs(y[60:-60] - 0.75).max() <= 3 * 48 * 2.0 ** -25


def _outputs(**defect):
    """What the named vectors give under a set of defect switches: samples, padded items and tempo factors"""
    ap = {k: v for k, v in defect.items() if k in ("nearest", "alpha_bits", "floor_count", "centre", "f64_sums", "fc_fixed", "clamp")}
    it = {k: v for k, v in defect.items() if k in ("floor_frames", "dirty_tail")}
    inv = defect.get("inverse", False)
    out = {}
    for name, (x, st, hop) in pr.VECTORS.items():
        row, Fp = pr.item(x, st, hop, **it)
        out[name] = (pr.apply(x, st, **ap), row, Fp, pr.length_scale(1.1, st, inverse=inv))
    return out


@pytest.fixture(scope="module")
def good():
    return _outputs()


def _same(a, b):
    return a[2] == b[2] and a[3] == b[3] and all(p.size == q.size and np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a[:2], b[:2]))


ALL_DEFECTS = dict(pr.DEFECTS, **pr.ITEM_DEFECTS, inverse=dict(inverse=True))


@pytest.mark.parametrize("name", sorted(ALL_DEFECTS))
def test_every_planted_defect_changes_a_named_vector(good, name):
    bad = _outputs(**ALL_DEFECTS[name])
    changed = [k for k in pr.VECTORS if not _same(good[k], bad[k])]
    assert changed, name
    assert "neutral" not in changed or name in pr.ITEM_DEFECTS  # Q == 2^32 is not a filter: no defect of the filter can show there


def test_item_pads_with_zeros_to_the_frame_boundary():
    for name, (x, st, hop) in pr.VECTORS.items():
        row, Fp = pr.item(x, st, hop)
        n = pr.count(x.size, pr.step(st))
        assert Fp == -(-n // hop) and row.size == Fp * hop and 0 <= row.size - n < hop
        assert not row[n:].any() and not np.signbit(row[n:]).any()


def test_tempo_factor():
    assert pr.length_scale(0.0, 12.0) == F32(2.0) and pr.length_scale(1.0, -12.0) == F32(0.5)
    assert pr.length_scale(1.1, 3.0) == F32(F32(1.1) * F32(5107605667 / 2.0 ** 32))
    assert pr.length_scale(0.8, 0.0) == F32(0.8)
