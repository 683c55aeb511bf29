"""CPU: the numpy restatement of the equaliser contract (tests/eq_ref.py) against itself and against the plain recurrence.

Measured here, on the 20 000-sample signal below: the block form differs from the sequential recurrence by 1.8e-12 (max|y| 3.96) with
F1, and by 2.4e-10·max|y| with F2 (max|y| 14.0); scipy's sosfilt gives the same figures. The bounds are 1e-9·max(1, max|y|) and
1e-8·max|y|. A cascade of linear time-invariant sections is
the same filter in any order, so the whole cascade reversed is an order defect (other roundings, the same sum); the arithmetic defect
"reverse" runs the blocks' sections last first on the contract's state layout, which the transitions do not match."""
import numpy as np
import pytest

import eq_ref as e

F32 = np.float32
RATE = 22050
ARITHMETIC = ["alpha_q", "a_db20", "reverse", "swap_shelf", "p_next", "zero_start", "pass_nonfinite"]
ORDER = ["ascending", "reverse_all"]


def signal(n=20000, seed=1):
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal(n)).astype(F32)
    x[n // 3: n // 3 + 500] *= F32(4.0)  # a loud stretch
    return x


@pytest.fixture(scope="module")
def x():
    return signal()


@pytest.fixture(scope="module")
def whole(x):
    """the contract's float64 y for F1 and F2, computed once"""
    return {"F1": e.apply64(x, e.F1, RATE), "F2": e.apply64(x, e.F2, RATE)}


@pytest.mark.parametrize("defect", ARITHMETIC)
def test_each_arithmetic_defect_moves_the_output(x, whole, defect):
    xd = x.copy()
    if defect == "pass_nonfinite":
        xd[[100, 7000]] = [np.nan, np.inf]
    y = e.apply64(np.where(np.isfinite(xd), xd, 0).astype(F32), e.F1, RATE)
    assert np.array_equal(y, whole["F1"]) or defect == "pass_nonfinite"
    z = e.apply64(xd, e.F1, RATE, defect)
    bound = 1e-6 * np.max(np.abs(y))
    moved = np.abs(z - y)
    print(f"{defect}: max move {np.nanmax(moved):.3e}, bound {bound:.3e}, NaN {int(np.isnan(moved).sum())}")
    assert not np.all(moved <= bound), defect


@pytest.mark.parametrize("defect", ORDER)
@pytest.mark.parametrize("fset", ["F1", "F2"])
def test_each_order_defect_changes_the_bits(x, whole, defect, fset):
    eq = getattr(e, fset)
    got = e.apply(x, eq, RATE, defect)
    want = whole[fset].astype(F32)
    differ = int(np.sum(got.view(np.int32) != want.view(np.int32)))
    print(f"{fset} {defect}: {differ} samples differ, max move {np.max(np.abs(e.apply64(x, eq, RATE, defect) - whole[fset])):.3e}")
    assert differ > 0


def test_reference_is_the_sequential_recurrence_up_to_rounding(x, whole):
    for fset, rel in (("F1", None), ("F2", 1e-8)):
        y, s = whole[fset], e.sequential(x, getattr(e, fset), RATE)
        d, m = float(np.max(np.abs(y - s))), float(np.max(np.abs(y)))
        print(f"{fset}: max|block − sequential| = {d:.3e}, max|y| = {m:.3f}, relative {d / m:.3e}")
        assert d <= (1e-9 * max(1.0, m) if rel is None else rel * m), fset


def test_scipy_sosfilt_agrees(x, whole):
    signal_ = pytest.importorskip("scipy.signal")
    for fset, rel in (("F1", None), ("F2", 1e-8)):
        co = e.design(getattr(e, fset), RATE)
        sos = np.array([[b0, b1, b2, 1.0, a1, a2] for b0, b1, b2, a1, a2 in co])
        s = signal_.sosfilt(sos, x.astype(np.float64))
        y = whole[fset]
        d, m = float(np.max(np.abs(y - s))), float(np.max(np.abs(y)))
        print(f"{fset}: max|block − sosfilt| = {d:.3e}")
        assert d <= (1e-9 * max(1.0, m) if rel is None else rel * m), fset


def test_zero_db_peaking_returns_its_input(x):
    for eq in ([(e.PEAKING, 1000.0, 0.707, 0.0)], [(e.PEAKING, 50.0, 30.0, 0.0), (e.PEAKING, 9000.0, 0.1, 0.0)]):
        co = e.design(eq, RATE)
        assert all(c[0] == 1.0 for c in co)
        assert np.array_equal(e.apply(x, eq, RATE).view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2373, 20000])
def test_streamed_form_equals_the_whole_item(n):
    x = signal(n, seed=n)
    steps, rng, left = [], np.random.default_rng(n), n
    while left > 0:
        s = min(left, 64 * int(rng.integers(8, 33)))  # 512 … 2048 samples, the last one what is left
        steps.append(s)
        left -= s
    for eq in (e.F1, e.F2):
        got, want = e.streamed(x, eq, RATE, steps), e.apply(x, eq, RATE)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, steps)


def test_non_finite_samples_read_as_zero(x):
    xd = x.copy()
    xd[[5, 900, 15000]] = [np.nan, np.inf, -np.inf]
    want = e.apply(np.where(np.isfinite(xd), xd, 0).astype(F32), e.F1, RATE)
    assert np.array_equal(e.apply(xd, e.F1, RATE).view(np.int32), want.view(np.int32))
