"""CPU: the numpy restatement of the join contract (tests/join_ref.py) validates itself — every planted defect is caught by its named
vector, and the properties the contract states hold: the layout, fades only at cut edges, bit-for-bit copies, +0 silences, the neutral
identities and the capacity bound."""
import numpy as np
import pytest

import join_ref as jr

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    return a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[0]), bits(b[0]))


@pytest.mark.parametrize("defect", sorted(jr.DEFECTS))
def test_every_planted_defect_is_caught_by_its_named_vector(defect):
    items, j, rate, gaps = jr.VECTORS[jr.DEFECTS[defect]]
    good = jr.join(items, j, rate, gaps)
    assert same(good, jr.join(items, j, rate, gaps)), "the reference is deterministic"
    assert not same(good, jr.join(items, j, rate, gaps, **{defect: True})), (defect, jr.DEFECTS[defect])


def test_every_vector_is_named_by_a_defect():
    assert set(jr.DEFECTS.values()) == set(jr.VECTORS)


def test_counts_round_half_up_from_the_widened_float():
    assert jr.S(0.75, 22050) == 17 and jr.S(0.75, 22050, trunc_s=True) == 16
    assert jr.S(200.0, 22050) == 4410 and jr.S(0.0, 48000) == 0 and jr.S(10000.0, 48000) == 480000
    # 0.1f is a little more than 0.1: the float is widened, not the decimal
    assert jr.S(0.1, 5000) == int(np.floor(float(F32(0.1)) * 5.0 + 0.5)) == 1


def test_layout_start_len_total():
    items, j, rate, gaps = jr.VECTORS["empty_middle"]
    y, start, length, total = jr.join(items, j, rate, gaps)
    assert length[1] == 0 and length[0] > 0 and length[2] > 0
    assert start[0] == 0 and start[1] == start[0] + length[0] + jr.S(2.0, rate) and start[2] == start[1] + jr.S(3.0, rate)
    assert total == y.size == start[2] + length[2]
    assert not y[start[0] + length[0]:start[2]].any()
    assert total <= jr.capacity([x.size for x in items], j, rate, gaps)


def test_fades_only_at_cut_edges_and_copies_are_bit_exact():
    items, j, rate, gaps = jr.VECTORS["uncut_edge"]
    y, start, length, _ = jr.join(items, j, rate, gaps)
    Fd = jr.S(j["fade_ms"], rate)
    x0 = items[0]
    k0 = y[start[0]:start[0] + length[0]]
    assert np.array_equal(bits(k0[:-Fd]), bits(x0[:length[0] - Fd])), "item 0: head uncut, copied"
    assert not np.array_equal(bits(k0[-Fd:]), bits(x0[length[0] - Fd:length[0]])), "item 0: tail cut, faded"
    g = jr.ramp(np.arange(Fd), Fd)
    assert g[-1] < 1.0 and g[0] > 0.0 and np.array_equal(k0[::-1][:Fd], x0[:length[0]][::-1][:Fd] * g)


def test_nan_and_inf_are_moved_bit_for_bit_and_inf_is_loud():
    x = np.zeros(32, F32)
    x[4], x[9], x[20] = np.inf, np.nan, -np.inf
    x.view(np.uint32)[9] = 0x7FC12345  # a payload
    y, start, length, _ = jr.join([x], dict(trim=1, trim_threshold=3e38), 8000)
    assert start[0] == 0 and length[0] == 17 and np.array_equal(bits(y), bits(x[4:21]))


def test_neutral_join_is_the_concatenation():
    items = [jr._noise(n, n) for n in (7, 0, 256, 1)]
    y, start, length, total = jr.join(items, {}, 22050)
    assert np.array_equal(bits(y), bits(np.concatenate(items))) and total == 264
    assert list(length) == [7, 0, 256, 1] and list(start) == [0, 7, 7, 263]
    y1, *_ = jr.join(items[2:3], dict(trim=0, trim_threshold=0.3, trim_pad_ms=5.0, fade_ms=5.0), 22050)
    assert np.array_equal(bits(y1), bits(items[2])), "without trim nothing is cut, so nothing fades"


def test_all_quiet_programme_is_only_silences():
    items = [np.zeros(10, F32), np.full(5, 0.01, F32)]
    y, start, length, total = jr.join(items, dict(trim=1, trim_threshold=0.1, lead_ms=1.0, gap_ms=2.0, tail_ms=3.0), 8000)
    assert total == 8 + 16 + 24 and not bits(y).any() and list(length) == [0, 0] and list(start) == [8, 24]
