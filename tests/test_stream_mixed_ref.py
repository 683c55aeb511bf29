"""CPU: the mixed-format reference (tests/mixed_ref.py) against the contracts it is built from — the layout rule on hand-written counts,
per format the concatenation of the step ranges against the whole-item conversion, and the defects a mixed step could have, each planted
into the reference and required to show."""
import numpy as np
import pytest

import mixed_ref as mr
import resample_ref as rr
from mixed_ref import Format

HOP, CHUNK, RATE = 256, 2, 22050


def signal(frames, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(frames * HOP, dtype=np.float64)
    x = 0.5 * np.sin(t * 0.031 * (1 + seed % 3)) + 0.2 * rng.standard_normal(t.size)
    return x.astype(np.float32)


def chunks_of(x, chunk_frames=CHUNK):
    step = chunk_frames * HOP
    return [x[i:i + step] for i in range(0, x.size, step)]


# ---- the layout rule

def test_layout_on_hand_written_counts():
    # an odd-length μ-law row in front of an s16 row: 5 bytes, then the s16 row at 8
    assert mr.layout([5, 3], [1, 2]) == ([0, 8], 14)
    # an empty row between two delivering rows owns nothing and reports where the next one starts
    assert mr.layout([3, 0, 2], [1, 2, 4]) == ([0, 4, 4], 12)
    # the first delivering row is at 0 whatever is empty in front of it; nothing follows the last row's end
    assert mr.layout([0, 0, 7, 1], [4, 1, 1, 2]) == ([0, 0, 0, 8], 10)
    assert mr.layout([0, 0], [2, 2]) == ([0, 0], 0)
    # ends that are multiples of 4 already are not padded
    assert mr.layout([4, 2, 1], [1, 2, 4]) == ([0, 4, 8], 12)
    # a trailing empty row reports the rounded end; the total does not count its pad
    assert mr.layout([1, 0], [1, 2]) == ([0, 4], 1)


def test_layout_defect_offset_not_rounded_up():
    good, bad = mr.layout([5, 3], [1, 2]), mr.layout([5, 3], [1, 2], round_up=False)
    assert bad == ([0, 5], 11) and bad != good
    # … and through expected(): the s16 row's bytes move
    a, b = signal(2, 1), signal(2, 2)
    sessions = [dict(row=0, start=0, chunks=[a[:5]], fmt=Format(0, "mulaw")), dict(row=1, start=0, chunks=[b[:3]], fmt=Format(0, "s16"))]
    want = mr.expected(sessions, 2, RATE, 1, 5)[0]
    off = mr.expected(sessions, 2, RATE, 1, 5, round_up=False)[0]
    assert want[1] == [0, 8] and off[1] == [0, 5] and not mr.same_step((off[0], off[1], off[2]), want)
    assert mr.same_step((want[0], want[1], want[2]), want)
    pad = want[2].copy()
    pad[~want[3]] ^= 0xFF  # the pad bytes are unspecified: whatever they hold, the step is the same
    assert (~want[3]).sum() == 3 and mr.same_step((want[0], want[1], pad), want)


# ---- per format: the steps of a row concatenate to the whole-item conversion

FORMATS = [Format(0, "s16", 1.0), Format(0, "mulaw", 0.5), Format(0, "alaw", 1.0), Format(0, "f32", 1.0),
           Format(8000, "mulaw", 1.0), Format(8000, "alaw", 1.7), Format(48000, "s16", 0.5), Format(16000, "alaw", 1.0),
           Format(11025, "f32", 1.0), Format(32000, "s16", 1.0), Format(48000, "f32", 1.0)]


@pytest.mark.parametrize("f", FORMATS, ids=lambda f: "%d-%s-%g" % f)
@pytest.mark.parametrize("chunk", [1, 2])
def test_steps_concatenate_to_the_whole_item(f, chunk):
    """Includes F32 at a rate, which no stream test covers elsewhere. 7 frames: the last chunk of a 2-frame stream is short."""
    x = signal(7, 3)
    steps = mr.row_steps(chunks_of(x, chunk), f, RATE, HOP, chunk)
    want = mr.whole(x, f, RATE)
    got = np.concatenate(steps)
    assert got.dtype == want.dtype == mr.DTYPE[f.enc] and got.size == mr.total_samples(x.size, f, RATE)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    bound = mr.step_bound_bytes(f, RATE, chunk * HOP)
    assert all(s.size * mr.ELEM[f.enc] <= bound for s in steps) and bound % 4 == 0
    if f.rate:
        L, M, P = rr.ratio(RATE, f.rate)
        assert [s.size for s in steps] == [b - a for a, b in rr.stream_ranges(7, chunk, HOP, L, M, P)]
    else:
        assert [s.size for s in steps] == [c.size for c in chunks_of(x, chunk)]


def test_an_unfinished_row_is_a_prefix():
    """a dropped row: its steps are the prefix of the whole item's, by the emit rule of a row whose item goes on"""
    f, x = Format(8000, "alaw"), signal(8, 5)
    full = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK)
    part = mr.row_steps(chunks_of(x)[:2], f, RATE, HOP, CHUNK, finished=False)
    assert len(part) == 2 and all(np.array_equal(a, b) for a, b in zip(part, full))


def test_expected_places_every_row_of_every_step():
    a, b, c = signal(4, 7), signal(2, 8), signal(3, 9)
    fa, fb, fc = Format(8000, "mulaw"), Format(48000, "s16", 0.5), Format(0, "f32")
    sessions = [dict(row=0, start=0, chunks=chunks_of(a), fmt=fa), dict(row=1, start=0, chunks=chunks_of(b), fmt=fb),
                dict(row=1, start=1, chunks=chunks_of(c), fmt=fc)]  # c takes row 1 after b's only step
    steps = mr.expected(sessions, 3, RATE, HOP, CHUNK)
    assert len(steps) == 3
    rows = {0: [], 1: []}
    for counts, offs, data, mask in steps:
        assert counts[2] == 0 and offs[0] == 0 and all(o % 4 == 0 for o in offs)
        for r in (0, 1):
            el = 1 if r == 0 else (2 if len(rows[1]) == 0 else 4)
            assert mask[offs[r]:offs[r] + counts[r] * el].all()
            rows[r].append(data[offs[r]:offs[r] + counts[r] * el])
    assert np.array_equal(np.concatenate(rows[0]), mr.whole(a, fa, RATE).view(np.uint8))
    assert np.array_equal(rows[1][0], mr.whole(b, fb, RATE).view(np.uint8))
    assert np.array_equal(np.concatenate(rows[1][1:]), mr.whole(c, fc, RATE).view(np.uint8))


# ---- planted defects: each must show against the honest reference

def test_defect_another_rows_filter():
    x = signal(6, 11)
    f, neighbour = Format(8000, "s16"), Format(11025, "s16")
    good = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK)
    bad = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK, as_format=neighbour)
    assert [s.size for s in good] != [s.size for s in bad]  # another (L, M, P): other counts in every step …
    g, b = np.concatenate(good), np.concatenate(bad)
    assert not np.array_equal(g, b[:g.size])  # … and other samples
    sessions = [dict(row=0, start=0, chunks=chunks_of(x), fmt=f), dict(row=1, start=0, chunks=chunks_of(x), fmt=neighbour)]
    swapped = [dict(sessions[0], as_format=neighbour), sessions[1]]
    for want, got in zip(mr.expected(sessions, 2, RATE, HOP, CHUNK), mr.expected(swapped, 2, RATE, HOP, CHUNK)):
        assert not mr.same_step(got[:3], want)


def test_defect_another_rows_gain():
    x = signal(4, 12)
    f, neighbour = Format(8000, "mulaw", 1.0), Format(8000, "mulaw", 0.5)
    good = np.concatenate(mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK))
    bad = np.concatenate(mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK, as_format=neighbour))
    assert good.size == bad.size and not np.array_equal(good, bad)
    s16 = Format(0, "s16", 0.5)
    assert not np.array_equal(mr.whole(x, s16, RATE), mr.whole(x, s16._replace(gain=1.0), RATE))


@pytest.mark.parametrize("f", [Format(8000, "mulaw"), Format(16000, "alaw"), Format(48000, "s16")], ids=lambda f: "%d-%s-%g" % f)
def test_defect_inherited_history(f):
    """a new occupant whose first step reads the previous occupant's last samples before its own sample 0"""
    prev, x = signal(3, 13), signal(4, 14)
    good = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK)
    bad = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK, inherit=prev)
    assert [s.size for s in good] == [s.size for s in bad]
    assert not np.array_equal(good[0], bad[0])  # the first chunk shows it …
    assert all(np.array_equal(a, b) for a, b in zip(good[1:], bad[1:]))  # … and only the first
    silent = mr.row_steps(chunks_of(x), f, RATE, HOP, CHUNK, inherit=np.zeros(HOP, np.float32))
    assert np.array_equal(good[0], silent[0])  # an inherited silence is the honest start: the planting itself is sound
