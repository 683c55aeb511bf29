"""CPU: the numpy restatement of the level contract (tests/level_ref.py) validates itself — every planted defect changes the output, the
ceiling holds, prefixes are final exactly up to ready(e), an item under the ceiling passes bit for bit, and the step ranges tile the item."""
import numpy as np
import pytest

import level_ref as lr

F32 = np.float32
LEVEL = (3.0, 0.5, 50.0)
RATE = 22050


def vector(n, seed=7):
    """Speech-like: a carrier under a slow envelope, so that some blocks exceed the ceiling after the drive and some never do."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = 0.02 + 0.3 * np.abs(np.sin(t / 900.0)) ** 4
    return (env * (np.sin(t * 0.21) + 0.3 * rng.standard_normal(n))).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def ref():
    x = vector(5000)
    return x, lr.apply(x, LEVEL, RATE)


def test_vector_limits_some_blocks_and_not_others(ref):
    x, y = ref
    u, node = lr.gains(x, LEVEL, RATE)
    peaks = np.abs(u[:4992]).reshape(-1, 32).max(axis=1)
    assert (peaks > 0.5).mean() >= 0.1
    assert (node == 1.0).any() and (node < 1.0).any()


@pytest.mark.parametrize("defect", [dict(fma_g=True), dict(fma_y=True), dict(lookahead=lr.W - 1), dict(release_after_min=True), dict(node_is_g=True)])
def test_every_planted_defect_changes_the_output(ref, defect):
    x, y = ref
    assert not np.array_equal(bits(lr.apply(x, LEVEL, RATE, **defect)), bits(y)), defect


def test_ceiling_holds_and_node_defect_breaks_it(ref):
    x, y = ref
    bound = F32(0.5) * (1.0 + 2.0 ** -22)
    assert float(np.abs(y).max()) <= bound
    # a sudden peak behind a quiet stretch: with node[k] = G[k] the ramp into the peak's block starts from the gain of the quiet one
    z = np.full(640, 0.1, F32)
    z[320] = 0.9
    assert float(np.abs(lr.apply(z, (1.0, 0.5, 50.0), RATE)).max()) <= bound
    z[320:352] = 0.9
    assert float(np.abs(lr.apply(z, (1.0, 0.5, 50.0), RATE)).max()) <= bound
    assert float(np.abs(lr.apply(z, (1.0, 0.5, 50.0), RATE, node_is_g=True)).max()) > bound


@pytest.mark.parametrize("e", [512, 777, 1024, 2049, 4000])
def test_prefix_is_final_up_to_ready_and_not_one_block_further(e):
    x = vector(5000, seed=e) * F32(0.1)  # quiet: nothing limits …
    x[e] = 0.95                          # … but a large peak just past e, which the prefix cannot know
    whole = lr.apply(x, (1.0, 0.5, 50.0), RATE)
    part = lr.apply(x[:e], (1.0, 0.5, 50.0), RATE)
    r = lr.ready(e)
    assert r == 32 * (e // 32 - 7) and r > 0
    assert np.array_equal(bits(part[:r]), bits(whole[:r]))
    assert not np.array_equal(bits(part[r:r + 32]), bits(whole[r:r + 32]))
    # the planted defects of ready: one block late is wrong on that vector, one block early wastes a block but is still exact
    late, early = lr.ready(e, +1), lr.ready(e, -1)
    assert late == r + 32 and early == r - 32
    assert not np.array_equal(bits(part[:late]), bits(whole[:late]))


def test_release_returns_to_unity():
    # a gain of 0.1 returns to exactly 1.0 in 32 blocks at 22 050 Hz / 50 ms
    rel = lr.rel((1, 1, 50), 22050)
    assert rel == F32(min(1.0, 32000.0 / (22050 * 50.0)))
    x = np.zeros(32 * 80, F32)
    x[0] = 10.0
    _, node = lr.gains(x, (1.0, 1.0, 50.0), 22050)
    assert node[0] == F32(1.0) / F32(10.0)
    first_one = int(np.argmax(node == 1.0))  # G[32] is the first G at 1.0, so node[33] = min(G[32], G[33]) is the first node there
    assert first_one == 33 and (node[first_one:] == 1.0).all() and node[32] < 1.0


def test_item_under_the_ceiling_passes_bit_for_bit():
    x = vector(3000) * F32(0.5)
    x[17] = np.nan
    assert float(np.nanmax(np.abs(x))) < 1.0
    y = lr.apply(x, (0, 0, 0), RATE)
    assert np.array_equal(bits(y), bits(x))


@pytest.mark.parametrize("hop,chunk", [(256, 2), (256, 3), (200, 3), (200, 7)])
@pytest.mark.parametrize("frames", [1, 2, 7, 19, 40])
def test_step_ranges_tile_the_item_within_the_bound(hop, chunk, frames):
    assert hop * chunk >= 512
    N = frames * hop
    ranges = lr.step_ranges(frames, chunk, hop)
    assert ranges[0][0] == 0 and ranges[-1][1] == N
    f = 0
    for i, (lo, hi) in enumerate(ranges):
        s, f = f * hop, min(frames, f + chunk)
        assert hi > lo, "a step delivers something"
        assert i == 0 or lo == ranges[i - 1][1]
        assert hi - lo <= lr.step_bound(f * hop - s)
        assert s - lo <= lr.CARRY
    assert sum(hi - lo for lo, hi in ranges) == N
    x = vector(N, seed=frames)
    assert np.array_equal(bits(lr.apply_chunked(x, LEVEL, RATE, frames, chunk, hop)), bits(lr.apply(x, LEVEL, RATE)))
