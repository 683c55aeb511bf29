"""rb_pair_kernel's column tiling: the halo of a tile is conv b's true reach pb = (K − 1)·dil_b / 2, so a 256-column x1 tile
yields 256 − 2·pb output columns in ceil(·/32) conv-b tiles (the last one partial, its dead columns masked in the epilogue), and
conv-b tile j runs on wave column j % 4.

GPU: the op-level ResBlock against the oracle at row lengths just below, at and just past one and two tile edges, and the same
cases bit for bit against the rounded tiling (PIPER_HIP_PAIR_HALO_ROUNDED=1: halos 16 / 48, blocked tile mapping).
CPU: the tile arithmetic restated — every output column is stored exactly once — and the makespans of the launch's snake order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import katdata as kd
from conftest import OP_TOL, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- the tile arithmetic of csrc/rb_pair.hip, restated
COLS_A, WAVE_COLS, SLOTS, MIN_LIVE = 256, 4, 2, 16  # x1 columns per tile; wave columns; conv-b tiles per wave; kMinLiveCols


def reach(K, dil):
    return (K - 1) * dil // 2


def halo_of(pb, exact):
    return pb if exact else (16 if pb <= 16 else 48)


def out_cols_of(pb, exact):
    """Output columns per tile. A partial last conv-b tile with fewer than MIN_LIVE live columns is dropped (232 → 224)."""
    n = COLS_A - 2 * halo_of(pb, exact)
    return n & ~31 if (n & 31) < MIN_LIVE else n


def wave_tiles(pb, exact):
    """Per wave column: the conv-b tiles (32 output columns each, by index) it computes."""
    nt = -(-out_cols_of(pb, exact) // 32)
    if exact:  # tile j on wave column j % 4
        return [[t for t in range(nt) if t % WAVE_COLS == wn][:SLOTS] for wn in range(WAVE_COLS)]
    return [[t for t in range(nt) if t // SLOTS == wn] for wn in range(WAVE_COLS)]  # blocked: tiles 2·wn, 2·wn + 1


def stores_per_column(L, pb, exact):
    """How often each output column of [0, L) is stored, over every (column block, wave column, tile slot, lane)."""
    ncb = out_cols_of(pb, exact)
    ntx = -(-L // ncb)
    hits = np.zeros(L, np.int64)
    max_read = 0
    for wn, tiles in enumerate(wave_tiles(pb, exact)):
        for t in tiles:
            colo = 32 * t + np.arange(32)                 # output column within the block's tile
            colo = colo[colo < ncb]                       # epilogue b's mask
            max_read = max(max_read, int(colo.max()) + halo_of(pb, exact) - pb + 2 * pb)  # last x1 column a STORED column reads
            g = (np.arange(ntx) * ncb)[:, None] + colo[None, :]
            np.add.at(hits, g[g < L], 1)
    return hits, max_read


def simd_loops(pb, exact, C):
    """Conv-b tile loops per SIMD of a block, wave i on SIMD i % 4 (wave = wm + (C/32)·wn)."""
    mt = C // 32
    per = [0] * 4
    for wn, tiles in enumerate(wave_tiles(pb, exact)):
        for wm in range(mt):
            per[(wm + mt * wn) % 4] += len(tiles)
    return per


TILE_COST = {7: 66, 5: 51, 3: 32}  # DESIGN.md finding 20: per-tile cost of the kernel-7 / 5 / 3 pairs of Piper medium
MEDIUM_PAIRS = ((7, 12), (5, 6), (3, 2))  # (K, dil_b), heaviest first as launch_rb_pair_multi orders them


def snake_makespan(L, slots, exact):
    """Tiles of the three pairs in one list, heaviest pair first; block b of G takes b, 2G−1−b, 2G+b, … Returns (tiles, makespan)."""
    tiles = []
    for K, d in MEDIUM_PAIRS:
        tiles += [TILE_COST[K]] * -(-L // out_cols_of(reach(K, d), exact))
    G = min(len(tiles), slots)
    load = [0] * G
    for idx, c in enumerate(tiles):
        rnd, o = divmod(idx, G)
        load[G - 1 - o if rnd & 1 else o] += c
    return len(tiles), max(load)


# ---------------------------------------------------------------- cases
# (type, K, dilations, row lengths): T just below, at and just past one and two tile edges of the exact tiling
# (252 / 232 / 184 columns for reach 2 / 12 / 36; the kernel-5 pair runs 224-column tiles, so 224 / 228 / 452 join its list)
TYPE2 = [(2, 7, [3, 12], [184, 188, 372]), (2, 5, [2, 6], [232, 236, 468, 224, 228, 452]), (2, 3, [1, 2], [252, 256, 508])]
# ResBlock1: conv b has dilation 1 ⇒ reach 1 / 3 / 5 ⇒ 254 / 250 / 246 columns (T must be a multiple of 4 for the pair kernel)
TYPE1 = [(1, 3, [1, 3, 5], [8, 252, 256, 508, 512]), (1, 7, [1, 3, 5], [8, 248, 252, 500, 504]), (1, 11, [1, 3, 5], [8, 244, 248, 492, 496])]
CASES = [(ty, C, T, K, dils, N) for ty, K, dils, Ts in TYPE2 + TYPE1 for T in Ts for C in (32, 64) for N in (1, 2)]
INVARIANCE = [c for c in CASES if c[5] == 2 and c[2] in (188, 372, 236, 228, 468, 256, 508, 8, 252, 504, 496)]
case_id = lambda c: f"rb{c[0]}_C{c[1]}_T{c[2]}_K{c[3]}_d{'-'.join(map(str, c[4]))}_n{c[5]}"


def inputs(case):
    """As test_gpu_ops.test_hifigan_resblock_fused_pairs builds them."""
    type_, Cc, T, K, dils, N = case
    sd = kd.case_seed("cfg", 500 + Cc + T + K)
    nconv = len(dils) * (2 if type_ == 1 else 1)
    x = kd.sym(sd, (N, Cc, T))
    ws = [kd.weight(sd + 1 + i, (Cc, Cc, K), Cc * K) for i in range(nconv)]
    bs = [kd.sym(sd + 40 + i, (Cc,), 0.1) for i in range(nconv)]
    return x, ws, bs


def run(b, case):
    type_, Cc, T, K, dils, N = case
    x, ws, bs = inputs(case)
    up = lambda a: b.uploadFloat32(np.ascontiguousarray(a, np.float32))
    out = b.hifiganResblockF32(type_, up(x), N, Cc, T, K, dils, [up(w) for w in ws], [up(v) for v in bs], 0.1)
    return b.downloadFloat32(out).reshape(N, Cc, T)


def dump(path):
    """Child process of test_tiling_invariance: the INVARIANCE cases → an .npz, with the tuning switches this process honoured."""
    import piper_hip as ph
    b = ph.HipBackend(0)
    out = {case_id(c): run(b, c) for c in INVARIANCE}
    out["config"] = np.array(ph.config_string())
    b.close()
    np.savez(path, **out)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tile_edges_against_oracle(case, backend):
    """A wrong epilogue mask, a wrong first column of conv b or an x1 over-read that reaches a stored value shows at these lengths."""
    import oracle as orc
    type_, Cc, T, K, dils, N = case
    x, ws, bs = inputs(case)
    got = run(backend, case)
    for n in range(N):
        assert_close(got[n], orc.hifigan_resblock(type_, x[n:n + 1], K, dils, ws, bs)[0], OP_TOL, f"item {n} vs oracle")


@pytest.mark.gpu
def test_tiling_invariance(tmp_path):
    """Exact and rounded tiling give every output element the same contraction order (bias-seeded, tap-major, channel pairs
    ascending): bit-identical, no tolerance. The switch is read once per process, so: two child processes."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport test_gpu_rb_pair_tiles as t\nt.dump(sys.argv[1])\n"
            % (os.path.join(ROOT, "piper-swift_amd", "python"), os.path.join(ROOT, "tests")))
    base = {k: v for k, v in os.environ.items() if not k.startswith("PIPER_HIP_")}
    a, r = str(tmp_path / "exact.npz"), str(tmp_path / "rounded.npz")
    subprocess.check_call([sys.executable, "-c", code, a], env=base, timeout=300)
    subprocess.check_call([sys.executable, "-c", code, r], env=dict(base, PIPER_HIP_TUNING="1", PIPER_HIP_PAIR_HALO_ROUNDED="1"), timeout=300)
    ea, er = np.load(a), np.load(r)
    assert "PIPER_HIP_PAIR_HALO_ROUNDED" not in str(ea["config"]) and "PIPER_HIP_PAIR_HALO_ROUNDED=1" in str(er["config"])
    for c in INVARIANCE:
        assert np.array_equal(ea[case_id(c)], er[case_id(c)]), case_id(c)


# ---------------------------------------------------------------- CPU
REACHES = sorted({reach(K, d) for _, K, dils, _ in TYPE2 for d in dils[1:]} | {reach(K, 1) for _, K, _, _ in TYPE1} | {16, 17, 48})
LENGTHS = sorted({T for _, _, _, Ts in TYPE2 + TYPE1 for T in Ts} | {21504, 86016})


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded"])
def test_every_output_column_is_stored_exactly_once(exact):
    for pb in REACHES:
        for L in LENGTHS:
            hits, max_read = stores_per_column(L, pb, exact)
            assert hits.min() == 1 and hits.max() == 1, (pb, L, int(hits.min()), int(hits.max()))
            assert max_read <= COLS_A - 1, (pb, max_read)  # a stored column reads only x1 columns the block computed
        assert all(len(t) <= SLOTS for t in wave_tiles(pb, exact))
        assert sum(len(t) for t in wave_tiles(pb, exact)) == -(-out_cols_of(pb, exact) // 32)  # no tile left without a wave


def test_exact_tiling_widths_and_simd_load():
    assert [out_cols_of(reach(K, d), True) for K, d in MEDIUM_PAIRS] == [184, 224, 252]
    assert [out_cols_of(reach(K, d), False) for K, d in MEDIUM_PAIRS] == [160, 224, 224]
    assert [out_cols_of(reach(K, 1), True) for K in (3, 7, 11)] == [254, 250, 246]
    assert [len(t) for t in wave_tiles(36, True)] == [2, 2, 1, 1] and [len(t) for t in wave_tiles(36, False)] == [2, 2, 1, 0]
    assert [len(t) for t in wave_tiles(2, True)] == [2, 2, 2, 2] and [len(t) for t in wave_tiles(2, False)] == [2, 2, 2, 1]
    for C in (32, 64):
        for pb in REACHES:  # tile j on wave column j % 4 spreads the tiles as evenly over the SIMDs as their count allows
            nt = -(-out_cols_of(pb, True) // 32)
            assert max(simd_loops(pb, True, C)) == -(-nt * (C // 32) // 4), (pb, C)
        for pb in (1, 2, 3, 5, 12, 36):  # Piper's reaches: the busiest SIMD carries no more tile loops than under the rounded tiling
            assert max(simd_loops(pb, True, C)) <= max(simd_loops(pb, False, C)), (pb, C)


def test_simulated_makespans():
    """Snake order over the heaviest-first tile list at costs 66 / 51 / 32: (tiles, makespan) of the two generator launches of
    Piper medium at factor 8 and factor 64, rounded → exact."""
    assert snake_makespan(21504, 256, False) == (327, 83) and snake_makespan(21504, 256, True) == (299, 66)
    assert snake_makespan(86016, 512, False) == (1306, 149) and snake_makespan(86016, 512, True) == (1194, 130)
    assert snake_makespan(8 * 21504, 256, False) == (2612, 560) and snake_makespan(8 * 21504, 256, True) == (2386, 494)
    assert snake_makespan(8 * 86016, 512, False) == (10445, 1092) and snake_makespan(8 * 86016, 512, True) == (9543, 962)
