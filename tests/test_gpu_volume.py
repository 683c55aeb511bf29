"""GPU: per-phoneme volume (include/piper_hip.h "Per-phoneme volume") — the gain envelope as a per-op, on every whole-item route and on
single streams, groups and pools. The raw
fp32 reference is always the GPU's own audio of the same request without a volume; on top of it tests/volume_ref.py and the existing
pcm_ref / level_ref / loudness_ref / mixed_ref are applied and compared bit for bit, counts included.

Gains cycle through (1, 0.25, 1, 2, 0, 1.5). With 3 frames per id a third of the samples lie in ramps and 2/9 sit at exactly 1.0; the
tests assert from the reference alone that at least 1/4 of the shaped samples are in ramps and at least 1/10 at exact unity, and that the
raw audio differs from v on more than half of the samples with e ≠ 1: a request that never ramps, or never rests, shows nothing. On
predicted durations the weaker form is asserted from the reported durations: at least one ramp and one stretch at unity."""
import os
import subprocess

import numpy as np
import pytest

import katdata as kd
import level_ref as lr
import loudness_ref as ld
import mixed_ref as mr
import pcm_ref
import piper_hip as ph
import volume_ref as vr
from mixed_ref import Format
from test_gpu_level import DEV, SINKS, collect_as, expected_row, item, rt_medium, same, shaped, stream_kw  # noqa: F401  (rt_medium: the fixture)
from test_gpu_resample import same_bits
from test_gpu_stream_mixed import TABLES
from test_volume_ref import CYCLE, signal

pytestmark = pytest.mark.gpu

F32 = np.float32


def cycle(n):
    return np.resize(np.array(CYCLE, F32), n)


def shares(gfs, hop):
    """(samples in ramps, samples at exactly 1.0 outside ramps, samples) over items with the gains per frame gfs"""
    ramp = unity = total = 0
    for gf in gfs:
        r, e = vr.in_ramp(gf, hop), vr.envelope(gf, hop)
        ramp, unity, total = ramp + int(r.sum()), unity + int((e[~r] == 1.0).sum()), total + e.size
    return ramp, unity, total


def differs_where_shaped(raws, gfs, hop):
    """the raw audio must differ from v on more than half of the samples with e ≠ 1"""
    diff = n = 0
    for x, gf in zip(raws, gfs):
        e = vr.envelope(gf, hop)
        diff, n = diff + int((vr.apply(x, gf, hop)[e != 1.0] != x[e != 1.0]).sum()), n + int((e != 1.0).sum())
    print(f"raw differs from v on {diff} of {n} samples with e != 1")
    assert n > 0 and diff * 2 > n, (diff, n)


# ---- 1. per-op

@pytest.mark.parametrize("hop", [256, 6, 250])
@pytest.mark.parametrize("frames", [1, 2, 37])
def test_per_op(backend, frames, hop):
    n = frames * hop
    x = signal(n, 17 * frames + hop)
    rng = np.random.default_rng(frames + hop)
    for gf in (cycle(frames), rng.uniform(0.0, 16.0, frames).astype(F32), np.ones(frames, F32)):
        want = vr.apply(x, gf, hop)
        assert same_bits(ph.volume_from_f32(x, gf, hop), want)
        g = backend.uploadFloat32(gf)
        # an aligned source into a buffer of the library's
        assert same_bits(backend.downloadFloat32(backend.volume(backend.uploadFloat32(x), g, hop), n), want), "aligned"
        # a source one float off the alignment
        buf = backend.uploadFloat32(np.concatenate([np.zeros(1, F32), x]))
        off = ph.DeviceBuffer(backend, buf.ptr + 4, n, owned=False)
        assert same_bits(backend.downloadFloat32(backend.volume(off, g, hop), n), want), "unaligned source"
        # a destination of the caller's, one float off too: the floats around it stay
        dst = backend.uploadFloat32(np.full(n + 2, 7.0, F32))
        out = backend.volume(backend.uploadFloat32(x), g, hop, out=dst.ptr + 4)
        assert out.ptr == dst.ptr + 4
        whole = backend.downloadFloat32(dst, n + 2)
        assert whole[0] == 7.0 and whole[-1] == 7.0 and same_bits(whole[1:-1], want), "caller's destination"
    assert same_bits(backend.downloadFloat32(backend.volume(backend.uploadFloat32(x), backend.uploadFloat32(np.ones(frames, F32)), hop), n), x)


def test_per_op_more_than_one_block_and_refusals(backend):
    frames, hop = 300, 256  # 76 800 samples: 75 thread blocks
    x = signal(frames * hop, 5)
    gf = cycle(frames)
    got = backend.downloadFloat32(backend.volume(backend.uploadFloat32(x), backend.uploadFloat32(gf), hop), x.size)
    assert same_bits(got, vr.apply(x, gf, hop))
    g, xb = backend.uploadFloat32(np.ones(3, F32)), backend.uploadFloat32(np.zeros(12, F32))
    with pytest.raises(ph.ShapeMismatch, match="11 samples"):
        backend.volume(xb, g, 4, count=11)
    with pytest.raises(ph.InvalidArgument, match="hop 0"):
        backend.volume(xb, g, 0, count=0)
    with pytest.raises(ph.InvalidArgument, match="hop 65537"):
        backend.volume(xb, g, 65537, count=12)
    assert backend.volume(xb, ph.DeviceBuffer(backend, g.ptr, 0, owned=False), 4).count == 0  # count may be 0


# ---- 2. whole items: a ragged batch, one item with zero-duration ids, one without a volume

RAGGED_DURS = ([3] * 12, [3, 0, 3, 3, 0, 3, 3, 3], [3] * 5)


def ragged_request(cfg):
    return [shaped(cfg, d, 40 + k) for k, d in enumerate(RAGGED_DURS)]


def ragged_volume():
    return [cycle(12), cycle(8)]  # the third item is past the list: it has none


@pytest.fixture(scope="module")
def ragged_case(rt_medium):
    """The request without a volume (its raw items, its steps, its plain bytes), then the same request with one, launched on slot 5.
    Computed once; the tests below only collect."""
    rt, hop = rt_medium, rt_medium.cfg.hop
    rt.slot_level(5, None)
    rt.slot_loudness(5, None)
    rt.prepare_batch(5, ragged_request(rt.cfg), 0.667)
    rt.launch(5)
    raw = rt.collect(5).copy()
    per, total = rt.prepared_samples(5)
    assert per == [sum(d) * hop for d in RAGGED_DURS] and raw.size == total
    steps = rt.steps(5)
    plain = {name: collect_as(rt, 5, name).copy() for name in SINKS}
    raws = np.split(raw, np.cumsum(per)[:-1])
    gfs = [vr.frame_gains(g, d) for g, d in zip(ragged_volume(), RAGGED_DURS)]
    ramp, unity, total_v = shares(gfs, hop)
    print(f"ragged: {ramp} of {total_v} shaped samples in ramps, {unity} at exact unity")
    assert ramp * 4 >= total_v and unity * 10 >= total_v, (ramp, unity, total_v)
    differs_where_shaped(raws, gfs, hop)
    v = [vr.apply(x, gf, hop) for x, gf in zip(raws, gfs)] + [raws[2]]
    rt.prepare_batch(5, ragged_request(rt.cfg), 0.667, volume=ragged_volume())
    rt.launch(5)
    return dict(raw=raw, raws=raws, v=v, gfs=gfs, per=per, steps=steps, plain=plain)


def test_whole_items_on_every_sink(rt_medium, ragged_case):
    rt, rate, c = rt_medium, rt_medium.cfg.sample_rate, ragged_case
    assert rt.prepared_samples(5)[0] == c["per"]  # no count changes
    for name, fmt in SINKS.items():
        want = np.concatenate([mr.whole(it, fmt, rate, TABLES) for it in c["v"]])
        assert same(collect_as(rt, 5, name), want), name
    # s16 with a gain of 0.5
    assert np.array_equal(rt.collect_pcm16(5, gain=0.5), pcm_ref.pcm16_items(c["v"], 0.5))
    # the item without a volume keeps its raw bits, the others do not
    got = np.split(rt.collect(5), np.cumsum(c["per"])[:-1])
    assert same_bits(got[2], c["raws"][2]) and not same_bits(got[0], c["raws"][0]) and not same_bits(got[1], c["raws"][1])
    # the plan's audio and the audio tap stay raw, and the steps are those of the request without a volume
    assert same_bits(rt.tap(5, "audio").reshape(-1), c["raw"])
    assert rt.steps(5) == c["steps"]
    # the tap: gf compacted to every item's true F
    want_gf = np.concatenate(c["gfs"] + [np.ones(len(RAGGED_DURS[2]) * 3, F32)])
    assert same_bits(rt.tap(5, "vol.gain").reshape(-1), want_gf)


def test_whole_items_normalize_reads_the_peak_of_v(rt_medium, ragged_case):
    rt, c = rt_medium, ragged_case
    for gain in (1.0, 0.5):
        got = rt.collect_pcm16(5, gain=gain, normalize=True)
        peaks = rt.peaks(5)
        assert peaks.tolist() == [float(np.abs(it).max()) for it in c["v"]]
        assert np.array_equal(got, pcm_ref.pcm16_items(c["v"], gain, normalize=True))
    assert peaks.tolist() != [float(np.abs(it).max()) for it in c["raws"]]  # (the cycle's gain of 2 or its mutes moved a peak)


def test_whole_items_with_a_level(rt_medium, ragged_case):
    rt, rate, c = rt_medium, rt_medium.cfg.sample_rate, ragged_case
    peak = max(float(np.abs(x).max()) for x in c["v"])
    level = (3.0 / peak, 0.5, 50.0)
    nodes = np.concatenate([lr.gains(x, level, rate)[1] for x in c["v"]])
    print(f"level {level}: {(nodes < 1.0).sum()} of {nodes.size} nodes under 1")
    assert (nodes < 1.0).any() and (nodes == 1.0).any()  # the limiter works on v somewhere and rests somewhere
    try:
        for name, fmt in SINKS.items():
            want = np.concatenate([mr.whole(lr.apply(it, level, rate), fmt, rate, TABLES) for it in c["v"]])
            assert same(collect_as(rt, 5, name, level=level), want), name
    finally:
        rt.slot_level(5, None)
    assert same_bits(rt.collect(5), np.concatenate(c["v"]))


def test_whole_items_with_a_loudness(rt_medium, ragged_case):
    rt, rate, c = rt_medium, rt_medium.cfg.sample_rate, ragged_case
    ref = [ld.lufs(x, rate) for x in c["v"]]
    raw_ref = [ld.lufs(x, rate) for x in c["raws"]]
    lufs, gain = rt.loudness(5)
    print("L of v:", ref, "device:", lufs.tolist(), "L of raw:", raw_ref)
    assert np.isfinite(ref[0]) and abs(ref[0] - raw_ref[0]) > 0.02  # measuring x in place of v would show
    for k, want in enumerate(ref):
        assert (lufs[k] == want) if want == -np.inf else abs(float(lufs[k]) - want) <= 0.002, (k, lufs[k], want)
    assert np.all(gain == F32(1.0))
    try:
        rt.slot_loudness(5, -16.0)
        l2, g = rt.loudness(5)
        assert same_bits(l2, lufs) and g[0] != F32(1.0)
        u = [ld.apply(x, gk) for x, gk in zip(c["v"], g)]
        for name, fmt in SINKS.items():
            want = np.concatenate([mr.whole(it, fmt, rate, TABLES) for it in u])
            assert same(collect_as(rt, 5, name), want), name
    finally:
        rt.slot_loudness(5, None)
    assert same_bits(rt.collect(5), np.concatenate(c["v"]))


def test_synthesize_twins_take_the_volume(rt_medium):
    rt, rate, hop = rt_medium, rt_medium.cfg.sample_rate, rt_medium.cfg.hop
    ids, dur, noise = item(rt.cfg, 14, 1)
    raw = rt.synthesize(ids, dur, noise, 0.667, level=None, loudness=None).copy()
    gf = vr.frame_gains(cycle(14), dur)
    v = vr.apply(raw, gf, hop)
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, volume=cycle(14)), v)
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667), raw)  # one-shot: the next call has none
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000, volume=cycle(14)), mr.whole(v, SINKS["s16@8000"], rate, TABLES))
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, volume=cycle(14)), mr.whole(v, SINKS["s16"], rate, TABLES))
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000, volume=cycle(14)), mr.whole(v, SINKS["mulaw@8000"], rate, TABLES))
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667), mr.whole(raw, SINKS["s16"], rate, TABLES))


# ---- 3. bounded prepare: device noise, predicted durations

def bounded_ids():
    return [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS]


def weaker_form(gfs, hop):
    ramp, unity, total = shares(gfs, hop)
    print(f"predicted durations: {ramp} of {total} samples in ramps, {unity} at exact unity")
    assert ramp >= 1 and unity >= 1, (ramp, unity)


@pytest.mark.parametrize("fit", [False, True], ids=["plain", "fit"])
def test_bounded_prepare(rt_medium, fit):
    rt, hop = rt_medium, rt_medium.cfg.hop
    id_lists = bounded_ids()
    pairs = [(ids, None) for ids in id_lists]
    totals = [int(d.sum()) for d, _ in rt.predict_durations(pairs, **DEV)]
    # fit: a bound between the two items' totals compresses the longer one on the device
    bound = sum(totals) // 2 if fit else max(totals) + 5
    kw = dict(prosody=[dict(fit=1), dict(fit=1)]) if fit else {}
    if fit:
        assert min(totals) < bound < max(totals), totals
    vol = [cycle(len(ids)) for ids in id_lists]
    rt.prepare_batch_bounded(5, pairs, bound, **DEV, **kw)
    rt.launch(5)
    raw = rt.collect(5).copy()
    per, _ = rt.prepared_samples(5)
    steps = rt.steps(5)
    rt.prepare_batch_bounded(5, pairs, bound, volume=vol, **DEV, **kw)
    rt.launch(5)
    with pytest.raises(ph.UnsupportedOp):  # the frame counts are still on the device
        rt.tap(5, "vol.gain")
    got = rt.collect(5).copy()
    assert rt.prepared_samples(5)[0] == per and rt.steps(5) == steps
    if fit:
        assert rt.prosody_report(5)[1] == ([1, 0] if totals[0] > totals[1] else [0, 1])
    durs = np.split(rt.durations(5), [len(id_lists[0])])
    gfs = [vr.frame_gains(g, d) for g, d in zip(vol, durs)]
    assert [gf.size * hop for gf in gfs] == per
    weaker_form(gfs, hop)
    raws = np.split(raw, np.cumsum(per)[:-1])
    differs_where_shaped(raws, gfs, hop)
    v = [vr.apply(x, gf, hop) for x, gf in zip(raws, gfs)]
    assert same_bits(got, np.concatenate(v))
    assert same_bits(rt.tap(5, "vol.gain").reshape(-1), np.concatenate(gfs))
    # the typed routes of a bounded slot read their lengths on the device: as the collecting call of a fresh launch
    for name in ("s16@8000", "mulaw@8000"):
        rt.prepare_batch_bounded(5, pairs, bound, volume=vol, **DEV, **kw)
        rt.launch(5)
        want = np.concatenate([mr.whole(it, SINKS[name], rt.cfg.sample_rate, TABLES) for it in v])
        assert same(collect_as(rt, 5, name), want), name


# ---- 7. invariance and lifecycle

def test_a_request_without_a_volume_finds_what_it_found_before(rt_medium):
    rt = rt_medium
    req = item(rt.cfg, 14, 3)
    rt.prepare(6, *req, 0.667)
    rt.launch(6)
    before, steps, info = rt.collect(6).copy(), rt.steps(6), rt.plan_info(6)
    rt.prepare(6, *req, 0.667, volume=cycle(14))  # a volume request on the same bucket
    rt.launch(6)
    assert not same_bits(rt.collect(6), before) and rt.steps(6) == steps
    rt.prepare(6, *req, 0.667)
    rt.launch(6)
    assert same_bits(rt.collect(6), before) and rt.steps(6) == steps
    assert rt.plan_info(6)["bucket_f"] == info["bucket_f"]
    with pytest.raises(ph.InvalidArgument, match="no volume"):
        rt.tap(6, "vol.gain")


def test_the_assignment_is_one_shot_and_a_refused_staging_clears_it(rt_medium):
    rt, hop = rt_medium, rt_medium.cfg.hop
    ids, dur, noise = item(rt.cfg, 14, 3)
    rt.prepare(6, ids, dur, noise, 0.667)
    rt.launch(6)
    raw = rt.collect(6).copy()
    v = vr.apply(raw, vr.frame_gains(cycle(14), dur), hop)
    rt.slot_volume(6, [cycle(14)])
    rt.prepare(6, ids, dur, noise, 0.667)
    rt.launch(6)
    assert same_bits(rt.collect(6), v)
    rt.prepare(6, ids, dur, noise, 0.667)  # the assignment went with the call before
    rt.launch(6)
    assert same_bits(rt.collect(6), raw)
    # a t mismatch: PIPER_HIP_ERR_SHAPE, nothing staged, and the assignment is gone
    rt.slot_volume(6, [cycle(13)])
    with pytest.raises(ph.ShapeMismatch, match="13 entries"):
        rt.prepare(6, ids, dur, noise, 0.667)
    rt.prepare(6, ids, dur, noise, 0.667)
    rt.launch(6)
    assert same_bits(rt.collect(6), raw)
    # a staging call refused for a reason of its own clears it too
    rt.slot_volume(6, [cycle(14)])
    with pytest.raises(ph.ExecutionError):
        rt.prepare(6, ids, [-1] * 14, None, 0.667)
    rt.prepare(6, ids, dur, noise, 0.667)
    rt.launch(6)
    assert same_bits(rt.collect(6), raw)
    # n = 0 clears
    rt.slot_volume(6, [cycle(14)])
    rt.slot_volume(6, [])
    rt.prepare(6, ids, dur, noise, 0.667)
    rt.launch(6)
    assert same_bits(rt.collect(6), raw)
    # a volume with supplied durations and a prosody's noise multiplier combine
    rt.prepare(6, ids, dur, noise, 0.667, prosody=dict(noise=np.full(14, 0.5, F32)))
    rt.launch(6)
    raw_p = rt.collect(6).copy()
    rt.prepare(6, ids, dur, noise, 0.667, prosody=dict(noise=np.full(14, 0.5, F32)), volume=cycle(14))
    rt.launch(6)
    assert same_bits(rt.collect(6), vr.apply(raw_p, vr.frame_gains(cycle(14), dur), hop))


@pytest.mark.parametrize("bad", [float("nan"), -0.25, 16.5])
def test_gains_outside_the_contract_name_the_entry_and_the_index(rt_medium, bad):
    rt = rt_medium
    g = cycle(14)
    g[9] = bad
    with pytest.raises(ph.InvalidArgument, match=r"volume 1: gain\[9\]"):
        rt.slot_volume(6, [cycle(14), g])
    with pytest.raises(ph.InvalidArgument, match="entries"):
        rt.slot_volume(6, [cycle(2)] * 257)
    with pytest.raises(ph.InvalidArgument):
        rt.slot_volume(-1, [cycle(2)])


# ---- 4 … 6. streams: the twin is the same stream run once without a volume

def split_like(x, chunks):
    return np.split(x, np.cumsum([c.size for c in chunks])[:-1])


def check_stream_row(got, raw, gf, fmt, chunk, hop, rate, what, level=None):
    """got: the typed chunks of one row; raw: the fp32 chunks of the same row of the run without a volume; gf: its gains per frame (None: the
    row has no volume). Every step equals the reference's step and the concatenation the whole-item conversion, counts included."""
    x = np.concatenate(raw)
    v = x if gf is None else vr.apply(x, gf, hop)
    shaped_chunks = split_like(v, raw)
    if level is not None:
        want = expected_row(shaped_chunks, level, fmt, chunk, hop, rate)
        whole = mr.whole(lr.apply(v, level, rate), fmt, rate, TABLES)
    else:
        want = mr.row_steps(shaped_chunks, fmt, rate, hop, chunk, tables=TABLES)
        whole = mr.whole(v, fmt, rate, TABLES)
    assert [c.size for c in got] == [c.size for c in want], what  # every n_samples is that of the run without a volume
    for k, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (what, k)
    assert same(np.concatenate(got), whole), what


@pytest.mark.parametrize("sink", ["f32", "s16@8000"])
def test_single_stream(rt_medium, sink):
    rt, hop, rate, fmt = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate, SINKS[sink]
    ids, dur, noise = item(rt.cfg, 7, 2)  # 21 frames in chunks of 8
    g = cycle(7)
    gf = vr.frame_gains(g, dur)
    raw = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3))
    assert [c.size for c in raw] == [8 * hop, 8 * hop, 5 * hop]
    weaker_form([gf], hop)
    differs_where_shaped([np.concatenate(raw)], [gf], hop)
    got = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3, volume=g, **stream_kw(fmt)))
    plain = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=3, **stream_kw(fmt)))  # one-shot: this one has none
    check_stream_row(got, raw, gf, fmt, 8, hop, rate, sink)
    check_stream_row(plain, raw, None, fmt, 8, hop, rate, sink + " plain")
    assert [c.size for c in got] == [c.size for c in plain]


GROUP_FORMATS = [Format(48000, "s16", 1.0), Format(8000, "mulaw", 1.0), Format(0, "f32", 1.0)]


def group_request(cfg):
    return [item(cfg, 10, 5), shaped(cfg, [1, 1], 6), item(cfg, 14, 7)]  # F = 30, 2 (one step), 42


def test_group_with_a_level_on_a_mixed_slot(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    utts = group_request(rt.cfg)
    vols = [cycle(10), None, cycle(14)]  # the one-step item has an all-1.0 record
    gfs = [vr.frame_gains(g, u[1]) for g, u in zip(vols, utts)]
    raw = [[] for _ in utts]
    for chunks in rt.synthesize_stream_batch(utts, 0.667, chunkFrames=8, slot=8):
        for i, c in enumerate(chunks):
            if c.size:
                raw[i].append(c)
    assert [len(r) for r in raw] == [4, 1, 6]
    v = [vr.apply(np.concatenate(r), gf, hop) for r, gf in zip(raw, gfs)]
    peak = max(float(np.abs(x).max()) for x in v)
    level = (3.0 / peak, 0.5, 50.0)
    assert any(lr.gains(x, level, rate)[1].min() < 1.0 for x in v)  # the limiter works on v somewhere
    fmts = [ph.stream_format(rate=f.rate, encoding=f.enc, gain=f.gain) for f in GROUP_FORMATS]
    got = [[] for _ in utts]
    for chunks in rt.synthesize_stream_batch(utts, 0.667, chunkFrames=8, slot=8, formats=fmts, level=level, volume=vols):
        for i, c in enumerate(chunks):
            if c.size:
                got[i].append(c)
    for i in range(3):
        check_stream_row(got[i], raw[i], gfs[i], GROUP_FORMATS[i], 8, hop, rate, ("group", i), level=level)
    assert same_bits(v[1], np.concatenate(raw[1]))  # a neutral record leaves the bits alone


def run_volume_pool(rt, fmt, with_volume):
    """Capacity 4: S and A join together, E joins alone, P by a bounded join with fit; when S has finished B takes its row. With a volume: S,
    A and P carry one, E and B none. Returns ({session: [chunk per step]}, P's durations)."""
    cfg = rt.cfg
    u = {"S": item(cfg, 5, 9), "A": item(cfg, 10, 5), "E": item(cfg, 14, 8), "B": shaped(cfg, [3] * 9, 4, quiet_at=0),
         "P": (kd.FIXTURE_IDS * 2, None, None, DEV)}
    (dP, _), = rt.predict_durations([(u["P"][0], None)], **DEV)
    cap = int(dP.sum()) - 7
    vol = (lambda names: [cycle(len(u[s][0])) for s in names]) if with_volume else (lambda names: None)
    pool = rt.stream_pool(10, 4, chunkFrames=8, work_slot=11, rate=fmt.rate or None)
    try:
        assert [i for i, _ in pool.join([u["S"], u["A"]], 0.667, volume=vol("SA"))] == [0, 1]
        assert [i for i, _ in pool.join([u["E"]], 0.667)] == [2]
        assert pool.join_bounded([u["P"]], cap, 0.667, prosody=[dict(fit=1)], volume=vol("P")) == [3]
        samples_p = pool.item_samples(3)
        dur_p = rt.durations(11).copy()
        assert rt.prosody_report(11)[1] == [1] and samples_p == mr.total_samples(max(int(dur_p.sum()), 1) * cfg.hop, fmt, cfg.sample_rate)
        who = {0: "S", 1: "A", 2: "E", 3: "P"}
        per = {s: [] for s in "SAEBP"}
        for k in range(64):
            if k == 2:  # S (15 frames) has finished
                assert pool.free_rows >= 1
                (row, _), = pool.join([u["B"]], 0.667)  # a new occupant without a volume
                assert row == 0
                who[0] = "B"
            out = pool.step(pcm=fmt.enc != "f32", gain=fmt.gain)
            if not out:
                break
            for r, c in out.items():
                per[who[r]].append(c)
    finally:
        pool.close()
    return per, {**{s: np.asarray(u[s][1]) for s in "SAEB"}, "P": dur_p}


@pytest.mark.parametrize("sink", ["f32", "s16@8000"])
def test_pool_with_a_bounded_join_and_a_new_occupant(rt_medium, sink):
    rt, hop, rate, fmt = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate, SINKS[sink]
    raw, durs = run_volume_pool(rt, SINKS["f32"], False)
    assert all(len(raw[s]) for s in "SAEBP")
    got, durs_v = run_volume_pool(rt, fmt, True)
    assert np.array_equal(durs["P"], durs_v["P"])
    gfs = {s: vr.frame_gains(cycle(len(durs[s])), durs[s]) if s in "SAP" else None for s in "SAEBP"}
    weaker_form([gfs["P"]], hop)
    differs_where_shaped([np.concatenate(raw[s]) for s in "SAP"], [gfs[s] for s in "SAP"], hop)
    for s in "SAEBP":
        check_stream_row(got[s], raw[s], gfs[s], fmt, 8, hop, rate, (sink, s))
    if sink == "f32":  # the rows without a volume, the new occupant of S's row among them, keep their raw bits
        for s in "EB":
            assert same_bits(np.concatenate(got[s]), np.concatenate(raw[s])), s


# ---- 8. command line

def test_cli_id_volume_equals_the_python_route(backend, voices, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    ids = kd.FIXTURE_IDS * 2
    raw, plain = tmp_path / "a.s16le", tmp_path / "b.s16le"
    base = [str(exe), "--phoneme-ids", ",".join(str(i) for i in ids), "--output-raw"]
    out = subprocess.run(base + [str(raw), "--id-volume", "2:9=0.25,9:12=0,20:28=2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    out = subprocess.run(base + [str(plain)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    bad = subprocess.run(base + [str(raw) + ".x", "--id-volume", "2:40=1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--id-volume" in bad.stderr
    gains = np.ones(len(ids), F32)
    gains[2:9], gains[9:12], gains[20:28] = 0.25, 0.0, 2.0
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        kw = dict(noise_mode="device", seed=1234)
        want = rt.synthesize_pcm16(ids, [3] * len(ids), None, 0.667, volume=gains, **kw).copy()
        want_plain = rt.synthesize_pcm16(ids, [3] * len(ids), None, 0.667, **kw).copy()
    finally:
        rt.close()
    assert np.array_equal(np.frombuffer(raw.read_bytes(), "<i2"), want)
    assert np.array_equal(np.frombuffer(plain.read_bytes(), "<i2"), want_plain) and not np.array_equal(want, want_plain)
