"""GPU: the join (include/piper_hip.h "Join") — per-op on synthetic vectors and on every whole-item voice route. The per-op cases are the
smallest shapes at which the three kernels can go wrong and are compared with tests/join_ref.py bit for bit, twice. On the voice routes the
raw reference is the GPU's own audio: the same launch collected without a join. tests/join_ref.py, followed by the existing pcm_ref /
resample_ref / g711_ref (through mixed_ref.whole), is applied to it and compared bit for bit with what the device delivers, counts and
report included.

The voice is the scaled-output-conv medium voice of tests/test_gpu_level.py; the injected noise carries an envelope that is 16 on the
body and 0 on chosen head and tail frames (one item of the ragged batch: 0 throughout). The threshold is taken from the raw audio: the
geometric mean of the quiet peak and the loud peak, where the quiet peak is taken over the all-quiet item and over the quiet edges less
the QUIET_HALO frames next to the body (the generator's and the flow's reach carries the body into those). Before anything is compared
the reference alone must show that a head loses at least a hop, a tail loses at least a hop, an edge is uncut and an item is empty.
Bounded slots draw their noise on the device, so there is no per-frame envelope: the noise scale varies per item (loud, less loud, 0), and
the quiet heads and tails come from the per-id noise multiplier of the prosody (0 on the first and last ids, held for min_frames)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import join_ref as jr
import katdata as kd
import mixed_ref as mr
import pcm_ref
import piper_hip as ph
from test_gpu_level import DEV, SINKS, collect_as, rt_medium, same  # noqa: F401
from test_gpu_stream_mixed import TABLES

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024        # samples of one block's pass of the write and edge kernels
QUIET_HALO = 12    # frames of a quiet edge next to the body that do not count as quiet
SLOT = 5


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- per-op

def loud(n, seed, lo=None, hi=None, quiet=1e-3):
    """n samples of noise at `quiet` with a body of |x| in [0.3, 0.9] on [lo, hi)"""
    rng = np.random.default_rng(seed)
    x = (quiet * rng.standard_normal(n)).astype(F32)
    lo, hi = (0, n) if lo is None else (lo, hi)
    x[lo:hi] = ((0.3 + 0.6 * rng.random(hi - lo)) * rng.choice([-1.0, 1.0], hi - lo)).astype(F32)
    return x


def per_op_cases():
    J = dict(trim=1, trim_threshold=0.25, trim_pad_ms=0.5, fade_ms=1.0, lead_ms=0.375, gap_ms=0.625, tail_ms=0.875)  # at 8 kHz: P 4, Fd 8, 3 / 5 / 7
    c = {}
    lens = [0, 1, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1]
    items = [loud(n, n, n // 4, n - n // 4) for n in lens]
    c["lengths"] = (items, J, [0.0, 0.125, 0.25, 0.375, 0.625, 0.0, 0.125, 0.25])  # gaps of 0, 1, 2, 3, 5 samples: every phase of dst
    c["lengths_no_trim"] = (items, dict(lead_ms=0.125, gap_ms=0.375, tail_ms=0.125), None)
    only = []
    for at in (0, 199, 100):  # the only loud sample first, last, in the middle
        x = np.zeros(200, F32)
        x[at] = -0.5
        only.append(x)
    c["one_loud_sample"] = (only, J, [0.125, 0.375])
    x = loud(300, 1, 100, 200)
    x[[90, 210]] = [0.25, -0.25]  # exactly at the threshold: not loud
    c["at_threshold"] = ([x, x[::-1].copy()], J, None)
    q = (1e-3 * np.random.default_rng(2).standard_normal(150)).astype(F32)
    c["quiet_first_last_between"] = ([q, loud(300, 3, 50, 250), q[:77], loud(130, 4, 0, 130), q[:5]], J, [0.25, 0.125, 0.375, 0.625])
    c["all_quiet"] = ([q, q[:3]], J, None)
    x = loud(400, 5, 150, 250)
    x[[10, 200, 390]] = [np.nan, np.nan, -np.nan]
    x.view(np.uint32)[200] = 0x7FC54321
    y = loud(400, 6, 150, 250)
    y[[20, 201, 380]] = [np.inf, -np.inf, np.inf]  # ±Inf is loud: the range opens to 20 … 380
    c["nan_inf"] = ([x, y], dict(J, fade_ms=0.0), None)
    c["fade_longer_than_kept"] = ([loud(100, 7, 48, 51), loud(64, 8, 30, 31)], dict(J, fade_ms=5.0, trim_pad_ms=0.0), None)
    c["pad_longer_than_item"] = ([loud(60, 9, 20, 40), loud(9, 10, 4, 5)], dict(J, trim_pad_ms=20.0), None)
    c["one_item"] = ([loud(777, 11, 200, 500)], J, None)
    c["two_items"] = ([loud(50, 12, 10, 20), loud(51, 13, 0, 40)], J, [0.125])
    tiny = [loud(n % 7, 100 + n, 0, n % 7) if n % 5 else np.zeros(n % 3, F32) for n in range(256)]
    c["256_tiny_items"] = (tiny, dict(J, lead_ms=0.125, tail_ms=0.125, gap_ms=0.125), [0.0, 0.125, 0.25] * 40)
    c["past_the_grid"] = ([loud(1024 * TILE + 5, 14, 3000, 1024 * TILE - 2000), loud(10, 15)], dict(J, fade_ms=2.0), None)
    return c


PER_OP = per_op_cases()


@pytest.mark.parametrize("name,shift", [(n, s) for n in sorted(PER_OP) for s in (0, 1) if not (s and n == "past_the_grid")])
def test_per_op(backend, name, shift):
    """shift = 1: x itself is not 16-byte aligned. The items lie in x behind 0 … 3 floats of filler, so their offsets meet all four phases.
    (The long item is checked once, aligned.)"""
    items, j, gaps = PER_OP[name]
    rate = 8000
    parts, off = [np.full(shift, 9.0, F32)], []
    at = shift
    for i, it in enumerate(items):
        fill = i % 4
        parts.append(np.full(fill, 9.0, F32))
        off.append(at + fill)
        parts.append(it)
        at += fill + it.size
    x = np.concatenate(parts + [np.full(4, 9.0, F32)])
    buf = backend.uploadFloat32(x)
    src = ph.DeviceBuffer(backend, buf.ptr + 4 * shift, x.size - shift, owned=False)
    want, wstart, wlen, wtotal = jr.join(items, j, rate, gaps)
    assert wtotal <= jr.capacity([it.size for it in items], j, rate, gaps)
    runs = []
    for _ in range(2):
        out, start, length, total = backend.join_f32(src, [o - shift for o in off], [it.size for it in items], rate, j, gaps)
        got = backend.downloadFloat32(out, total) if total else np.empty(0, F32)
        assert total == wtotal and np.array_equal(start, wstart) and np.array_equal(length, wlen), (name, start, wstart, length, wlen)
        assert np.array_equal(bits(got), bits(want)), (name, np.flatnonzero(bits(got) != bits(want))[:8])
        runs.append(got)
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    if name == "lengths" and not shift:
        assert {int(s) % 4 for s in wstart} == {0, 1, 2, 3}, "dst_off meets all four phases"
        assert {o % 4 for o in off} == {0, 1, 2, 3}, "and so do the sources"
        tw = ph.join_from_f32(items, j, rate, gaps)
        assert np.array_equal(bits(tw[0]), bits(want)) and tw[3] == wtotal


def test_per_op_refusals(backend):
    buf = backend.uploadFloat32(np.zeros(8, F32))
    with pytest.raises(ph.InvalidArgument):
        backend.join_f32(buf, [0], [8], 8000, dict(gap_ms=-1.0))
    with pytest.raises(ph.InvalidArgument):
        backend.join_f32(buf, [0] * 257, [0] * 257, 8000, {})
    with pytest.raises(ph.ShapeMismatch):
        backend.join_f32(buf, [0, 0], [8, -1], 8000, {})


# ---- voice routes

def enveloped(cfg, n_ids, seed, head=0, tail=0):
    """(ids, durations, noise) with 3 frames per id: the noise is 16 × the usual on the body, 0 on the first `head` and the last `tail`
    frames (head ≥ the item's frames: 0 throughout)."""
    F = 3 * n_ids
    env = np.full(F, 16.0, F32)
    env[:head] = 0.0
    if tail:
        env[F - tail:] = 0.0
    return (kd.FIXTURE_IDS * 4)[:n_ids], [3] * n_ids, kd.sym(700 + seed, (cfg.inter, F), 1.7320508) * env


def threshold_of(items, quiet, hop):
    """items: raw audio per item; quiet: (head frames, tail frames) per item, head ≥ the item's frames meaning all of it"""
    q = 0.0
    for x, (h, t) in zip(items, quiet):
        F = x.size // hop
        if h >= F:
            q = max(q, float(np.abs(x).max()))
            continue
        if h > QUIET_HALO:
            q = max(q, float(np.abs(x[:(h - QUIET_HALO) * hop]).max()))
        if t > QUIET_HALO:
            q = max(q, float(np.abs(x[x.size - (t - QUIET_HALO) * hop:]).max()))
    peak = max(float(np.abs(x).max()) for x in items)
    print(f"quiet peak {q:.3e}, loud peak {peak:.3e}")
    assert 0.0 < q < peak
    return float(np.sqrt(q * peak))


def show_and_require(items, j, rate, hop, need):
    """the kept ranges of the reference alone; `need`: which of the four conditions this slot can show"""
    p = jr.params(j)
    P = jr.S(p["trim_pad_ms"], rate)
    rng = [jr.kept_range(x, p, P) for x in items]
    seen = dict(head=any(t > s and s >= hop for s, t in rng), tail=any(t > s and x.size - t >= hop for (s, t), x in zip(rng, items)),
                uncut=any(t > s and (s == 0 or t == x.size) for (s, t), x in zip(rng, items)), empty=any(t == s for s, t in rng))
    print("kept ranges", [(s, t, x.size) for (s, t), x in zip(rng, items)], seen)
    for k in need:
        assert seen[k], (k, rng)


def wanted(items, j, rate, gaps=None):
    prog, start, length, total = jr.join(items, j, rate, gaps)
    w = {name: mr.whole(prog, f, rate, TABLES) for name, f in SINKS.items()}
    w["normalized"] = pcm_ref.pcm16_items([prog], 1.0, normalize=True)
    return prog, start, length, total, w


def deliver(rt, slot, name, **kw):
    if name == "normalized":
        return rt.collect_pcm16(slot, normalize=True, **kw)
    return collect_as(rt, slot, name, **kw)


def check_all_sinks(rt, slot, items, j, gaps=None):
    rate = rt.cfg.sample_rate
    prog, start, length, total, want = wanted(items, j, rate, gaps)
    rt.slot_join(slot, j, gaps)
    for name in list(SINKS) + ["normalized"]:
        got = deliver(rt, slot, name)
        assert same(got, want[name]), (name, got.size, want[name].size)
        gs, gl, gt = rt.join_report(slot)
        assert gt == total and np.array_equal(gs, start) and np.array_equal(gl, length), name
        if name == "normalized":
            assert np.array_equal(rt.peaks(slot), np.array([np.abs(prog).max() if prog.size else 0.0], F32)), "ONE peak, over the programme"
    for name, f in SINKS.items():  # the delivered count is resample_count(rate, out_rate, total)
        assert want[name].size == (ph.resample_count(rate, f.rate, total) if f.rate else total)
    rt.slot_join(slot, None)


def clear(rt, *slots):
    for s in slots:
        rt.slot_join(s, None)
        rt.slot_level(s, None)
        rt.slot_eq(s, None)


def raw_items(rt, slot):
    raw = rt.collect(slot, join=None).copy()
    per, total = rt.prepared_samples(slot)
    assert raw.size == total
    return np.split(raw, np.cumsum(per)[:-1])


def the_join(thr):
    return dict(lead_ms=5.0, gap_ms=20.0, tail_ms=7.3, trim=1, trim_threshold=thr, trim_pad_ms=10.0, fade_ms=3.0)


RAGGED = [(40, 24, 0), (20, 60, 0), (30, 0, 24), (14, 0, 0)]  # (ids, quiet head frames, quiet tail frames); item 1 is quiet throughout


def prepare_ragged(rt, slot):
    rt.prepare_batch(slot, [enveloped(rt.cfg, n, k, h, t) for k, (n, h, t) in enumerate(RAGGED)], 0.667)
    return [(h, t) for _, h, t in RAGGED]


def prepare_plain(rt, slot):
    rt.prepare(slot, *enveloped(rt.cfg, 40, 9, 24, 24), 0.667)
    return [(24, 24)]


def test_plain_slot_every_sink(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    quiet = prepare_plain(rt, SLOT)
    rt.launch(SLOT)
    items = raw_items(rt, SLOT)
    j = the_join(threshold_of(items, quiet, hop))
    show_and_require(items, j, rate, hop, ["head", "tail"])
    check_all_sinks(rt, SLOT, items, j)
    assert same(rt.collect(SLOT), items[0]), "the plan's audio is unchanged"


def test_ragged_slot_every_sink(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    quiet = prepare_ragged(rt, SLOT)
    rt.launch(SLOT)
    items = raw_items(rt, SLOT)
    assert len({x.size for x in items}) == 4
    j = the_join(threshold_of(items, quiet, hop))
    show_and_require(items, j, rate, hop, ["head", "tail", "uncut", "empty"])
    check_all_sinks(rt, SLOT, items, j)
    check_all_sinks(rt, SLOT, items, j, gaps=[0.0, 3.1, 11.0])
    rt.slot_join(SLOT, j)
    assert rt.join_capacity(SLOT) == jr.capacity([x.size for x in items], j, rate)
    assert rt.join_capacity(SLOT, 8000) == ph.resample_count(rate, 8000, rt.join_capacity(SLOT))
    rt.slot_join(SLOT, None)


def prepare_bounded(rt, slot):
    """four items with a noise scale each (loud, less loud, 0, loud); the prosody's per-id noise multiplier is 0 on the first ids of item 0
    and the last ids of item 1, held for 8 frames each, which gives a quiet head and a quiet tail of 24 frames. Returns (quiet, their ids)."""
    id_lists = [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS + kd.FIXTURE_IDS[:6], kd.FIXTURE_IDS, kd.FIXTURE_IDS[:10]]
    scales = (0.667 * 16, 0.667 * 12, 0.0, 0.667 * 16)
    pro = []
    for i, ids in enumerate(id_lists):
        noise, mn = np.ones(len(ids), F32), np.zeros(len(ids), np.int32)
        if i == 0:
            noise[:3], mn[:3] = 0.0, 8
        if i == 1:
            noise[-3:], mn[-3:] = 0.0, 8
        pro.append(dict(noise=noise, min_frames=mn) if i < 2 else None)
    bound = max(int(d.sum()) for d, _ in rt.predict_durations([(ids, None) for ids in id_lists], **DEV)) + 24 + 5
    arr, keep = (ph.Utterance * 4)(), []
    for i, (ids, scale) in enumerate(zip(id_lists, scales)):
        arr[i], k = rt._utt(ids, None, None, scale, **DEV)
        keep.append(k)
    rt._stage_prosody(slot, pro, [len(ids) for ids in id_lists])
    assert rt.lib.piper_hip_voice_prepare_batch_bounded(rt.voice, arr, 4, slot, bound) >= 0
    tot = C.c_int64()
    ph._check(rt.lib.piper_hip_voice_prepared_samples(rt.voice, slot, None, 0, C.byref(tot)))
    rt._keep[slot] = (keep, int(tot.value), True)
    return id_lists


def bounded_quiet(rt, slot, id_lists):
    d = np.split(rt.durations(slot), np.cumsum([len(i) for i in id_lists])[:-1])
    return [(int(d[0][:3].sum()), 0), (0, int(d[1][-3:].sum())), (10 ** 6, 0), (0, 0)]


def test_bounded_slot_every_sink(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    id_lists = prepare_bounded(rt, SLOT)
    rt.launch(SLOT)
    items = raw_items(rt, SLOT)  # (the collecting call of this launch)
    quiet = bounded_quiet(rt, SLOT, id_lists)
    assert quiet[0][0] >= 24 and quiet[1][1] >= 24
    j = the_join(threshold_of(items, quiet, hop))
    show_and_require(items, j, rate, hop, ["head", "tail", "uncut", "empty"])
    check_all_sinks(rt, SLOT, items, j)
    # the same request again, and every sink as the launch's COLLECTING call: the lengths are still on the device when the join runs
    prog, start, length, total, want = wanted(items, j, rate)
    for name in list(SINKS) + ["normalized"]:
        prepare_bounded(rt, SLOT)
        rt.launch(SLOT)
        rt.slot_join(SLOT, j)
        cap = rt.join_capacity(SLOT)
        assert cap >= total and cap == jr.capacity([rt._keep[SLOT][1] // 4] * 4, j, rate), "a bounded slot: its frame capacity per item"
        got = deliver(rt, SLOT, name)
        assert same(got, want[name]), name
        gs, gl, gt = rt.join_report(SLOT)
        assert gt == total and np.array_equal(gs, start) and np.array_equal(gl, length), name
        assert [x.size for x in items] == rt.prepared_samples(SLOT)[0], "and the lengths arrived with it"
        rt.slot_join(SLOT, None)
    again = raw_items(rt, SLOT)
    assert all(same(a, b) for a, b in zip(again, items))


def test_synthesize_twins(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, 0)
    ids, dur, noise = enveloped(rt.cfg, 40, 9, 24, 24)
    raw = rt.synthesize(ids, dur, noise, 0.667, join=None).copy()
    j = the_join(threshold_of([raw], [(24, 24)], hop))
    show_and_require([raw], j, rate, hop, ["head", "tail"])
    prog, start, length, total, want = wanted([raw], j, rate)
    assert same(rt.synthesize(ids, dur, noise, 0.667, join=j), want["f32"])
    assert rt.join_report(0)[2] == total
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667), want["s16"])  # the join stays
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000), want["s16@8000"])
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=48000, gain=0.5), want["s16@48000"])
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000), want["mulaw@8000"])
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, normalize=True), want["normalized"])
    assert same(rt.synthesize(ids, dur, noise, 0.667, join=None), raw)
    clear(rt, 0)


def test_join_reads_the_limited_eq_items(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    quiet = prepare_ragged(rt, SLOT)
    rt.launch(SLOT)
    raw = raw_items(rt, SLOT)
    level = (3.0 / max(float(np.abs(x).max()) for x in raw), 0.5, 50.0)
    eq = [("highpass", 300.0, 0.707), ("peaking", 2500.0, 1.0, 6.0)]
    rt.slot_level(SLOT, level)
    rt.slot_eq(SLOT, eq)
    items = raw_items(rt, SLOT)  # un-joined: the limited, EQ'd items
    assert not same(items[0], raw[0])
    j = the_join(threshold_of(items, quiet, hop))
    show_and_require(items, j, rate, hop, ["head", "tail"])
    prog, start, length, total, want = wanted(items, j, rate)
    rt.slot_join(SLOT, j)
    for name in SINKS:
        assert same(collect_as(rt, SLOT, name), want[name]), name
    assert rt.join_report(SLOT)[2] == total
    assert all(same(a, b) for a, b in zip(raw_items(rt, SLOT), items))
    clear(rt, SLOT)
    assert all(same(a, b) for a, b in zip(raw_items(rt, SLOT), raw))


def test_neutral_identities(rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    prepare_plain(rt, SLOT)
    rt.launch(SLOT)
    plain = {name: deliver(rt, SLOT, name).copy() for name in list(SINKS) + ["normalized"]}
    for name, w in plain.items():  # one item: every sink
        assert same(deliver(rt, SLOT, name, join=ph.Join()), w), name
    rt.slot_join(SLOT, None)
    prepare_ragged(rt, SLOT)
    rt.launch(SLOT)
    own_rate = ["f32", "s16"]
    plain = {name: deliver(rt, SLOT, name).copy() for name in own_rate}
    plain["alaw"] = rt.collect_g711(SLOT, "alaw").copy()
    for name in own_rate:  # a batch: the sinks at the voice's own rate
        assert same(deliver(rt, SLOT, name, join={}), plain[name]), name
    assert same(rt.collect_g711(SLOT, "alaw"), plain["alaw"])
    per, total = rt.prepared_samples(SLOT)
    s, l, t = rt.join_report(SLOT)
    assert t == total and list(l) == per and list(s) == list(np.cumsum([0] + per[:-1]))
    clear(rt, SLOT)


@pytest.mark.parametrize("order", ["joins_first", "plain_first"])
def test_two_joins_and_a_plain_collect_after_one_launch(rt_medium, order):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    quiet = prepare_ragged(rt, SLOT)
    rt.launch(SLOT)
    items = raw_items(rt, SLOT)
    a = the_join(threshold_of(items, quiet, hop))
    b = dict(a, lead_ms=0.0, gap_ms=33.3, trim_pad_ms=1.0, fade_ms=0.5, tail_ms=0.0)
    wa, wb = wanted(items, a, rate), wanted(items, b, rate)
    rt.launch(SLOT)
    steps = ["a", "b", "plain", "b", "a"] if order == "joins_first" else ["plain", "b", "a", "plain"]
    for k, st in enumerate(steps):
        name = ("f32", "s16@8000", "s16")[k % 3]
        if st == "plain":
            got = collect_as(rt, SLOT, name, join=None)
            assert same(got, np.concatenate([mr.whole(x, SINKS[name], rate, TABLES) for x in items])), (k, st)
            if k == 0:  # no joined collect since the launch
                with pytest.raises(ph.InvalidArgument):
                    rt.join_report(SLOT)
        else:
            w = wa if st == "a" else wb
            assert same(collect_as(rt, SLOT, name, join=a if st == "a" else b), w[4][name]), (k, st)
            assert rt.join_report(SLOT)[2] == w[3]
    clear(rt, SLOT)


def test_short_buffer_is_refused_and_the_slot_stays_collectable(rt_medium):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    clear(rt, SLOT)
    quiet = prepare_ragged(rt, SLOT)
    rt.launch(SLOT)
    items = raw_items(rt, SLOT)
    j = the_join(threshold_of(items, quiet, hop))
    prog, start, length, total, want = wanted(items, j, rate)
    rt.launch(SLOT)
    with pytest.raises(ph.InvalidArgument):
        rt.join_report(SLOT)  # not collected with a join since its last launch
    rt.slot_join(SLOT, j)
    cap = rt.join_capacity(SLOT)
    f = np.empty(cap, F32)
    assert rt.lib.piper_hip_voice_collect(rt.voice, SLOT, f.ctypes.data_as(ph.c_f32p), cap - 1) == ph.ShapeMismatch.code
    p16 = np.empty(cap, np.int16)
    prm = ph.PcmParams(1.0, 0)
    assert rt.lib.piper_hip_voice_collect_pcm16(rt.voice, SLOT, C.byref(prm), p16.ctypes.data_as(ph.c_i16p), cap - 1) == ph.ShapeMismatch.code
    cap8 = rt.join_capacity(SLOT, 8000)
    assert rt.lib.piper_hip_voice_collect_g711(rt.voice, SLOT, C.byref(prm), 1, 8000, p16.ctypes.data_as(ph.c_u8p), cap8 - 1) == ph.ShapeMismatch.code
    assert same(rt.collect(SLOT), want["f32"]) and same(rt.collect_pcm16(SLOT), want["s16"])
    with pytest.raises(ph.InvalidArgument):
        rt.slot_join(SLOT, dict(j, fade_ms=101.0))
    assert same(rt.collect_g711(SLOT, "mulaw", rate=8000), want["mulaw@8000"]), "a refused join leaves the slot's join as it was"
    clear(rt, SLOT)
    with pytest.raises(ph.InvalidArgument):
        rt.join_capacity(SLOT)


# ---- command line

def build_cli(tmp_path):
    lib = os.path.join(ROOT, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])

    def run(ids_arg, *flags):
        raw = tmp_path / ("o%d.s16le" % len(list(tmp_path.iterdir())))
        out = subprocess.run([str(exe), "--phoneme-ids", ids_arg, "--output-raw", str(raw)] + list(flags), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return np.frombuffer(raw.read_bytes(), "<i2"), out.stderr
    return run


CLI_A, CLI_B = kd.FIXTURE_IDS * 2, (kd.FIXTURE_IDS * 2)[::-1]
# Two short sentences (10 and 7 ids: 30 and 21 frames). The library chooses its generator kernels by the work of a launch — frames times
# items: the ResBlock pair kernel from 128 frames in the launch on, the pipelined conv by the launch's flops — so a batch of two computes
# the bits of two single runs only where both fall on the same side of every such choice. Measured on an MI355X, batch of two against
# two single runs, int16 samples that differ (always by one count; fp32 at most 3.6e-6; the flow's z always bit-identical):
#   ids  5 + 5: 0      10 + 7: 0      14 + 14: 88 of 21 504      20 + 14: 150 of 26 112      28 + 28: 236 of 43 008      56 + 56: 549 of 86 016
# The comparison with single runs below is therefore made where the schedules coincide; test_cli_programme_equals_the_python_route holds the
# longer sentences against the library's own batch.
CLI_SHORT_A, CLI_SHORT_B = kd.FIXTURE_IDS[:10], kd.FIXTURE_IDS[::-1][:7]


def ids_text(ids):
    return ",".join(str(i) for i in ids)


def test_cli_two_sentences_with_sentence_silence(backend, tmp_path):
    """Two sentences with --sentence-silence 0.2 --output-raw equal the two single-sentence outputs with S(200) = 4410 zeros between
    them, and each sentence's start is printed. (The sentences are short: see CLI_SHORT_A above for what longer ones give and why.)"""
    run = build_cli(tmp_path)
    one_a, _ = run(ids_text(CLI_SHORT_A))
    one_b, _ = run(ids_text(CLI_SHORT_B))
    both, err = run(ids_text(CLI_SHORT_A) + "/" + ids_text(CLI_SHORT_B), "--sentence-silence", "0.2")
    gap = jr.S(200.0, 22050)
    assert gap == 4410 and one_a.size == 30 * 256 and one_b.size == 21 * 256
    want = np.concatenate([one_a, np.zeros(gap, np.int16), one_b])
    assert both.size == want.size and not both[one_a.size:one_a.size + gap].any()
    assert "sentence 0 starts at 0.000" in err and "sentence 1 starts at %.3f" % ((one_a.size + gap) / 22050.0) in err
    d = both.astype(np.int32) - want.astype(np.int32)
    print(f"programme vs single runs: {int((d != 0).sum())} of {d.size} samples differ, max |d| {int(np.abs(d).max())}")
    assert np.array_equal(both, want)


def test_cli_programme_equals_the_python_route(backend, voices, tmp_path):
    """the CLI's programme is the joined batch of the library: the same two sentences through prepare_batch and a join in Python, and that
    launch's un-joined items with the silences between them"""
    run = build_cli(tmp_path)
    flags = ["--sentence-silence", "0.2", "--lead-ms", "10", "--tail-ms", "20"]
    both, err = run(ids_text(CLI_A) + "/" + ids_text(CLI_B), *flags)
    trimmed, terr = run(ids_text(CLI_A) + "/" + ids_text(CLI_B), *flags, "--trim-silence", "0.5:2:3", "--output-rate", "8000")
    single, _ = run(ids_text(CLI_A))
    joined_single, _ = run(ids_text(CLI_A), "--lead-ms", "10")
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        kw = dict(noise_mode="device", seed=1234)
        rt.prepare_batch(0, [(i, [3] * len(i), None, dict(kw)) for i in (CLI_A, CLI_B)], 0.667)
        rt.launch(0)
        items = np.split(rt.collect_pcm16(0).copy(), 2)
        j = dict(gap_ms=200.0, lead_ms=10.0, tail_ms=20.0)
        want = rt.collect_pcm16(0, join=j).copy()
        start = rt.join_report(0)[0]
        want8 = rt.collect_pcm16(0, rate=8000, join=dict(j, trim=1, trim_threshold=0.5, trim_pad_ms=2.0, fade_ms=3.0)).copy()
        start8 = rt.join_report(0)[0]
    finally:
        rt.close()
    z = lambda ms: np.zeros(jr.S(ms, 22050), np.int16)  # noqa: E731
    assert np.array_equal(both, want) and np.array_equal(both, np.concatenate([z(10.0), items[0], z(200.0), items[1], z(20.0)]))
    assert np.array_equal(trimmed, want8)
    for e, st in ((err, start), (terr, start8)):
        assert all("sentence %d starts at %.3f s" % (i, s / 22050.0) in e for i, s in enumerate(st)), e
    assert np.array_equal(joined_single, np.concatenate([z(10.0), single])), "one list under a join flag: a batch of one is the single plan"
