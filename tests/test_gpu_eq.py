"""GPU: the equaliser (include/piper_hip.h "Equaliser") as a per-op and on every whole-item route. Every comparison is bit for bit
against the library's host twin, piper_hip_eq_from_f32 (which tests/test_eq_abi.py holds bit for bit to the numpy restatement
tests/eq_ref.py), applied to the GPU's own un-EQ'd output of the same launch; on top of it the existing pcm_ref / level_ref /
loudness_ref / mixed_ref contracts give every other format. The loudness the device measures over the EQ'd items is held to the
existing 0.002 LU of loudness_ref on the EQ'd float64 signal.

The voice is the one of tests/test_gpu_level.py (output conv × 0.02, noise envelope 16 / 0), whose waveform follows the latent instead
of sitting in the tanh's saturation, so an EQ visibly changes the loudness and the peaks."""
import os
import re
import subprocess

import numpy as np
import pytest

import katdata as kd
import level_ref as lr
import loudness_ref as ld
import mixed_ref as mr
import pcm_ref
import piper_hip as ph
from mixed_ref import Format
from test_gpu_level import (DEV, SINKS, check_row, collect_as, group_items, item, pool_sessions, rt_medium, same,  # noqa: F401
                            single_item, single_twin, group_twin, pool_twin, stream_kw)  # (rt_medium and the twins: fixtures)
from test_gpu_resample import same_bits
from test_gpu_stream_mixed import TABLES

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wg_blocks():
    """W: the blocks per workgroup the kernels use (eq.h kEqWgBlocks), one lane per block of 64 samples"""
    with open(os.path.join(ROOT, "piper-swift_amd", "csrc", "eq.h")) as f:
        return int(re.search(r"kEqWgBlocks = (\d+);", f.read()).group(1))


W = wg_blocks()
# Block 2W is the first whose start state folds an aggregate the cross-workgroup launch built (level log2(W) + 1): the smallest item
# that reaches every level of the launch hierarchy — LDS tree, cross-workgroup levels, fold — is one sample into that block.
CROSS = 2 * W * 64 + 1

A = [(ph.EQ_HIGHPASS, 40.0, 0.707), (ph.EQ_PEAKING, 3000.0, 1.0, 6.0), (ph.EQ_HIGHSHELF, 6000.0, 0.707, -3.0), (ph.EQ_LOWPASS, 7000.0, 0.707)]
B = [(ph.EQ_LOWSHELF, 200.0, 0.8, 8.0), (ph.EQ_NOTCH, 1000.0, 2.0), (ph.EQ_HIGHPASS, 120.0, 0.707)]
F2 = [(ph.EQ_HIGHPASS, 10.0, 5.0), (ph.EQ_PEAKING, 50.0, 30.0, -30.0), (ph.EQ_PEAKING, 100.0, 0.1, 30.0), (ph.EQ_LOWPASS, 9900.0, 10.0)]
SETS = {"one": [(ph.EQ_BANDPASS, 1500.0, 0.9)], "two": [(ph.EQ_HIGHPASS, 300.0, 0.707), (ph.EQ_LOWPASS, 3400.0, 0.707)], "three": B,
        "A": A, "F2": F2}
ZERO_DB = [(ph.EQ_PEAKING, 1000.0, 1.0, 0.0)]


def vector(n, seed):
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal(n)).astype(F32)
    if n > 40:
        x[[7, n // 2, n - 3]] = [np.nan, np.inf, -np.inf]  # read as 0
    return x


def eq_items(items, eq, rate):
    return [ph.eq_from_f32(x, eq, rate) for x in items]


def sinks_of(ys, rate):
    return {name: np.concatenate([mr.whole(y, f, rate, TABLES) for y in ys]) for name, f in SINKS.items()}


# ---- per-op

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, W * 64 - 1, W * 64, W * 64 + 1, CROSS, 98404])
def test_per_op(backend, n):
    x = vector(n, 500 + n)
    buf = backend.uploadFloat32(x if n else np.zeros(1, F32))
    for name, eq in SETS.items():
        out = backend.eq_f32(buf, 22050, eq, count=n)
        got = backend.downloadFloat32(out, n) if n else np.empty(0, F32)
        assert same_bits(got, ph.eq_from_f32(x, eq, 22050)), (n, name)


def test_per_op_unaligned_source_and_destination(backend):
    x = vector(20001, 9)
    want = ph.eq_from_f32(x, A, 16000)
    src = backend.uploadFloat32(np.concatenate([np.zeros(1, F32), x]))
    shifted = ph.DeviceBuffer(backend, src.ptr + 4, x.size, owned=False)  # one float off 16-byte alignment
    dst = backend.uploadFloat32(np.zeros(x.size + 1, F32))
    dshift = ph.DeviceBuffer(backend, dst.ptr + 4, x.size, owned=False)
    backend.eq_f32(shifted, 16000, A, out=dshift)
    assert same_bits(backend.downloadFloat32(dst, x.size + 1)[1:], want)
    assert same_bits(backend.downloadFloat32(backend.eq_f32(shifted, 16000, A), x.size), want)
    with pytest.raises(ph.InvalidArgument):
        backend.eq_f32(src, 8000, [(ph.EQ_LOWPASS, 3700.0, 0.707)])  # f0 above 0.45 · 8000


# ---- whole items

def plain(rt, slot):
    rt.prepare(slot, *item(rt.cfg, 14, 1), 0.667)


def ragged(rt, slot):
    rt.prepare_batch(slot, [item(rt.cfg, n, k) for k, n in enumerate((40, 14, 23))], 0.667)


def bounded(rt, slot):
    """prepare_batch_bounded of two items, a loud and a quieter one (the device draws the noise)"""
    import ctypes as C
    id_lists = [kd.FIXTURE_IDS * 2, kd.FIXTURE_IDS]
    bound = max(int(d.sum()) for d, _ in rt.predict_durations([(ids, None) for ids in id_lists], **DEV)) + 5
    arr, keep = (ph.Utterance * 2)(), []
    for i, (ids, scale) in enumerate(zip(id_lists, (0.667 * 16, 0.667 * 4))):
        arr[i], k = rt._utt(ids, None, None, scale, **DEV)
        keep.append(k)
    assert rt.lib.piper_hip_voice_prepare_batch_bounded(rt.voice, arr, 2, slot, bound) >= 0
    tot = C.c_int64()
    ph._check(rt.lib.piper_hip_voice_prepared_samples(rt.voice, slot, None, 0, C.byref(tot)))
    rt._keep[slot] = (keep, int(tot.value), True)


def clear(rt, *slots):
    for s in slots:
        rt.slot_eq(s, None)
        rt.slot_level(s, None)
        rt.slot_loudness(s, None)


@pytest.mark.parametrize("prep", [plain, ragged, bounded])
def test_whole_items(rt_medium, prep):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    clear(rt, 5, 6)
    prep(rt, 5)
    rt.launch(5)
    raw = rt.collect(5).copy()  # (a bounded slot: its collecting call)
    per, total = rt.prepared_samples(5)
    assert raw.size == total
    items = np.split(raw, np.cumsum(per)[:-1])
    steps = rt.steps(5)
    plain_bytes = {name: collect_as(rt, 5, name).copy() for name in SINKS}  # a slot that never had an EQ
    want = {k: sinks_of(eq_items(items, eq, rate), rate) for k, eq in (("A", A), ("B", B))}
    assert not same(want["A"]["f32"], raw) and not same(want["B"]["f32"], want["A"]["f32"])
    for k in ("A", "B", "A"):  # collects with different EQs on one launch, in any order
        eq = A if k == "A" else B
        for name in SINKS:
            assert same(collect_as(rt, 5, name, eq=eq), want[k][name]), (k, name)
    assert same_bits(rt.tap(5, "audio").reshape(-1), raw)  # the audio tap stays raw
    alaw = Format(0, "alaw", 1.0)  # A-law at the voice's own rate
    assert same(rt.collect_g711(5, "alaw", eq=A), np.concatenate([mr.whole(y, alaw, rate, TABLES) for y in eq_items(items, A, rate)]))
    assert rt.steps(5) == steps
    for name in SINKS:  # a cleared EQ: the bits of a slot that never had one
        assert same(collect_as(rt, 5, name, eq=None), plain_bytes[name]), (name, "cleared")
    assert not np.any((raw == 0) & np.signbit(raw))  # (a −0 would come back +0 through any EQ)
    for name in SINKS:  # a 0 dB peaking EQ passes the items unchanged
        assert same(collect_as(rt, 5, name, eq=ZERO_DB), plain_bytes[name]), (name, "0 dB")
    assert rt.steps(5) == steps
    # the EQ's collect as the first thing that reads a new run
    prep(rt, 6)
    rt.launch(6)
    assert same(rt.collect(6, eq=A), want["A"]["f32"])
    assert same_bits(rt.collect(6, eq=None), raw)
    clear(rt, 5, 6)


def test_volume_eq_loudness_and_level_together(rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    clear(rt, 5)
    ids, dur, noise = item(rt.cfg, 40, 11)
    vol = np.resize(np.array([1.0, 0.25, 1.0, 2.0, 0.0, 1.5], F32), len(ids))
    rt.prepare(5, ids, dur, noise, 0.667, volume=vol)
    rt.launch(5)
    v = rt.collect(5).copy()  # the volume's output: what the EQ reads
    e = ph.eq_from_f32(v, A, rate)
    L_raw, L_eq = ld.lufs(v, rate), ld.lufs(e, rate)
    print(f"L of v {L_raw:.4f}, of the EQ'd v {L_eq:.4f}")
    assert abs(L_raw - L_eq) > 0.1  # the EQ moves the loudness: a measurement of the un-EQ'd signal would be seen
    rt.slot_eq(5, A)
    rt.slot_loudness(5, (-16.0, 0.0))
    lufs, g = rt.loudness(5)
    assert abs(float(lufs[0]) - L_eq) <= 0.002, (lufs[0], L_eq)
    u = ld.apply(e, g[0])
    level = (3.0 / max(float(np.abs(u).max()), 1e-6), 0.5, 50.0)
    y = lr.apply(u, level, rate)
    for name, f in SINKS.items():
        assert same(collect_as(rt, 5, name, level=level), mr.whole(y, f, rate, TABLES)), name
    # a change of the EQ drops the measurement taken behind the old one
    rt.slot_eq(5, B)
    l2, _ = rt.loudness(5)
    assert abs(float(l2[0]) - ld.lufs(ph.eq_from_f32(v, B, rate), rate)) <= 0.002
    clear(rt, 5)
    assert same_bits(rt.collect(5), v)


def test_normalize_peaks_are_taken_over_the_eq_output(rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    clear(rt, 5)
    ragged(rt, 5)
    rt.launch(5)
    raw = rt.collect(5).copy()
    per, _ = rt.prepared_samples(5)
    es = eq_items(np.split(raw, np.cumsum(per)[:-1]), B, rate)
    got = rt.collect_pcm16(5, gain=0.5, normalize=True, eq=B)
    peaks = rt.peaks(5)
    want_peaks = np.array([np.max(np.abs(x)) for x in es], F32)
    assert np.array_equal(peaks, want_peaks)
    assert not np.array_equal(want_peaks, np.array([np.max(np.abs(x)) for x in np.split(raw, np.cumsum(per)[:-1])], F32))
    assert np.array_equal(got, pcm_ref.pcm16_items(es, 0.5, normalize=True))
    clear(rt, 5)


def test_synthesize_twins_and_x_low(backend, rt_medium):
    rt, rate = rt_medium, rt_medium.cfg.sample_rate
    clear(rt, 0)
    ids, dur, noise = item(rt.cfg, 14, 1)
    raw = rt.synthesize(ids, dur, noise, 0.667).copy()
    e = ph.eq_from_f32(raw, A, rate)
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, eq=A), e)
    assert same(rt.synthesize_pcm16(ids, dur, noise, 0.667, rate=8000), mr.whole(e, SINKS["s16@8000"], rate, TABLES))  # the EQ stays
    assert same(rt.synthesize_g711(ids, dur, "mulaw", noise, 0.667, rate=8000), mr.whole(e, SINKS["mulaw@8000"], rate, TABLES))
    assert same_bits(rt.synthesize(ids, dur, noise, 0.667, eq=None), raw)
    # the 16 kHz tier: the EQ runs at the voice's own rate
    cfg = ph.voice_config("x_low")
    lo = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    try:
        F = 3 * len(ids)
        nz = kd.sym(77, (cfg.inter, F), 1.7320508)
        tel = [(ph.EQ_HIGHPASS, 300.0, 0.707), (ph.EQ_PEAKING, 2500.0, 1.2, 4.0), (ph.EQ_LOWPASS, 3400.0, 0.707)]
        raw16 = lo.synthesize(ids, dur, nz, 0.667).copy()
        assert same_bits(lo.synthesize(ids, dur, nz, 0.667, eq=tel), ph.eq_from_f32(raw16, tel, cfg.sample_rate))
        with pytest.raises(ph.InvalidArgument):  # 7500 Hz is above 0.45 · 16000, though not above 0.45 · 22050
            lo.slot_eq(0, [(ph.EQ_LOWPASS, 7500.0, 0.707)])
        rt.slot_eq(7, [(ph.EQ_LOWPASS, 7500.0, 0.707)])
    finally:
        lo.close()
    clear(rt, 0, 7)


def test_state_rules(rt_medium):
    rt = rt_medium
    for bad in ([], [(ph.EQ_LOWPASS, 5.0, 0.707)], [(ph.EQ_PEAKING, 1000.0, 1.0, 31.0)], [(ph.EQ_LOWPASS, 1000.0, 0.707, 1.0)],
                [(9, 1000.0, 1.0)], [(ph.EQ_NOTCH, 1000.0, 0.05)]):
        with pytest.raises(ph.InvalidArgument):
            rt.slot_eq(5, bad)
    with pytest.raises(ph.InvalidArgument):
        rt.slot_eq(-1, A)
    rt.slot_eq(5, None)


# ---- command line

def test_cli_eq_equals_the_python_route(backend, voices, tmp_path):
    lib = os.path.join(ROOT, "piper-swift_amd", "lib")
    exe = tmp_path / "piper_hip_cli"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "piper_hip_cli.c"), "-L" + lib, "-lpiper_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    ids = kd.FIXTURE_IDS * 2
    raw = tmp_path / "a.s16le"
    flags = ["--eq", "highpass:300:0.707", "--eq", "peaking:2500:1:6", "--eq", "lowshelf:150:0.8:-4"]
    out = subprocess.run([str(exe), "--phoneme-ids", ",".join(str(i) for i in ids), "--output-raw", str(raw)] + flags,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    bad = subprocess.run([str(exe), "--phoneme-ids", "1,2", "--output-raw", str(raw), "--eq", "wobble:300:0.7"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 2 and "--eq" in bad.stderr
    cfg, blob = voices["medium"]
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        eq = [("highpass", 300.0, 0.707), ("peaking", 2500.0, 1.0, 6.0), ("lowshelf", 150.0, 0.8, -4.0)]
        want = rt.synthesize_pcm16(ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234, eq=eq).copy()
        plain = rt.synthesize_pcm16(ids, [3] * len(ids), None, 0.667, noise_mode="device", seed=1234, eq=None).copy()
    finally:
        rt.close()
    got = np.frombuffer(raw.read_bytes(), "<i2")
    assert np.array_equal(got, want) and not np.array_equal(got, plain)


# ---- streams: the twin is the same stream run without an EQ (tests/test_gpu_level.py); the EQ'd chunks are the host twin on the
# concatenated raw chunks, cut where the raw steps were cut (the EQ adds no delay and changes no count)

def eq_chunks(raw_chunks, eq, rate):
    y = ph.eq_from_f32(np.concatenate(raw_chunks), eq, rate)
    return np.split(y, np.cumsum([c.size for c in raw_chunks])[:-1])


def level_on(chunks):
    return (3.0 / max(float(np.abs(np.concatenate(chunks)).max()), 1e-6), 0.5, 50.0)


@pytest.mark.parametrize("chunk", [2, 3])
def test_single_stream(rt_medium, single_twin, chunk):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    ids, dur, noise = single_item(rt.cfg)
    raw = single_twin[chunk]
    want = eq_chunks(raw, A, rate)
    got = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3, eq=A))
    assert [g.size for g in got] == [w.size for w in want] and all(same_bits(g, w) for g, w in zip(got, want)), chunk
    level, fmt = level_on(want), SINKS["s16@8000"]
    got = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3, eq=A, level=level, **stream_kw(fmt)))
    check_row(got, want, level, fmt, chunk, hop, rate, ("single", chunk))
    again = list(rt.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=chunk, slot=3))  # a new begin clears the EQ
    assert len(again) == len(raw) and all(same_bits(a, b) for a, b in zip(again, raw))


def run_group(rt, chunk, eq, level=None, fmt=SINKS["f32"], drop=(0, 4)):
    per = [[] for _ in range(3)]
    for k, chunks in enumerate(rt.synthesize_stream_batch(group_items(rt.cfg), 0.667, chunkFrames=chunk, slot=8, eq=eq, level=level,
                                                           **stream_kw(fmt))):
        for i, c in enumerate(chunks):
            if c.size:
                per[i].append(c)
        if k == drop[1] - 1:
            rt.stream_drop(8, drop[0])
    return per


@pytest.mark.parametrize("chunk", [2, 3])
def test_group_of_three(rt_medium, group_twin, chunk):
    rt, hop, rate = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate
    raw = group_twin[chunk]
    got = run_group(rt, chunk, B)
    for i in range(3):
        want = eq_chunks(raw[i], B, rate)
        assert [g.size for g in got[i]] == [w.size for w in want] and all(same_bits(g, w) for g, w in zip(got[i], want)), (chunk, i)
    level, fmt = level_on([np.concatenate(eq_chunks(r, B, rate)) for r in raw]), SINKS["mulaw@8000"]
    got = run_group(rt, chunk, B, level, fmt)
    for i in range(3):
        check_row(got[i], eq_chunks(raw[i], B, rate), level, fmt, chunk, hop, rate, ("group", chunk, i), finished=i != 0)


def run_pool(rt, chunk, eq, level=None, formats=None):
    """Capacity 4: S (15 frames), E and A join, and P by a bounded join; when S has finished B takes its row — a new occupant that must
    start at block 0 with an empty carry. formats: {session: Format} on a mixed pool. Returns {session: [chunk per step]}."""
    u = pool_sessions(rt)
    mixed = formats is not None
    pool = rt.stream_pool(10, 4, chunkFrames=chunk, work_slot=11, mixed=mixed, eq=eq, level=level)
    assert rt.stream_eq(10).sections() == ph.Eq(eq).sections()
    lf = (lambda names: [ph.stream_format(rate=formats[s].rate, encoding=formats[s].enc, gain=formats[s].gain) for s in names]) if mixed else (lambda names: None)
    assert [i for i, _ in pool.join([u["S"], u["E"], u["A"]], 0.667, formats=lf("SEA"))] == [0, 1, 2]
    assert pool.join_bounded([u["P"]], 400, 0.667, formats=lf("P")) == [3]
    with pytest.raises(ph.InvalidArgument):  # after the first join the EQ is fixed
        pool.set_eq(eq)
    who = {0: "S", 1: "E", 2: "A", 3: "P"}
    per = {s: [] for s in "SEABP"}
    for k in range(256):
        if k == -(-15 // chunk):
            (row, _), = pool.join([u["B"]], 0.667, formats=lf("B"))
            assert row == 0
            who[0] = "B"
        if mixed:
            st = pool.step_mixed(raw=True)
            if not any(st[0]):
                break
            for r, c in enumerate(st[0]):
                if c:
                    f = formats[who[r]]
                    per[who[r]].append(st[2][st[1][r]:st[1][r] + c * mr.ELEM[f.enc]].view(mr.DTYPE[f.enc]).copy())
        else:
            out = pool.step()
            if not out:
                break
            for r, c in out.items():
                per[who[r]].append(c)
    pool.close()
    return per


def test_pool_with_a_retaken_row(rt_medium, pool_twin):
    rt, rate, chunk = rt_medium, rt_medium.cfg.sample_rate, 3
    raw = pool_twin[chunk]
    got = run_pool(rt, chunk, A)
    for s_ in "SEABP":
        want = eq_chunks(raw[s_], A, rate)
        assert [g.size for g in got[s_]] == [w.size for w in want] and all(same_bits(g, w) for g, w in zip(got[s_], want)), s_
    # the reference with S's carry planted in front of B (B continuing S's block count) differs from what B delivered
    s_all = np.concatenate(raw["S"])
    pad = (-s_all.size) % 64
    lead = np.concatenate([s_all, np.zeros(pad, F32)])
    haunted = ph.eq_from_f32(np.concatenate([lead] + raw["B"]), A, rate)[lead.size:]
    assert not same_bits(haunted, np.concatenate(got["B"]))


MIXED = {"S": Format(0, "f32", 1.0), "E": Format(8000, "s16", 1.0), "A": Format(8000, "mulaw", 1.0), "B": Format(0, "alaw", 1.0),
         "P": Format(8000, "alaw", 1.0)}


def test_mixed_pool_with_a_level(rt_medium, pool_twin):
    rt, hop, rate, chunk = rt_medium, rt_medium.cfg.hop, rt_medium.cfg.sample_rate, 2
    raw = pool_twin[chunk]
    eqd = {s_: eq_chunks(raw[s_], A, rate) for s_ in "SEABP"}
    level = level_on([np.concatenate(eqd[s_]) for s_ in "SEABP"])
    got = run_pool(rt, chunk, A, level, formats=MIXED)
    for s_ in "SEABP":
        check_row(got[s_], eqd[s_], level, MIXED[s_], chunk, hop, rate, ("mixed", s_))


def test_stream_state_rules(rt_medium):
    import ctypes as C
    rt, lib, hop = rt_medium, rt_medium.lib, rt_medium.cfg.hop
    ids, dur, noise = single_item(rt.cfg)
    u, keep = rt._utt(ids, dur, noise, 0.667)
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_eq(12, A)  # no stream there
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 3) > 0
    with pytest.raises(ph.InvalidArgument):
        rt.stream_eq(3)  # none yet
    with pytest.raises(ph.InvalidArgument):
        rt.stream_set_eq(3, [(ph.EQ_LOWPASS, 5.0, 0.707)])
    rt.stream_set_eq(3, B)
    rt.stream_set_eq(3, A)  # before the first step the EQ may still change
    assert rt.stream_eq(3).sections() == ph.Eq(A).sections()
    assert rt.stream_step_capacity(3) == 3 * hop  # no change to any count
    buf, got_n = np.empty(3 * hop, F32), C.c_int64()
    ph._check(lib.piper_hip_voice_stream_next(rt.voice, 3, buf.ctypes.data_as(ph.c_f32p), buf.size, C.byref(got_n)))
    assert got_n.value == 3 * hop
    with pytest.raises(ph.InvalidArgument):  # after a step the EQ is fixed
        rt.stream_set_eq(3, B)
    assert lib.piper_hip_voice_stream_begin(rt.voice, C.byref(u), 3, 3) > 0  # a new begin clears it
    with pytest.raises(ph.InvalidArgument):
        rt.stream_eq(3)
    del keep
