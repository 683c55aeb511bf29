"""GPU: per-phoneme prosody (include/piper_hip.h "Per-phoneme prosody") on every route. The frame rule from w0 on is integers behind one
correctly rounded multiply, so durations are held to tests/prosody_ref.py by equality, with no element left out; the noise rule is held
bit for bit where a multiplier is 0 or 1 and to the float64 restatement under front_ref's op rule otherwise. A neutral prosody must
reproduce the request without prosody bit for bit, through plans of its own (the "_prosody" step names).

The taps compact every item to its true length; what lies past it in the bucket row is read through the whole-row views "dp.w.row" and
"dp.dur.row" of the prosody predictor plan."""
import numpy as np
import pytest

import front_ref
import katdata as kd
import piper_hip as ph
import prosody_ref as pr
from conftest import WAVE_TOL, assert_close
from test_gpu_stream_batch import TOL as STREAM_TOL

pytestmark = pytest.mark.gpu

IDS = list(kd.FIXTURE_IDS)
SD = kd.case_seed("dp", 0) + 900
DEV = {"noise_mode": "device", "seed": 2718}


def dpn(k, ids):
    return kd.sym(SD + k, (2, len(ids)), 1.7320508)


def neutral(t):
    return dict(length=np.ones(t, np.float32), min_frames=np.zeros(t, np.int32), max_frames=np.zeros(t, np.int32), noise=np.ones(t, np.float32))


def split(flat, lens, C_=1):
    offs = np.concatenate([[0], np.cumsum([C_ * n for n in lens])])
    return [flat[offs[i]:offs[i + 1]].reshape(C_, -1) for i in range(len(lens))]


def run(rt, slot):
    rt.launch(slot)
    return rt.collect(slot).copy()


@pytest.fixture(scope="module")
def rt(backend, voices):
    cfg, blob = voices["medium"]
    r = ph.HipRuntime(backend, cfg, blob)
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------ 1. neutral is the identity
def test_neutral_prosody_is_the_identity_on_plans_of_its_own(rt):
    cfg = rt.cfg
    a, b = IDS * 3, IDS * 2
    kw = dict(length_scale=1.1, noise_w=0.8, dp_noise=dpn(1, a), **DEV)
    # prepare, predicted
    rt.prepare(1, a, None, None, 0.667, **kw)
    plain, dur = run(rt, 1), rt.durations(1).copy()
    steps, psteps, bucket = rt.steps(1), rt.steps(1, predict=True), rt.plan_info(1)["bucket_f"]
    assert "expand_noise" in steps and "dp.affine_exp_ceil" in psteps
    assert not any(s.endswith("_prosody") for s in steps + psteps)
    rt.prepare(1, a, None, None, 0.667, prosody=neutral(len(a)), **kw)
    got = run(rt, 1)
    assert rt.plan_info(1)["bucket_f"] == bucket
    assert np.array_equal(rt.durations(1), dur) and np.array_equal(got, plain)
    s2, p2 = rt.steps(1), rt.steps(1, predict=True)
    assert "expand_noise_prosody" in s2 and "expand_noise" not in s2 and len(s2) == len(steps)
    assert "dp.affine_exp_ceil_prosody" in p2 and "dp.affine_exp_ceil" not in p2 and len(p2) == len(psteps)
    assert [x for x in s2 if x != "expand_noise_prosody"] == [x for x in steps if x != "expand_noise"]
    assert rt.prosody_report(1) == ([int(dur.sum())], [0])
    # time_subset reaches the predictor plan's step through "predict:", and only there
    assert rt.time_subset(1, "predict:dp.affine_exp_ceil_prosody|expand_noise_prosody", 2)[1] == 1
    assert rt.time_subset(1, "dp.affine_exp_ceil_prosody|expand_noise_prosody", 2)[1] == 1
    assert rt.time_subset(1, "dp.affine_exp_ceil_prosody|", 2)[1] == 0
    assert np.array_equal(run(rt, 1), plain)
    # the request without prosody afterwards still finds the plain plans
    rt.prepare(1, a, None, None, 0.667, **kw)
    assert rt.steps(1) == steps and rt.steps(1, predict=True) == psteps and np.array_equal(run(rt, 1), plain)
    # prepare_batch, ragged: a predicted item with a neutral prosody next to an item with supplied durations and none
    durb = [2, 3] * len(IDS)
    nzb = kd.sym(SD + 2, (cfg.inter, sum(durb)), 1.7320508)
    items = [(a, None, None, kw), (b, durb, nzb)]
    rt.prepare_batch(2, items, 0.667)
    plain2, dur2 = run(rt, 2), rt.durations(2).copy()
    steps2 = rt.steps(2)
    assert "expand_noise" in steps2
    rt.prepare_batch(2, items, 0.667, prosody=[neutral(len(a))])
    assert "expand_noise_prosody" in rt.steps(2) and len(rt.steps(2)) == len(steps2)
    assert np.array_equal(rt.durations(2), dur2) and np.array_equal(run(rt, 2), plain2)
    # prepare_batch_bounded
    bound = int(dur.sum()) + 9
    pairs = [(a, dpn(1, a)), (b, dpn(3, b))]
    rt.prepare_batch_bounded(3, pairs, bound, length_scale=1.1, **DEV)
    plain3, dur3 = run(rt, 3), rt.durations(3).copy()
    rt.prepare_batch_bounded(3, pairs, bound, length_scale=1.1, prosody=[neutral(len(a)), None], **DEV)
    got3 = run(rt, 3)
    assert "expand_noise_prosody" in rt.steps(3) and "dp.affine_exp_ceil_prosody" in rt.steps(3, predict=True)
    assert np.array_equal(rt.durations(3), dur3) and np.array_equal(got3, plain3)
    assert np.array_equal(dur3[:len(a)], dur)
    wanted, fitted = rt.prosody_report(3)
    assert wanted == [int(dur3[:len(a)].sum()), int(dur3[len(a):].sum())] and fitted == [0, 0]


# ------------------------------------------------------------------------------------------------ 2. the duration rule, exact
def test_duration_rule_is_exact_in_a_ragged_batch(rt):
    cfg = rt.cfg
    lists = [IDS * 4, IDS * 2, IDS * 3]
    lens = [len(x) for x in lists]
    ls = 1.3
    items = [(ids, None, None, dict(length_scale=ls, noise_w=0.8, dp_noise=dpn(10 + i, ids), **DEV)) for i, ids in enumerate(lists)]
    length = np.tile(np.array([0.0, 0.5, 1.0, 1.7], np.float32), lens[0] // 4 + 1)[:lens[0]]
    # w0 does not depend on the prosody: learn it with the multipliers alone, then put two ceilings below what the rule predicts there
    rt.prepare_batch(4, items, 0.667, prosody=[dict(length=length)])
    w0_first = split(rt.tap(4, "predict:dp.w"), lens)[0][0]
    d_len = pr.durations(w0_first, dict(length=length))
    big = [int(t) for t in np.nonzero(d_len >= 2)[0]]
    assert len(big) >= 3, d_len
    ceil_ids, both = big[:2], big[2]
    mx0, mn0 = np.zeros(lens[0], np.int32), np.zeros(lens[0], np.int32)
    mx0[ceil_ids] = 1
    floor_ids = [t for t in range(lens[0]) if t not in big][:2]
    mn0[floor_ids] = [9, 12]
    mn0[both], mx0[both] = 4, 6  # both a floor and a ceiling (the prediction lies below the floor or inside: the rule decides)
    pros = [dict(length=length, min_frames=mn0, max_frames=mx0),
            dict(min_frames=np.where(np.arange(lens[1]) % 9 == 4, 7, 0).astype(np.int32)), None]
    rt.prepare_batch(4, items, 0.667, prosody=pros)
    audio = run(rt, 4)
    w0 = split(rt.tap(4, "predict:dp.w"), lens)
    logw = split(rt.tap(4, "predict:dp.logw"), lens)
    dd = split(rt.tap(4, "predict:dp.dur").view(np.int32), lens)
    used = split(rt.durations(4), lens)
    assert np.array_equal(w0[0][0], w0_first)
    # ids past an item's length are 0: the whole bucket rows [T] of the three items, the two shorter ones with a tail
    T = rt.plan_info(4)["bucket_t"]
    w_rows = rt.tap(4, "predict:dp.w.row").reshape(3, T)
    d_rows = rt.tap(4, "predict:dp.dur.row").view(np.int32).reshape(3, T)
    assert T >= lens[0] and T - lens[1] >= 16 and T - lens[2] >= 8
    for i in range(3):
        assert np.array_equal(w_rows[i, :lens[i]], w0[i][0]) and np.array_equal(d_rows[i, :lens[i]], dd[i][0])
        assert np.all(w_rows[i, lens[i]:] == 0.0) and np.all(d_rows[i, lens[i]:] == 0), i
    total = 0
    for i in range(3):
        ref = pr.durations(w0[i][0], pros[i])
        assert np.array_equal(dd[i][0], ref), (i, np.nonzero(dd[i][0] != ref)[0])
        assert ref.sum() >= 1 and np.array_equal(used[i][0], ref)
        r = front_ref.compare(w0[i][0], np.exp(logw[i][0].astype(np.float64)) * np.float64(np.float32(ls)))
        print(f"item {i}: dp.w vs float64  max|Δ| = {r['err']:.3e}  bound {r['bound']:.3e}")
        assert r["ok"], r
        total += pr.frame_count(ref)
    d0 = dd[0][0]
    assert np.all(d0[length == 0.0][mn0[length == 0.0] == 0] == 0)  # length 0 silences an id that has no floor
    assert d0[ceil_ids].tolist() == [1, 1] and d0[floor_ids].tolist() == [9, 12] and 4 <= d0[both] <= 6
    assert audio.size == total * cfg.hop
    assert rt.prepared_samples(4)[0] == [pr.frame_count(x[0]) * cfg.hop for x in dd]
    assert rt.prosody_report(4) == ([int(x[0].sum()) for x in dd], [0, 0, 0])


# ------------------------------------------------------------------------------------------------ 3. fit
def test_fit_compresses_to_the_bound_on_the_device(rt):
    cfg, hop = rt.cfg, rt.cfg.hop
    a, b = IDS * 4, IDS * 2
    pairs = [(a, dpn(20, a)), (b, dpn(21, b))]
    kw = dict(length_scale=1.2, **DEV)
    rt.prepare_batch_bounded(5, pairs, 1024, **kw)  # unfitted, to learn the totals
    run(rt, 5)
    d_plain = split(rt.durations(5), [len(a), len(b)])
    FA, FB = int(d_plain[0].sum()), int(d_plain[1].sum())
    cap = (FA + FB) // 2
    assert FB < cap < FA, (FA, FB)
    rt.prepare_batch_bounded(5, pairs, cap, prosody=[dict(fit=1), dict(fit=1)], **kw)
    audio = run(rt, 5)  # collect succeeds
    assert rt.prosody_report(5) == ([FA, FB], [1, 0])
    used = split(rt.durations(5), [len(a), len(b)])
    dd = split(rt.tap(5, "predict:dp.dur").view(np.int32), [len(a), len(b)])
    assert np.array_equal(dd[0][0], d_plain[0][0]) and np.array_equal(dd[1][0], d_plain[1][0])  # dp.dur stays what the rule wanted
    fitted, S, flag = pr.fit(dd[0][0], cap)
    assert (S, flag) == (FA, 1)
    assert np.array_equal(used[0][0], fitted) and np.array_equal(used[0][0], (dd[0][0].astype(np.int64) * cap // FA).astype(np.int32))
    assert int(used[0][0].sum()) <= cap
    assert np.array_equal(used[1][0], d_plain[1][0])  # the second item is unchanged
    Fa = pr.frame_count(fitted)
    assert rt.prepared_samples(5)[0] == [Fa * hop, FB * hop] and audio.size == (Fa + FB) * hop
    bucket = rt.plan_info(5)["bucket_f"]
    # the same waveform as a plain prepare_batch with the fitted durations supplied, the same device seed
    rt.prepare_batch(6, [(a, fitted, None, DEV), (b, d_plain[1][0], None, DEV)], 0.667)
    ref = run(rt, 6)
    same_bucket = rt.plan_info(6)["bucket_f"] == bucket
    print(f"fit: FA {FA} FB {FB} cap {cap} -> {Fa}; buckets {bucket} / {rt.plan_info(6)['bucket_f']}; max|Δ| = {np.abs(audio - ref).max():.3e}")
    if same_bucket:
        assert np.array_equal(audio, ref), np.abs(audio - ref).max()
    else:
        assert_close(audio, ref, WAVE_TOL, "fitted bounded request vs prepare_batch with the fitted durations")
    # without fit the same request fails as it always did
    rt.prepare_batch_bounded(5, pairs, cap, prosody=[dict(fit=0), dict(fit=0)], **kw)
    rt.launch(5)
    with pytest.raises(ph.ShapeMismatch, match=f"wants {FA} frames"):
        rt.collect(5)


# ------------------------------------------------------------------------------------------------ 4. noise
def test_noise_multipliers_per_id(rt):
    cfg = rt.cfg
    ids = IDS * 3
    t, I = len(ids), cfg.inter
    kw = dict(length_scale=1.1, noise_w=0.8, dp_noise=dpn(30, ids), **DEV)
    rt.prepare(7, ids, None, None, 0.667, **kw)
    run(rt, 7)
    d = rt.durations(7).copy()
    F = int(d.sum())
    zp_plain = rt.tap(7, "z_p").reshape(I, F).copy()
    f2i = pr.frame_ids(d)
    # all 0: the latent is the expanded mean, bit for bit
    rt.prepare(7, ids, None, None, 0.667, prosody=dict(noise=np.zeros(t, np.float32)), **kw)
    run(rt, 7)
    assert np.array_equal(rt.durations(7), d)
    m_p = rt.tap(7, "m_p").reshape(I, t)
    assert np.array_equal(rt.tap(7, "z_p").reshape(I, F), m_p[:, f2i])
    # a 0/1 pattern: the frames of the 1-ids are the run without prosody, those of the 0-ids the mean
    pat = (np.arange(t) % 3 != 1).astype(np.float32)
    rt.prepare(7, ids, None, None, 0.667, prosody=dict(noise=pat), **kw)
    run(rt, 7)
    zp = rt.tap(7, "z_p").reshape(I, F)
    on = pat[f2i] == 1.0
    assert on.any() and (~on).any()
    assert np.array_equal(zp[:, on], zp_plain[:, on]) and np.array_equal(zp[:, ~on], m_p[:, f2i][:, ~on])
    # general multipliers, injected noise, supplied durations (noise alone is allowed there) against float64
    dur = [(3 * k) % 5 for k in range(t)]
    Fs = sum(dur)
    nz = kd.sym(SD + 31, (I, Fs), 1.7320508)
    p = dict(noise=(0.25 + 1.5 * kd.sym(SD + 32, (t,), 0.5).astype(np.float32) ** 2 * 4).astype(np.float32))
    rt.prepare(7, ids, dur, nz, 0.667, prosody=p)
    run(rt, 7)
    assert "expand_noise_prosody" in rt.steps(7) and np.array_equal(rt.durations(7), dur)
    m_p, logs_p = rt.tap(7, "m_p").reshape(I, t), rt.tap(7, "logs_p").reshape(I, t)
    got = rt.tap(7, "front.zp@expand_noise_prosody").reshape(I, Fs)
    r = front_ref.compare(got, pr.expand(m_p, logs_p, dur, nz, 0.667, p))
    print(f"expand_noise_prosody vs float64: max|Δ| = {r['err']:.3e}  bound {r['bound']:.3e}")
    assert r["ok"], r
    plain = front_ref.compare(got, pr.expand(m_p, logs_p, dur, nz, 0.667, None))
    assert not plain["ok"]  # the multipliers are visible at this bound


# ------------------------------------------------------------------------------------------------ 5. routes
def test_group_stream_with_a_pause_floor(rt):
    hop = rt.cfg.hop
    a, b = IDS * 3, IDS * 2
    items = [(a, None, None, dict(dp_noise=dpn(40, a), **DEV)), (b, None, None, dict(dp_noise=dpn(41, b), **DEV))]
    mn = np.zeros(len(a), np.int32)
    mn[13], mn[27] = 25, 18  # pauses behind two words
    pros = [dict(min_frames=mn), None]
    rt.prepare_batch(8, items, 0.667, prosody=pros)
    whole = run(rt, 8)
    per = rt.prepared_samples(8)[0]
    d = rt.durations(8)
    assert d[13] == 25 and d[27] == 18
    chunks = list(rt.synthesize_stream_batch(items, 0.667, chunkFrames=32, slot=8, prosody=pros))
    got = [np.concatenate([c[i] for c in chunks]) for i in range(2)]
    assert [g.size for g in got] == per
    assert_close(np.concatenate(got), whole, STREAM_TOL, "group chunks vs collect of the same request")


def test_pool_joins_with_a_pause_floor_and_with_fit(rt):
    hop = rt.cfg.hop
    ids = IDS * 2
    utt = (ids, None, None, dict(dp_noise=dpn(50, ids), **DEV))
    mn = np.zeros(len(ids), np.int32)
    mn[13] = 21
    whole = rt.synthesize(ids, None, None, 0.667, dp_noise=dpn(50, ids), prosody=dict(min_frames=mn), **DEV)
    d_floor = rt.durations(0).copy()
    assert d_floor[13] == 21
    rt.prepare(0, ids, None, None, 0.667, dp_noise=dpn(50, ids), **DEV)
    d_plain = rt.durations(0).copy()
    F = int(d_plain.sum())
    pool = rt.stream_pool(10, 4, chunkFrames=32, work_slot=11)
    try:
        # a join refused before it reaches the library leaves no assignment behind for the next, unrelated join
        with pytest.raises(ph.InvalidArgument, match="formats"):
            pool.join([utt], 0.667, formats=[None, None], prosody=[dict(min_frames=mn)])
        ((item, samples),) = pool.join([utt], 0.667)
        assert samples == F * hop and np.array_equal(rt.durations(11), d_plain)
        pool.drop(item)
        # a plain join whose item carries a pause floor: against samples_out
        ((item, samples),) = pool.join([utt], 0.667, prosody=[dict(min_frames=mn)])
        assert samples == int(d_floor.sum()) * hop and np.array_equal(rt.durations(11), d_floor)
        got = []
        for _ in range(64):
            out = pool.step()
            if not out:
                break
            got.append(out[item])
        got = np.concatenate(got)
        assert got.size == samples
        assert_close(got, whole, STREAM_TOL, "pool session with a pause floor vs the whole utterance")
        # a bounded join with a tight bound and fit: an ordinary active row of Σ fitted · hop samples
        cap = F - 7
        fitted, S, flag = pr.fit(d_plain, cap)
        assert (S, flag) == (F, 1)
        (item,) = pool.join_bounded([utt], cap, 0.667, prosody=[dict(fit=1)])
        want = pr.frame_count(fitted) * hop
        assert pool.item_samples(item) == want
        assert np.array_equal(rt.durations(11), fitted) and rt.prosody_report(11) == ([F], [1])
        n = 0
        for _ in range(64):
            out = pool.step()
            if not out:
                break
            n += out[item].size
        assert n == want
        # the same tight bound without fit fails as it does today: the row never delivers
        (item,) = pool.join_bounded([utt], cap, 0.667, prosody=[dict(fit=0)])  # (the prosody plans and their generate_path, fit off)
        with pytest.raises(ph.ShapeMismatch, match=f"{F}"):
            pool.item_samples(item)
        assert pool.step() == {} and pool.free_rows == 4
    finally:
        pool.close()


def other_voice_checks(r, what):
    ids = IDS * 2
    t = len(ids)
    kw = dict(length_scale=1.15, noise_w=0.8, dp_noise=dpn(60, ids), **DEV)
    r.prepare(1, ids, None, None, 0.667, **kw)
    plain, dur = run(r, 1), r.durations(1).copy()
    r.prepare(1, ids, None, None, 0.667, prosody=neutral(t), **kw)
    assert np.array_equal(run(r, 1), plain) and np.array_equal(r.durations(1), dur), what
    assert "dp.affine_exp_ceil_prosody" in r.steps(1, predict=True) and "expand_noise_prosody" in r.steps(1)
    p = dict(length=np.tile(np.array([0.5, 1.7, 1.0, 0.0], np.float32), t // 4), min_frames=np.where((np.arange(t) % 7 == 6) & (np.arange(t) % 5 != 0), 5, 0).astype(np.int32),
             max_frames=np.where(np.arange(t) % 5 == 0, 2, 0).astype(np.int32))
    r.prepare(1, ids, None, None, 0.667, prosody=p, **kw)
    audio = run(r, 1)
    w0 = r.tap(1, "predict:dp.w")
    ref = pr.durations(w0, p)
    assert np.array_equal(r.tap(1, "predict:dp.dur").view(np.int32), ref), what
    assert np.array_equal(r.durations(1), ref) and audio.size == pr.frame_count(ref) * r.cfg.hop, what


def test_x_low_voice(backend):
    cfg = ph.voice_config("x_low")
    r = ph.HipRuntime(backend, cfg, ph.synthetic_blob(cfg, 1234))
    try:
        other_voice_checks(r, "x_low")
    finally:
        r.close()


def test_voice_with_a_speaker_table(backend, voices):
    cfg, blob = voices["medium"]
    r = ph.HipRuntime(backend, cfg, blob)
    try:
        scfg = ph.speaker_config(4, 16)
        r.attach_speakers(scfg, ph.synthetic_speaker_blob(cfg, scfg, 4321))
        r.slot_speakers(1, [{1: 0.75, 3: 0.25}])
        other_voice_checks(r, "speakers")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. lifecycle and refusals
def test_lifecycle_and_refusals(rt):
    ids = IDS * 2
    t = len(ids)
    kw = dict(dp_noise=dpn(70, ids), **DEV)
    # consumed once
    rt.slot_prosody(9, [dict(length=np.full(t, 0.5, np.float32))])
    rt.prepare(9, ids, None, None, 0.667, **kw)
    assert "expand_noise_prosody" in rt.steps(9)
    short = rt.durations(9).copy()
    rt.prepare(9, ids, None, None, 0.667, **kw)
    assert "expand_noise" in rt.steps(9) and rt.durations(9).sum() >= short.sum()
    a = run(rt, 9)
    # a refused staging call clears the assignment and stages nothing: what the slot held is still collectable
    rt.slot_prosody(9, [dict(length=np.ones(t - 1, np.float32))])
    with pytest.raises(ph.ShapeMismatch, match="prosody has"):
        rt.prepare(9, ids, None, None, 0.667, **kw)
    assert np.array_equal(rt.collect(9), a)
    rt.prepare(9, ids, None, None, 0.667, **kw)  # the refused call took the assignment with it
    assert "expand_noise" in rt.steps(9) and np.array_equal(run(rt, 9), a)
    # duration fields on an item whose durations are supplied; noise alone passes
    dur = [2] * t
    for field in (dict(length=np.ones(t, np.float32)), dict(min_frames=np.zeros(t, np.int32)), dict(max_frames=np.zeros(t, np.int32)), dict(fit=1)):
        with pytest.raises(ph.InvalidArgument, match="durations are supplied"):
            rt.prepare(9, ids, dur, None, 0.667, prosody=field)
    rt.prepare(9, ids, dur, None, 0.667, prosody=dict(noise=np.ones(t, np.float32)))
    # fit on routes without a frame bound
    with pytest.raises(ph.InvalidArgument, match="frame bound"):
        rt.prepare(9, ids, None, None, 0.667, prosody=dict(fit=1), **kw)
    with pytest.raises(ph.InvalidArgument, match="frame bound"):
        list(rt.synthesize_stream_batch([(ids, None, None, kw)], 0.667, slot=9, prosody=[dict(fit=1)]))
    rt.prepare(9, ids, None, None, 0.667, max_frames=512, prosody=dict(fit=1), **kw)  # allowed where there is a bound
    # the size of an assignment, and a bad entry, are refused on the host and leave the assignment in place
    arr = (ph.Prosody * 257)()
    assert rt.lib.piper_hip_voice_slot_prosody(rt.voice, 9, arr, 257) == -7
    with pytest.raises(ph.InvalidArgument, match=r"prosody 1: noise\[2\]"):
        rt.slot_prosody(9, [dict(t=t), dict(noise=[1.0, 1.0, -2.0])])
    rt.slot_prosody(9, [])  # n = 0 clears
    rt.prepare(9, ids, None, None, 0.667, **kw)
    assert "expand_noise" in rt.steps(9)
