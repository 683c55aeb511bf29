"""GPU: the 16 kHz tier. x_low (hidden 96, two heads of head_dim 48, the medium generator) through every entry point, and low (the
medium geometry at 16 000 Hz).

An x_low voice needs two things the 192-channel voices never asked for: `voice_create` has to take inter = 96 (it wanted inter % 64 == 0:
ShapeMismatch), and the length-aware attention kernels have to exist at head_dim 48 — every plan passes the true length of each item, so
without them the first launch of any x_low plan is refused (UnsupportedOp). Routes by bucket T (csrc/attention.hip): the staged-tile kernel up
to 1024 (key-split in parts + merge from two key tiles on), the register-fragment kernel with 16 query rows per block up to 2048 and
with 8 above.

Tolerances are the ones tests/test_gpu_voice.py applies to the medium voice for the same quantity: OP_TOL on the taps, WAVE_TOL on the
waveform (both against the oracle), 2e-5 streamed against whole, 35 dB for the bf16 generator; LOGW_TOL of
tests/test_duration_predictor.py for the predictor; the bounds of tests/test_gpu_front_exact.py for the teacher-forced steps.
Durations are 1 … 3 frames per id so the CPU oracle's generator stays cheap; every oracle result is computed once per module."""
import wave

import numpy as np
import pytest

import att_ref
import front_ref as fr
import katdata as kd
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, WAVE_TOL, assert_close
from test_duration_predictor import LOGW_TOL, ceil_safe
from test_gpu_front_exact import prepare_predicted, report_line, run_and_verify
from test_gpu_voice import BF16_MIN_SNR_DB, run_with_taps, snr_db

pytestmark = pytest.mark.gpu

SD = kd.case_seed("mod", 0) + 16000
STREAM_TOL = 2e-5
TAPS = ("enc_out", "m_p", "z_p", "z")


@pytest.fixture(scope="module")
def xl():
    cfg = ph.voice_config("x_low")
    return cfg, ph.synthetic_blob(cfg, 1234)


@pytest.fixture(scope="module")
def rt_xl(backend, xl):
    rt = ph.HipRuntime(backend, *xl)
    yield rt
    rt.close()


def utterance(cfg, T, seed=0):
    """T ids, 1 … 3 frames each (mostly 1), injected noise."""
    rng = np.random.RandomState(100 + T + seed)
    ids = rng.randint(0, 130, size=T).tolist()
    dur = [(1, 1, 2, 1, 3, 1, 1, 2)[(i + T + seed) % 8] for i in range(T)]
    return ids, dur, kd.sym(SD + T + 7 * seed, (cfg.inter, sum(dur)), 1.7320508)


@pytest.fixture(scope="module")
def refs(xl):
    """oracle.synthesize(..., taps=True) of utterance(cfg, T), computed on first use and only read afterwards."""
    cfg, blob = xl
    cache = {}

    def get(T):
        if T not in cache:
            ids, dur, noise = utterance(cfg, T)
            audio, taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
            for a in [audio] + list(taps.values()):
                a.setflags(write=False)
            cache[T] = (audio, taps)
        return cache[T]
    return get


def check_against_oracle(audio, taps, ref, what, names=TAPS):
    ref_audio, ref_taps = ref
    for k in names:
        assert_close(taps[k], ref_taps[k], OP_TOL, f"{what}: {k} vs oracle")
    assert_close(audio, ref_audio, WAVE_TOL, f"{what}: audio vs oracle")


# ------------------------------------------------------------------------------------------------ single utterances
@pytest.mark.parametrize("T,bucket", [(1, 16), (5, 16), (16, 16), (17, 32), (130, 144)])
def test_single_utterance_vs_oracle(T, bucket, rt_xl, xl, refs):
    """Bucket 144 is two key tiles: 9 · 2 blocks leave room for two parts per head on any device with 36 CUs or more, so the attention
    core runs key-split with the merge kernel (rel_attention_split_parts > 1)."""
    cfg, _ = xl
    ids, dur, noise = utterance(cfg, T)
    audio, taps = run_with_taps(rt_xl, ids, dur, noise)
    assert rt_xl.plan_info(0)["bucket_t"] == bucket
    assert audio.size == sum(dur) * 256 == rt_xl.num_samples(ids, dur)
    steps = rt_xl.steps(0)
    assert sum(s.endswith(".rel_attention") for s in steps) == cfg.n_layers, steps
    check_against_oracle(audio, taps, refs(T), f"x_low T={T}")
    rt_xl.launch(0)
    assert np.array_equal(rt_xl.collect(0), audio), "graph replay is not deterministic"


# ------------------------------------------------------------------------------------------------ long rows
@pytest.mark.parametrize("T,bucket", [(1030, 1040), (2050, 2064)])
def test_long_rows_encoder_vs_oracle(T, bucket, rt_xl, xl):
    """Above 1024 the register-fragment kernels: att_mfma<48, 16> up to 2048, att_mfma<48, 8> above (id rows are bucketed in steps of 16 at
    every length: 1040 and 2064). The true lengths lie 10 and 14 columns below the bucket, so what this reaches of the length masking is
    the last key tile only, and enc_out under the rule with the floor; lengths far below the bucket and at the tile and chunk edges, and
    the attention step itself without the floor, are in tests/test_gpu_attention_lengths.py. Only the encoder is compared (enc_out, m_p,
    logs_p against oracle.text_encoder) so the CPU generator is not paid for; one frame per id."""
    cfg, blob = xl
    ids = np.random.RandomState(T).randint(0, 130, size=T).tolist()
    dur = [1] * T
    audio, taps = run_with_taps(rt_xl, ids, dur, None, slot=2)
    assert rt_xl.plan_info(2)["bucket_t"] == bucket
    assert audio.size == T * 256 and np.all(np.isfinite(audio))
    enc, stats = orc.text_encoder(cfg, blob, ids)
    assert_close(taps["enc_out"], enc, OP_TOL, f"x_low T={T}: enc_out")
    assert_close(taps["m_p"], stats[:cfg.inter], OP_TOL, f"x_low T={T}: m_p")
    assert_close(taps["logs_p"], stats[cfg.inter:], OP_TOL, f"x_low T={T}: logs_p")


# ------------------------------------------------------------------------------------------------ ragged batch
def test_ragged_batch_items_equal_their_single_runs(rt_xl, xl, refs):
    """7, 16 and 40 ids in one plan (bucket 48): the per-item true lengths mask keys and rows in the attention. Each item against its own
    single-utterance run on the GPU and against the oracle."""
    cfg, _ = xl
    Ts = (7, 16, 40)
    utts = [utterance(cfg, T) for T in Ts]
    singles = []
    for u in utts:
        a, t = run_with_taps(rt_xl, *u, slot=3)
        singles.append((a.copy(), {k: v.copy() for k, v in t.items()}))
    rt_xl.prepare_batch(4, utts, 0.667)
    assert rt_xl.plan_info(4)["bucket_t"] == 48
    rt_xl.launch(4)
    audio = rt_xl.collect(4)
    H, I = cfg.hidden, cfg.inter
    Fs = [sum(u[1]) for u in utts]
    got = {"enc_out": rt_xl.tap(4, "enc_out", H * sum(Ts)), "m_p": rt_xl.tap(4, "m_p", I * sum(Ts)),
           "z_p": rt_xl.tap(4, "z_p", I * sum(Fs)), "z": rt_xl.tap(4, "z", I * sum(Fs))}
    rows = {"enc_out": (H, Ts), "m_p": (I, Ts), "z_p": (I, Fs), "z": (I, Fs)}
    off = dict.fromkeys(got, 0)
    aoff = 0
    for b, T in enumerate(Ts):
        taps = {}
        for k, (ch, lens) in rows.items():
            taps[k] = got[k][off[k]:off[k] + ch * lens[b]]
            off[k] += ch * lens[b]
        a = audio[aoff:aoff + Fs[b] * 256]
        aoff += Fs[b] * 256
        check_against_oracle(a, taps, refs(T), f"ragged item {b} (T={T})")
        for k in TAPS:
            assert_close(taps[k], singles[b][1][k], OP_TOL, f"ragged item {b}: {k} vs its single run")
        assert_close(a, singles[b][0], WAVE_TOL, f"ragged item {b}: audio vs its single run")
    assert aoff == audio.size


# ------------------------------------------------------------------------------------------------ every front step, teacher-forced
@pytest.mark.parametrize("T,F", [(1, 1), (14, 42), (130, 390)])
def test_front_steps_float64(T, F, rt_xl, xl):
    """Every encoder and flow step of the x_low schedule against the float64 formulas of tests/front_ref.py, fed the GPU's own buffers
    through the "@step" taps, at that file's bounds (the walker fails on a step name it does not know)."""
    cfg, blob = xl
    _, rows, steps = run_and_verify(rt_xl, blob, 5, [fr.utterance(cfg, T, F, 2000 + T + F)], f"x_low T={T} F={F}", check_z=False)
    assert "embed" in steps and "expand_noise" in steps and sum(s.endswith(".rel_attention") for s in steps) == cfg.n_layers
    assert {r[0] for r in rows} == set(steps)


def test_front_steps_float64_ragged_batch(rt_xl, xl):
    cfg, blob = xl
    utts = [fr.utterance(cfg, T, 2 * T, 2300 + T) for T in (40, 7, 16)]
    _, rows, _ = run_and_verify(rt_xl, blob, 5, utts, "x_low ragged 40/7/16", check_z=False)
    assert {r[2] for r in rows} == {0, 1, 2}


def test_predictor_steps_float64(rt_xl, xl):
    """The encoder + predictor plan (durations = NULL) step by step, as tests/test_gpu_front_exact.py::test_predictor_plan does for medium."""
    cfg, blob = xl
    ids = list(np.random.RandomState(9).randint(1, 130, size=14))
    dpn = fr.dp_noise(14, 1)
    prepare_predicted(rt_xl, 6, [(ids, dpn)], 0.8)
    rt_xl.launch(6)
    rt_xl.collect(6)
    pdev = fr.GpuDevice(rt_xl, 6, [14], [0], predict=True)
    rows, ref_s = fr.verify(pdev, cfg, blob, [fr.Inputs(ids, dp_noise=dpn, noise_w=0.8)], "x_low predict T=14")
    assert "dp.affine_exp_ceil" in pdev.steps()
    report_line("x_low predict T=14", rows, ref_s)


# ------------------------------------------------------------------------------------------------ predicted durations
def test_predict_durations_vs_oracle(rt_xl, xl):
    cfg, blob = xl
    items = []
    for i, T in enumerate((14, 40, 5)):
        ids = np.random.RandomState(40 + i).randint(0, 130, size=T).tolist()
        items.append((ids, kd.sym(SD + 300 + i, (2, T), 1.7320508)))
    for (ids, nz), (d, lw) in zip(items, rt_xl.predict_durations(items, noise_w=0.8, length_scale=1.1)):
        enc, _ = orc.text_encoder(cfg, blob, ids)
        lw_ref = orc.duration_logw(cfg, blob, enc, nz, 0.8)
        err = np.abs(lw - lw_ref).max()
        print(f"x_low T={len(ids)}: max|Δ logw| = {err:.2e}")
        assert err <= LOGW_TOL, err
        d_ref = orc.durations_from_logw(lw_ref, 1.1)
        ok = ceil_safe(lw_ref, 1.1)
        assert ok.sum() >= ok.size - 2
        assert np.array_equal(d[ok], d_ref[ok]) and np.all(np.abs(d - d_ref) <= 1)


def test_bounded_prepare_equals_prepare(rt_xl, xl):
    """piper_hip_voice_prepare_batch_bounded (the frame count stays on the device) against prepare_batch with durations = NULL: same
    durations, same lengths, and with the bound in the same bucket the same samples bit for bit."""
    cfg, blob = xl
    ids_a, ids_b = np.random.RandomState(50).randint(0, 130, size=20).tolist(), np.random.RandomState(51).randint(0, 130, size=9).tolist()
    na, nb = kd.sym(SD + 310, (2, 20), 1.7320508), kd.sym(SD + 311, (2, 9), 1.7320508)
    prepare_predicted(rt_xl, 7, [(ids_a, na), (ids_b, nb)], 0.8)
    rt_xl.launch(7)
    two_step = rt_xl.collect(7).copy()
    dur = rt_xl.durations(7).copy()
    Fa, Fb = int(dur[:20].sum()), int(dur[20:].sum())
    info = rt_xl.plan_info(7)
    rt_xl.prepare_batch_bounded(8, [(ids_a, na), (ids_b, nb)], max(Fa, Fb), noise_mode="injected")
    assert rt_xl.plan_info(8)["bucket_f"] == info["bucket_f"]
    rt_xl.launch(8)
    audio = rt_xl.collect(8)
    assert rt_xl.prepared_samples(8)[0] == [Fa * 256, Fb * 256]
    assert np.array_equal(rt_xl.durations(8), dur)
    assert np.array_equal(audio, two_step)
    ref_a = orc.synthesize(cfg, blob, ids_a, dur[:20].tolist(), np.zeros((cfg.inter, Fa), np.float32), 0.667)
    assert_close(audio[:Fa * 256], ref_a, WAVE_TOL, "bounded prepare, item a vs oracle")


# ------------------------------------------------------------------------------------------------ serving paths
@pytest.fixture(scope="module")
def sessions(rt_xl, xl):
    """Three utterances (F = 19, 43, 27 or so) with their whole-utterance waveforms, computed once."""
    cfg, _ = xl
    out = {}
    for name, T in (("A", 14), ("B", 30), ("C", 20)):
        u = utterance(cfg, T, seed=3)
        whole = rt_xl.synthesize(*u, 0.667)
        whole.setflags(write=False)
        out[name] = (u, whole)
    return out


def test_stream_chunks_equal_whole(rt_xl, sessions):
    (ids, dur, noise), whole = sessions["B"]
    F = sum(dur)
    chunks = list(rt_xl.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=9))
    assert len(chunks) == -(-F // 8) and all(c.size == 8 * 256 for c in chunks[:-1])
    assert_close(np.concatenate(chunks), whole, STREAM_TOL, "x_low streamed (chunk 8) vs whole")


def test_pool_sessions_equal_their_single_streams(rt_xl, sessions):
    """A pool of 4 rows, chunk 8: A joins alone, B one step later, C two steps after that; each session's chunks against its own
    stream_begin / stream_next run and against the whole utterance."""
    pool = rt_xl.stream_pool(10, 4, chunkFrames=8, work_slot=11)
    got, row, want = {}, {}, {}

    def join(name):
        (item, samples), = pool.join([sessions[name][0]], 0.667)
        row[item], got[name], want[name] = name, [], samples

    def step():
        out = pool.step()
        for item, chunk in out.items():
            got[row[item]].append(chunk)
        return out
    join("A")
    assert sorted(step()) == [0]
    join("B")
    step()
    step()
    join("C")
    for _ in range(32):
        if not step():
            break
    else:
        raise AssertionError("the pool did not go idle")
    assert pool.free_rows == 4
    pool.close()
    for name, ((ids, dur, noise), whole) in sessions.items():
        audio = np.concatenate(got[name])
        assert audio.size == want[name] == whole.size
        single = np.concatenate(list(rt_xl.synthesize_stream(ids, dur, noise, 0.667, chunkFrames=8, slot=9)))
        assert_close(audio, single, STREAM_TOL, f"pool session {name} vs its single stream")
        assert_close(audio, whole, STREAM_TOL, f"pool session {name} vs whole")


def test_collect_pcm16_is_bit_equal(rt_xl, sessions):
    (ids, dur, noise), whole = sessions["C"]
    rt_xl.prepare(12, ids, dur, noise, 0.667)
    rt_xl.launch(12)
    f32 = rt_xl.collect(12).copy()
    assert np.array_equal(rt_xl.collect_pcm16(12), ph.pcm16(f32))
    assert np.array_equal(f32, whole)


# ------------------------------------------------------------------------------------------------ bf16 generator
def test_bf16_generator_snr(backend, xl):
    cfg, blob = xl
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        ids, dur, noise = utterance(cfg, 28, seed=5)
        fp32 = rt.synthesize(ids, dur, noise, 0.667)
        rt.set_precision("bf16")
        bf = rt.synthesize(ids, dur, noise, 0.667)
        s = snr_db(bf, fp32)
        print(f"x_low: bf16 generator SNR vs fp32 = {s:.1f} dB")
        assert s >= BF16_MIN_SNR_DB, s
        assert not np.array_equal(bf, fp32)
    finally:
        rt.close()


# ------------------------------------------------------------------------------------------------ preset 2 (low)
def test_low_voice_vs_oracle_and_wav_rate(backend, tmp_path):
    cfg = ph.voice_config("low")
    blob = ph.synthetic_blob(cfg, 1234)
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        ids, dur = kd.FIXTURE_IDS, [3] * 14
        noise = kd.sym(SD + 80, (cfg.inter, 42), 1.7320508)
        audio, taps = run_with_taps(rt, ids, dur, noise)
        ref_audio, ref_taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
        for k in TAPS:
            assert_close(taps[k], ref_taps[k], OP_TOL, f"low: {k}")
        assert_close(audio, ref_audio, WAVE_TOL, "low: audio")
        assert rt.cfg.sample_rate == 16000
        p = tmp_path / "low.wav"
        ph.wav_write(p, audio, rt.cfg.sample_rate)
        with wave.open(str(p), "rb") as w:
            assert w.getframerate() == 16000 and w.getnframes() == audio.size
    finally:
        rt.close()


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("d", [48, 96])
@pytest.mark.parametrize("T", [4, 132, 1040])
def test_rel_attention_op(d, T, backend):
    """piper_hip_rel_attention_f32 at head_dim 48 on the three routes (one key tile; two key tiles, key-split; register fragments above
    1024) and the same at 96: the old route still answers."""
    H, w = 2, 4
    q, k, v = (kd.sym(SD + 500 + j + 10 * T + d, (1, H * d, T)) for j in range(3))
    ek, ev = kd.sym(SD + 505 + d, (2 * w + 1, d), 0.1), kd.sym(SD + 506 + d, (2 * w + 1, d), 0.1)
    b = backend
    out, shp = b.relAttentionF32(*(b.uploadFloat32(a) for a in (q, k, v, ek, ev)), 1, H, d, T, w)
    got = b.downloadFloat32(out, int(np.prod(shp))).reshape(shp)
    assert_close(got, orc.rel_attention(q, k, v, ek, ev, H, d, T, w), OP_TOL, f"rel_attention d={d} T={T}")
    r = att_ref.floorless(got, att_ref.rel_attention(q, k, v, ek, ev, H, d, T, w))  # and without the floor, against float64
    assert r["ok"], f"d={d} T={T}: max|Δ| {r['err']:.3e} is {r['ratio']:.2f} × OP_TOL · ‖ref‖∞"
