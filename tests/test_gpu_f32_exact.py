"""GPU: every unit of the fp32 generator against a float64 reference (tests/f32_ref.py), teacher-forced from the GPU's own taps.

The chain per item: z (checked against the oracle at OP_TOL) → conv_pre → per stage: ConvTranspose of lrelu(input) (input = conv_pre output, or
the mean of the previous stage's three tapped ResBlock outputs, or the stored lrelu(mean) of the per-conv schedule) → every tapped ResBlock
step from the nearest tapped tensor upstream (a pair launch or an overwritten step is checked as the composition of its steps) → the
waveform. No link is skipped, every unit meets the plain rule |Δ| ≤ OP_TOL · max(1, ‖ref‖∞) — no allowance; the waveform is compared in front
of tanh's saturation (f32_ref.Waveform). Per unit the run prints max|Δ|, the bound and their ratio, per case one `F32EXACT {json}` line.

A tap is compacted to each item's true length; the reference feeds zeros past it. The fp32 streams are NOT zeroed there on the device, so
a kernel that forgets len_ptr shows in the last `reach` columns of its output — most of all on a reused plan after a longer utterance.
Window plans of the streaming path are not attached to a slot id: tests/test_gpu_stream_windows.py reaches them through the tap's "window:"
selector and runs this chained check on every step of a stream; the streams themselves stay pinned to the whole utterance at 2e-5
(test_gpu_voice.py, test_gpu_stream_batch.py).

Which kernel a launch takes follows from the builder (csrc/voice.hip) and launch_conv_win_multi (csrc/conv_win.hip). Where the step name or the
`flops` field of the profile tells, the cases assert it. A plan is built for the BUCKET of its longest item, Fb = ⌈F / 16⌉ · 16 (⌈F / 64⌉ · 64
above 1024 frames): the selection rules and the tile counts see Fb, the kernels mask by each item's true length. One utterance (NB = 1), 256 CUs:

  merged schedule     the three ResBlocks of a stage advance in one launch. NB · Fb < 128 (pair_min_f): conv by conv at every stage — up to
                      F = 112; F = 113 … 127 already land on the 128-frame plan. NB · Fb ≥ 128: the pair kernel on the 32- and 64-channel stages
                      (medium s1 s2, high s2 s3); the 128- / 256-channel stages stay conv by conv and move from the window kernel to
                      conv_pipe once the launch holds ≥ 5 GFLOP (pipe_min_flops): medium s0 from Fb = 1280, high s0 from 240, high s1 from 128.
  K-split of the window kernel: wanted KS = 1 for tiles ≥ 2048, 2 for tiles ≥ 1024, else 4 (tiles = MT · ⌈columns / 32⌉ · convs per launch),
  halved while a wave would keep fewer than 16 steps of the launch's shortest contraction (32 channels · K 3 = 48 steps: never 4); rows of
  ≥ 128 channels that want KS = 4 take the 8-wave block with KS = 2 instead ("2*"). KS by Fb (– = never taken):

    voice   stage  ConvTranspose: tiles   KS 4 / 2 / 1 from Fb =    three ResBlock convs: tiles   KS 4 / 2 / 1 from Fb =
    medium  s0     32 · ⌈Fb / 32⌉         16 / 993 / 2017           3 Fb                          – / 16 (2*), 352 / 688    conv_pipe from 1280
    medium  s1     4 Fb                   16 / 256 / 512            12 Fb                         16 / 96 / –               pair from 128
    medium  s2     8 Fb                   16 / 128 / 256            24 Fb                         – / 16 / 96               pair from 128
    high    s0     64 · ⌈Fb / 32⌉         16 / 481 / 993            6 Fb                          – / 16 (2*), 176 / –      conv_pipe from 240
    high    s1     8 Fb                   16 / 128 / 256            24 Fb                         – / 16 (2*), 48 / 96      conv_pipe from 128
    high    s2     8 Fb                   16 / 128 / 256            24 Fb                         16 / 48 / 96              pair from 128
    high    s3     8 Fb                   16 / 128 / 256            24 Fb                         – / 16 / 96               pair from 128

  The frame counts below reach, per stage kind, every KS it can take: F = 1 … 42 (KS 4, or 2 where 4 is never taken), F = 61 (Fb = 64: the
  24 Fb launches at 1536 tiles, KS 2), F = 112 (the 12 Fb and 24 Fb launches at KS 2 and 1, still conv by conv), F = 127 … 336 (ConvTranspose at
  KS 2 and 1 on the late stages), high F = 200 (s0's ResBlocks at 1248 tiles: plain KS 2, between the 8-wave block and conv_pipe), medium F = 400 and 700 (s0's
  ResBlocks at 1200 and 2112 tiles: KS 2, then KS 1) and medium F = 2688 (BASELINE configs[2]: every ConvTranspose at KS 1, s0 on conv_pipe).
  Not reached: stage 0's ConvTranspose at KS 2 (Fb 993 … 2016 on the medium voice, 481 … 992 on the high voice) and the high voice's at KS 1
  (Fb ≥ 993, 600 GFLOP of float64 reference per utterance); the same kernel instances run on the later stages' ConvTransposes.
  The float64 reference of medium F = 2688 takes well under two minutes (printed as ref_s), so every stage is checked on every column."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process of test_fallback_schedules_in_child_processes: no conftest has set the path up
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.join(os.path.dirname(_here), "piper-swift_amd", "python")]

import f32_ref as fr
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, assert_close

pytestmark = pytest.mark.gpu
PIPE_MIN_FLOPS = 5e9
PAIR_NAMES = {1: "ab_lrelu_conv_lrelu_conv_res_x3", 2: "_lrelu_conv_res_pair_x3"}


def run_and_verify(rt, blob, slot, utts, label, items=None):
    """prepare + launch + collect, z of every checked item against the oracle, then the chained check. → (audio, rows, tap names of item 0)."""
    cfg = rt.cfg
    if len(utts) == 1:
        rt.prepare(slot, *utts[0], fr.NOISE_SCALE)
    else:
        rt.prepare_batch(slot, utts, fr.NOISE_SCALE)
    rt.launch(slot)
    audio = rt.collect(slot).copy()
    frames = [int(np.sum(u[1])) for u in utts]
    items = list(range(len(utts))) if items is None else list(items)
    z = rt.tap(slot, "z", cfg.inter * sum(frames))
    offs = np.concatenate([[0], np.cumsum(frames)]) * cfg.inter
    for b in items:  # the first link: z against the fp32 oracle
        _, taps = orc.synthesize(cfg, blob, utts[b][0], utts[b][1], utts[b][2], fr.NOISE_SCALE, taps=True)
        assert_close(z[offs[b]:offs[b + 1]], taps["z"].reshape(-1), OP_TOL, f"{label}[{b}]: z vs oracle")
    rows, ref_s, names = fr.verify_slot(rt, blob, slot, frames, audio, label, items)
    shares = [r["floor_share"] for _, r in rows if "floor_share" in r]
    print("F32EXACT " + json.dumps(dict(case=label, frames=[frames[b] for b in items], worst={k: round(v, 5) for k, v in fr.worst_by_kind(rows).items()},
                                        floor_share=round(max(shares), 5), ref_s=round(ref_s, 2))))
    return audio, rows, names


def steps_of(rt, slot):
    """[(step name, algorithmic flops)] of the slot's schedule. Profiling replays the plan: call it after the taps have been read."""
    return [(s["name"], s["flops"]) for s in rt.profile(slot, iters=1) if not s["name"].startswith("(")]


def stage_channels(cfg, u):
    return cfg.up_initial >> (u + 1)


def rb_steps(steps, u):
    return [(n, f) for n, f in steps if n.startswith(f"dec.s{u}.rb")]


def assert_merged(cfg, steps, names, pair):
    """The merged schedule: `_x3` launches only; pair=True: the pair kernel on every 32- / 64-channel stage, conv by conv elsewhere."""
    last = cfg.rb_n_dil - 1
    for u in range(cfg.n_ups):
        st = rb_steps(steps, u)
        assert st and all(n.endswith("_x3") for n, _ in st), (u, st)
        paired = [n for n, _ in st if PAIR_NAMES[cfg.resblock_type] in n]
        want_pair = pair and stage_channels(cfg, u) in (32, 64)
        assert (len(paired) == len(st)) if want_pair else not paired, (u, pair, st)
        kept = {d for d in range(cfg.rb_n_dil) if f"dec.s{u}.rb0.c{d}" in names}
        assert kept == ({last} if want_pair and cfg.resblock_type == 2 else {d for d in range(cfg.rb_n_dil) if d + 2 > last}), (u, kept)
        assert f"dec.s{u}.mean_lrelu" not in names and f"dec.s{u}.up" in names
    assert any(n == "dec.mrfmean_conv_post_tanh" for n, _ in steps)


def pipe_launches(cfg, steps):
    """ResBlock launches that the builder hands to conv_pipe: conv by conv, ≥ 128 channels, ≥ 5 GFLOP in the launch."""
    return [n for u in range(cfg.n_ups) if stage_channels(cfg, u) >= 128
            for n, f in rb_steps(steps, u) if PAIR_NAMES[cfg.resblock_type] not in n and f >= PIPE_MIN_FLOPS]


@pytest.fixture(scope="module")
def rts(backend, voices):
    out = {q: ph.HipRuntime(backend, *voices[q]) for q in ("medium", "high")}
    yield out
    for rt in out.values():
        rt.close()


def single(rts, voices, quality, F, slot, seed=0):
    cfg, blob = voices[quality]
    rt = rts[quality]
    _, rows, names = run_and_verify(rt, blob, slot, [fr.utterance(cfg, F, seed + F)], f"{quality} F={F}")
    assert rt.plan_info(slot)["bucket_f"] == bucket_f(F)
    return cfg, rows, names, steps_of(rt, slot)


def bucket_f(F):
    return -(-F // 16) * 16 if F <= 1024 else -(-F // 64) * 64


@pytest.mark.parametrize("F", [42, 2, 112])
@pytest.mark.parametrize("quality", ["medium", "high"])
def test_merged_schedule_conv_by_conv(quality, F, rts, voices):
    """NB · Fb < 128 (pair_min_f): every ResBlock conv through launch_conv_win_multi, three per launch. F = 112 is the longest such plan
    (F = 127 runs in test_lengths_off_the_tile_grid: its bucket is 128, the shortest plan on the pair kernel)."""
    cfg, rows, names, steps = single(rts, voices, quality, F, 0)
    assert_merged(cfg, steps, names, pair=False)
    assert not pipe_launches(cfg, steps)
    assert ("rb_composed" in fr.worst_by_kind(rows)) == (cfg.rb_n_dil > 2)  # ResBlock1: c0 is overwritten by c2, c1 is checked as c0 ∘ c1


@pytest.mark.parametrize("F", [128, 336])
@pytest.mark.parametrize("quality", ["medium", "high"])
def test_merged_schedule_pair_kernel(quality, F, rts, voices):
    """The pair kernel on the 32- and 64-channel stages. High voice: its 256- / 128-channel stages run conv_pipe from F ≈ 230 / 115."""
    cfg, rows, names, steps = single(rts, voices, quality, F, 1)
    assert_merged(cfg, steps, names, pair=True)
    pipes = pipe_launches(cfg, steps)
    if quality == "high":
        assert any(n.startswith("dec.s1.") for n in pipes) and any(n.startswith("dec.s0.") for n in pipes) == (F == 336), pipes
    else:
        assert not pipes and "rb_step" not in {r["kind"] for n, r in rows if n.startswith(("dec.s1.", "dec.s2."))}


def test_chunk_pipelined_kernel_on_the_medium_voice(rts, voices):
    """BASELINE configs[2], once: 2688 frames = 688 128 samples. Stage 0 (128 channels) holds ≥ 5 GFLOP per launch from F ≈ 1 300."""
    cfg, rows, names, steps = single(rts, voices, "medium", 2688, 2)
    assert_merged(cfg, steps, names, pair=True)
    pipes = pipe_launches(cfg, steps)
    assert pipes and all(n.startswith("dec.s0.") for n in pipes), pipes


@pytest.mark.parametrize("quality,F", [("medium", 129), ("medium", 131), ("medium", 35), ("medium", 1), ("medium", 127),
                                       ("high", 129), ("high", 131), ("high", 35), ("high", 1), ("high", 127)])
def test_lengths_off_the_tile_grid(quality, F, rts, voices):
    """F = 129 / 131: every stage is 1 / 3 frames' worth past a multiple of 128 frames and off the 256-column tiles of the pair kernel, 15 / 13
    frames short of the plan's rows; F = 127: one frame short of the 128-frame plan; F = 35: 2240 = 8.75 tiles at the 64-columns-per-frame
    stage; F = 1: stage 0 is 8 columns long in a 128-column row — the window kernel's L % 4 limit is two steps away, and the zero halo is most
    of every window (K 11 · dilation 5 reaches 25 positions either side)."""
    cfg, rows, names, steps = single(rts, voices, quality, F, 3)
    assert_merged(cfg, steps, names, pair=bucket_f(F) >= 128)
    if quality == "high" and F >= 113:
        assert any(n.startswith("dec.s1.") for n in pipe_launches(cfg, steps))


@pytest.mark.parametrize("quality,F", [("medium", 61), ("high", 61), ("high", 200), ("medium", 400), ("medium", 700)])
def test_k_split_variants_of_the_window_kernel(quality, F, rts, voices):
    """The K-split table of the module docstring: F = 61 (Fb = 64) puts the 24 Fb launches at 1536 tiles; medium F = 400 / 700 put stage 0's
    ResBlock launches (3 Fb tiles, 128 channels, still below conv_pipe's 5 GFLOP) at 1200 / 2112 tiles, high F = 200 (Fb = 208) its
    stage 0's (6 Fb tiles, 256 channels) at 1248."""
    cfg, rows, names, steps = single(rts, voices, quality, F, 4)
    assert_merged(cfg, steps, names, pair=F >= 128)
    assert not [n for n in pipe_launches(cfg, steps) if not (quality == "high" and F == 200 and n.startswith("dec.s1."))]


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_ragged_batch_every_item(quality, rts, voices):
    cfg, blob = voices[quality]
    utts = [fr.utterance(cfg, F, 300 + F) for F in (84, 5, 61, 1)]
    _, rows, _ = run_and_verify(rts[quality], blob, 5, utts, f"{quality} ragged 84/5/61/1")
    assert sum(1 for n, _ in rows if n == "audio") == 4


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_batch_of_twenty(quality, rts, voices):
    """NB · F = 20 × 84: fp32 stays on the merged schedule at every size (merged_max = 1 << 40), with the pair kernel."""
    cfg, blob = voices[quality]
    rt = rts[quality]
    utts = [fr.utterance(cfg, 84, 100 + b, T=28) for b in range(20)]
    _, rows, names = run_and_verify(rt, blob, 6, utts, f"{quality} 20x84", items=(0, 7, 19))
    assert_merged(cfg, steps_of(rt, 6), names, pair=True)


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_plan_reuse_with_a_shorter_utterance(quality, rts, voices):
    """The stale-tail case: nothing zeroes the fp32 streams past the true length, so after a longer utterance on the same plan every kernel
    that reads past the new true length without masking by len_ptr convolves the previous utterance's tail in."""
    cfg, blob = voices[quality]
    rt = rts[quality]
    long_, short = fr.utterance(cfg, 126, 400, T=40), fr.utterance(cfg, 113, 401, T=40)  # one bucket: 40 ids, 128 frames
    run_and_verify(rt, blob, 7, [long_], f"{quality} long")
    bucket = rt.plan_info(7)["bucket_f"]
    audio, _, _ = run_and_verify(rt, blob, 7, [short], f"{quality} short after long")
    assert rt.plan_info(7)["bucket_f"] == bucket, "the shorter utterance must land on the same plan"
    fresh = ph.HipRuntime(rt.backend, cfg, blob)
    try:
        fresh.prepare(0, *short, fr.NOISE_SCALE)
        fresh.launch(0)
        assert np.array_equal(fresh.collect(0), audio), "a reused plan must give what a fresh runtime gives"
    finally:
        fresh.close()


@pytest.mark.parametrize("switch", ["PIPER_HIP_NO_MERGED_RB", "PIPER_HIP_NO_RB_PAIR", "PIPER_HIP_NO_WIN"])
def test_fallback_schedules_in_child_processes(switch):
    """The A/B switches are read once per process (and need PIPER_HIP_TUNING=1): one child per switch, high F = 84 and medium F = 336 in each.
    NO_MERGED_RB: the per-conv schedule — fork / join lanes, the mean folded into the last conv's epilogue, lrelu(mean) stored;
    NO_RB_PAIR: two launches per ResBlock1 step (one per ResBlock2 step) at every size; NO_WIN: the streaming MFMA kernels with the
    ConvTranspose epilogue, on the per-conv schedule."""
    env = dict(os.environ, PIPER_HIP_TUNING="1")
    env[switch] = "1"
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", switch], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{switch}: the child hung on the GPU; nothing more is started on it", returncode=3)
    print(out.stdout[-30000:])
    if out.returncode < 0 or out.returncode in (134, 139):  # died on a signal: a GPU fault or an abort — a finding, not a test to go on from
        pytest.exit(f"{switch}: the child died with status {out.returncode}; nothing more is started on the GPU\n" + out.stderr[-3000:], returncode=3)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "child ok" in out.stdout


def _child(switch):
    backend = ph.HipBackend(0)
    try:
        # medium F = 84 under NO_WIN: the regression case of the streaming kernel's ConvTranspose — a true length that is a multiple of its
        # 32-column tile and shorter than the plan's row (84 · 8 = 21 · 32 of 768) had its last `pad` outputs skipped (as high F = 84 has)
        for quality, F in (("high", 84), ("medium", 336)) + ((("medium", 84),) if switch == "PIPER_HIP_NO_WIN" else ()):
            cfg = ph.voice_config(quality)
            blob = ph.synthetic_blob(cfg, 1234)
            rt = ph.HipRuntime(backend, cfg, blob)
            try:
                _, rows, names = run_and_verify(rt, blob, 0, [fr.utterance(cfg, F, 500 + F)], f"{switch[10:]} {quality} F={F}")
                steps = steps_of(rt, 0)
                if switch == "PIPER_HIP_NO_RB_PAIR":
                    assert_merged(cfg, steps, names, pair=False)
                else:
                    last = cfg.rb_n_dil - 1
                    for u in range(cfg.n_ups):
                        st = [n for n, _ in rb_steps(steps, u)]
                        assert len(st) == 3 * cfg.rb_n_dil * (2 if cfg.resblock_type == 1 else 1) and not any(n.endswith("_x3") for n in st), st
                        assert sum(n.endswith("_mrfmean") for n in st) == 1 and st[-1].startswith(f"dec.s{u}.rb2.c{last}"), st
                        assert {f"dec.s{u}.fork", f"dec.s{u}.join"} <= {n for n, _ in steps}
                        assert f"dec.s{u}.mean_lrelu" in names and f"dec.s{u}.rb2.c{last}" not in names and f"dec.s{u}.rb1.c{last}" in names
                    assert sum(r["kind"] == "mean_lrelu" for _, r in rows) == cfg.n_ups
                    assert any(n == "dec.conv_post_tanh" for n, _ in steps)
            finally:
                rt.close()
    finally:
        backend.close()
    print("child ok")


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    _child(sys.argv[2])
