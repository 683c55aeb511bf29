"""GPU: every unit of the bf16 generator against the rounding-exact reference (tests/bf16_ref.py), teacher-forced from the GPU's own taps.

The chain per item: z (checked against the oracle at OP_TOL) → conv_pre → per stage ConvTranspose, every ResBlock step, the bf16 image of
lrelu(MRF mean) → the last stage's fp32 mean → conv_post + tanh = the collected waveform. No link is skipped; a tensor a schedule never stores
(the last ResBlock's closing step where the mean is folded into its epilogue) is covered by the unit that consumes it (bf16_ref.mean_act /
mean_from_rb). Per unit the run prints max|Δ|, the bound, and the share of elements that carry / needed the flip allowance.

A tap is compacted to each item's true length, so "zero past the true length" is checked where it matters: the reference feeds zeros there, and
a stale image tail would show in the last `reach` columns of the consumer. The fp32 streams themselves are not zero past the true length by
design (nobody reads them there). Window plans of the streaming path are not attached to a slot id: tests/test_gpu_stream_windows.py
reaches them through the tap's "window:" selector and runs this chained check on every step of a stream; the streams keep their SNR checks
next to it (test_gpu_voice.py, test_gpu_stream_batch.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process of test_unfused_twin_in_a_child_process: no conftest has set the path up
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.join(os.path.dirname(_here), "piper-swift_amd", "python")]

import bf16_ref as br
import katdata as kd
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL, assert_close

pytestmark = pytest.mark.gpu
SD = kd.case_seed("cfg", 50)


def utterance(cfg, F, seed, T=None):
    """T ids with durations that sum to F frames (at least one id per 3 frames)."""
    T = T or max(1, -(-F // 3))
    rng = np.random.RandomState(seed)
    dur = np.full(T, F // T, np.int32)
    dur[:F - int(dur.sum())] += 1
    return list(rng.randint(1, 130, size=T)), list(int(d) for d in dur), kd.sym(SD + seed, (cfg.inter, F), 1.7320508)


def run_and_verify(rt, blob, slot, utts, label, items=None, check_z=True):
    cfg = rt.cfg
    if len(utts) == 1:
        rt.prepare(slot, *utts[0], 0.667)
    else:
        rt.prepare_batch(slot, utts, 0.667)
    rt.launch(slot)
    audio = rt.collect(slot).copy()
    frames = [int(np.sum(u[1])) for u in utts]
    if check_z:  # the first link: z against the fp32 oracle
        _, taps = orc.synthesize(cfg, blob, utts[0][0], utts[0][1], utts[0][2], 0.667, taps=True)
        z = rt.tap(slot, "z", cfg.inter * sum(frames))[:cfg.inter * frames[0]]
        assert_close(z, taps["z"].reshape(-1), OP_TOL, label + ": z vs oracle")
    return audio, br.verify_slot(rt, blob, slot, frames, audio, label, items)


@pytest.fixture(scope="module")
def rts(backend, voices):
    out = {}
    for q in ("medium", "high"):
        rt = ph.HipRuntime(backend, *voices[q])
        rt.set_precision("bf16")
        out[q] = rt
    yield out
    for rt in out.values():
        rt.close()


@pytest.mark.parametrize("quality,F", [("medium", 42), ("medium", 336), ("high", 42), ("high", 336)])
def test_merged_schedule_factor1_and_factor8(quality, F, rts, voices):
    run_and_verify(rts[quality], voices[quality][1], 0, [utterance(voices[quality][0], F, F)], f"{quality} F={F}")


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_per_conv_schedule_large_batch(quality, rts, voices):
    """NB · F = 20 × 84 > 1536: one launch per conv; the high voice with parallel graph branches and the mean folded into rb2's epilogue."""
    cfg, blob = voices[quality]
    utts = [utterance(cfg, 84, 100 + b, T=28) for b in range(20)]
    run_and_verify(rts[quality], blob, 1, utts, f"{quality} 20x84", items=(0, 7, 19))


@pytest.mark.parametrize("quality,F", [("medium", 2), ("medium", 129), ("medium", 131), ("high", 2), ("high", 129), ("high", 35)])
def test_lengths_off_the_tile_grid(quality, F, rts, voices):
    """F = 129 / 131: every stage is 1 / 3 frames' worth past a multiple of 128 (and off the 224 / 256-column tiles); F = 35: 35 · 64 = 2240 =
    10 × 224; F = 2: the zero halo is most of every window (K 11 · dilation 5 reaches 25 positions either side of a 16-position row)."""
    run_and_verify(rts[quality], voices[quality][1], 2, [utterance(voices[quality][0], F, 200 + F)], f"{quality} F={F}")


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_ragged_batch_every_item(quality, rts, voices):
    cfg, blob = voices[quality]
    utts = [utterance(cfg, F, 300 + F) for F in (84, 5, 61, 1)]
    run_and_verify(rts[quality], blob, 3, utts, f"{quality} ragged 84/5/61/1")


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_plan_reuse_with_a_shorter_utterance(quality, rts, voices):
    """The stale-tail case: the C8 images are zeroed once per build, so the second, shorter utterance on the same plan relies on every
    producer rewriting the tail past the new true length with zeros."""
    cfg, blob = voices[quality]
    rt = rts[quality]
    long_, short = utterance(cfg, 126, 400, T=40), utterance(cfg, 113, 401, T=40)  # one bucket: 40 ids, 128 frames
    run_and_verify(rt, blob, 4, [long_], f"{quality} long")
    bucket = rt.plan_info(4)["bucket_f"]
    audio, _ = run_and_verify(rt, blob, 4, [short], f"{quality} short after long")
    assert rt.plan_info(4)["bucket_f"] == bucket, "the shorter utterance must land on the same plan"
    fresh = ph.HipRuntime(rt.backend, cfg, blob)
    try:
        fresh.set_precision("bf16")
        fresh.prepare(0, *short, 0.667)
        fresh.launch(0)
        assert np.array_equal(fresh.collect(0), audio), "a reused plan must give what a fresh runtime gives"
    finally:
        fresh.close()


def test_unfused_twin_in_a_child_process():
    """PIPER_HIP_NO_RB_PAIR is read once per process: the two-launch ResBlock1 path (what 256-channel stages always take) at every stage."""
    env = dict(os.environ, PIPER_HIP_NO_RB_PAIR="1", PIPER_HIP_TUNING="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "child ok" in out.stdout


def _child():
    cfg = ph.voice_config("high")
    blob = ph.synthetic_blob(cfg, 1234)
    backend = ph.HipBackend(0)
    rt = ph.HipRuntime(backend, cfg, blob)
    try:
        rt.set_precision("bf16")
        rows = run_and_verify(rt, blob, 0, [utterance(cfg, 84, 500)], "high unfused F=84")[1]
        assert not any(n.endswith("rb2.c2") for n, _ in rows), "the unfused path folds the mean: rb2's closing step has no tensor"
    finally:
        rt.close()
        backend.close()
    print("child ok")


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
