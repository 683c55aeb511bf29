"""CPU: the 16 kHz tier — presets 2 (low: the medium geometry at 16 000 Hz) and 3 (x_low: hidden 96, inter 96, ffn 384, two heads of
head_dim 48, the medium generator) — through the preset, the blob layout, the synthetic generator, the ONNX loader and the oracle.

The oracle has never run at 96 channels, so before the GPU tests lean on it (tests/test_gpu_low_voices.py) it is itself checked
against the torch restatement (tests/torch_ref.py) on one tiny x_low utterance."""
import ctypes as C
import json
import wave

import numpy as np
import pytest

import katdata as kd
import onnx_writer as ow
import oracle as orc
import piper_hip as ph

SCALARS = ["n_vocab", "hidden", "n_heads", "n_layers", "ffn", "ffn_kernel", "window", "inter", "n_flows", "wn_layers", "wn_kernel",
           "up_initial", "n_ups", "resblock_type", "n_rb", "rb_n_dil", "sample_rate", "dp_present", "dp_kernel", "dp_dds_layers",
           "dp_n_flows", "dp_bins", "dp_tail_bound"]


def fields(cfg):
    out = {f: getattr(cfg, f) for f in SCALARS}
    out["ups"] = [(cfg.up_rates[u], cfg.up_kernels[u]) for u in range(cfg.n_ups)]
    out["rb"] = [(cfg.rb_kernels[j], [cfg.rb_dilations[j][d] for d in range(cfg.rb_n_dil)]) for j in range(cfg.n_rb)]
    return out


def layout_dicts(cfg):
    return [dict(name=t["name"], offset=t["offset"], count=t["count"], shape=list(t["shape"])) for t in ph.blob_layout(cfg)]


def numpy_blob(cfg, seed):
    """The synthetic voice restated with katdata's generator: tensor i of the layout is seeded with tensor_seed(seed, i)."""
    out = np.empty(ph.blob_floats(cfg), np.float32)
    for i, e in enumerate(ph.blob_layout(cfg)):
        s, n = kd.tensor_seed(seed, i), e["count"]
        if e["kind"] in (0, 4):
            v = kd.sym(s, (n,), np.float32(np.sqrt(3.0 / e["fan_in"])))
        elif e["kind"] == 1:
            v = kd.sym(s, (n,), np.float32(0.01 * np.sqrt(3.0)))
        elif e["kind"] == 2:
            v = np.float32(1.0) + kd.sym(s, (n,), np.float32(0.1))
        else:
            v = kd.sym(s, (n,), np.float32(0.1))
        out[e["offset"]:e["offset"] + n] = v
    return out


def test_preset_fields():
    lib = ph.load_library()
    medium = fields(ph.voice_config("medium"))
    by_number = {}
    for q in (2, 3):
        cfg = ph.VoiceConfig()
        ph._check(lib.piper_hip_voice_config_preset(q, C.byref(cfg)))
        by_number[q] = fields(cfg)
    low, x_low = fields(ph.voice_config("low")), fields(ph.voice_config("x_low"))
    assert by_number == {2: low, 3: x_low}
    assert low == dict(medium, sample_rate=16000)
    assert x_low == dict(medium, sample_rate=16000, hidden=96, inter=96, ffn=384)
    assert (x_low["n_heads"], x_low["hidden"] // x_low["n_heads"], x_low["up_initial"], x_low["resblock_type"]) == (2, 48, 256, 2)
    assert ph.voice_config("x_low").hop == ph.voice_config("low").hop == 256
    for bad in (4, 7, -1):
        with pytest.raises(ph.InvalidArgument):
            ph._check(lib.piper_hip_voice_config_preset(bad, C.byref(ph.VoiceConfig())))
    with pytest.raises(KeyError):
        ph.voice_config("x-low")


def test_blob_floats_and_layout():
    low, x_low = ph.voice_config("low"), ph.voice_config("x_low")
    assert ph.blob_floats(low) == ph.blob_floats(ph.voice_config("medium")) == 15650459
    lay = ph.blob_layout(x_low)
    off = 0
    for e in lay:
        assert e["offset"] == off and e["count"] == int(np.prod(e["shape"]))
        off += e["count"]
    assert off == ph.blob_floats(x_low)
    by_name = {e["name"]: e["shape"] for e in lay}
    assert by_name["enc_p.emb.weight"] == [256, 96]
    assert by_name["enc_p.encoder.attn_layers.0.conv_q.weight"] == [96, 96, 1]
    assert by_name["enc_p.encoder.attn_layers.0.emb_rel_k"][-2:] == [9, 48]
    assert by_name["enc_p.encoder.ffn_layers.0.conv_1.weight"] == [384, 96, 3]
    assert by_name["enc_p.encoder.ffn_layers.0.conv_2.weight"] == [96, 384, 3]
    assert by_name["enc_p.proj.weight"] == [192, 96, 1]
    assert by_name["flow.flows.0.pre.weight"] == [96, 48, 1]
    assert by_name["flow.flows.0.post.weight"] == [48, 96, 1]
    assert by_name["dec.conv_pre.weight"] == [256, 96, 7]
    assert by_name["dp.pre.weight"] == [96, 96, 1]
    # the generator behind conv_pre is the medium one, tensor for tensor
    med = {e["name"]: e["shape"] for e in ph.blob_layout(ph.voice_config("medium"))}
    gen = [n for n in med if n.startswith("dec.") and n != "dec.conv_pre.weight"]
    assert len(gen) > 40 and all(by_name[n] == med[n] for n in gen)


@pytest.mark.parametrize("quality", ["low", "x_low"])
def test_synthetic_blob_equals_the_numpy_generator(quality):
    cfg = ph.voice_config(quality)
    assert np.array_equal(ph.synthetic_blob(cfg, 1234), numpy_blob(cfg, 1234))


def test_x_low_onnx_roundtrip_and_sample_rate_from_json(tmp_path):
    cfg = ph.voice_config("x_low")
    blob = ph.synthetic_blob(cfg, 1234)
    path = tmp_path / "x_low.onnx"
    path.write_bytes(ow.piper_voice_onnx(cfg, blob, layout_dicts(cfg)))
    m = ph.OnnxModel(path)
    got = m.infer_config()
    # the sample rate is not in the graph (it lives in the .onnx.json): everything else is the preset
    assert fields(got) == dict(fields(cfg), sample_rate=22050)
    m.verify_graph(got)
    m.verify_graph(cfg)
    assert np.array_equal(m.build_blob(cfg), blob)
    m.close()
    (tmp_path / "x_low.onnx.json").write_text(json.dumps({
        "audio": {"sample_rate": 16000, "quality": "x_low"}, "espeak": {"voice": "en-gb"},
        "inference": {"noise_scale": 0.667, "length_scale": 1.0, "noise_w": 0.8}, "num_symbols": 256, "num_speakers": 1}))
    cfg2, blob2, info = ph.load_voice(path)
    assert fields(cfg2) == fields(cfg) and cfg2.sample_rate == info.sample_rate == 16000
    assert np.array_equal(blob2, blob)
    wav = tmp_path / "x.wav"
    ph.wav_write(wav, np.zeros(160, np.float32), cfg2.sample_rate)
    with wave.open(str(wav), "rb") as w:
        assert w.getframerate() == 16000 and w.getnframes() == 160


def test_low_onnx_is_the_medium_graph(tmp_path):
    cfg = ph.voice_config("low")
    blob = ph.synthetic_blob(cfg, 1234)
    assert np.array_equal(blob, ph.synthetic_blob(ph.voice_config("medium"), 1234))
    m = ph.OnnxModel(data=ow.piper_voice_onnx(cfg, blob, layout_dicts(cfg)))
    assert fields(m.infer_config()) == dict(fields(cfg), sample_rate=22050)
    m.verify_graph(cfg)
    m.close()


def test_graph_verifier_tells_x_low_from_medium():
    """An x_low graph is not accepted as a medium voice, nor the other way round: the verifier's channel counts come from cfg."""
    xl, med = ph.voice_config("x_low"), ph.voice_config("medium")
    m = ph.OnnxModel(data=ow.piper_voice_onnx(xl, ph.synthetic_blob(xl, 7), layout_dicts(xl)))
    with pytest.raises(ph.ExecutionError):
        m.verify_graph(med)
    m.close()


def test_oracle_at_x_low_matches_torch_ref():
    """5 ids, 2 frames each: the C oracle against the torch restatement at hidden 96 / head_dim 48, at the bounds
    tests/test_hf_crosscheck.py applies to the medium voice (1e-4 on the taps, 1e-3 on the waveform)."""
    torch = pytest.importorskip("torch")
    import torch_ref
    torch.set_num_threads(4)
    cfg = ph.voice_config("x_low")
    blob = ph.synthetic_blob(cfg, 1234)
    ids, dur = [1, 20, 0, 120, 2], [2] * 5
    noise = kd.sym(4712, (cfg.inter, 10), 1.7320508)
    with torch.no_grad():
        r = torch_ref.Ref(cfg, blob).synthesize(ids, dur, noise, 0.667)
    audio, taps = orc.synthesize(cfg, blob, ids, dur, noise, 0.667, taps=True)
    assert taps["enc_out"].size == 96 * 5 and taps["z"].size == 96 * 10 and audio.size == 10 * 256
    for k in ("enc_out", "z_p", "z"):
        np.testing.assert_allclose(taps[k].reshape(-1), r[k].numpy().reshape(-1), atol=1e-4, rtol=0)
    np.testing.assert_allclose(audio, r["audio"].numpy(), atol=1e-3, rtol=0)


@pytest.mark.parametrize("schedule", ["default", "seam_stats", "plain", "predict"])
def test_front_ref_runs_at_x_low(schedule):
    """tests/front_ref.py takes the geometry as data: its float64 formulas against an honest fp32 stand-in at hidden 96 / head_dim 48, on
    every schedule the GPU test may meet (the teacher-forced GPU check of the x_low steps leans on it)."""
    import front_ref as fr
    cfg = ph.voice_config("x_low")
    blob = ph.synthetic_blob(cfg, 1234)
    ids, dur, noise = fr.utterance(cfg, 5, 11, 11)
    inp = fr.Inputs(ids, dur, noise, dp_noise=fr.dp_noise(5, 3))
    names = dict(default=fr.default_steps(cfg), seam_stats=fr.default_steps(cfg, fold=False, ln="stats"),
                 plain=fr.default_steps(cfg, fold=False, ln="plain"), predict=fr.default_steps(cfg, predict=True))[schedule]
    dev = fr.SimDevice(cfg, fr.FrontRef(cfg, blob, np.float32, reverse=True), names, [inp])
    rows, _ = fr.verify(dev, cfg, blob, [inp], f"x_low {schedule}", report=lambda *_: None)
    assert {r[0] for r in rows} == set(names) and all(r[4]["ok"] for r in rows)
