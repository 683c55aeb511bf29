"""Multi-speaker voices, the host-only part (include/piper_hip.h "Multi-speaker voices"): the speaker blob against its numpy twin, the
argument refusals that need no device, and the opt-in loader route against files written by tests/onnx_writer.py — next to the old
entry points, which must refuse the same files exactly as before. CPU-only."""
import ctypes as C
import json

import numpy as np
import pytest

import onnx_writer as ow
import piper_hip as ph
import spk_ref as sr


def layout_dicts(cfg):
    return [dict(name=t["name"], offset=t["offset"], count=t["count"], shape=list(t["shape"])) for t in ph.blob_layout(cfg)]


@pytest.mark.parametrize("quality,S,gin,ctot", [("medium", 5, 512, 6592), ("high", 2, 512, 6848), ("x_low", 3, 36, 3424)])
def test_speaker_blob_layout_and_numpy_twin(quality, S, gin, ctot):
    cfg = ph.voice_config(quality)
    scfg = ph.speaker_config(S, gin)
    assert sr.row_floats(cfg) == ph.speaker_row_floats(cfg) == ctot
    lay = ph.speaker_blob_layout(cfg, scfg)
    ref = sr.layout(cfg, S, gin)
    assert [e["name"] for e in lay] == [r[0] for r in ref]
    off = 0
    for e, (_name, kind, shape, fan_in) in zip(lay, ref):
        assert e["kind"] == kind and tuple(e["shape"]) == tuple(shape) and e["fan_in"] == fan_in
        assert e["offset"] == off and e["count"] == int(np.prod(shape))
        off += e["count"]
    assert off == ph.speaker_blob_floats(cfg, scfg) == S * gin + ctot * (gin + 1)  # the table, then a cond row and a cond bias per speaker-row entry
    blob = ph.synthetic_speaker_blob(cfg, scfg, 4321)
    assert np.array_equal(blob, sr.synthetic_blob(cfg, S, gin, 4321))  # every tensor, bit for bit
    emb = blob[:S * gin]
    assert abs(float(emb.var()) - 1.0) < 0.15  # unit variance, like nn.Embedding: speakers differ by an amount a test can see
    # its own seed: not a prefix of the voice blob, and another seed is another table
    assert not np.array_equal(blob[:1000], ph.synthetic_blob(cfg, 4321)[:1000])
    assert not np.array_equal(blob, ph.synthetic_speaker_blob(cfg, scfg, 4322))
    # without the predictor there are no dp.cond tensors and no dp.pre rows
    cfg.dp_present = 0
    assert "dp.cond.weight" not in [e["name"] for e in ph.speaker_blob_layout(cfg, scfg)]
    assert ph.speaker_row_floats(cfg) == sr.row_floats(cfg) == ctot - cfg.hidden


def test_speaker_config_limits():
    cfg = ph.voice_config("medium")
    for S, gin in ((0, 512), (65537, 512), (5, 0), (5, 2), (5, 1028), (5, 510)):
        with pytest.raises(ph.ShapeMismatch):
            ph.speaker_blob_floats(cfg, ph.speaker_config(S, gin))
        with pytest.raises(ph.ShapeMismatch):
            ph.speaker_blob_layout(cfg, ph.speaker_config(S, gin))
    assert ph.speaker_blob_floats(cfg, ph.speaker_config(65536, 4)) > 0 and ph.speaker_blob_floats(cfg, ph.speaker_config(1, 1024)) > 0
    lib = ph.load_library()
    scfg = ph.speaker_config(5, 512)
    small = np.empty(16, np.float32)
    assert lib.piper_hip_speaker_synthetic_blob(C.byref(cfg), C.byref(scfg), 1, small.ctypes.data_as(ph.c_f32p), small.size) == ph.ShapeMismatch.code
    assert lib.piper_hip_speaker_synthetic_blob(C.byref(cfg), C.byref(scfg), 1, None, 0) == ph.InvalidArgument.code
    assert lib.piper_hip_speaker_blob_floats(C.byref(cfg), None, None) == ph.InvalidArgument.code
    bad = ph.voice_config("medium")
    bad.n_heads = 5
    with pytest.raises(ph.ShapeMismatch):  # the voice geometry is validated as by the voice twins
        ph.speaker_blob_floats(bad, scfg)


def test_null_voice_refusals():
    lib = ph.load_library()
    scfg = ph.speaker_config(5, 512)
    blob = np.zeros(8, np.float32)
    assert lib.piper_hip_voice_num_speakers(None) == 0
    assert lib.piper_hip_voice_attach_speakers(None, C.byref(scfg), blob.ctypes.data_as(ph.c_vp), 0) == ph.InvalidArgument.code
    assert lib.piper_hip_voice_slot_speakers(None, 0, None, 0) == ph.InvalidArgument.code
    dur = np.zeros(4, np.int32)
    assert lib.piper_hip_voice_predict_durations_speakers(None, None, 1, None, dur.ctypes.data_as(ph.c_i32p), None, 4) == ph.InvalidArgument.code


def test_speaker_record_shim():
    s = ph._speaker(3)
    assert (s.n, s.ids[0], s.weights[0]) == (1, 3, 1.0)
    s = ph._speaker({1: 0.25, 4: 0.75})
    assert s.n == 2 and list(s.ids[:2]) == [1, 4] and list(s.weights[:2]) == [0.25, 0.75]
    assert ph._speaker([(0, 1.0)] * 5).n == 5  # handed on for the library to refuse
    assert C.sizeof(ph.Speaker) == 36 and C.sizeof(ph.SpeakerConfig) == 8


WN = "flow.flows.2.enc.cond_layer.weight"  # the cond tensor the test file keeps as a weight_g / weight_v pair


def cond_inits(cfg, S, gin, sblob, weight_norm=(WN,), drop=()):
    """The speaker blob's tensors as onnx_writer extra_inits; those in `weight_norm` as g = ‖w‖ per row, v = 3·w."""
    out = []
    for name, data in sr.tensors(cfg, S, gin, sblob).items():
        if name in drop:
            continue
        if name in weight_norm:
            w = data.reshape(data.shape[0], -1).astype(np.float64)
            g = np.sqrt((w ** 2).sum(1)).astype(np.float32)
            out.append((name + "_g", [data.shape[0], 1, 1], g))
            out.append((name + "_v", list(data.shape), (3.0 * data).astype(np.float32)))
        else:
            out.append((name, list(data.shape), np.ascontiguousarray(data)))
    return out


@pytest.fixture(scope="module")
def spk_file(voices):
    cfg, blob = voices["medium"]
    S, gin = 5, 36
    sblob = ph.synthetic_speaker_blob(cfg, ph.speaker_config(S, gin), 99)
    data = ow.piper_voice_onnx(cfg, blob, layout_dicts(cfg), extra_inits=cond_inits(cfg, S, gin, sblob))
    return cfg, blob, S, gin, sblob, data


def test_loader_round_trip(spk_file, tmp_path):
    cfg, blob, S, gin, sblob, data = spk_file
    m = ph.OnnxModel(data=data)
    cfg2 = m.infer_config_speakers()
    for f in ("hidden", "inter", "n_flows", "wn_layers", "up_initial", "n_ups", "dp_present", "n_vocab", "resblock_type"):
        assert getattr(cfg2, f) == getattr(cfg, f), f
    scfg = m.speaker_config(cfg2)
    assert (scfg.n_speakers, scfg.gin) == (S, gin)
    got = m.build_speaker_blob(cfg2, scfg)
    off = 0
    for name, _kind, shape, _f in sr.layout(cfg, S, gin):
        n = int(np.prod(shape))
        if name == WN:  # folded: w = g · v / ‖v‖ in the loader's arithmetic
            np.testing.assert_allclose(got[off:off + n], sblob[off:off + n], rtol=2e-6, atol=1e-9)
            assert not np.array_equal(got[off:off + n], 3.0 * sblob[off:off + n])
        else:
            assert np.array_equal(got[off:off + n], sblob[off:off + n]), name
        off += n
    assert np.array_equal(m.build_blob(cfg2, verify=False), blob)  # the main blob of such a file: build_blob_unchecked
    lib = ph.load_library()
    short = np.empty(got.size - 1, np.float32)
    assert lib.piper_hip_onnx_build_speaker_blob(m.h, C.byref(cfg2), C.byref(scfg), short.ctypes.data_as(ph.c_f32p), short.size) == ph.ShapeMismatch.code
    # the json check of the opt-in route wants the table's row count
    for said, ok in ((S, True), (904, False), (1, False)):
        info = ph.piper_json(json.dumps({"audio": {"sample_rate": 22050}, "num_symbols": 256, "num_speakers": said}))
        rc = lib.piper_hip_voice_check_json_speakers(C.byref(cfg2), C.byref(scfg), C.byref(info))
        assert rc == (0 if ok else ph.ShapeMismatch.code), said
    info = ph.piper_json(json.dumps({"audio": {"sample_rate": 22050}, "num_symbols": 130, "num_speakers": S}))
    assert lib.piper_hip_voice_check_json_speakers(C.byref(cfg2), C.byref(scfg), C.byref(info)) == ph.ShapeMismatch.code
    m.close()
    # … and through load_voice
    path = tmp_path / "multi.onnx"
    path.write_bytes(data)
    (tmp_path / "multi.onnx.json").write_text(json.dumps({"audio": {"sample_rate": 16000}, "num_symbols": 256, "num_speakers": S}))
    c3, b3, info3, s3, sb3 = ph.load_voice(path, speakers=True)
    assert (s3.n_speakers, s3.gin, c3.sample_rate, info3.num_speakers) == (S, gin, 16000, S)
    assert np.array_equal(b3, blob) and np.array_equal(sb3, got)
    (tmp_path / "multi.onnx.json").write_text(json.dumps({"audio": {"sample_rate": 16000}, "num_symbols": 256, "num_speakers": S + 1}))
    with pytest.raises(ph.ShapeMismatch):
        ph.load_voice(path, speakers=True)


def test_old_entry_points_still_refuse(spk_file, voices, tmp_path):
    cfg, blob, S, gin, sblob, data = spk_file
    m = ph.OnnxModel(data=data)
    with pytest.raises(ph.UnsupportedOp) as e:
        m.infer_config()
    assert "multi-speaker" in str(e.value)
    m.close()
    path = tmp_path / "multi.onnx"
    path.write_bytes(data)
    with pytest.raises(ph.UnsupportedOp):
        ph.load_voice(path)
    with pytest.raises(ph.UnsupportedOp):
        ph.load_voice(path, verify=False)
    # a json that says many speakers over a file without a table: check_json refuses as it did, with or without speakers=True
    lay = layout_dicts(cfg)
    single = tmp_path / "single.onnx"
    single.write_bytes(ow.piper_voice_onnx(cfg, blob, lay))
    (tmp_path / "single.onnx.json").write_text(json.dumps({"audio": {"sample_rate": 22050}, "num_symbols": 256, "num_speakers": 904}))
    with pytest.raises(ph.UnsupportedOp):
        ph.load_voice(single)
    with pytest.raises(ph.UnsupportedOp):
        ph.load_voice(single, speakers=True)
    info = ph.piper_json(json.dumps({"audio": {"sample_rate": 22050}, "num_symbols": 256, "num_speakers": 2}))
    assert ph.load_library().piper_hip_voice_check_json(C.byref(cfg), C.byref(info)) == ph.UnsupportedOp.code
    # a file without a table through the opt-in route: no speakers, and then everything as before
    (tmp_path / "single.onnx.json").write_text(json.dumps({"audio": {"sample_rate": 22050}, "num_symbols": 256, "num_speakers": 1}))
    c2, b2, _info, s2, sb2 = ph.load_voice(single, speakers=True)
    assert s2.n_speakers == 0 and s2.gin == 0 and sb2 is None and np.array_equal(b2, blob)
    # the graph verifier keeps refusing a graph with a `sid` input; build_blob (= verify, then fill) with it
    m = ph.OnnxModel(data=ow.piper_voice_onnx(cfg, blob, lay, inputs=("input", "input_lengths", "scales", "sid"),
                                              extra_inits=cond_inits(cfg, S, gin, sblob)))
    c4 = m.infer_config_speakers()
    with pytest.raises(ph.UnsupportedOp):
        m.verify_graph(c4)
    with pytest.raises(ph.UnsupportedOp):
        m.build_blob(c4)
    m.close()


def test_speaker_config_names_the_missing_or_misshapen_tensor(voices):
    cfg, blob = voices["medium"]
    S, gin = 5, 36
    sblob = ph.synthetic_speaker_blob(cfg, ph.speaker_config(S, gin), 99)
    lay = layout_dicts(cfg)
    m = ph.OnnxModel(data=ow.piper_voice_onnx(cfg, blob, lay, extra_inits=cond_inits(cfg, S, gin, sblob, drop=("dec.cond.bias",))))
    with pytest.raises(ph.ShapeMismatch) as e:
        m.speaker_config(m.infer_config_speakers())
    assert "dec.cond.bias" in str(e.value)
    m.close()
    inits = [(n, d, a) if n != "dp.cond.weight" else (n, [cfg.hidden, gin // 2, 2], a) for n, d, a in cond_inits(cfg, S, gin, sblob)]
    m = ph.OnnxModel(data=ow.piper_voice_onnx(cfg, blob, lay, extra_inits=inits))
    with pytest.raises(ph.ShapeMismatch) as e:
        m.speaker_config(m.infer_config_speakers())
    assert "dp.cond.weight" in str(e.value)
    m.close()
    m = ph.OnnxModel(data=ow.piper_voice_onnx(cfg, blob, lay, extra_inits=[("emb_g.weight", [4, 6], np.zeros((4, 6), np.float32))]))
    with pytest.raises(ph.ShapeMismatch) as e:  # gin must be a multiple of 4
        m.speaker_config(m.infer_config_speakers())
    assert "emb_g.weight" in str(e.value)
    m.close()
