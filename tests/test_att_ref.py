"""CPU: tests/att_ref.py proves itself and its cases before tests/test_gpu_attention.py relies on them.

  * the reference equals front_ref.FrontRef.attention in float64 (a synthetic medium voice's layer-0 tables, whole and with a true
    length) and the C oracle at OP_TOL on small T;
  * for the inputs of EVERY op-level GPU case: the same formulas in fp32 numpy stay at or below FP32_SHARE of the floorless bound, and every
    applicable planted defect — one query row of one head — is at least DEFECT_FACTOR times beyond it. Both are conditions on the case
    list: a case that misses one gets other inputs, the factors stay. Above 2048 rows only att_ref.check_rows are evaluated (the norm of
    the bound is then the norm over those rows);
  * the same for ragged items (true lengths 1030 in 1040 and 2050 in 2064, the lengths of the voice-plan cases), where one key past the
    length can be planted;
  * route_of over the GPU cases reaches all six routes, every part count a 256-CU device can produce, both scalar strip heights; eight
    parts need 456 CUs, which is asserted from the rule;
  * front_ref.verify(att_floorless=True) catches at the attention step what the floor lets through."""
import json

import numpy as np
import pytest

import att_ref as ar
import front_ref as fr
import katdata as kd
import oracle as orc
from conftest import OP_TOL, assert_close

FP32_SHARE = 0.1
DEFECT_FACTOR = 5.0
ALL_CASES = ar.GPU_CASES + ar.FORCED_PARTS_CASES


def test_equals_front_ref_attention(voices):
    cfg, blob = voices["medium"]
    R = fr.FrontRef(cfg, blob)
    H, nh, w = cfg.hidden, cfg.n_heads, cfg.window
    d = H // nh
    ek, ev = (R.W(f"enc_p.encoder.attn_layers.0.emb_rel_{x}").reshape(-1, d) for x in "kv")
    for T, L in ((50, None), (1, None), (48, 37), (16, 1)):
        qkv = kd.sym(ar.SD + T, (3 * H, T))
        ref = R.attention(qkv, 0, length=L)
        got = ar.rel_attention(qkv[None, :H], qkv[None, H:2 * H], qkv[None, 2 * H:], ek, ev, nh, d, T, w, lengths=None if L is None else [L])[0]
        n = T if L is None else L
        assert np.abs(got[:, :n] - ref[:, :n]).max() < 1e-13, (T, L)
        assert not got[:, n:].any()


@pytest.mark.parametrize("d,T,w,H", [(96, 1, 4, 2), (96, 14, 4, 2), (48, 40, 4, 2), (96, 130, 4, 2), (32, 33, 2, 3), (96, 20, 8, 1)])
def test_matches_the_oracle(d, T, w, H):
    q, k, v, ek, ev = ar.inputs("diffuse", d, T, w, H, 1)
    ref = ar.rel_attention(q, k, v, ek, ev, H, d, T, w)
    assert_close(orc.rel_attention(q, k, v, ek, ev, H, d, T, w), ref, OP_TOL, f"oracle vs float64 d={d} T={T}")


def test_row_subsets_and_batches_equal_the_whole():
    d, T, w, H, N = 48, 70, 4, 2, 3
    q, k, v, ek, ev = ar.inputs("peaked", d, T, w, H, N)
    lens = [70, 33, 1]
    whole = ar.rel_attention(q, k, v, ek, ev, H, d, T, w, lengths=lens)
    rows = np.array([0, 1, 32, 33, 69])
    sub = ar.rel_attention(q, k, v, ek, ev, H, d, T, w, lengths=lens, rows=rows)
    assert sub.shape == (N, H * d, 5) and np.abs(sub - whole[:, :, rows]).max() < 1e-13  # (the matrix products block by shape)
    for n in range(N):  # an item of a batch = the item alone, cut to its length
        L = lens[n]
        alone = ar.rel_attention(q[n:n + 1, :, :L], k[n:n + 1, :, :L], v[n:n + 1, :, :L], ek, ev, H, d, L, w)
        assert np.abs(alone[0] - whole[n][:, :L]).max() < 1e-13 and not whole[n][:, L:].any()
    f32 = ar.rel_attention(q, k, v, ek, ev, H, d, T, w, lengths=lens, dt=np.float32)
    assert f32.dtype == np.float32 and ar.floorless(f32, whole, lens)["ok"] and not np.array_equal(f32, whole.astype(np.float32))


def test_floorless_rule():
    ref = np.zeros((2, 4, 8))
    ref[0, 1, 2], ref[1, 0, 0] = 0.05, 2.0
    got = ref.copy()
    got[0, 3, 3] = 4e-6  # within 1e-4 · 0.05
    assert ar.floorless(got, ref)["ok"]
    got[0, 3, 3] = 6e-6  # beyond it, though far inside the rule with the floor (1e-4) and inside item 1's own bound (2e-4)
    r = ar.floorless(got, ref)
    assert not r["ok"] and r["item"] == 0 and abs(r["ratio"] - 1.2) < 1e-9
    got[0, 3, 3] = 0.0
    got[1, 2, 7] = np.nan
    assert not ar.floorless(got, ref)["ok"]
    assert ar.floorless(got, ref, lengths=[8, 7])["ok"]  # rows past the length are not compared


def conditions(c, lengths=None):
    """→ (fp32 ratio, {defect: ratio}) of one case over att_ref.check_rows."""
    d, T, w, H, N, kind = (c[x] for x in ("d", "T", "w", "H", "N", "kind"))
    L = T if lengths is None else lengths[0]
    x = ar.inputs(kind, d, T, w, H, N)
    rows = ar.check_rows(T, L)
    ref = ar.rel_attention(*x, H, d, T, w, lengths=lengths, rows=rows)
    lens_r = None if lengths is None else [int((rows < l).sum()) for l in lengths]
    f32 = ar.floorless(ar.rel_attention(*x, H, d, T, w, lengths=lengths, rows=rows, dt=np.float32), ref, lens_r)["ratio"]
    out = {}
    x0 = (x[0][:1], x[1][:1], x[2][:1], x[3], x[4])  # the defect sits in the last head of item 0
    len0 = None if lengths is None else lengths[:1]
    bound = OP_TOL * float(np.abs(ref[0][:, :rows.size if lens_r is None else lens_r[0]]).max())
    hs = slice((H - 1) * d, H * d)
    for name in ar.DEFECTS:
        if ar.applicable(name, T, L, kind):
            i = ar.logit_defect_row(name, x[0][0, hs], x[1][0, hs], x[3], w, L, rows) if name in ar.LOGIT_DEFECTS else ar.defect_row(L)
            one = np.array([i])
            ref_i = ar.rel_attention(*x0, H, d, T, w, lengths=len0, rows=one)
            bad = ar.rel_attention(*x0, H, d, T, w, lengths=len0, rows=one, defect=(name, 0, H - 1, i))
            assert np.array_equal(bad[:, :(H - 1) * d], ref_i[:, :(H - 1) * d])  # confined to its head
            out[name] = float(np.abs(bad - ref_i).max() / bound)
    return f32, out


@pytest.mark.parametrize("c", ALL_CASES, ids=ar.case_id)
def test_case_conditions(c):
    f32, defects = conditions(c)
    print("ATTCOND " + json.dumps(dict(case=ar.case_id(c), fp32=round(f32, 5), defects={k: round(v, 1) for k, v in defects.items()})))
    assert f32 <= FP32_SHARE, f"fp32 numpy at {f32:.3f} of the floorless bound"
    assert "rel_value_tap_lost" in defects or c["kind"] == "peaked"
    for name, ratio in defects.items():
        assert ratio >= DEFECT_FACTOR, f"{name}: only {ratio:.2f} × the bound"


@pytest.mark.parametrize("d", [48, 96])
@pytest.mark.parametrize("T,L", [(1040, 1030), (2064, 2050), (2064, 97), (656, 129)])
def test_ragged_conditions(d, T, L):
    """The lengths of the voice-plan cases, on diffuse inputs: every defect applies, one key past the length among them."""
    c = dict(d=d, T=T, w=4, H=2, N=2, kind="diffuse")
    f32, defects = conditions(c, lengths=[L, T])
    print("ATTCOND " + json.dumps(dict(case=ar.case_id(c) + f"-len{L}", fp32=round(f32, 5), defects={k: round(v, 1) for k, v in defects.items()})))
    assert f32 <= FP32_SHARE
    assert set(defects) == set(ar.DEFECTS)
    assert min(defects.values()) >= DEFECT_FACTOR, defects


def test_routes_reached():
    got = {}
    for c in ar.GPU_CASES:
        got.setdefault(ar.route_of(c["d"], c["T"], c["w"], c["H"], c["N"]), []).append(c)
    routes = {r for r, _ in got}
    assert routes == set(ar.ROUTES), routes
    assert {p for r, p in got if r == "lds_split"} == {2, 3, 4, 5, 6}
    for d in (48, 96):  # each MFMA route at both head dims
        for r in ("lds", "lds_split", "mfma16", "mfma8"):
            assert any(c["d"] == d for (rr, _), cs in got.items() if rr == r for c in cs), (d, r)
    # the part count shrinks as the grid grows: T = 260, three items
    assert ar.route_of(96, 260, 4, 1, 3) == ("lds_split", 3) and ar.route_of(96, 260, 4, 3, 3) == ("lds", 1)
    # window 8 and the head dims without an MFMA instantiation go to the scalar kernel; its strip height by grid size and by T
    assert ar.route_of(96, 300, 8, 2, 1) == ("scalar4", 1) and ar.route_of(96, 300, 7, 2, 1)[0] == "lds_split"
    for d, w in ((32, 4), (64, 4), (80, 4), (96, 8)):
        assert [ar.route_of(d, T, w, 2, 1)[0] for T in (1, 7, 128, 129, 300, 1100, 2100)] == ["scalar4"] * 5 + ["scalar8", "scalar4"]
    assert ar.route_of(80, 1100, 4, 2, 1, num_cus=304)[0] == "scalar4"
    # what the edges of the T list are there for
    assert [ar.route_of(96, T, 4, 2, 1)[0] for T in (3, 4, 5, 128, 129, 132, 1024, 1025, 2048, 2049, 4096)] == \
        ["mfma16", "lds", "mfma16", "lds", "mfma16", "lds_split", "lds_split", "mfma16", "mfma16", "mfma8", "mfma8"]
    with pytest.raises(ValueError):
        ar.route_of(96, 4097, 4, 2, 1)


def test_eight_parts_need_more_cus_than_256():
    """min(⌈T/128⌉, CUs // (⌈T/16⌉·H·N)) = 8 needs eight key tiles, T ≥ 897, hence ⌈T/16⌉ ≥ 57 blocks even for one head of one item:
    8 · 57 = 456 CUs. On 256 the rule stops at 6 parts; the 8-part launch is run through PIPER_HIP_ATT_SPLIT=8 (FORCED_PARTS_CASES)."""
    assert ar.max_parts(256) == (6, 644)
    assert ar.split_parts(96, 656, 4, 1, 1) == 6 and ar.split_parts(96, 640, 4, 1, 1) == 5 and ar.split_parts(96, 512, 4, 1, 1) == 4
    assert max(ar.split_parts(96, T, 4, 1, 1, 455) for T in range(132, 1025, 4)) == 7
    assert ar.split_parts(96, 900, 4, 1, 1, 456) == 8 and ar.max_parts(456)[0] == 8
    for c in ar.FORCED_PARTS_CASES:  # launch_rel_attention_split accepts the forced count
        assert ar.FORCED_PARTS <= -(-c["T"] // 128) and c["T"] % 4 == 0 and c["T"] <= 1024 and c["d"] in (48, 96)


def test_verify_keyword_catches_what_the_floor_lets_through(voices):
    import piper_hip as ph
    cfg, blob = voices["medium"]
    step = "enc2.rel_attention"
    blob = np.array(blob, np.float32)  # a voice whose layer-2 values are small, as the attention output of a long row is
    for e in ph.blob_layout(cfg):
        if e["name"].startswith("enc_p.encoder.attn_layers.2.") and ("conv_v" in e["name"] or "emb_rel_v" in e["name"]):
            blob[e["offset"]:e["offset"] + e["count"]] *= np.float32(0.05)
    ids, dur, noise = fr.utterance(cfg, 14, 14, 5)
    inp = fr.Inputs(ids, dur, noise)
    names = fr.default_steps(cfg)
    R32 = fr.FrontRef(cfg, blob, np.float32, reverse=True)
    seen = {}

    def defect(name, R_, b, i_, out):
        if name == step:
            att = np.array(out["front.att"], np.float32)
            seen["norm"] = float(np.abs(att).max())
            att[3, 7] += np.float32(0.5 * OP_TOL)
            return {"front.att": att}

    dev = fr.SimDevice(cfg, R32, names, [inp], defect)
    assert seen["norm"] < 0.4  # so that half of OP_TOL lies between the two bounds
    rows, _ = fr.verify(dev, cfg, blob, [inp], "floor", report=lambda *_: None)
    assert all("floorless" not in r[4] for r in rows)
    with pytest.raises(fr.UnitMismatch) as e:
        fr.verify(dev, cfg, blob, [inp], "no floor", report=lambda *_: None, att_floorless=True)
    assert e.value.step == step and e.value.result["ratio"] < 1 < e.value.result["floorless"]
    clean = fr.SimDevice(cfg, R32, names, [inp])
    rows, _ = fr.verify(clean, cfg, blob, [inp], "clean", report=lambda *_: None, att_floorless=True)
    att = [r[4] for r in rows if r[3] == "rel_attention"]
    assert len(att) == cfg.n_layers and all(0 < r["floorless"] <= FP32_SHARE for r in att)
    assert "rel_attention (no floor)" in fr.worst_by_kind(rows)
