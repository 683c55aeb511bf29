"""CPU: the route-record parser, the production table's consistency, and the reach of the float64 conv reference at the tile-edge shapes
of tests/conv_route_cases.py — every planted tile-edge defect breaks |Δ| ≤ OP_TOL · max(1, ‖ref‖∞) there, and an fp32 evaluation of the
same sums in two accumulation orders stays below a tenth of it (as tests/test_f32_ref.py shows for the generator units)."""
import numpy as np
import pytest

import conv_ref as cr
import conv_route_cases as cc
import conv_route_plans as rp
import conv_routes_table as tb
import oracle as orc

REC = "stream K=3 TM=16 NT=1 KS=8 BT=512 gate=0 pro=none epi=store res=0 conv | Cout=256 Cin=192 Lout=17 N=1 CUs=256"


def test_record_parser_and_normaliser():
    v, shape = cr.parse_record(REC)
    assert v == "stream K=3 TM=16 NT=1 KS=8 BT=512 gate=0 pro=none epi=store res=0 conv"
    assert shape == dict(Cout=256, Cin=192, Lout=17, N=1, CUs=256)
    assert cr.family_of(v) == "stream"
    assert cr.params_of(v) == dict(K="3", TM="16", NT="1", KS="8", BT="512", gate="0", pro="none", epi="store", res="0", kind="conv")
    other = REC.replace("Lout=17", "Lout=4096").replace("N=1", "N=20")
    assert cr.variant_of(other) == v and cr.variants([REC, other]) == [v]  # the shape is dropped: one variant
    assert cr.variants([REC, REC.replace("KS=8 BT=512", "KS=4 BT=256")]) == sorted([v, v.replace("KS=8 BT=512", "KS=4 BT=256")])
    assert cr.params_of("win K=16 WM=4 WN=1 KS=1 multi=1 xcd=0 avg3=1 convT")["kind"] == "convT"
    assert cr.cus_of([REC, other]) == 256
    for bad in ("", "stream K=3", "stream K=3 | Cout=1", REC + " extra=1", REC.replace("Cin=192", "Cin=x"), " | Cout=1 Cin=1 Lout=1 N=1 CUs=1",
                REC.replace(" N=1", " N=1 N=2")):
        with pytest.raises(ValueError):
            cr.parse_record(bad)
    with pytest.raises(ValueError):
        cr.params_of("stream K=3 oops")
    with pytest.raises(AssertionError):
        cr.cus_of([REC, REC.replace("CUs=256", "CUs=304")])


def test_merge_keeps_variants_without_shapes():
    out = {}
    n = rp.merge(out, [("enc0.qkv", [REC]), ("gather", []), ("enc1.qkv", [REC.replace("Lout=17", "Lout=33")]), ("enc0.qkv", [REC])])
    assert n == 3 and out == {cr.variant_of(REC): ["enc0.qkv", "enc1.qkv"]}


def test_every_table_variant_has_exactly_one_witness():
    assert tb.NUM_CUS == 256
    assert set(tb.TABLE) == set(tb.WITNESS) == {rp.voice_key(*v) for v in rp.VOICES}
    for voice, uses in tb.TABLE.items():
        assert set(tb.WITNESS[voice]) == set(uses), voice  # a dict: one witness each; the share left out is zero
        for var, ws in uses.items():
            cr.params_of(var)  # well-formed
            assert ws and set(ws) <= set(rp.WORKLOADS), (voice, var, ws)
            w = tb.WITNESS[voice][var]
            if w[0] == "ladder":
                assert w[1] in rp.LADDER_F and w[2] in rp.LADDER_N, (voice, var, w)
            else:
                assert w[0] == "production" and w[1] in ws, (voice, var, w)  # marked as a production shape, and one that uses the variant


def test_reference_agrees_with_the_fp32_oracle():
    """Another implementation of the same ops (the C oracle, fp32) on cases with stride, groups, dilation, pads and output padding."""
    for i, c in enumerate(cc.CASES):
        if c["id"] not in ("direct_stride2_L17", "direct_depthwise", "small_cout3_cin33", "stream16_k5_d6_L33", "win_k3_p1", "convt_stream16_L15",
                           "convt_direct_groups2", "convt_direct_dil2"):
            continue
        x, w, b = cc.inputs(i)
        ref = cc.reference(i, x=x, w=w, b=b)
        if c["op"] == "conv":
            got = orc.conv1d(x, w, b, c["stride"], c["dil"], c["pl"], c["pr"], c["groups"])
        else:
            got = orc.convtranspose1d(x, w, b, c["stride"], c["dil"], c["pl"], c["pr"], c["out_pad"], c["groups"])
        assert got.shape == ref.shape, c["id"]
        assert cr.judge(got, ref)["ratio"] < 0.1, c["id"]
    x, w, b = cc.inputs(cc.IDS.index("rb_pair_t2_c32_L220"))
    c = cc.CASES[cc.IDS.index("rb_pair_t2_c32_L220")]
    assert cr.judge(orc.hifigan_resblock(2, x, c["K"], c["dils"], w, b, 0.1), cc.reference(cc.IDS.index("rb_pair_t2_c32_L220")))["ratio"] < 0.1


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=cc.IDS)
def test_planted_defects_break_the_bound_and_fp32_stays_inside(i):
    c = cc.CASES[i]
    x, w, b = cc.inputs(i)
    ref = cc.reference(i, x=x, w=w, b=b)
    bd = cr.bound(ref)
    assert cr.judge(ref, ref)["ok"]
    # fp32 in two accumulation orders (taps ascending / descending; the ResBlock composition has one order)
    orders = (None,) if c["op"] == "rb" else (None, list(range(c["K"]))[::-1])
    for taps in orders:
        r = cr.judge(cc.reference(i, np.float32, taps, x, w, b), ref)
        assert r["err"] <= 0.1 * bd, f"{c['id']}: fp32 ({'descending' if taps else 'ascending'} taps) is at {r['ratio']:.3f} of the bound"
    redo = None
    if c["op"] != "rb" and c["K"] > 1:
        # the centre tap: with "same" padding it reads real input at every column (an outer tap of a dilated conv may only ever see padding)
        redo = lambda: cc.reference(i, np.float64, [k for k in range(c["K"]) if k != c["K"] // 2], x, w, b)
    pad = c["pl"] if c["op"].startswith("convt") else 0
    planted = 0
    for d in cr.DEFECTS:
        bad = cr.plant(d, ref, c["col"], c["row"], redo, pad)
        if bad is None:
            continue
        planted += 1
        r = cr.judge(bad, ref)
        assert not r["ok"] and r["ratio"] > 5, f"{c['id']}: {d} stays at {r['ratio']:.2f} of the bound"
    assert planted >= (2 if c["op"] == "rb" or c["K"] == 1 else 3)
