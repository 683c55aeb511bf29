"""Speaker conditioning (include/piper_hip.h "Multi-speaker voices") in numpy: the speaker blob's layout and synthetic generator (the
twin of piper_hip_speaker_synthetic_blob), the float64 reference of the speaker rows with its a-priori bound, and the FOLD — an item's
speaker row written into the biases of a copy of the voice blob, which makes a plain single-speaker voice that must synthesise what
the conditioned run synthesises, bit for bit."""
import numpy as np

import katdata as kd


def dp_rows(cfg):
    return cfg.hidden if cfg.dp_present else 0


def row_floats(cfg):
    """Ctot"""
    return dp_rows(cfg) + cfg.n_flows * cfg.wn_layers * 2 * cfg.hidden + cfg.up_initial


def layout(cfg, n_speakers, gin):
    """[(name, kind, shape, fan_in)] in blob order; kind 0 weight, 1 bias, 4 embedding."""
    H = cfg.hidden
    out = [("emb_g.weight", 4, (n_speakers, gin), 1)]

    def conv(prefix, cout):
        out.append((prefix + ".weight", 0, (cout, gin, 1), gin))
        out.append((prefix + ".bias", 1, (cout,), 0))
    if cfg.dp_present:
        conv("dp.cond", H)
    for f in range(cfg.n_flows):
        conv(f"flow.flows.{2 * f}.enc.cond_layer", 2 * H * cfg.wn_layers)
    conv("dec.cond", cfg.up_initial)
    return out


def synthetic_blob(cfg, n_speakers, gin, seed):
    """The SplitMix64 rule of katdata, tensor i of the speaker blob with index i: weights U(±√(3/fan_in)), biases U(±0.01·√3)."""
    parts = []
    for i, (_name, kind, shape, fan_in) in enumerate(layout(cfg, n_speakers, gin)):
        s = kd.tensor_seed(seed, i)
        if kind == 1:
            parts.append(kd.sym(s, shape, np.float32(0.01 * np.sqrt(3.0))).reshape(-1))
        else:
            parts.append(kd.weight(s, shape, fan_in).reshape(-1))
    return np.concatenate(parts)


def tensors(cfg, n_speakers, gin, blob):
    out, off = {}, 0
    for name, _kind, shape, _f in layout(cfg, n_speakers, gin):
        n = int(np.prod(shape))
        out[name] = blob[off:off + n].reshape(shape)
        off += n
    assert off == blob.size
    return out


def conditioned_biases(cfg):
    """The voice blob's bias tensors in speaker-row order: [(name, rows)]."""
    H = cfg.hidden
    out = [("dp.pre.bias", H)] if cfg.dp_present else []
    for f in range(cfg.n_flows):
        for l in range(cfg.wn_layers):
            out.append((f"flow.flows.{2 * f}.enc.in_layers.{l}.bias", 2 * H))
    out.append(("dec.conv_pre.bias", cfg.up_initial))
    return out


def row_tables(cfg, n_speakers, gin, sblob, voice_layout, voice_blob):
    """W [Ctot, gin], bc [Ctot], b [Ctot] in speaker-row order (float32, as stored)."""
    t = tensors(cfg, n_speakers, gin, sblob)
    names = (["dp.cond"] if cfg.dp_present else []) + [f"flow.flows.{2 * f}.enc.cond_layer" for f in range(cfg.n_flows)] + ["dec.cond"]
    W = np.concatenate([t[n + ".weight"].reshape(-1, gin) for n in names])
    bc = np.concatenate([t[n + ".bias"] for n in names])
    by = {e["name"]: e for e in voice_layout}
    b = np.concatenate([voice_blob[by[n]["offset"]:by[n]["offset"] + by[n]["count"]] for n, _ in conditioned_biases(cfg)])
    assert W.shape == (row_floats(cfg), gin) and bc.shape == b.shape == (row_floats(cfg),)
    return t["emb_g.weight"], W, bc, b


def mix_f32(emb, mix):
    """g as the contract states it: fp32, from 0.0f, ascending k, product rounded, then the sum."""
    g = np.zeros(emb.shape[1], np.float32)
    for i, w in mix:
        g = (g + (np.float32(w) * emb[i]).astype(np.float32)).astype(np.float32)
    return g


def reference(emb, W, bc, b, mix):
    """float64 (g, e) and the bound of the issue, per element:
    |e − ref| ≤ (gin + 8) · 2⁻²⁴ · (|b| + |bc| + Σ_j |W_cj| · Σ_k |w_k · emb_jk|)."""
    gin = emb.shape[1]
    g = np.zeros(gin, np.float64)
    ga = np.zeros(gin, np.float64)
    for i, w in mix:
        g += np.float64(np.float32(w)) * emb[i].astype(np.float64)
        ga += np.abs(np.float64(np.float32(w)) * emb[i].astype(np.float64))
    W64 = W.astype(np.float64)
    e = b.astype(np.float64) + (bc.astype(np.float64) + W64 @ g)
    bound = (gin + 8) * 2.0 ** -24 * (np.abs(b).astype(np.float64) + np.abs(bc).astype(np.float64) + np.abs(W64) @ ga)
    return g, e, bound


def fold(cfg, voice_layout, voice_blob, row):
    """A copy of the voice blob whose dp.pre / in_layers / dec.conv_pre biases ARE the speaker row `row` [Ctot]: the plain voice that
    the conditioned run must equal (the consumers add one float per channel where they add their bias)."""
    out = voice_blob.copy()
    by = {e["name"]: e for e in voice_layout}
    off = 0
    for name, rows in conditioned_biases(cfg):
        e = by[name]
        assert e["count"] == rows
        out[e["offset"]:e["offset"] + rows] = row[off:off + rows]
        off += rows
    assert off == row.size == row_floats(cfg)
    return out
