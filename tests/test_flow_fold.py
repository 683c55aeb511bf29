"""CPU: the fold of a flow coupling's linear tail, stated in numpy (what fold_flow_tail in csrc/flow_fold.hip multiplies out).

Behind the last gated conv of a coupling's WaveNet the reverse flow is linear up to the next coupling's first gated conv:
    skip = skip_acc + W_rs·acts + b_rs ;  m = W_post·skip + b_post ;  x1new = x1 − m ;  Flip ;  h' = W_pre'·x0' + b_pre'
With A1 = W_post·W_rs, c1 = W_post·b_rs + b_post and P = W_pre' with its columns reversed (the Flip):
    x1new = x1 − (A1·acts + W_post·skip_acc + c1)
    h'    = P·x1 − (P·A1)·acts − (P·W_post)·skip_acc + (b_pre' − P·c1)
(1) in float64 the folded and the unfolded flow agree to rounding; (2) with the folded matrices rounded ONCE to fp32 and fp32
arithmetic, z stays within the project's op-level rule |Δ| ≤ OP_TOL·max(1, ‖ref‖∞) of the C oracle."""
import numpy as np
import pytest

import katdata as kd
import oracle as orc
import piper_hip as ph
from conftest import OP_TOL

F = 53  # frames: odd, not a multiple of anything the kernels tile by


def weights(cfg, blob, dtype):
    lay = {t["name"]: t for t in ph.blob_layout(cfg)}

    def get(name):
        t = lay[name]
        return blob[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]).astype(dtype)

    out = []
    for f in range(cfg.n_flows):
        p = f"flow.flows.{2 * f}."
        out.append(dict(
            pre_w=get(p + "pre.weight")[:, :, 0], pre_b=get(p + "pre.bias"), post_w=get(p + "post.weight")[:, :, 0], post_b=get(p + "post.bias"),
            in_w=[get(p + f"enc.in_layers.{i}.weight") for i in range(cfg.wn_layers)], in_b=[get(p + f"enc.in_layers.{i}.bias") for i in range(cfg.wn_layers)],
            rs_w=[get(p + f"enc.res_skip_layers.{i}.weight")[:, :, 0] for i in range(cfg.wn_layers)],
            rs_b=[get(p + f"enc.res_skip_layers.{i}.bias") for i in range(cfg.wn_layers)]))
    return out


def gated(h, w, b):
    """acts = tanh(a)·sigmoid(b) of the 'same'-padded conv [2H, H, K] (dilation 1), in h's dtype."""
    H, K = h.shape[0], w.shape[2]
    pad = (K - 1) // 2
    hp = np.pad(h, ((0, 0), (pad, pad)))
    a = b[:, None] + sum(w[:, :, k] @ hp[:, k:k + h.shape[1]] for k in range(K))
    one = a.dtype.type(1)
    return np.tanh(a[:H]) * (one / (one + np.exp(-a[H:])))


def wavenet_head(h, W, n_layers):
    """Everything up to the last gated conv: (acts of the last layer, skip sum of the layers before it)."""
    H = h.shape[0]
    skip = np.zeros_like(h)
    for i in range(n_layers - 1):
        rs = W["rs_w"][i] @ gated(h, W["in_w"][i], W["in_b"][i]) + W["rs_b"][i][:, None]
        h = h + rs[:H]
        skip = skip + rs[H:]
    return gated(h, W["in_w"][n_layers - 1], W["in_b"][n_layers - 1]), skip


def flow_unfolded(cfg, Ws, zp):
    x = zp
    half = cfg.inter // 2
    for f in range(cfg.n_flows - 1, -1, -1):
        W = Ws[f]
        x = x[::-1]
        x0, x1 = x[:half], x[half:]
        acts, skip = wavenet_head(W["pre_w"] @ x0 + W["pre_b"][:, None], W, cfg.wn_layers)
        skip = skip + W["rs_w"][-1] @ acts + W["rs_b"][-1][:, None]
        x = np.concatenate([x0, x1 - (W["post_w"] @ skip + W["post_b"][:, None])])
    return x


def fold(cfg, Ws64, dtype):
    """Per coupling f: the matrices of its tail, formed in float64 and rounded once to `dtype`."""
    out = []
    for f in range(cfg.n_flows):
        W = Ws64[f]
        A1 = W["post_w"] @ W["rs_w"][-1]
        c1 = W["post_w"] @ W["rs_b"][-1] + W["post_b"]
        d = dict(A1=A1, Wpost=W["post_w"], c1=c1)
        if f > 0:
            P = Ws64[f - 1]["pre_w"][:, ::-1]
            d.update(P=P, PA1=P @ A1, PW=P @ W["post_w"], ch=Ws64[f - 1]["pre_b"] - P @ c1)
        out.append({k: v.astype(dtype) for k, v in d.items()})
    return out


def flow_folded(cfg, Ws, folded, zp):
    half = cfg.inter // 2
    x = zp[::-1]
    h = Ws[cfg.n_flows - 1]["pre_w"] @ x[:half] + Ws[cfg.n_flows - 1]["pre_b"][:, None]
    for f in range(cfg.n_flows - 1, -1, -1):
        G = folded[f]
        x0, x1 = x[:half], x[half:]
        acts, skip_acc = wavenet_head(h, Ws[f], cfg.wn_layers)
        x1new = x1 - (G["c1"][:, None] + G["A1"] @ acts + G["Wpost"] @ skip_acc)
        if f > 0:
            h = G["ch"][:, None] + G["P"] @ x1 - G["PW"] @ skip_acc - G["PA1"] @ acts
        x = np.concatenate([x0, x1new])
        if f > 0:
            x = x[::-1]
    return x


@pytest.mark.parametrize("quality", ["medium", "high"])
def test_fold_equals_the_flow(quality, voices, capsys):
    cfg, blob = voices[quality]
    assert cfg.wn_layers >= 2
    zp = kd.sym(kd.case_seed("mod", 0) + 7100, (cfg.inter, F), 1.7320508)
    W64 = weights(cfg, blob, np.float64)
    # (1) float64: the same function
    z_ref64 = flow_unfolded(cfg, W64, zp.astype(np.float64))
    z_fold64 = flow_folded(cfg, W64, fold(cfg, W64, np.float64), zp.astype(np.float64))
    scale = max(1.0, float(np.max(np.abs(z_ref64))))
    assert np.max(np.abs(z_fold64 - z_ref64)) <= 1e-11 * scale
    # (2) fp32 matrices (rounded once) and fp32 arithmetic against the C oracle
    z32 = flow_folded(cfg, weights(cfg, blob, np.float32), fold(cfg, W64, np.float32), zp)
    assert z32.dtype == np.float32
    ref = orc.flow_reverse(cfg, blob, zp)
    bound = OP_TOL * max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(z32 - ref)))
    err_unfolded = float(np.max(np.abs(flow_unfolded(cfg, weights(cfg, blob, np.float32), zp) - ref)))
    with capsys.disabled():
        print(f"\nflow fold, {quality}: max|dz| / bound = {err / bound:.4f} (folded, fp32), {err_unfolded / bound:.4f} (unfolded numpy fp32); bound {bound:.3e}")
    assert err <= bound, f"{quality}: max|Δ|={err:.3e} > {bound:.3e}"
