"""float64 reference of the relative-position attention core (csrc/attention.hip), its inputs, its bound, planted defects and the dispatch
rule restated — TEST INFRASTRUCTURE (numpy on the CPU).

  scores[i][j] = (q_i/√d)·k_j + (q_i/√d)·E_k[j−i+w]   (second term only for |j−i| ≤ w),   p = softmax_j over the REAL keys j < len,
  out_i = Σ_j p[i][j]·v_j + Σ_{|δ|≤w} p[i][i+δ]·E_v[δ+w]                                  rows i ≥ len are not compared.

THE RULE.  |Δ| ≤ OP_TOL · ‖ref‖∞ per batch item — the project's op-level OP_TOL (conftest) with the `max(1, ·)` floor REMOVED. An attention
output is a softmax-weighted mean of v, so it shrinks as the row grows: with inputs in ±1, ‖ref‖∞ is 0.2 at T = 144 and 0.035 at T = 4096.
The floor turns the project's rule into an absolute 1e-4 there, 0.3 % of the signal, and a defect confined to one query row (a skew off by
one, one relative-value tap lost) stays below it. Without the floor the bound is relative to what the op produces; an fp32 evaluation of the
same formulas in numpy stays below a tenth of it on every case of this file (tests/test_att_ref.py asserts that, and that every planted
defect is at least five times beyond it), so a correct kernel pays nothing for the tighter rule.

INPUTS (katdata.sym).  `diffuse`: q, k, v and both tables in ±1 — the logits have standard deviation ⅓, every key carries weight, so a lost,
extra or misplaced key shows. `peaked`: q, k and the key table times √12 — logits of standard deviation ≈ 4, a few keys carry the row, so a
wrong logit (skew, relative-key term) shows large. Mask and coverage defects are judged on diffuse inputs, logit defects on both.

`route_of` restates launch_rel_attention / launch_rel_attention_split / rel_attention_split_parts for the op-level entry point
(piper_hip_rel_attention_f32: contiguous, 16-byte aligned, no true lengths); tests/test_att_ref.py asserts which routes GPU_CASES reach."""
import numpy as np

import katdata as kd
from conftest import OP_TOL

SD = kd.case_seed("mod", 0) + 31000
SQRT12 = np.float32(np.sqrt(12.0))
ROW_CHUNK = 512  # query rows per evaluation block: a [512, 4096] float64 score strip is 16 MiB

# ------------------------------------------------------------------------------------------------ planted defects
# Each alters ONE query row of one head of one item:
DEFECTS = (
    "skew_off_by_one",      # the row reads relative-key logit m + 1 where it should read m
    "rel_value_tap_lost",   # the centre relative-value tap (δ = 0: j = i) is dropped
    "rel_key_logit_lost",   # the centre relative-key logit is dropped
    "last_key_lost",        # key len − 1 is not part of the softmax
    "key_past_length",      # key len is part of the softmax (ragged items only)
    "tile_neighbour_key",   # the first key (and value) of the last 16-key tile comes from the tile in front of it
)
LOGIT_DEFECTS = ("skew_off_by_one", "rel_key_logit_lost")


def defect_row(L):
    """The row a defect is planted into: the middle of the item, whose window lies on real keys wherever the item is longer than it."""
    return L // 2


def logit_defect_row(defect, q, k, ek, w, L, rows):
    """The row of `rows` a LOGIT defect is planted into: a wrong logit moves the output only through keys that carry weight without carrying
    the whole row, so the row is the one with the largest Σ_j p_ij (1 − p_ij) |Δs_ij| — the first-order change of the softmax for the
    logit changes Δs the defect makes. Chosen from the float64 reference of one head (q, k [d, T], ek [2w + 1, d]), never from the
    defective output."""
    d = q.shape[0]
    rows = np.asarray(rows, np.int64)
    rows = rows[rows < L]
    q, k, ek = (np.asarray(a, np.float64) for a in (q, k, ek))
    qs = (q[:, rows] / np.sqrt(np.float64(d))).T
    s = qs @ k[:, :L]
    rel = qs @ ek.T
    j = rows[:, None] + np.arange(-w, w + 1)[None, :]
    ok = (j >= 0) & (j < L)
    rr = np.broadcast_to(np.arange(rows.size)[:, None], j.shape)
    s[rr[ok], j[ok]] += rel[ok]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    pw = np.where(ok, p[rr, np.clip(j, 0, L - 1)], 0.0)
    if defect == "skew_off_by_one":
        ds = np.concatenate([rel[:, 1:], np.zeros((rows.size, 1))], 1) - rel
    else:
        ds = np.zeros_like(rel)
        ds[:, w] = rel[:, w]
    return int(rows[np.argmax((pw * (1 - pw) * np.abs(ds)).sum(-1))])


def applicable(defect, T, L, kind):
    """Can the defect change the output at all? One key: the softmax is 1 whatever the logits. Peaked inputs judge the logit defects only
    (a single key may carry no weight there by construction)."""
    if kind == "peaked" and defect not in LOGIT_DEFECTS:
        return False
    if defect in ("skew_off_by_one", "rel_key_logit_lost", "last_key_lost"):
        return L >= 2
    if defect == "key_past_length":
        return L < T
    if defect == "tile_neighbour_key":
        return L >= 17
    return True


def _defect_row(q, k, v, ek, ev, w, L, i, defect):
    """float64 [d] of row i of one head with `defect` planted; q, k, v [d, T], tables [2w + 1, d]."""
    d = q.shape[0]
    W = 2 * w + 1
    nk = L - 1 if defect == "last_key_lost" else L + 1 if defect == "key_past_length" else L
    kk, vv = k[:, :nk].copy(), v[:, :nk].copy()
    if defect == "tile_neighbour_key":
        j0 = 16 * ((L - 1) // 16)
        kk[:, j0], vv[:, j0] = k[:, j0 - 16], v[:, j0 - 16]
    qs = q[:, i] / np.sqrt(np.float64(d))
    s = qs @ kk
    rel = ek @ qs
    for m in range(W):
        j = i + m - w
        mm = m + 1 if defect == "skew_off_by_one" else m
        if 0 <= j < nk and mm < W and not (defect == "rel_key_logit_lost" and m == w):
            s[j] += rel[mm]
    p = np.exp(s - s.max())
    p /= p.sum()
    out = vv @ p
    for m in range(W):
        j = i + m - w
        if 0 <= j < nk and not (defect == "rel_value_tap_lost" and m == w):
            out += p[j] * ev[m]
    return out


# ------------------------------------------------------------------------------------------------ the reference
def _head(q, k, v, ek, ev, w, L, rows, dt):
    """[d, len(rows)] of one head: q, k, v [d, T] and the tables [2w + 1, d] in dt; keys < L."""
    d = q.shape[0]
    out = np.zeros((d, rows.size), dt)
    K, Vt = k[:, :L], np.ascontiguousarray(v[:, :L].T)
    scale = dt(np.sqrt(dt(d)))
    off = np.arange(-w, w + 1)
    for c0 in range(0, rows.size, ROW_CHUNK):
        r = rows[c0:c0 + ROW_CHUNK]
        qs = (q[:, r] / scale).T                       # [R, d]
        s = qs @ K                                     # [R, L]
        rel = qs @ ek.T                                # [R, 2w + 1]
        j = r[:, None] + off[None, :]
        ok = (j >= 0) & (j < L)
        rr = np.broadcast_to(np.arange(r.size)[:, None], j.shape)[ok]
        s[rr, j[ok]] += rel[ok]                        # rel→abs skew as an index; every (row, key) pair occurs once
        s -= s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        pw = np.zeros(j.shape, dt)
        pw[ok] = p[rr, j[ok]]                          # abs→rel skew
        out[:, c0:c0 + r.size] = (p @ Vt + pw @ ev).T
    return out


def rel_attention(q, k, v, ek, ev, H, d, T, w, lengths=None, rows=None, dt=np.float64, defect=None):
    """q, k, v [N, H·d, T], ek, ev [2w + 1, d] → [N, H·d, T] (rows=None) or [N, H·d, len(rows)] for the query rows `rows` (ascending).
    lengths[n]: keys at and past it are excluded and rows at and past it are left zero (they are not compared).
    dt=np.float32: the same formulas in fp32 through numpy (another summation order than any kernel's) — how far honest fp32 sits inside
    the bound. defect=(name, item, head, row): that row of the float64 result replaced by its planted-defect variant."""
    q, k, v = (np.asarray(a, dt).reshape(-1, H, d, T) for a in (q, k, v))
    ek, ev = (np.asarray(a, dt).reshape(2 * w + 1, d) for a in (ek, ev))
    N = q.shape[0]
    rows = np.arange(T) if rows is None else np.asarray(rows, np.int64)
    out = np.zeros((N, H, d, rows.size), dt)
    for n in range(N):
        L = T if lengths is None else int(lengths[n])
        live = rows < L
        for h in range(H):
            out[n, h][:, live] = _head(q[n, h], k[n, h], v[n, h], ek, ev, w, L, rows[live], dt)
            if defect is not None and (defect[1], defect[2]) == (n, h):
                assert dt == np.float64 and defect[0] in DEFECTS
                at = np.nonzero(rows == defect[3])[0]
                assert at.size == 1 and defect[3] < L, "the defect's row must be one of the evaluated, real rows"
                out[n, h][:, at[0]] = _defect_row(q[n, h], k[n, h], v[n, h], ek, ev, w, L, defect[3], defect[0])
    return out.reshape(N, H * d, rows.size)


def floorless(got, ref, lengths=None):
    """|Δ| ≤ OP_TOL · ‖ref‖∞ per batch item over its real rows. → dict(ok, ratio (worst item), err, bound, item)."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    worst = dict(ok=True, ratio=0.0, err=0.0, bound=0.0, item=0)
    for n in range(ref.shape[0]):
        L = ref.shape[-1] if lengths is None else int(lengths[n])
        r, g = ref[n][..., :L], got[n][..., :L]
        if not r.size:
            continue
        bound = OP_TOL * float(np.max(np.abs(r)))
        dlt = np.abs(g - r)
        err = float(np.where(np.isfinite(dlt), dlt, np.inf).max())  # NaN counts as beyond
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
        if not err <= bound:
            worst["ok"] = False
        if ratio >= worst["ratio"]:
            worst.update(ratio=ratio, err=err, bound=bound, item=n)
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def inputs(kind, d, T, w, H, N, seed=0):
    """(q, k, v, ek, ev) in float32: q, k, v [N, H·d, T], tables [2w + 1, d]."""
    assert kind in ("diffuse", "peaked")
    sd = SD + seed + 13 * T + 100003 * d + 1009 * w + 101 * H + 7 * N + (50021 if kind == "peaked" else 0)
    q, k, v = (kd.sym(sd + j, (N, H * d, T)) for j in range(3))
    ek, ev = kd.sym(sd + 5, (2 * w + 1, d)), kd.sym(sd + 6, (2 * w + 1, d))
    if kind == "peaked":
        q, k, ek = q * SQRT12, k * SQRT12, ek * SQRT12
    return q, k, v, ek, ev


# ------------------------------------------------------------------------------------------------ the dispatch rule
ROUTES = ("lds", "lds_split", "mfma16", "mfma8", "scalar4", "scalar8")
LDS_LIMIT = 160 * 1024


def split_parts(d, T, w, H, N, num_cus=256):
    """rel_attention_split_parts: as many key parts as keep the grid within one block per CU, at most one per 128-key tile, at most 8."""
    if d not in (48, 96) or T < 129 or T > 1024 or T % 4 or 2 * w + 1 > 16:
        return 1
    ntile = -(-T // 128)
    blocks = -(-T // 16) * H * N
    return max(1, min(ntile, num_cus // max(1, blocks), 8))


def route_of(d, T, w, H, N, num_cus=256):
    """(route, key parts) piper_hip_rel_attention_f32 takes for contiguous [N, H·d, T] inputs. The scalar routes are named by their strip
    height R. Raises ValueError where the library refuses the shape."""
    mfma_ok = d in (48, 96) and 2 * w + 1 <= 16
    parts = split_parts(d, T, w, H, N, num_cus)
    if parts > 1:
        return "lds_split", parts
    if mfma_ok and 4 <= T <= 1024 and T % 4 == 0:
        return "lds", 1
    if mfma_ok and T <= 4096:
        return ("mfma16" if T <= 2048 else "mfma8"), 1
    if d > 256 or T > 4096:
        raise ValueError("rel_attention: unsupported shape")
    R = 4 if T > 2048 or -(-T // 8) * H * N < num_cus else 8
    G, TK, W = 256 // d, min(T, 128), 2 * w + 1
    if 4 * (R * d + R * W + G * R * d + d * (TK + 1) + R * T + 2 * W * d + 256 * R) > LDS_LIMIT:
        raise ValueError("rel_attention: needs more than 160 KiB of LDS")
    return f"scalar{R}", 1


def max_parts(num_cus=256, H=1, N=1):
    """The largest part count any T reaches on `num_cus` CUs, with one T that reaches it."""
    best = (1, 0)
    for T in range(132, 1025, 4):
        p = split_parts(96, T, 4, H, N, num_cus)
        if p > best[0]:
            best = (p, T)
    return best


# ------------------------------------------------------------------------------------------------ the GPU cases
def case_id(c):
    return "d{d}-T{T}-w{w}-H{H}-N{N}-{kind}".format(**c)


def _cases():
    out = []

    def add(d, T, w, H, N, peaked=False):
        out.append(dict(d=d, T=T, w=w, H=H, N=N, kind="diffuse"))
        if peaked:
            out.append(dict(d=d, T=T, w=w, H=H, N=N, kind="peaked"))

    for d in (48, 96):
        # the staged-tile kernels and mfma16 at their edges (key tiles of 16, prefetch chunks of 32, staged tiles of 128, T % 4), mfma16
        # above 1024, mfma8 above 2048
        for T in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 124, 128, 129, 132, 260, 656, 1020, 1024, 1025, 1028, 2047, 2048,
                  2049, 2052, 4095, 4096):
            add(d, T, 4, 2, 1, peaked=T in (3, 17, 65, 132, 656, 1028, 2049, 4096))
        # windows: the one-entry table, three entries, and 15 of the 16 slots (four relative-value MFMA steps)
        for w in (0, 1, 7):
            for T in (16, 132, 1028, 2052):
                add(d, T, w, 2, 1, peaked=w != 1 and T in (132, 2052))
        # batch stride, head count, and the part count shrinking as the grid grows
        for H in (1, 3):
            for T in (36, 260, 1028):
                add(d, T, 4, H, 3, peaked=(H, T) in ((3, 260), (1, 1028)))
    # the scalar kernel: head dims without an MFMA instantiation, and a window of 17 entries
    for d, w in ((32, 4), (64, 4), (80, 4), (96, 8)):
        for T in (1, 7, 128, 129, 300, 1100, 2100):
            add(d, T, w, 2, 1, peaked=(d in (80, 96) and T in (129, 1100)) or (d == 32 and T == 300))
    # one head, one item: the grid is small enough for 4, 5 and 6 key parts on 256 CUs
    for d, T in ((96, 512), (96, 640), (96, 656), (48, 656)):
        add(d, T, 4, 1, 1, peaked=(d, T) == (96, 656))
    return out


GPU_CASES = _cases()
# Eight parts: min(⌈T/128⌉, CUs // (⌈T/16⌉·H·N)) = 8 needs T ≥ 897 and ⌈T/16⌉ ≥ 57 blocks per head, so 8 · 57 = 456 CUs; a 256-CU device
# stops at 6 (T = 644 … 672, one head, one item). The 8-part launch is reached through the tuning switch PIPER_HIP_ATT_SPLIT=8 instead:
# eight parts of one key tile each at T = 1024, and at T = 900 with a last part of 4 keys.
FORCED_PARTS = 8
FORCED_PARTS_CASES = [dict(d=d, T=T, w=4, H=1, N=1, kind=kind) for d in (96, 48) for T in (1024, 900) for kind in ("diffuse", "peaked")]


def check_rows(T, L=None):
    """The query rows the CPU conditions evaluate: all of them up to 2048, else 64 spread rows, both ends and the defect's row."""
    L = T if L is None else L
    if T <= 2048:
        return np.arange(L)
    return np.unique(np.concatenate([np.linspace(0, L - 1, 64).astype(np.int64), np.arange(8), np.arange(L - 8, L), [defect_row(L)]]))
