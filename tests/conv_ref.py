"""Route records of the conv launchers (piper_hip_routes_arm) and a float64 reference of Conv / ConvTranspose — TEST INFRASTRUCTURE
(numpy on the CPU).

A RECORD is "<variant> | Cout=… Cin=… Lout=… N=… CUs=…": the variant names the kernel family, its template and launch parameters, gate,
prologue, epilogue and conv / convT; the shape (and the CU count the heuristics weighed it against) stands apart. `variant_of` drops the
shape, so two launches compare by the code that ran. `family_of` / `params_of` take a variant apart.

THE RULE is the project's op-level one, |Δ| ≤ OP_TOL · max(1, ‖ref‖∞) (conftest), against the float64 evaluation of the same sums. The
bf16 ops are judged on operands rounded to bf16 first (products of two bf16 values are exact in fp32: only the accumulation order differs),
as tests/test_gpu_ops.py::test_conv1d_bf16 does.

PLANTED DEFECTS (`plant`) are what a tiled kernel gets wrong at a tile edge; tests/test_conv_routes.py asserts that each breaks the rule at
every edge shape of tests/test_gpu_conv_routes.py where it applies, and that an fp32 evaluation in two accumulation orders stays below a
tenth of it: a correct kernel passes with room, a kernel with one of these defects cannot."""
import numpy as np

from conftest import OP_TOL

# ------------------------------------------------------------------------------------------------ records


def parse_record(rec):
    """→ (variant, shape dict). Raises ValueError on anything that is not a record."""
    variant, sep, shape = rec.partition(" | ")
    if not sep or not variant.strip() or variant != variant.strip():
        raise ValueError(f"not a route record: {rec!r}")
    out = {}
    for tok in shape.split():
        k, eq, v = tok.partition("=")
        if not eq or k in out:
            raise ValueError(f"bad shape field {tok!r} in {rec!r}")
        out[k] = int(v)
    if set(out) != {"Cout", "Cin", "Lout", "N", "CUs"}:
        raise ValueError(f"shape fields {sorted(out)} in {rec!r}")
    return variant, out


def variant_of(rec):
    """The record with its shape dropped."""
    return parse_record(rec)[0]


def family_of(variant):
    return variant.split()[0]


def params_of(variant):
    """{"K": "3", "TM": "16", …, "kind": "conv" | "convT"} of a variant (values as text)."""
    toks = variant.split()[1:]
    out = {}
    for t in toks:
        k, eq, v = t.partition("=")
        if eq:
            out[k] = v
        elif t in ("conv", "convT"):
            out["kind"] = t
        else:
            raise ValueError(f"bad token {t!r} in variant {variant!r}")
    return out


def variants(records):
    """Sorted distinct variants of an iterable of records."""
    return sorted({variant_of(r) for r in records})


def cus_of(records):
    cus = {parse_record(r)[1]["CUs"] for r in records}
    assert len(cus) == 1, cus
    return cus.pop()


# ------------------------------------------------------------------------------------------------ the reference
def conv1d(x, w, b=None, stride=1, dil=1, pad_l=0, pad_r=0, groups=1, dt=np.float64, taps=None, lrelu=None):
    """[N, Cout, Lout] in dt. x [N, Cin, L], w [Cout, Cin / groups, K]. taps: the tap indices summed, in this order (None: 0 … K − 1);
    lrelu: slope of a LeakyReLU applied to x first."""
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    if lrelu is not None:
        x = np.where(x >= 0, x, x * dt(lrelu))
    N, Cin, L = x.shape
    Cout, cig, K = w.shape
    Lout = (L + pad_l + pad_r - dil * (K - 1) - 1) // stride + 1
    if Lout <= 0:
        return np.zeros((N, Cout, max(Lout, 0)), dt)
    xp = np.zeros((N, Cin, L + pad_l + pad_r), dt)
    xp[:, :, pad_l:pad_l + L] = x
    y = np.zeros((N, Cout, Lout), dt)
    cog = Cout // groups
    for k in (range(K) if taps is None else taps):
        xs = xp[:, :, k * dil:k * dil + (Lout - 1) * stride + 1:stride]
        for g in range(groups):
            y[:, g * cog:(g + 1) * cog] += np.einsum("oc,ncl->nol", w[g * cog:(g + 1) * cog, :, k], xs[:, g * cig:(g + 1) * cig], optimize=True)
    if b is not None:
        y += np.asarray(b, dt)[None, :, None]
    return y


def convtranspose1d(x, w, b=None, stride=1, dil=1, pad_l=0, pad_r=0, out_pad=0, groups=1, dt=np.float64, taps=None):
    """[N, Cout, Lout] in dt. x [N, Cin, L], w [Cin, Cout / groups, K]: y[t] = Σ x[i] w[k] over t = i·stride − pad_l + k·dil."""
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    N, Cin, L = x.shape
    _, cog, K = w.shape
    Cout = cog * groups
    cig = Cin // groups
    Lout = (L - 1) * stride - pad_l - pad_r + dil * (K - 1) + out_pad + 1
    full = np.zeros((N, Cout, (L - 1) * stride + dil * (K - 1) + 1 + out_pad + pad_l + pad_r), dt)
    for k in (range(K) if taps is None else taps):
        for g in range(groups):
            z = np.einsum("co,ncl->nol", w[g * cig:(g + 1) * cig, :, k], x[:, g * cig:(g + 1) * cig], optimize=True)
            full[:, g * cog:(g + 1) * cog, k * dil:k * dil + (L - 1) * stride + 1:stride] += z
    y = full[:, :, pad_l:pad_l + Lout].copy()
    if b is not None:
        y += np.asarray(b, dt)[None, :, None]
    return y


def resblock(type_, x, K, dils, ws, bs, slope=0.1, dt=np.float64):
    """HiFi-GAN ResBlock1 (pairs of convs, the second at dilation 1) / ResBlock2 (one conv per dilation), residual around each."""
    x = np.asarray(x, dt)
    for i, d in enumerate(dils):
        if type_ == 1:
            t = conv1d(x, ws[2 * i], bs[2 * i], 1, d, (K * d - d) // 2, (K * d - d) // 2, dt=dt, lrelu=slope)
            x = x + conv1d(t, ws[2 * i + 1], bs[2 * i + 1], 1, 1, (K - 1) // 2, (K - 1) // 2, dt=dt, lrelu=slope)
        else:
            x = x + conv1d(x, ws[i], bs[i], 1, d, (K * d - d) // 2, (K * d - d) // 2, dt=dt, lrelu=slope)
    return x


def bound(ref):
    return OP_TOL * max(1.0, float(np.max(np.abs(ref)))) if ref.size else OP_TOL


def judge(got, ref):
    """{"err", "bound", "ratio", "ok"} of the rule; got in any float type, ref float64."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    bd = bound(ref)
    return dict(err=err, bound=bd, ratio=err / bd, ok=bool(np.all(np.isfinite(got))) and err <= bd)


# ------------------------------------------------------------------------------------------------ planted defects
DEFECTS = ("last_col_tile_skipped", "tap_dropped", "last_row_tile_dropped", "convt_last_pad_stale")
STALE = 0.0  # what a skipped store leaves behind: the pool hands out recycled blocks, zero stands for "not what the conv gives"


def plant(defect, ref, col_tile, row_tile, redo=None, pad=0):
    """A copy of `ref` [N, C, L] with the defect, or None where the shape cannot show it.
    last_col_tile_skipped: the columns of the last `col_tile`-wide tile are left stale; last_row_tile_dropped: the rows of the last (ragged
    or whole) `row_tile`-high tile; convt_last_pad_stale: the last `pad` columns; tap_dropped: `redo()` re-evaluates the reference
    without one tap."""
    out = np.array(ref, np.float64)
    N, C, L = out.shape
    if defect == "last_col_tile_skipped":
        out[:, :, (L - 1) // col_tile * col_tile:] = STALE
    elif defect == "last_row_tile_dropped":
        out[:, (C - 1) // row_tile * row_tile:, :] = STALE
    elif defect == "convt_last_pad_stale":
        if pad < 1:
            return None
        out[:, :, L - pad:] = STALE
    elif defect == "tap_dropped":
        if redo is None:
            return None
        out = redo()
    else:
        raise ValueError(defect)
    return out
