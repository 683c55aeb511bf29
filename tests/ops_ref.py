"""float64 references of the op-level C ABI (csrc/ops_basic.hip and the two module entry points of csrc/ops_conv.cpp), the bound each op is
held to, and the case tables of tests/test_gpu_ops_edges.py — TEST INFRASTRUCTURE (numpy on the CPU).

THE RULES (u = 2⁻²⁴, the unit roundoff of fp32). Every formula is evaluated in float64 on the float32 inputs.
  pad, slice, transpose, expand, concat, split, NEG, CEIL, RELU, ADD, SUB, MUL    bit-equal to numpy on float32 (`judge_exact`)
  matmul        per element |got − ref| ≤ (K + 2)·u·(|A|·|B|)ᵢⱼ: the a-priori bound of a K-term fp32 sum in any order (γ_K ≤ K·u/(1 − K·u),
                one rounding of ref to spare). A dropped or doubled term is about 1/K of that sum, thousands of times beyond it.
  reduce_mean   per row |got − ref| ≤ (cols + 2)·u·mean|x|: cols − 1 additions in any order and one division.
  softmax       1e-6 absolute (outputs ≤ 1), the figure tests/test_gpu_ops.py::test_softmax uses.
  add_layernorm, wavenet_layer, hifigan_resblock      conftest.assert_close at OP_TOL, the project's op rule.
  other unary ops, DIV, POW                           the tolerance tests/test_gpu_ops.py holds that op to (UNARY_TOL, BINARY_TOL), assert_close.
No constant here was measured on a kernel.

INPUTS are katdata.sym streams under seeds of this file (SD). Special values are finite: ±0, ±50 for tanh and sigmoid, ±100 for softplus,
±6 for erf; no NaN, Inf or denormal goes in (what the reference's shaders do there is not settled by its code).

tests/test_ops_ref.py ties every formula to tests/oracle.py on the katdata cases and checks, from the inputs alone, what the GPU cases rely
on: no fully masked softmax row, positive matmul bounds, finite exp / pow / sqrt, LayerNorm variances far above eps."""
import itertools
import math

import numpy as np

import conv_ref as cr
import katdata as kd
import piper_hip as ph
from conftest import OP_TOL

U = 2.0 ** -24
SD = kd.case_seed("mod", 0) + 47000  # disjoint from att_ref (31000 …) and the katdata ranges
MASK_FILL = np.float32(-1e4)         # what VITS attention writes over masked scores
BIG = 3 * (1 << 20) + 5              # elements past the grid cap of 8·CUs blocks × 1024 elements on 256 CUs (2²¹), and ≡ 1 mod 4

# ------------------------------------------------------------------------------------------------ the rules
UNARY_EXACT = (ph.NEG, ph.CEIL, ph.RELU)
UNARY_TOL = {ph.LEAKYRELU: 2e-6, ph.TANH: 2e-6, ph.SIGMOID: 2e-6, ph.ERF: 2e-6, ph.SOFTPLUS: 2e-6, ph.EXP: 1e-5, ph.SQRT: 1e-6}
UNARY_NAMES = {ph.RELU: "relu", ph.LEAKYRELU: "leakyrelu", ph.TANH: "tanh", ph.SIGMOID: "sigmoid", ph.EXP: "exp", ph.NEG: "neg", ph.SQRT: "sqrt",
               ph.SOFTPLUS: "softplus", ph.CEIL: "ceil", ph.ERF: "erf"}
BINARY_EXACT = (ph.ADD, ph.SUB, ph.MUL)
BINARY_TOL = {ph.DIV: 1e-6, ph.POW: 1e-5}
BINARY_NAMES = {ph.ADD: "add", ph.SUB: "sub", ph.MUL: "mul", ph.DIV: "div", ph.POW: "pow"}
SOFTMAX_TOL = 1e-6


def judge_exact(got, ref):
    """Bit-equal float32 → ratio 0.0, else inf (and the first differing flat index)."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    if got.shape != ref.shape:
        return dict(ok=False, ratio=math.inf, at=None)
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
    return dict(ok=bad.size == 0, ratio=math.inf if bad.size else 0.0, at=int(bad[0]) if bad.size else None)


def judge_elem(got, ref, bound):
    """Per element |got − ref| ≤ bound (both float64 arrays of ref's shape). → dict(ok, ratio, at): the worst ratio and its flat index."""
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    if not ref.size:
        return dict(ok=True, ratio=0.0, at=None)
    dlt = np.abs(got - ref)
    dlt = np.where(np.isfinite(dlt), dlt, np.inf)  # NaN counts as beyond
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, dlt / bound, np.where(dlt == 0, 0.0, np.inf))
    at = int(np.argmax(ratio))
    return dict(ok=bool(np.all(dlt <= bound)), ratio=float(ratio.reshape(-1)[at]), at=at)


def judge_tol(got, ref, tol):
    """conftest.assert_close's rule, |Δ| ≤ tol·max(1, ‖ref‖∞), as a ratio (ref rounded to float32 as assert_close does)."""
    ref = np.asarray(ref, np.float32).astype(np.float64)
    bd = tol * max(1.0, float(np.max(np.abs(ref)))) if ref.size else tol
    return judge_elem(got, ref, np.full(ref.shape, bd))


# ------------------------------------------------------------------------------------------------ the formulas
def _erf(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def unary(op, x, alpha=0.0):
    """float32 (bit-exact rule) for NEG / CEIL / RELU, float64 else."""
    x32 = np.asarray(x, np.float32)
    if op == ph.NEG:
        return -x32
    if op == ph.CEIL:
        return np.ceil(x32)
    if op == ph.RELU:
        return np.where(x32 > 0, x32, np.float32(0.0))  # −0 and 0 both give +0, as `x > 0 ? x : 0` does
    x = x32.astype(np.float64)
    if op == ph.LEAKYRELU:
        return np.where(x >= 0, x, np.float64(np.float32(alpha)) * x)
    if op == ph.TANH:
        return np.tanh(x)
    if op == ph.SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    if op == ph.EXP:
        return np.exp(x)
    if op == ph.SQRT:
        return np.sqrt(x)
    if op == ph.SOFTPLUS:
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    if op == ph.ERF:
        return _erf(x)
    raise ValueError(op)


def binary(op, a, b):
    """float32 (bit-exact rule) for ADD / SUB / MUL, float64 for DIV / POW; numpy broadcasting is the ABI's (trailing dims aligned)."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if op == ph.ADD:
        return a32 + b32
    if op == ph.SUB:
        return a32 - b32
    if op == ph.MUL:
        return a32 * b32
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    if op == ph.DIV:
        return a / b
    if op == ph.POW:
        return np.power(a, b)
    raise ValueError(op)


def pad(x, pads, value=0.0):
    """pads = begins of every axis, then ends (ONNX Pad)."""
    x = np.asarray(x, np.float32)
    r = x.ndim
    return np.pad(x, [(pads[d], pads[r + d]) for d in range(r)], constant_values=np.float32(value))


def slice_(x, axis, start, end, step=1):
    """Indices start, start + step, … short of end — Python's range; end = −1 with a negative step runs down to index 0."""
    return np.take(np.asarray(x, np.float32), list(range(start, end, step)), axis=axis)


def transpose(x, perm):
    return np.ascontiguousarray(np.transpose(np.asarray(x, np.float32), perm))


def expand(x, out_shape):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), out_shape))


def concat2_axis1(a, b):
    return np.concatenate([np.asarray(a, np.float32), np.asarray(b, np.float32)], 1)


def split2_axis1(x, c0):
    x = np.asarray(x, np.float32)
    return np.ascontiguousarray(x[:, :c0]), np.ascontiguousarray(x[:, c0:])


def matmul(a, b):
    """→ (ref, bound) in float64: lead dims broadcast where one side is 1 (or the result is empty where one is 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    K = a.shape[-1]
    return np.matmul(a, b), (K + 2) * U * np.matmul(np.abs(a), np.abs(b))


def reduce_mean(x):
    """→ (ref, bound) in float64 over the last dim."""
    x = np.asarray(x, np.float64)
    return x.mean(-1), (x.shape[-1] + 2) * U * np.abs(x).mean(-1)


def softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def layernorm_stats(x, y):
    """(mean, variance) [N, T] of x + y over the channels, float64, two passes."""
    v = np.asarray(x, np.float64) + (0.0 if y is None else np.asarray(y, np.float64))
    return v.mean(1), v.var(1)


def add_layernorm(x, y, gamma, beta, eps=1e-5):
    """x, y [N, C, T] → ((x + y) − mean) / sqrt(var + eps) · gamma + beta over C, float64."""
    v = np.asarray(x, np.float64) + (0.0 if y is None else np.asarray(y, np.float64))
    mean = v.mean(1, keepdims=True)
    var = ((v - mean) ** 2).mean(1, keepdims=True)
    g, b = (np.asarray(t, np.float64)[None, :, None] for t in (gamma, beta))
    return (v - mean) / np.sqrt(var + np.float64(np.float32(eps))) * g + b


def wavenet_layer(x, skip_in, w_in, b_in, w_rs, b_rs, K, dil, last):
    """in-conv (2C rows, `same` padding) → tanh(first C rows) · sigmoid(last C rows) → 1 × 1 conv → split, float64.
    Not last: w_rs has 2C rows, x_out = x + rs[:C], skip_out = skip_in + rs[C:]. Last: C rows, skip_out = skip_in + rs, x_out None."""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    p = (K * dil - dil) // 2
    h = cr.conv1d(x, w_in, b_in, 1, dil, p, p)
    acts = np.tanh(h[:, :C]) * (1.0 / (1.0 + np.exp(-h[:, C:])))
    rs = cr.conv1d(acts, w_rs, b_rs)
    sk = 0.0 if skip_in is None else np.asarray(skip_in, np.float64)
    if last:
        return None, sk + rs
    return x + rs[:, :C], sk + rs[:, C:]


def hifigan_resblock(type_, x, K, dils, ws, bs, slope=0.1):
    return cr.resblock(type_, x, K, dils, ws, bs, np.float64(np.float32(slope)))


# ------------------------------------------------------------------------------------------------ case tables and inputs
# ---- add_layernorm: add_layernorm_kernel<12> (C ≤ 192), <32> (C ≤ 512), add_layernorm_big_kernel above; 16 time steps × 16 channel lanes
# per block. (C, T, N, with_y, offset); offset: a common-mode value added to every element of x (tests/test_gpu_voice.py's +60).
LN_OFFSET = 60.0
LN_CASES = [
    # add_layernorm_kernel<12>
    (1, 17, 1, True, 0.0),      # one channel: only lane group 0 of slot 0 is real, the deviation is exactly 0, the output is beta
    (5, 15, 3, False, 0.0),     # c < C masks inside slot 0, t < T masks inside the only block, batch stride, no residual
    (16, 16, 1, True, 0.0),     # exactly one slot, exactly one block
    (96, 1, 1, True, 0.0),      # one time step
    (100, 45, 3, True, 0.0),    # C % 16 = 4: the mask inside slot 6; three blocks, the last ragged
    (192, 17, 1, False, 0.0),   # the last C of this kernel: all 12 slots full; one column in the second block
    (192, 16, 1, True, LN_OFFSET),
    # add_layernorm_kernel<32>
    (193, 15, 1, True, 0.0),    # the first C of this kernel: one channel in slot 12
    (208, 45, 3, False, 0.0),   # 13 full slots
    (500, 17, 1, True, 0.0),    # C % 16 = 4 in slot 31
    (512, 16, 3, True, 0.0),    # the last C of this kernel: all 32 slots full
    (512, 1, 1, False, 0.0),
    (500, 45, 1, True, LN_OFFSET),
    # add_layernorm_big_kernel
    (513, 17, 1, True, 0.0),    # the first C of this kernel: lane group 0 walks one channel more than the others
    (513, 16, 1, False, 0.0),
    (768, 15, 1, True, 0.0),
    (768, 45, 3, False, 0.0),
    (768, 16, 1, True, LN_OFFSET),
]
LN_EPS = 1e-5


def ln_kernel(C):
    return "ln12" if C <= 192 else "ln32" if C <= 512 else "big"


def ln_inputs(idx):
    """(x, y or None, gamma, beta) in float32."""
    C, T, N, with_y, offset = LN_CASES[idx]
    sd = SD + 1000 + 10 * idx
    x = kd.sym(sd, (N, C, T), 2.0) + np.float32(offset)
    y = kd.sym(sd + 1, (N, C, T), 2.0) if with_y else None
    return x, y, np.float32(1.0) + kd.sym(sd + 2, (C,), 0.1), kd.sym(sd + 3, (C,), 0.1)


# ---- matmul: 64 × 64 output tiles (blockIdx.y = M tile, blockIdx.x = N tile), K staged 16 at a time, lead dims by stride-0 broadcast;
# the outer lead dim is a host loop. (a_shape, b_shape)
MATMUL_CASES = [
    ((65, 1), (1, 65)),              # K = 1: one k of the first stage is real; one row and one column in the second tiles
    ((130, 17), (17, 64)),           # three M tiles (blockIdx.y = 2 holds two rows), K = 16 + 1, N exactly one tile
    ((64, 16), (16, 129)),           # M and K exactly one tile / one stage, three N tiles
    ((1, 33), (33, 1)),              # one output element, K = 2·16 + 1
    ((127, 96), (96, 200)),          # Piper's K, ragged last tiles both ways
    ((2, 1, 66, 9), (1, 3, 9, 5)),   # mixed lead broadcast: the host loop runs with a NON-zero A stride and a zero B stride, blockIdx.z the reverse
    ((2, 3, 5, 20), (2, 3, 20, 67)),  # no broadcast: both strides in the loop and in blockIdx.z
    ((3, 66, 7), (1, 7, 3)),         # rank 3, B broadcast
    ((1, 4, 18), (3, 18, 70)),       # rank 3, A broadcast
    ((0, 4, 5), (1, 5, 6)),          # a zero lead dim: an empty result with its shape
]


def matmul_inputs(idx):
    sa, sb = MATMUL_CASES[idx]
    sd = SD + 2000 + 10 * idx
    return kd.sym(sd, sa), kd.sym(sd + 1, sb)


# ---- softmax: softmax_wave_kernel (one wave per row, 32 register slots of 64 lanes) up to 2048 columns, softmax_block_kernel above; the
# wave kernel's grid stops at 8·CUs blocks of 4 waves (8192 rows on 256 CUs), the block kernel's at 8·CUs rows. (rows, cols, masked)
SOFTMAX_CASES = [
    (5, 63, False), (5, 64, False), (5, 65, False),        # the lane edge: slot 0 ragged, exactly full, one column in slot 1
    (5, 2047, False), (5, 2048, False),                    # the last slot ragged / every slot full: the last widths of the wave kernel
    (5, 2049, False),                                      # the first width of the block kernel: one column in the ninth pass of thread 0
    (20011, 7, False),                                     # past the wave kernel's row cap: every wave walks 2 or 3 rows
    (2051, 2049, False),                                   # past the block kernel's row cap: three blocks walk two rows
    (6, 70, True), (4, 2049, True),                        # −1e4 mask fill next to ordinary scores, both kernels
]


def softmax_input(idx):
    rows, cols, masked = SOFTMAX_CASES[idx]
    x = kd.sym(SD + 3000 + idx, (rows, cols), 8.0)
    if masked:  # row r keeps its first cols − (r + 1)·cols // (rows + 1) scores, as a padded batch item does
        for r in range(rows):
            x[r, cols - (r + 1) * cols // (rows + 1):] = MASK_FILL
        x[rows - 1, 1:] = MASK_FILL  # and one row with a single real key
    return x


# ---- reduce_mean: one wave per row, the same row cap. (rows, cols)
REDUCE_CASES = [(5, 1), (5, 63), (5, 64), (5, 65), (5, 1000), (20011, 3)]


def reduce_input(idx):
    rows, cols = REDUCE_CASES[idx]
    return kd.sym(SD + 4000 + idx, (rows, cols), 3.0) + np.float32(0.5)


# ---- the gather family (gather4_kernel: every output element divides its index down the ranks): ranks 1 to 4 with odd sizes
GATHER_SHAPES = [(7,), (5, 3), (3, 5, 7), (3, 5, 2, 7)]
PAD_VALUE = 2.5
PERM_SHAPE = (3, 5, 2, 7)
PERMS4 = [list(p) for p in itertools.permutations(range(4))]
# (axis length 10) start, end, step: an empty range, steps that do not divide the range, negative steps with and without the −1 end
SLICES = [(4, 4, 1), (7, 2, 1), (0, 10, 3), (1, 9, 3), (2, 10, 7), (9, 0, -2), (9, -1, -2), (8, 1, -3)]
SLICE_SHAPES = [((10,), 0), ((3, 10), 1), ((10, 3, 5), 0), ((3, 2, 10, 5), 2)]
EXPANDS = [((1, 5, 1, 7), (3, 5, 2, 7)), ((3, 1, 1), (3, 4, 5)), ((1, 1), (6, 7)), ((1,), (9,))]
BIG_PAD = ((21, 136769), [1, 1, 1, 1])  # → 23 × 136771 = 3·2²⁰ + 5 outputs: past the grid cap, every thread walks its stride loop
assert (BIG_PAD[0][0] + 2) * (BIG_PAD[0][1] + 2) == BIG


def gather_input(shape, salt=0):
    return kd.sym(SD + 5000 + salt + sum(shape), shape)


def pads_for(shape):
    """Pads on both sides of every axis, all different: begins 1, 2, …, ends 2, 3, …"""
    r = len(shape)
    return [d + 1 for d in range(r)] + [d + 2 for d in range(r)]


# ---- unary / binary (unary_kernel, binary_flat_kernel, binary_bcast_kernel): float4 body + scalar tail on 16-byte aligned pointers, the
# scalar loop (vec_ok == 0) otherwise
UNARY_N = 1031  # ≡ 3 mod 4, more than one block of 1024 elements
UNARY_ALPHA = {ph.LEAKYRELU: 0.1}
UNARY_OPS = tuple(range(ph.ERF + 1))
SPECIALS = {ph.TANH: (50.0, -50.0), ph.SIGMOID: (50.0, -50.0), ph.SOFTPLUS: (100.0, -100.0), ph.ERF: (6.0, -6.0)}


def unary_input(op, n=UNARY_N):
    x = kd.sym(SD + 6000 + op, (n,), 6.0)
    sp = (0.0, -0.0) + SPECIALS.get(op, ())
    x[:len(sp)] = np.array(sp, np.float32)
    if op == ph.SQRT:
        x = np.abs(x)  # |−0| = +0
    return x


# binary on the aligned flat path: sizes 4k + 1, + 2, + 3 reach the scalar tail of binary_flat_kernel; (a_shape, b_shape)
BINARY_TAIL_CASES = [((1029,), (1029,)), ((1030,), (1030,)), ((1031,), (1031,)), ((7, 11, 3), (7, 11, 3)),
                     ((1029,), (1,)), ((5, 206), (1, 1))]                   # the scalar-b path with a tail
# broadcasts with DIV and POW: the scalar-b path and a-side broadcasts (binary_bcast_kernel with a zero A stride)
BINARY_BCAST_CASES = [((3, 5, 7), (1,)), ((1, 1, 7), (3, 5, 7)), ((1,), (4, 9)), ((5, 1, 7), (1, 3, 1)), ((2, 1, 3, 1), (5, 1, 4))]
BINARY_N = 1031  # the misaligned cases


def binary_inputs(sa, sb, op, salt=0):
    """a, b in ±2; DIV: |b| + 0.5; POW: |a| + 0.1 (what tests/test_gpu_ops.py::test_binary feeds)."""
    sd = SD + 7000 + 10 * salt + op
    a, b = kd.sym(sd, sa, 2.0), kd.sym(sd + 1, sb, 2.0)
    if op == ph.DIV:
        b = np.abs(b) + np.float32(0.5)
    if op == ph.POW:
        a = np.abs(a) + np.float32(0.1)
    return a, b


# ---- wavenet_layer: (C, T, K, dilation, N, last, with_skip_in). On 256 CUs conv_pick_tile gives 32-wide tiles from 8·CUs = 2048 tiles of
# 64 gated rows × 32 columns on: ⌈2C / 64⌉ · ⌈T / 32⌉ · N ≥ 2048 — C = 32, N = 2: T > 32 · 1023.
WN_T32 = 32 * 1023 + 1
WN_CASES = [
    (96, 17, 3, 1, 2, False, True),      # 16-wide, dilation 1: the gate-interleaved image is packed, no kernel of it covers Cin = 96 → plain image
    (32, 700, 5, 2, 1, False, True),     # dilation 2: plain 16-wide image only
    (64, 2000, 1, 1, 1, True, True),     # last layer (C res/skip rows), k = 1
    (192, 300, 5, 1, 3, False, False),   # Piper's geometry: the gate-interleaved image; skip_in = NULL with !last; batch strides
    (32, WN_T32, 3, 1, 2, False, True),  # 32-wide images for both convs
]
WN_IMAGES = ("gate16", "plain16", "wide32")


def wn_tile(num_cus, C, T, N):
    """conv_pick_tile for the gated in-conv of piper_hip_wavenet_layer_f32 (2C rows, gate = 1): 16 or 32."""
    tiles32 = -(-2 * C // 64) * -(-T // 32) * N
    return 16 if tiles32 < 8 * num_cus and (2 * C) % 32 == 0 else 32


def image_of_record(rec):
    """The weight image a route record of a gated conv names, or None for a conv that is not gated: the gate-interleaved 16-wide image is
    read by conv_gate_kernel (lean_gate) and conv_short's gated variant, the streaming kernel reads the plain image of its tile width."""
    v = cr.variant_of(rec)
    p = cr.params_of(v)
    if p.get("gate") != "1":
        return None
    fam = cr.family_of(v)
    if fam in ("lean_gate", "short"):
        return "gate16"
    if fam == "stream":
        return "plain16" if p["TM"] == "16" else "wide32"
    raise ValueError(f"gated conv on an unknown family: {rec}")


def wn_inputs(idx):
    C, T, K, dil, N, last, with_skip = WN_CASES[idx]
    sd = SD + 8000 + 10 * idx
    Crs = C if last else 2 * C
    return dict(x=kd.sym(sd, (N, C, T)), sk=kd.sym(sd + 1, (N, C, T)) if with_skip else None, w_in=kd.weight(sd + 2, (2 * C, C, K), C * K),
                b_in=kd.sym(sd + 3, (2 * C,), 0.1), w_rs=kd.weight(sd + 4, (Crs, C, 1), C), b_rs=kd.sym(sd + 5, (Crs,), 0.1))


# ---- hifigan_resblock: (type, C, T, K, dilations, N, slope). Slope 1.5 is outside (0, 1), where max(x, slope·x) is no LeakyReLU: the fused
# pair kernel is refused and every conv runs on its own (launch_conv_mfma). C = 6 is below conv_mfma_eligible's 8 output channels:
# launch_conv_direct with the LeakyReLU prologue and the residual.
RB_CASES = [
    (1, 32, 228, 3, [1, 3], 2, 1.5), (2, 32, 228, 3, [1, 3], 2, 1.5),
    (1, 6, 37, 3, [1, 3], 2, 0.1), (2, 6, 37, 5, [1, 2, 3], 2, 0.1),
]


def rb_inputs(idx):
    type_, C, T, K, dils, N, slope = RB_CASES[idx]
    sd = SD + 9000 + 40 * idx
    nconv = len(dils) * (2 if type_ == 1 else 1)
    return (kd.sym(sd, (N, C, T)), [kd.weight(sd + 1 + i, (C, C, K), C * K) for i in range(nconv)],
            [kd.sym(sd + 20 + i, (C,), 0.1) for i in range(nconv)])
