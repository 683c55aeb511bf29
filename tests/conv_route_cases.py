"""Tile-edge cases for the conv variants the op API reaches — the table tests/test_gpu_conv_routes.py runs on the GPU and
tests/test_conv_routes.py judges the float64 reference on (TEST INFRASTRUCTURE).

Per variant: the smallest shape that selects it on 256 CUs, its column tile c, Lout ∈ {c·m − 1, c·m, c·m + 1} for the smallest m that keeps
the variant, one shape whose Cout is no multiple of the row tile, one whose Cin is no multiple of the contraction step (where the kernel
takes such a Cin), and for ConvTranspose a row whose length is a multiple of the column tile. `want` is the variant the case is there for, as
the prefix of the record the launcher must leave (conv_ref.variant_of). Kernels that need 16-byte rows (window, chunk-pipelined, the
wide Cout = 1 kernels) get their ± 1 through the pads, or ± 4 where the output is as long as the input.

Why the odd input channel counts: a long row (Lout ≥ 1024) with an even Cin and Lin % 4 == 0 goes to the window kernels; 33 channels keep it on
the streaming / tile kernels and are no multiple of their contraction step at the same time."""
import numpy as np

import conv_ref as cr
import katdata as kd

SD = kd.case_seed("cfg", 4000)


def _c(id_, want, cin, cout, K, L, N=1, dil=1, pads=None, stride=1, groups=1, col=16, row=16, op="conv", bias=True):
    pl, pr = ((K * dil - dil) // 2,) * 2 if pads is None else pads
    return dict(id=id_, op=op, want=want, cin=cin, cout=cout, K=K, L=L, N=N, dil=dil, pl=pl, pr=pr, stride=stride, groups=groups, col=col, row=row,
                bias=bias)


def _t(id_, want, cin, cout, K, s, L, N=1, pad=None, dil=1, groups=1, out_pad=0, col=16, row=16, op="convt"):
    pad = (K - s) // 2 if pad is None else pad
    return dict(id=id_, op=op, want=want, cin=cin, cout=cout, K=K, L=L, N=N, dil=dil, pl=pad, pr=pad, stride=s, groups=groups, out_pad=out_pad,
                col=col, row=row, bias=True)


def _rb(id_, want, type_, C, K, dils, L, N=1, col=256):
    return dict(id=id_, op="rb", want=want, type=type_, cin=C, cout=C, K=K, dils=list(dils), L=L, N=N, col=col, row=32)


S16 = "stream K=3 TM=16 NT=1 KS=8 BT=512"
CASES = (
    # ---- streaming kernel, 16-wide tiles, contraction split over 8 waves: c = TM · NT = 16
    [_c(f"stream16_k3_L{L}", S16, 192, 256, 3, L) for L in (15, 16, 17)] +
    [_c("stream16_k3_cout250", S16, 192, 250, 3, 17), _c("stream16_k3_cin190", S16, 190, 256, 3, 17)] +
    # 16 slices, BT = 1024; dilation 6: the halo is wider than the row
    [_c(f"stream16_k5_d6_L{L}", "stream K=5 TM=16 NT=1 KS=16 BT=1024", 128, 128, 5, L, dil=6) for L in (31, 32, 33)] +
    [_c(f"stream16_k11_d5_L{L}", "stream K=11 TM=16 NT=1 KS=16 BT=1024", 256, 256, 11, L, dil=5) for L in (16, 17)] +
    [_c("stream16_k3_ks2_cin37_cout40", "stream K=3 TM=16 NT=1 KS=2 BT=256", 37, 40, 3, 17)] +
    # ---- streaming kernel, 32-wide tiles (≥ 2048 tiles): NT = 1, 2, 4 → c = 32, 64, 128. 33 input channels: see the module docstring
    [_c(f"stream32_nt1_L{L}", "stream K=3 TM=32 NT=1 KS=1 BT=256", 33, 256, 3, L, N=8, col=32, row=32) for L in (1023, 1024, 1025)] +
    [_c("stream32_nt1_cout250", "stream K=3 TM=32 NT=1 KS=1 BT=256", 33, 250, 3, 1025, N=8, col=32, row=32)] +
    [_c(f"stream32_nt2_L{L}", "stream K=1 TM=32 NT=2 KS=1 BT=256", 33, 256, 1, L, N=32, col=64, row=32) for L in (1023, 1024, 1025)] +
    [_c(f"stream32_nt4_L{L}", "stream K=1 TM=32 NT=4 KS=1 BT=256", 33, 256, 1, L, N=64, col=128, row=32) for L in (1023, 1025)] +
    # ---- tile kernel (Lout ≥ 2048, ≥ 4 blocks per CU, ≤ 64 output channels per block): c = 128 · NTW = 256
    [_c(f"tile_k1_L{L}", "tile K=1 MT=2 NTW=2", 33, 64, 1, L, N=8, col=256, row=32) for L in (32767, 32768, 32769)] +
    [_c("tile_k1_cout40", "tile K=1 MT=2 NTW=2", 33, 40, 1, 32769, N=8, col=256, row=32)] +
    [_c("tile_k7_d3_mt1", "tile K=7 MT=1 NTW=2", 31, 32, 7, 32769, N=8, dil=3, col=256, row=32)] +
    # ---- short-row kernel (k 7 with few tiles): c = 16 · NT = 16
    [_c(f"short_k7_L{L}", "short K=7 NT=1 KS=8 BT=512 QC=6", 192, 256, 7, L) for L in (15, 16, 17)] +
    [_c("short_k7_cout250", "short K=7 NT=1 KS=8 BT=512 QC=6", 192, 250, 7, 17), _c("short_k7_cin190", "short K=7 NT=1 KS=8 BT=512 QC=6", 190, 256, 7, 17)] +
    # ---- lean k = 1 kernel (96 or 192 input channels, 16 × 16 tiles)
    [_c(f"lean_k1_L{L}", "lean_k1 K=1 NQ=6", 192, 192, 1, L) for L in (15, 16, 17)] +
    [_c("lean_k1_cout200", "lean_k1 K=1 NQ=6", 192, 200, 1, 17), _c("lean_k1_nq3", "lean_k1 K=1 NQ=3", 96, 192, 1, 33)] +
    # ---- window kernel (Lout ≥ 1024, rows of whole float4s): c = 32 · WN; Lout = L − 1, L, L + 1 through the pads
    [_c(f"win_k3_{n}", "win K=3 WM=1 WN=1 KS=4", 48, 40, 3, 1056, pads=p, col=32, row=32) for n, p in (("m1", (1, 0)), ("0", (1, 1)), ("p1", (2, 1)))] +
    [_c("win_k3_cin34_cout72", "win K=3", 34, 72, 3, 1060, col=32, row=32)] +
    # ---- chunk-pipelined kernel (Cin % 32 == 0): c = 32 · WN · NTW
    [_c(f"pipe_k3_{n}", "pipe K=3 WM=1 WN=4 NTW=1", 32, 32, 3, 1152, pads=p, col=128, row=32) for n, p in (("m1", (1, 0)), ("0", (1, 1)), ("p1", (2, 1)))] +
    [_c("pipe_k3_cout40", "pipe K=3 WM=2 WN=2 NTW=1", 32, 40, 3, 1088, pads=(2, 1), col=64, row=32)] +
    [_c(f"pipe_k3_ntw2_{n}", "pipe K=3 WM=2 WN=2 NTW=2", 32, 64, 3, 8192, N=8, pads=p, col=128, row=32) for n, p in (("m1", (1, 0)), ("0", (1, 1)), ("p1", (2, 1)))] +
    # ---- thread-per-output kernel (stride 2; depthwise groups): 256 outputs per block
    [_c(f"direct_stride2_L{L}", "direct stride=2 groups=1", 16, 32, 4, L, pads=(1, 1), stride=2, col=8, row=1) for L in (15, 17, 19)] +
    [_c("direct_depthwise", "direct stride=1 groups=48", 48, 48, 3, 17, dil=3, groups=48, col=256, row=1)] +
    # ---- few output channels: 256 columns per block, 32 input channels per stage
    [_c(f"small_cout1_L{L}", "small_cout CO=1", 32, 1, 7, L, col=256, row=1) for L in (255, 256, 257)] +
    [_c("small_cout3_cin33", "small_cout CO=3", 33, 3, 5, 257, dil=2, col=256, row=4), _c("small_cout4_nobias", "small_cout CO=4", 64, 4, 3, 513, col=256, row=4, bias=False)] +
    # ---- Cout = 1, k 7, rows of whole float4s from 4096: four channel-splitting waves per 256 outputs; 1024 outputs per block from 2 blocks per CU
    # (± 4 in place of ± 1, and m + 1 tiles for the − 4: shorter rows take the small-Cout kernel)
    [_c(f"cout1_split_L{L}", "cout1_split K=7", 36, 1, 7, L, col=256, row=1) for L in (4096, 4100, 4348)] +
    [_c(f"cout1_wide_L{L}", "cout1_wide K=7 BT=256", 20, 1, 7, L, N=128, col=1024, row=1) for L in (4096, 4100, 5116)] +
    # ---- ConvTranspose on the streaming kernel (phase decomposition: rows Cout · stride, taps K / stride, columns Lin + 1): a row whose
    # length is a multiple of the column tile had its last `pad` outputs skipped once (profiles/f32_exact_units.md)
    [_t(f"convt_stream16_L{L}", "stream K=2 TM=16 NT=1", 64, 32, 8, 4, L) for L in (14, 15, 16, 31, 32)] +
    [_t("convt_stream16_cout24_cin62", "stream K=2 TM=16 NT=1", 62, 24, 8, 4, 16)] +
    [_t(f"convt_stream32_L{L}", "stream K=2 TM=32 NT=1 KS=1 BT=256", 64, 32, 8, 4, L, N=80, col=32, row=32) for L in (222, 223, 224)] +
    [_t("convt_stream32_cout24_cin62", "stream K=2 TM=32 NT=1 KS=1 BT=256", 62, 24, 8, 4, 223, N=100, col=32, row=32)] +
    # ---- ConvTranspose on the window kernel (Lin ≥ 256, rows of whole float4s): Lin = 32 · m and 32 · m + 4
    [_t(f"convt_win_L{L}", "win K=8", 64, 32, 8, 4, L, col=32, row=32) for L in (256, 260, 288)] +
    # ---- thread-per-output ConvTranspose (groups; dilation)
    [_t("convt_direct_groups2", "convt_direct stride=2 groups=2", 8, 6, 4, 2, 43, pad=1, groups=2, col=256, row=1),
     _t("convt_direct_dil2", "convt_direct stride=2 groups=1", 8, 8, 3, 2, 17, pad=1, dil=2, col=256, row=1)] +
    # ---- the ResBlock pair kernel: 256 − 2 · (conv b's reach) output columns per tile, dropped to a multiple of 32 when the rest is < 16
    [_rb(f"rb_pair_t1_c64_L{L}", "rb_pair MT=2 exact=1 Ka=3 da=1 Kb=3 db=1", 1, 64, 3, [1], L, col=254) for L in (252, 256, 508)] +
    [_rb(f"rb_pair_t2_c32_L{L}", "rb_pair MT=1 exact=1 Ka=7 da=1 Kb=7 db=3", 2, 32, 7, [1, 3], L, col=224) for L in (220, 224, 228, 448)] +
    # ---- bf16 operands: c = 32 · WN · NTW
    [_c(f"bf16_k3_L{L}", "bf16 K=3 MTW=1 NTW=1 WM=1", 32, 32, 3, L, col=128, row=32, op="conv_bf16") for L in (127, 128, 129)] +
    [_c("bf16_k3_cout40", "bf16 K=3 MTW=1 NTW=1 WM=2", 32, 40, 3, 65, col=64, row=32, op="conv_bf16")] +
    [_t(f"convt_bf16_L{L}", "bf16 K=8 MTW=1 NTW=1 WM=1", 64, 32, 8, 4, L, col=128, row=32, op="convt_bf16") for L in (127, 128, 129)]
)
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(IDS)


def inputs(i):
    """(x, w or [w…], b or [b…]) of case i in fp32."""
    c = CASES[i]
    sd = SD + 97 * i
    x = kd.sym(sd, (c["N"], c["cin"], c["L"]))
    if c["op"] == "rb":
        n = len(c["dils"]) * (2 if c["type"] == 1 else 1)
        return x, [kd.weight(sd + 1 + j, (c["cin"], c["cin"], c["K"]), c["cin"] * c["K"]) for j in range(n)], [kd.sym(sd + 40 + j, (c["cin"],), 0.1) for j in range(n)]
    if c["op"] in ("convt", "convt_bf16"):
        w = kd.weight(sd + 1, (c["cin"], c["cout"] // c["groups"], c["K"]), max(1, c["cin"] // c["groups"] * c["K"] // c["stride"]))
    else:
        w = kd.weight(sd + 1, (c["cout"], c["cin"] // c["groups"], c["K"]), c["cin"] // c["groups"] * c["K"])
    return x, w, (kd.sym(sd + 2, (c["cout"],), 0.1) if c["bias"] else None)


def reference(i, dt=np.float64, taps=None, x=None, w=None, b=None):
    """The case's output in dt from its inputs (or the given ones); taps as conv_ref.conv1d."""
    c = CASES[i]
    if x is None:
        x, w, b = inputs(i)
    if c["op"] == "rb":
        return cr.resblock(c["type"], x, c["K"], c["dils"], w, b, 0.1, dt)
    if c["op"].endswith("bf16"):
        x, w = kd.bf16_round(x), kd.bf16_round(w)
    if c["op"].startswith("convt"):
        return cr.convtranspose1d(x, w, b, c["stride"], c["dil"], c["pl"], c["pr"], c["out_pad"], c["groups"], dt, taps)
    return cr.conv1d(x, w, b, c["stride"], c["dil"], c["pl"], c["pr"], c["groups"], dt, taps)
