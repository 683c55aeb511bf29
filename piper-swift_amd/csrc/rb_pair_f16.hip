// rb_pair_f16.hip — two chained ResBlock convs of the HiFi-GAN generator with fp16 operands in ONE kernel:
//     form 1 (ResBlock1 pair, C ∈ {32, 64, 128})       y = x + conv_b(lrelu(conv_a(lrelu x) + b_a)) + b_b      (Piper "high")
//     form 2 (ResBlock2 steps i, i+1, C ∈ {32, 64})    x1 = x + conv_a(lrelu x) + b_a ;  y = x1 + conv_b(lrelu x1) + b_b   ("medium", "low")
// The arithmetic is conv_f16.h's with the rounding points of the two-launch path — lrelu(·) clamped to ±65504 and rounded to nearest
// even into fp16, weights as the scaled fp16 fragment images, v_mfma_f32_32x32x16_f16 into fp32, accumulator · 2^−e, THEN the bias in
// fp32 — so fused equals unfused up to fp32 summation order.
//
// What was chosen, and why:
//   tile      One block = 256 intermediate columns of one batch item = Wo = 256 − 2·pb output columns, pb conv b's true reach (254 / 250 /
//             246 at K = 3 / 7 / 11 against rb_pair_bf16's fixed 224): 9–12 % fewer tiles on the high voice. Every pair of a multi
//             launch has its own Wo; the grid is sized by the narrowest and blocks past a pair's last tile leave at once.
//   waves     (C/32 or C/64) along rows × 4 along columns, two 32-column tiles per wave. At 128 channels a wave owns two row tiles, so a
//             B fragment read from LDS feeds two MFMAs and the block stays at 512 threads; its window (up to 145 KB) allows one block per
//             CU, two waves per SIMD.
//   staging   lrelu(x) of the window (256 + 2·pa columns) is read once from the fp32 stream with aligned float4 loads, clamped, rounded
//             and laid out as one C8 plane [C/8][Wx] of 16-byte entries, zeros outside [0, true length): conv a's zero padding. A lane's
//             B fragment is one ds_read_b128.
//   middle    conv a's result never leaves the CU: scaled, biased, lrelu'd, clamped and rounded in registers into a second C8 plane
//             [C/8][256], zeros outside [0, true length) — conv b's zero padding — plus 32 readable entries that conv b's last, partial
//             column tile runs into (their products land in columns nobody stores).
//   epilogue  The accumulators start at ZERO, not at the bias as in the bf16 kernels: the scale stands between accumulator and bias, and
//             a bias pre-multiplied by 2^e would lose small biases under large e. Scales and biases of both convs wait in LDS ([4][C]
//             floats, loaded under the staging barrier) and are applied as acc · 2^−e + b, conv_f16_kernel's expression.
//   weights   wsrc=l2 at every instance: each wave streams its A fragments from L2 through a register ring eight steps deep, as
//             rb_pair_bf16 does. profiles/f16.md found conv_f16's LDS ring 4–8 % SLOWER where the weights were L2-resident anyway — the
//             L2 reads it saved were not the limit — and the pairs' weights (≤ 22.5 KB per conv at 32 channels, ≤ 352 KB at 128) are
//             L2-resident by the second block. The alternative, a conv's whole fragment set resident in LDS, was weighed for the
//             32-channel instance, the one place where four waves share a row tile: per step a wave already reads two B fragments from
//             LDS for two MFMAs, a third ds_read_b128 for A adds half again to the traffic of the pipe this loop leans on hardest, and
//             both sets at K = 11 (45 KB) beside the 36 KB of planes end the two blocks per CU. It saves what the profile says is not
//             scarce and spends what is. The K-loops hold no block barrier: the kernel has two, one behind each staging phase.
//   x1        Form 2 needs x1 twice: rounded to fp16 as conv b's operand (the middle plane, as in form 1) and in fp32 as conv b's residual,
//             at other lanes than the ones that computed it (conv b's output column c is the intermediate's column c + pb). Split-bf16
//             parks it over its dead x planes (4·C·Wx bytes); one fp16 plane has 2·C·Wx and the Wo ≤ 256 output columns need 4·C·Wo, so it
//             does not fit there. Here conv a's epilogue adds the fp32 x (buffer loads, 0 outside the row), stores the rounded lrelu(x1) to
//             the middle plane and x1 itself to a region of its own behind the epilogue table, [C][Wo] floats sized for Wo = 256
//             (32 / 64 KB), under the barrier the kernel has anyway; conv b's epilogue reads it in the place of form 1's x. At 32
//             channels the block grows from 35 to 67 KB: two per CU where form 1's registers allow three. At 64 channels 134 KB is
//             one block per CU, which is what form 1 has there already (140 registers, 512 threads). The
//             alternative — x1 held in conv a's accumulator registers through conv b's K-loop and exchanged through the dead planes behind
//             two more barriers — costs no LDS and was built for 128 channels, the one count where LDS cannot hold x1 (268 KB): at
//             16·MTW·kNTW = 64 more live registers the instance spilled (448 bytes of scratch per lane at this ring depth, 176 at half, 32
//             with a ring of two steps, where the loop would wait on L2). No instance may use scratch, so form 2 is not eligible at
//             128 channels and that stage keeps the two-launch path; it is the medium voice's shortest row (8·F columns).
//   rows      A row of true length 0 is skipped; a tile entirely past the true length only zeroes its part of `act`.
// Per pair this removes one launch and the round trip of the intermediate's fp16 image through HBM; form 2 also the fp32 x1's.
#include <algorithm>
#include <type_traits>

#include "conv_f16.h"
#include "conv_win.h"

namespace ph {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWN = 4, kNTW = 2;
constexpr int kW1 = 32 * kWN * kNTW;  // intermediate columns per tile
constexpr int kTail = 32;             // readable entries behind the intermediate plane
constexpr int kDA = 8, kDB = 4;       // weight ring / LDS fragment ring depths (steps)
constexpr size_t kLdsMax = 160 * 1024;

__device__ __forceinline__ float clamp_f16(float v) { return __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }
__device__ __forceinline__ unsigned pack2_f16(float a, float b) {
  f16x2 v = {(_Float16)clamp_f16(a), (_Float16)clamp_f16(b)};  // plain casts: round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float lrelu1(float v, float alpha) { return v >= 0.0f ? v : v * alpha; }  // conv_f16.hip's form
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, float v, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}

struct RbPairF16Multi {
  RbPairF16Args c[kWinMulti];
};

// C = 32·MT channels; a wave owns MTW row tiles × kNTW column tiles; the block has (MT / MTW) · kWN waves. FORM: 1 or 2 (header).
template <int MT, int MTW, int FORM>
__global__ __launch_bounds__((MT / MTW) * kWN * 64, 2) void rb_pair_f16_kernel(const RbPairF16Multi multi, const int batch, const int order, const int Wx) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  constexpr int WMB = MT / MTW, BT = WMB * kWN * 64;
  constexpr int C = 32 * MT, CB = C / 8, C16 = C / 16;
  constexpr bool RB2 = FORM == 2;
  const int jz = blockIdx.y / batch;
  const RbPairF16Args& p = multi.c[(order >> (4 * jz)) & 15];  // heaviest pair first
  const int n = blockIdx.y - jz * batch;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave % WMB, wn = wave / WMB;
  const int mt0 = wm * MTW;
  const int r = lane & 31, h = lane >> 5;
  const int pa = (p.Ka - 1) * p.dila / 2, pb = (p.Kb - 1) * p.dilb / 2;
  const int Wo = kW1 - 2 * pb;  // output columns of this pair's tiles
  const int c0 = blockIdx.x * Wo;
  if (c0 >= p.L) return;  // the grid is sized by the launch's narrowest tile
  const int Lv = p.len_ptr ? min(p.len_ptr[n] * p.len_mul, p.L) : p.L;
  if (p.len_ptr && Lv == 0) return;  // a row of length 0 (batched streaming) is read by nobody, its image included
  if (c0 >= Lv) {  // nothing anyone reads — except the activation image, whose "zero past the true length" invariant must hold
    if (p.act) {
      for (int i = threadIdx.x; i < CB * Wo; i += BT) {
        const int cb = i / Wo, g = c0 + (i - cb * Wo);
        if (g < p.L) ((uint4*)p.act)[((int64_t)n * CB + cb) * p.act_row + kC8Halo + g] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  const int g0 = c0 - pb - pa;  // input position read by the first tap of intermediate column 0
  const int ga = g0 & ~3;       // window column 0 (aligned for the float4 loads; L % 4 == 0)
  const int shift = g0 - ga;
  uint4* xs = lds;                                  // lrelu(x) as fp16 C8 [CB][Wx]
  uint4* x1s = lds + CB * Wx;                       // the intermediate as fp16 C8 [CB][kW1], kTail readable entries
  float* epS = (float*)(x1s + CB * kW1 + kTail);    // [4][C]: 2^−e_a, b_a, 2^−e_b, b_b
  float* x1f = epS + 4 * C;                         // form 2: x1 in fp32, [C][Wo]
  for (int i = threadIdx.x; i < 4 * C; i += BT) {
    const int which = i / C, co = i - which * C;
    epS[i] = which == 0 ? p.sa[co] : which == 1 ? p.ba[co] : which == 2 ? p.sb[co] : p.bb[co];
  }
  const float alpha = p.alpha;

  // ---- weight ring (uniform base + 32-bit lane offset); conv a's first steps are requested before the window exists. The ring runs up
  // to kDA − 1 steps past a row tile's last fragment: into the next row tile, or into the image's readable pad (kBf16WeightPad).
  const int Sa = p.Ka * C16, Sb = p.Kb * C16;
  const unsigned lane16 = (unsigned)lane * 16u;
  uint4 a[kDA][MTW];
  const char* wr = nullptr;
  int64_t wtile = 0;
  auto load_a = [&](int slot, int ahead) {
#pragma unroll
    for (int m = 0; m < MTW; m++) a[slot][m] = *(const uint4*)(wr + m * wtile + ahead * 1024 + lane16);
  };
  auto ring_start = [&](const uint16_t* w, int S) {
    wtile = (int64_t)S * 1024;
    wr = (const char*)w + (int64_t)mt0 * wtile;
#pragma unroll
    for (int d = 0; d < kDA - 1; d++) load_a(d, d);
  };
  ring_start(p.wa, Sa);

  // ---- stage lrelu(x) → the plane. item = (channel block, 4 consecutive positions): 8 aligned float4 loads (the block's channel rows),
  // 4 entries written. Two items per thread and pass: 16 loads in flight. Loads are clamped and unconditional, stores masked.
  {
    const float* xb = p.x + (int64_t)n * C * p.L;
    const int W4 = Wx >> 2, items = CB * W4;
    for (int base = threadIdx.x; base < items; base += 2 * BT) {
      float4 t[2][8];
      int dst[2], nv[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int i = base + u * BT;
        const int ic = min(i, items - 1);
        const int cb = ic / W4, p4 = ic - cb * W4;
        const int pos = ga + 4 * p4;
        const bool inb = pos >= 0 && pos < p.L;
        nv[u] = inb ? Lv - pos : 0;
        dst[u] = i < items ? cb * Wx + 4 * p4 : -1;
#pragma unroll
        for (int e = 0; e < 8; e++) t[u][e] = *(const float4*)(xb + (int64_t)(cb * 8 + e) * p.L + (inb ? pos : 0));
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (dst[u] < 0) continue;
        const float* f = (const float*)&t[u][0];  // f[4·e + k]: channel e, position k
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint4 o;
          o.x = pack2_f16(lrelu1(f[0 + k], alpha), lrelu1(f[4 + k], alpha));
          o.y = pack2_f16(lrelu1(f[8 + k], alpha), lrelu1(f[12 + k], alpha));
          o.z = pack2_f16(lrelu1(f[16 + k], alpha), lrelu1(f[20 + k], alpha));
          o.w = pack2_f16(lrelu1(f[24 + k], alpha), lrelu1(f[28 + k], alpha));
          if (nv[u] <= k) o = make_uint4(0u, 0u, 0u, 0u);
          xs[dst[u] + k] = o;
        }
      }
    }
  }
  __syncthreads();

  // ---- one conv over this wave's tiles: B fragments by ds_read_b128 from a C8 plane [CB][Wrow], A through the ring; fp32 from zero
  f32x16 acc[MTW][kNTW];
  auto run_conv = [&](auto nt_tag, const uint4* img, const int Wrow, const int S, const int dil, const int col0) {
    constexpr int NT = decltype(nt_tag)::value;
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < kNTW; j++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[m][j][q] = 0.0f;
    const int lbase = h * Wrow + col0 + r;
    uint4 b[kDB][NT];
    int sidx = 0, c_n = 0, left = S - 1;  // step = tap·C16 + c16: the scalar part of the index, 2·c16·Wrow + tap·dil
    const int wrap_delta = dil - 2 * Wrow * (C16 - 1);
    auto read_b = [&](int slot) {
      const int idx = lbase + sidx;
#pragma unroll
      for (int j = 0; j < NT; j++) b[slot][j] = img[idx + 32 * j];
      c_n++;
      const bool wrap = c_n == C16;
      c_n = wrap ? 0 : c_n;
      const int delta = wrap ? wrap_delta : 2 * Wrow;
      sidx += left > 0 ? delta : 0;  // stops after the last step: the ring never reads outside the plane and its tail
      left--;
    };
    auto step = [&](int u) {
      load_a((u + kDA - 1) % kDA, kDA - 1 + u);
      read_b((u + kDB - 1) % kDB);
      __builtin_amdgcn_sched_barrier(0);  // ring load and the LDS read stay ahead of this step's MFMAs
#pragma unroll
      for (int m = 0; m < MTW; m++)
#pragma unroll
        for (int j = 0; j < NT; j++)
          acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[u][m]), __builtin_bit_cast(f16x8, b[u % kDB][j]), acc[m][j], 0, 0,
                                                             0);
    };
#pragma unroll
    for (int d = 0; d < kDB - 1; d++) read_b(d);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): clean state for the loop's counted waits
    const int full = S / kDA;
    for (int g = 0; g < full; g++) {
#pragma unroll
      for (int u = 0; u < kDA; u++) step(u);
      wr += kDA * 1024;
    }
    const int rem = S - full * kDA;
#pragma unroll
    for (int u = 0; u < kDA - 1; u++)
      if (u < rem) step(u);
  };
  // acc · 2^−e + b for the 4 consecutive rows of register group g4 (register q of lane (r,h): row (q&3) + 8·(q>>2) + 4·h)
  auto scale_bias = [&](const f32x16& c, int which, int row0, int g4, float (&v)[4]) {
    const float4 sc = *(const float4*)(epS + (2 * which) * C + row0 + 8 * g4);
    const float4 bi = *(const float4*)(epS + (2 * which + 1) * C + row0 + 8 * g4);
    v[0] = c[4 * g4] * sc.x + bi.x; v[1] = c[4 * g4 + 1] * sc.y + bi.y;  // × 2^−e is exact; no contraction (-ffp-contract=off)
    v[2] = c[4 * g4 + 2] * sc.z + bi.z; v[3] = c[4 * g4 + 3] * sc.w + bi.w;
  };

  // ======== conv a: intermediate columns [c0 − pb, c0 − pb + 256)
  run_conv(std::integral_constant<int, kNTW>{}, xs, Wx, Sa, p.dila, shift + wn * kNTW * 32);
  ring_start(p.wb, Sb);  // conv b's ring: lands behind the epilogue and the barrier
#pragma unroll
  for (int m = 0; m < MTW; m++)
#pragma unroll
    for (int j = 0; j < kNTW; j++) {
      const int colw = (wn * kNTW + j) * 32 + r;
      const int g = c0 - pb + colw;
      const bool in = g >= 0 && g < Lv;  // zero outside [0, true length): conv b's zero padding
      f32x16 x1;
      if constexpr (RB2) {  // the residual of conv a: x at the intermediate's columns, 0 outside the row
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (int64_t)n * C * p.L), 0, C * p.L * 4, 0x00020000);
        const int voff = (g >= 0 && g < p.L) ? (((mt0 + m) * 32 + 4 * h) * p.L + g) * 4 : -4;
#pragma unroll
        for (int q = 0; q < 16; q++) x1[q] = bload(rx, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {  // a lane holds 4 consecutive channels of one column: 8 bytes of an entry
        float v[4];
        scale_bias(acc[m][j], 0, (mt0 + m) * 32 + 4 * h, g4, v);
        if constexpr (RB2) {  // x1 = (acc · 2^−e_a + b_a) + x in fp32; only conv b's operand below is rounded
#pragma unroll
          for (int i = 0; i < 4; i++) x1[4 * g4 + i] = v[i] = v[i] + x1[4 * g4 + i];
        }
        uint2 o;
        o.x = in ? pack2_f16(lrelu1(v[0], alpha), lrelu1(v[1], alpha)) : 0u;
        o.y = in ? pack2_f16(lrelu1(v[2], alpha), lrelu1(v[3], alpha)) : 0u;
        ((uint2*)(x1s + ((mt0 + m) * 4 + g4) * kW1 + colw))[h] = o;
      }
      if constexpr (RB2) {  // the output columns' x1 → x1f: the lane that owns a column here is not the one that adds it below
        const int colo = colw - pb;
        if (colo >= 0 && colo < Wo) {
#pragma unroll
          for (int q = 0; q < 16; q++) x1f[((mt0 + m) * 32 + 4 * h + (q & 3) + 8 * (q >> 2)) * Wo + colo] = x1[q];
        }
      }
    }
  __syncthreads();

  // ======== conv b: ⌈Wo/32⌉ output column tiles, two per wave column (the last wave columns get one or none)
  const int ntb = min(max(((Wo + 31) >> 5) - wn * kNTW, 0), kNTW);  // wave-uniform
  if (ntb == 0) return;
  if (ntb == 2) run_conv(std::integral_constant<int, 2>{}, x1s, kW1, Sb, p.dilb, wn * kNTW * 32);
  else run_conv(std::integral_constant<int, 1>{}, x1s, kW1, Sb, p.dilb, wn * kNTW * 32);

  {  // y = (acc · 2^−e_b + b_b) + x (form 2: + x1) → fp32; optionally the C8 image of lrelu(y) for a conv that is not fused
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (int64_t)n * C * p.L), 0, C * p.L * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y ? p.y + (int64_t)n * C * p.L : nullptr), 0, p.y ? C * p.L * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rma = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mrf_a ? p.mrf_a + (int64_t)n * C * p.L : nullptr), 0, p.mrf_a ? C * p.L * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rmb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mrf_b ? p.mrf_b + (int64_t)n * C * p.L : nullptr), 0, p.mrf_b ? C * p.L * 4 : 0, 0x00020000);
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < kNTW; j++) {
        if (j >= ntb) break;
        const int colo = (wn * kNTW + j) * 32 + r;
        const int g = c0 + colo;
        const int rowl = (mt0 + m) * 32 + 4 * h;
        const bool ok = colo < Wo && g < p.L;
        const int voff = ok ? (rowl * p.L + g) * 4 : -4;  // −4: out of range ⇒ loads give 0, stores are dropped
        float xr[16];
#pragma unroll
        for (int q = 0; q < 16; q++)
          xr[q] = RB2 ? x1f[(rowl + (q & 3) + 8 * (q >> 2)) * Wo + min(colo, Wo - 1)] : bload(rx, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
        float v[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          float t[4];
          scale_bias(acc[m][j], 1, rowl, g4, t);
#pragma unroll
          for (int i = 0; i < 4; i++) v[4 * g4 + i] = t[i] + xr[4 * g4 + i];
        }
        if (p.mrf_a) {  // ((mrf_a + mrf_b) + v) / 3: the association of the graph's Add, Add, Div
          float ta[16], tb[16];
#pragma unroll
          for (int q = 0; q < 16; q++) {
            ta[q] = bload(rma, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
            tb[q] = bload(rmb, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
          }
#pragma unroll
          for (int q = 0; q < 16; q++) v[q] = ((ta[q] + tb[q]) + v[q]) / 3.0f;
        }
#pragma unroll
        for (int q = 0; q < 16; q++) bstore(ry, v[q], voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);  // no y: zero-sized descriptor, stores dropped
        if (p.act && ok) {
          const bool live = g < Lv;  // past the true length the image must hold zeros
#pragma unroll
          for (int g4 = 0; g4 < 4; g4++) {
            uint2 o;
            o.x = live ? pack2_f16(lrelu1(v[4 * g4], alpha), lrelu1(v[4 * g4 + 1], alpha)) : 0u;
            o.y = live ? pack2_f16(lrelu1(v[4 * g4 + 2], alpha), lrelu1(v[4 * g4 + 3], alpha)) : 0u;
            ((uint2*)((uint4*)p.act + ((int64_t)n * CB + (mt0 + m) * 4 + g4) * p.act_row + kC8Halo + g))[h] = o;
          }
        }
      }
  }
}

struct PairGeom {
  int Wx;
  size_t lds;
};
// x window: 256 + 2·pa columns, up to 3 more in front for the float4 alignment, rounded up to whole float4s; form 2: the fp32 x1 of up to
// 256 output columns behind the epilogue table
PairGeom pair_geom(int C, int pa_max, int form) {
  PairGeom g;
  g.Wx = (kW1 + 2 * pa_max + 3 + 3) & ~3;
  g.lds = ((size_t)(C / 8) * (g.Wx + kW1) + kTail) * 16 + (size_t)4 * C * sizeof(float);
  if (form == 2) g.lds += (size_t)C * kW1 * sizeof(float);
  return g;
}

template <int MT, int MTW, int FORM>
void launch_inst(hipStream_t s, const RbPairF16Multi& m, int batch, int order, const PairGeom& g, dim3 grid) {
  static bool raised[kMaxDevices] = {};
  if (g.lds > 64 * 1024 && lds_optin_needed(raised))
    (void)hipFuncSetAttribute((const void*)rb_pair_f16_kernel<MT, MTW, FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
  hipLaunchKernelGGL((rb_pair_f16_kernel<MT, MTW, FORM>), grid, dim3((MT / MTW) * kWN * 64), g.lds, s, m, batch, order, g.Wx);
}
template <int MT, int MTW>
void launch_form(int form, hipStream_t s, const RbPairF16Multi& m, int batch, int order, const PairGeom& g, dim3 grid) {
  if (form == 2) launch_inst<MT, MTW, 2>(s, m, batch, order, g, grid);
  else launch_inst<MT, MTW, 1>(s, m, batch, order, g, grid);
}

}  // namespace

bool rb_pair_f16_eligible(int C, int Ka, int dila, int Kb, int dilb, int L, int form) {
  if (C != 32 && C != 64 && C != 128) return false;
  if (form != 1 && !(form == 2 && C <= 64)) return false;  // form 2 at 128 channels: header, "x1"
  if (Ka < 1 || Kb < 1 || !(Ka & 1) || !(Kb & 1) || dila < 1 || dilb < 1 || L < 4 || (L & 3)) return false;
  if ((int64_t)(Ka - 1) * dila / 2 > kC8Halo || (int64_t)(Kb - 1) * dilb / 2 > kC8Halo) return false;  // pb ≤ 64: Wo ≥ 128
  if ((int64_t)C * L * 4 >= (int64_t)1 << 31) return false;  // 32-bit byte offsets into one item
  return pair_geom(C, (Ka - 1) * dila / 2, form).lds <= kLdsMax;
}

int launch_rb_pair_f16_multi(piper_hip_ctx* ctx, hipStream_t s, const RbPairF16Args* pairs, int count) {
  if (count < 1 || count > kWinMulti) PH_FAIL(PIPER_HIP_ERR_ARG, "rb_pair_f16: %d pairs in one launch (1..%d)", count, kWinMulti);
  const RbPairF16Args& a = pairs[0];
  if (a.N <= 0 || a.L <= 0) return PIPER_HIP_OK;
  int pa_max = 0, pb_max = 0, idx[kWinMulti] = {0, 1, 2};
  for (int i = 0; i < count; i++) {
    const RbPairF16Args& b = pairs[i];
    if (b.N != a.N || b.C != a.C || b.L != a.L || b.form != a.form)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "rb_pair_f16: pairs of one launch must share N, C, L and form");
    if (!rb_pair_f16_eligible(b.C, b.Ka, b.dila, b.Kb, b.dilb, b.L, b.form))
      PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "rb_pair_f16: geometry not covered (C=%d K=%d,%d d=%d,%d L=%d form=%d)", b.C, b.Ka, b.Kb, b.dila, b.dilb, b.L, b.form);
    if (!b.x || (!b.y && !b.act) || b.x == b.y || !b.wa || !b.wb || !b.sa || !b.sb || !b.ba || !b.bb || (!b.mrf_a != !b.mrf_b) ||
        (b.act && b.act_row < kC8Halo + b.L))
      PH_FAIL(PIPER_HIP_ERR_ARG, "rb_pair_f16: null or aliased operand");
    pa_max = std::max(pa_max, (b.Ka - 1) * b.dila / 2);
    pb_max = std::max(pb_max, (b.Kb - 1) * b.dilb / 2);
  }
  const PairGeom g = pair_geom(a.C, pa_max, a.form);
  if (g.lds > kLdsMax) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "rb_pair_f16: window of %zu bytes exceeds LDS", g.lds);
  std::sort(idx, idx + count, [&](int l, int r2) { return pairs[l].Ka + pairs[l].Kb > pairs[r2].Ka + pairs[r2].Kb; });
  int order = 0;
  for (int i = 0; i < count; i++) order |= idx[i] << (4 * i);
  RbPairF16Multi m;
  for (int i = 0; i < kWinMulti; i++) m.c[i] = pairs[i < count ? i : 0];
  // each pair's tiles are sized by its own conv b; the grid by the narrowest, blocks past a pair's last tile leave at once
  const dim3 grid((unsigned)ceil_div(a.L, kW1 - 2 * pb_max), (unsigned)(a.N * count));
  if (a.C == 32) launch_form<1, 1>(a.form, s, m, a.N, order, g, grid);
  else if (a.C == 64) launch_form<2, 1>(a.form, s, m, a.N, order, g, grid);
  else launch_inst<4, 2, 1>(s, m, a.N, order, g, grid);
  for (int i = 0; i < count; i++) {
    const RbPairF16Args& b = pairs[i];
    if (a.form == 2)
      PH_ROUTE(ctx, b.C, b.C, b.L, b.N, "rb_pair_f16 MT=%d MTW=%d form=2 Ka=%d da=%d Kb=%d db=%d W1=%d wsrc=l2 multi=%d conv", a.C / 32, a.C == 128 ? 2 : 1, b.Ka,
               b.dila, b.Kb, b.dilb, kW1, count);
    else
      PH_ROUTE(ctx, b.C, b.C, b.L, b.N, "rb_pair_f16 MT=%d MTW=%d Ka=%d da=%d Kb=%d db=%d W1=%d wsrc=l2 multi=%d conv", a.C / 32, a.C == 128 ? 2 : 1, b.Ka, b.dila,
               b.Kb, b.dilb, kW1, count);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "rb_pair_f16 launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(rb_pair_f16, (rb_pair_f16_kernel<1, 1, 1>)); } }
