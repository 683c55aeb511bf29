// rb_pair_bf16x3.hip — two chained ResBlock convs of the HiFi-GAN generator with SPLIT bf16 operands in ONE kernel, C ∈ {32, 64}:
//     form 2 (ResBlock2 steps i, i+1)   x1 = x + conv_a(lrelu x) + b_a ;  y = x1 + conv_b(lrelu x1) + b_b        (any dilations)
//     form 1 (ResBlock1 pair)           y = x + conv_b(lrelu(conv_a(lrelu x) + b_a)) + b_b
// The arithmetic is conv_bf16x3.h's — every contraction is W_lo·X_hi + W_hi·X_lo + W_hi·X_hi into one fp32 accumulator that starts at
// the bias — with the rounding points of the two-launch path, so fused equals unfused up to fp32 summation order.
//
// One block = a tile of kW1 = 256 intermediate columns of one batch item = Wo = 256 − 2·pb output columns (pb = conv b's true reach each
// side); C/32 waves along rows × 4 along columns, a wave owns one 32-row tile × two 32-column tiles.
//   1. lrelu(x) of the tile's window (256 + 2·pa columns) is read ONCE from the fp32 stream, split, and laid into LDS as two C8 planes
//      [C/8][Wx] of 16-byte entries, zeros outside [0, true length): conv a's zero padding;
//   2. conv a: A_hi / A_lo fragments from L2 through two register rings, B_hi / B_lo by ds_read_b128 from the planes, three MFMAs per
//      tile and step issued term-major (conv_bf16x3_kernel's order). Its epilogue (form 2: + the fp32 x) splits lrelu(result) in
//      registers into a second pair of planes [C/8][256], zeros outside [0, true length): conv b's zero padding;
//   3. form 2 keeps x1 in fp32 for conv b's residual add. It does not get LDS of its own: once every wave has left conv a's K-loop
//      the x planes are dead, and the Wo output columns of x1, C·Wo·4 bytes, always fit in their 4·C·Wx bytes. One more barrier;
//   4. conv b over ⌈Wo/32⌉ column tiles from the second pair of planes; epilogue: + x1 (LDS) or + x (HBM), MRF mean, fp32 store and,
//      for a consumer that is not fused, both planes of lrelu(y) in HBM, zeros past the true length.
// Per pair and element this moves 8 bytes of the fp32 stream where the two-launch path moves 32 (two planes in, the residual in, the
// stream and two planes out, twice).
#include <algorithm>
#include <type_traits>

#include "conv_bf16x3.h"
#include "conv_win.h"

namespace ph {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWN = 4, kNTW = 2;
constexpr int kW1 = 32 * kWN * kNTW;  // intermediate columns per tile
constexpr int kTail = 32;             // readable entries behind the second pair of planes: conv b's last, partial column tile reads < 32 past it
constexpr int kDA = 4, kDB = 4;       // weight rings / LDS fragment rings, in steps
constexpr int kMaxReach = 64;         // pa, pb ≤ 64: Wo ≥ 128
constexpr size_t kLdsMax = 160 * 1024;

__device__ __forceinline__ unsigned pack2(float a, float b) {
  bf16x2 v = {(__bf16)a, (__bf16)b};  // v_cvt_pk_bf16_f32, round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
// conv_bf16x3.hip's split: hi = bf16(a), lo = bf16(a − hi) with the exact fp32 residual
__device__ __forceinline__ unsigned split2(float a, float b, unsigned& lo) {
  const unsigned hi = pack2(a, b);
  lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
  return hi;
}
__device__ __forceinline__ float lrelu1(float v, float alpha) { return v >= 0.0f ? v : v * alpha; }
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, float v, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}

struct RbPairX3Multi {
  RbPairBf16Args c[kWinMulti];
};

// C = 32·MT channels, MT · kWN waves; RB2: form 2
template <int MT, bool RB2>
__global__ __launch_bounds__(MT * kWN * 64, 2) void rb_pair_bf16x3_kernel(const RbPairX3Multi multi, const int batch, const int order, const int Wx) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  constexpr int BT = MT * kWN * 64;
  constexpr int C = 32 * MT, CB = C / 8, C16 = C / 16;
  const int jz = blockIdx.y / batch;
  const RbPairBf16Args& p = multi.c[(order >> (4 * jz)) & 15];  // heaviest pair first
  const int n = blockIdx.y - jz * batch;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave % MT, wn = wave / MT;
  const int r = lane & 31, h = lane >> 5;
  const int pa = (p.Ka - 1) * p.dila / 2, pb = (p.Kb - 1) * p.dilb / 2;
  const int Wo = kW1 - 2 * pb;  // output columns of this pair's tiles
  const int c0 = blockIdx.x * Wo;
  if (c0 >= p.L) return;  // the grid is sized by the launch's narrowest tile
  const int Lv = p.len_ptr ? min(p.len_ptr[n] * p.len_mul, p.L) : p.L;
  if (p.len_ptr && Lv == 0) return;  // a row of length 0 (batched streaming) is read by nobody, its image included
  const int64_t aplane = (int64_t)batch * CB * p.act_row;  // entries from the hi plane of the output image to its lo plane
  if (c0 >= Lv) {  // nothing anyone reads — except the activation image, whose "zero past the true length" invariant must hold
    if (p.act) {
      for (int i = threadIdx.x; i < CB * Wo; i += BT) {
        const int cb = i / Wo, g = c0 + (i - cb * Wo);
        if (g < p.L) {
          uint4* slot = (uint4*)p.act + ((int64_t)n * CB + cb) * p.act_row + kC8Halo + g;
          slot[0] = make_uint4(0u, 0u, 0u, 0u);
          slot[aplane] = make_uint4(0u, 0u, 0u, 0u);
        }
      }
    }
    return;
  }
  const int g0 = c0 - pb - pa;  // input position read by the first tap of intermediate column 0
  const int ga = g0 & ~3;       // window column 0 (aligned for the float4 loads; L % 4 == 0)
  const int shift = g0 - ga;
  uint4* xs = lds;                              // lrelu(x): hi [CB][Wx], lo [CB][Wx]
  uint4* x1s = lds + 2 * CB * Wx;               // the intermediate: hi [CB][kW1], lo [CB][kW1], kTail readable entries
  float* biasS = (float*)(x1s + 2 * CB * kW1 + kTail);  // [2][C]
  float* x1f = (float*)lds;                     // form 2: fp32 x1 [C][Wo] over the dead x planes
  for (int i = threadIdx.x; i < 2 * C; i += BT) biasS[i] = i < C ? p.ba[i] : p.bb[i - C];
  const float alpha = p.alpha;

  // ---- weight rings, one per image (uniform base + 32-bit lane offset). The lo image lies MT row tiles and the pad behind the hi image
  // (pack_conv_weights_bf16x3); each image's pad covers the rings' run past the last step.
  const int Sa = p.Ka * C16, Sb = p.Kb * C16;
  const unsigned lane16 = (unsigned)lane * 16u;
  uint4 ah[kDA], al[kDA];
  const char *wh = nullptr, *wl = nullptr;
  auto load_a = [&](int slot, int ahead) {
    ah[slot] = *(const uint4*)(wh + ahead * 1024 + lane16);
    al[slot] = *(const uint4*)(wl + ahead * 1024 + lane16);
  };
  auto ring_start = [&](const uint16_t* w, int S) {
    const int64_t wtile = (int64_t)S * 1024;
    wh = (const char*)w + (int64_t)wm * wtile;
    wl = wh + (int64_t)MT * wtile + (int64_t)kBf16WeightPad * 2;
#pragma unroll
    for (int d = 0; d < kDA - 1; d++) load_a(d, d);
  };
  ring_start(p.wa, Sa);  // in flight before the window exists

  // ---- stage lrelu(x) → both planes. item = (channel block, 4 consecutive positions): 8 aligned float4 loads (the block's channel
  // rows), 4 entries per plane. Two items per thread and pass: 16 loads in flight. Loads are clamped and unconditional, stores masked.
  {
    const float* xb = p.x + (int64_t)n * C * p.L;
    uint4* xlo = xs + CB * Wx;
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
          uint4 hi, lo;
          hi.x = split2(lrelu1(f[0 + k], alpha), lrelu1(f[4 + k], alpha), lo.x);
          hi.y = split2(lrelu1(f[8 + k], alpha), lrelu1(f[12 + k], alpha), lo.y);
          hi.z = split2(lrelu1(f[16 + k], alpha), lrelu1(f[20 + k], alpha), lo.z);
          hi.w = split2(lrelu1(f[24 + k], alpha), lrelu1(f[28 + k], alpha), lo.w);
          if (nv[u] <= k) hi = lo = make_uint4(0u, 0u, 0u, 0u);
          xs[dst[u] + k] = hi;
          xlo[dst[u] + k] = lo;
        }
      }
    }
  }
  __syncthreads();

  // ---- one conv over this wave's tiles: B fragments by ds_read_b128 from a pair of planes [2][CB][Wrow], A through the rings
  f32x16 acc[kNTW];
  auto run_conv = [&](auto nt_tag, const uint4* img, const int Wrow, const int S, const int dil, const int col0, const int bias_off) {
    constexpr int NT = decltype(nt_tag)::value;
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {  // accumulators start at the bias; register q of lane (r,h): row (q&3) + 8·(q>>2) + 4·h
      const float4 bv = *(const float4*)(biasS + bias_off + wm * 32 + 4 * h + 8 * g4);
#pragma unroll
      for (int j = 0; j < kNTW; j++) { acc[j][4 * g4] = bv.x; acc[j][4 * g4 + 1] = bv.y; acc[j][4 * g4 + 2] = bv.z; acc[j][4 * g4 + 3] = bv.w; }
    }
    const int PW = CB * Wrow;  // entries from the hi plane to the lo plane
    const int lbase = h * Wrow + col0 + r;
    uint4 bh[kDB][NT], bl[kDB][NT];
    int sidx = 0, c_n = 0, left = S - 1;  // step = tap·C16 + c16: the scalar part of the index, 2·c16·Wrow + tap·dil
    const int wrap_delta = dil - 2 * Wrow * (C16 - 1);
    auto read_b = [&](int slot) {
      const int idx = lbase + sidx;
#pragma unroll
      for (int j = 0; j < NT; j++) {
        bh[slot][j] = img[idx + 32 * j];
        bl[slot][j] = img[idx + PW + 32 * j];
      }
      c_n++;
      const bool wrap = c_n == C16;
      c_n = wrap ? 0 : c_n;
      const int delta = wrap ? wrap_delta : 2 * Wrow;
      sidx += left > 0 ? delta : 0;  // stops after the last step: the ring never reads outside the planes
      left--;
    };
    auto mfma = [&](const uint4& a, const uint4& b, f32x16 c) {
      return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    };
    auto step = [&](int u) {
      load_a((u + kDA - 1) % kDA, kDA - 1 + u);
      __builtin_amdgcn_sched_barrier(0);  // keep the rings' loads at the top of their step
      read_b((u + kDB - 1) % kDB);
      const int v = u % kDB;
      // term-major: with two tiles no MFMA waits on the accumulator just written, and each tile's small terms enter before its large one
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j] = mfma(al[u], bh[v][j], acc[j]);  // W_lo · X_hi
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j] = mfma(ah[u], bl[v][j], acc[j]);  // W_hi · X_lo
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j] = mfma(ah[u], bh[v][j], acc[j]);  // W_hi · X_hi
    };
#pragma unroll
    for (int d = 0; d < kDB - 1; d++) read_b(d);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): clean state for the loop's counted waits
    const int full = S / kDA;
    for (int g = 0; g < full; g++) {
#pragma unroll
      for (int u = 0; u < kDA; u++) step(u);
      wh += kDA * 1024;
      wl += kDA * 1024;
    }
    const int rem = S - full * kDA;
#pragma unroll
    for (int u = 0; u < kDA - 1; u++)
      if (u < rem) step(u);
  };

  const int rowl = wm * 32 + 4 * h;  // row of accumulator register 0; register q: + (q&3) + 8·(q>>2)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (int64_t)n * C * p.L), 0, C * p.L * 4, 0x00020000);

  // ======== conv a: intermediate columns [c0 − pb, c0 − pb + 256)
  run_conv(std::integral_constant<int, kNTW>{}, xs, Wx, Sa, p.dila, shift + wn * kNTW * 32, 0);
  ring_start(p.wb, Sb);  // conv b's rings: they land behind the epilogue and the barriers
#pragma unroll
  for (int j = 0; j < kNTW; j++) {
    const int colw = (wn * kNTW + j) * 32 + r;
    const int g = c0 - pb + colw;
    if (RB2) {  // x1 = x + conv_a + b_a, in fp32
      const int voff = (g >= 0 && g < p.L) ? (rowl * p.L + g) * 4 : -4;  // −4: out of range ⇒ the load gives 0
      float xr[16];
#pragma unroll
      for (int q = 0; q < 16; q++) xr[q] = bload(rx, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
#pragma unroll
      for (int q = 0; q < 16; q++) acc[j][q] += xr[q];
    }
    // lrelu(intermediate), split, zero outside [0, true length); a lane holds 4 consecutive channels of one column: 8 bytes per plane
    const bool in = g >= 0 && g < Lv;
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      uint2 oh, ol;
      oh.x = split2(lrelu1(acc[j][4 * g4], alpha), lrelu1(acc[j][4 * g4 + 1], alpha), ol.x);
      oh.y = split2(lrelu1(acc[j][4 * g4 + 2], alpha), lrelu1(acc[j][4 * g4 + 3], alpha), ol.y);
      if (!in) oh = ol = make_uint2(0u, 0u);
      uint4* slot = x1s + (wm * 4 + g4) * kW1 + colw;
      ((uint2*)slot)[h] = oh;
      ((uint2*)(slot + CB * kW1))[h] = ol;
    }
  }
  if (RB2) {
    __syncthreads();  // every wave has left conv a's K-loop: the x planes are dead
#pragma unroll
    for (int j = 0; j < kNTW; j++) {
      const int colo = (wn * kNTW + j) * 32 + r - pb;
      if (colo >= 0 && colo < Wo) {
#pragma unroll
        for (int q = 0; q < 16; q++) x1f[(rowl + (q & 3) + 8 * (q >> 2)) * Wo + colo] = acc[j][q];
      }
    }
  }
  __syncthreads();

  // ======== conv b: ⌈Wo/32⌉ output column tiles, two per wave column (the last wave columns get one or none)
  const int ntb = min(max(((Wo + 31) >> 5) - wn * kNTW, 0), kNTW);  // wave-uniform
  if (ntb == 0) return;
  if (ntb == 2) run_conv(std::integral_constant<int, 2>{}, x1s, kW1, Sb, p.dilb, wn * kNTW * 32, C);
  else run_conv(std::integral_constant<int, 1>{}, x1s, kW1, Sb, p.dilb, wn * kNTW * 32, C);

  {  // y = residual + acc (bias inside) → fp32; optionally both planes of lrelu(y) for a conv that is not fused
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y ? p.y + (int64_t)n * C * p.L : nullptr), 0, p.y ? C * p.L * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rma = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mrf_a ? p.mrf_a + (int64_t)n * C * p.L : nullptr), 0, p.mrf_a ? C * p.L * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rmb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mrf_b ? p.mrf_b + (int64_t)n * C * p.L : nullptr), 0, p.mrf_b ? C * p.L * 4 : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < kNTW; j++) {
      if (j >= ntb) break;
      const int colo = (wn * kNTW + j) * 32 + r;
      const int g = c0 + colo;
      const bool ok = colo < Wo && g < p.L;
      const int voff = ok ? (rowl * p.L + g) * 4 : -4;  // −4: out of range ⇒ loads give 0, stores are dropped
      float xr[16];
#pragma unroll
      for (int q = 0; q < 16; q++)
        xr[q] = RB2 ? x1f[(rowl + (q & 3) + 8 * (q >> 2)) * Wo + min(colo, Wo - 1)] : bload(rx, voff, ((q & 3) + 8 * (q >> 2)) * p.L * 4);
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) v[q] = acc[j][q] + xr[q];
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
        const bool live = g < Lv;  // past the true length both planes must hold zeros
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          uint2 oh, ol;
          oh.x = split2(lrelu1(v[4 * g4], alpha), lrelu1(v[4 * g4 + 1], alpha), ol.x);
          oh.y = split2(lrelu1(v[4 * g4 + 2], alpha), lrelu1(v[4 * g4 + 3], alpha), ol.y);
          if (!live) oh = ol = make_uint2(0u, 0u);
          uint4* slot = (uint4*)p.act + ((int64_t)n * CB + wm * 4 + g4) * p.act_row + kC8Halo + g;
          ((uint2*)slot)[h] = oh;
          ((uint2*)(slot + aplane))[h] = ol;
        }
      }
    }
  }
}

struct PairGeom {
  int Wx;
  size_t lds;
};
// x window: 256 + 2·pa columns, up to 3 more in front for the float4 alignment, rounded up to whole float4s
PairGeom pair_geom(int C, int pa_max) {
  PairGeom g;
  g.Wx = (kW1 + 2 * pa_max + 3 + 3) & ~3;
  g.lds = ((size_t)2 * (C / 8) * (g.Wx + kW1) + kTail) * 16 + (size_t)2 * C * sizeof(float);
  return g;
}

template <int MT, bool RB2>
void launch_inst(hipStream_t s, const RbPairX3Multi& m, int batch, int order, const PairGeom& g, dim3 grid) {
  static bool raised[kMaxDevices] = {};
  if (g.lds > 64 * 1024 && lds_optin_needed(raised))
    (void)hipFuncSetAttribute((const void*)rb_pair_bf16x3_kernel<MT, RB2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
  hipLaunchKernelGGL((rb_pair_bf16x3_kernel<MT, RB2>), grid, dim3(MT * kWN * 64), g.lds, s, m, batch, order, g.Wx);
}

}  // namespace

bool rb_pair_bf16x3_eligible(int C, int Ka, int dila, int Kb, int dilb, int L, int form) {
  if (C != 32 && C != 64) return false;
  if (form != 1 && form != 2) return false;
  if (Ka < 1 || Kb < 1 || !(Ka & 1) || !(Kb & 1) || dila < 1 || dilb < 1 || L < 4 || (L & 3)) return false;
  if ((int64_t)(Ka - 1) * dila / 2 > kMaxReach || (int64_t)(Kb - 1) * dilb / 2 > kMaxReach) return false;
  if ((int64_t)C * L * 4 >= (int64_t)1 << 31) return false;  // 32-bit byte offsets into one item
  return pair_geom(C, (Ka - 1) * dila / 2).lds <= kLdsMax;
}

int launch_rb_pair_bf16x3_multi(piper_hip_ctx* ctx, hipStream_t s, const RbPairBf16Args* pairs, int count) {
  if (count < 1 || count > kWinMulti) PH_FAIL(PIPER_HIP_ERR_ARG, "rb_pair_bf16x3: %d pairs in one launch (1..%d)", count, kWinMulti);
  const RbPairBf16Args& a = pairs[0];
  if (a.N <= 0 || a.L <= 0) return PIPER_HIP_OK;
  int pa_max = 0, pb_max = 0, idx[kWinMulti] = {0, 1, 2};
  for (int i = 0; i < count; i++) {
    const RbPairBf16Args& b = pairs[i];
    if (b.N != a.N || b.C != a.C || b.L != a.L || b.form != a.form)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "rb_pair_bf16x3: pairs of one launch must share N, C, L and form");
    if (!rb_pair_bf16x3_eligible(b.C, b.Ka, b.dila, b.Kb, b.dilb, b.L, b.form))
      PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "rb_pair_bf16x3: geometry not covered (C=%d K=%d,%d d=%d,%d L=%d form=%d)", b.C, b.Ka, b.Kb, b.dila, b.dilb, b.L,
              b.form);
    if (!b.x || (!b.y && !b.act) || b.x == b.y || !b.wa || !b.wb || !b.ba || !b.bb || (!b.mrf_a != !b.mrf_b) || (b.act && b.act_row < kC8Halo + b.L))
      PH_FAIL(PIPER_HIP_ERR_ARG, "rb_pair_bf16x3: null or aliased operand");
    pa_max = std::max(pa_max, (b.Ka - 1) * b.dila / 2);
    pb_max = std::max(pb_max, (b.Kb - 1) * b.dilb / 2);
  }
  const PairGeom g = pair_geom(a.C, pa_max);
  if (g.lds > kLdsMax) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "rb_pair_bf16x3: window of %zu bytes exceeds LDS", g.lds);
  std::sort(idx, idx + count, [&](int l, int r2) { return pairs[l].Ka + pairs[l].Kb > pairs[r2].Ka + pairs[r2].Kb; });
  int order = 0;
  for (int i = 0; i < count; i++) order |= idx[i] << (4 * i);
  RbPairX3Multi m;
  for (int i = 0; i < kWinMulti; i++) m.c[i] = pairs[i < count ? i : 0];
  // each pair's tiles are sized by its own conv b; the grid by the narrowest, blocks past a pair's last tile leave at once
  const dim3 grid((unsigned)ceil_div(a.L, kW1 - 2 * pb_max), (unsigned)(a.N * count));
  const bool rb2 = a.form == 2;
  if (a.C == 32) { if (rb2) launch_inst<1, true>(s, m, a.N, order, g, grid); else launch_inst<1, false>(s, m, a.N, order, g, grid); }
  else { if (rb2) launch_inst<2, true>(s, m, a.N, order, g, grid); else launch_inst<2, false>(s, m, a.N, order, g, grid); }
  for (int i = 0; i < count; i++)
    PH_ROUTE(ctx, pairs[i].C, pairs[i].C, pairs[i].L, pairs[i].N, "rb_pair_bf16x3 MT=%d form=%d Ka=%d da=%d Kb=%d db=%d W1=%d multi=%d conv", a.C / 32, a.form,
             pairs[i].Ka, pairs[i].dila, pairs[i].Kb, pairs[i].dilb, kW1, count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "rb_pair_bf16x3 launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(rb_pair_bf16x3, (rb_pair_bf16x3_kernel<1, true>)); } }
