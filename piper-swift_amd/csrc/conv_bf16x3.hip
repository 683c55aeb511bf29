// conv_bf16x3.hip — Conv1d / ConvTranspose1d with SPLIT bf16 operands: fp32-grade results on v_mfma_f32_32x32x16_bf16.
//
// Role: the generator of the voice path at PIPER_HIP_PRECISION_BF16X3 (voice.hip) and the op-level piper_hip_conv1d_bf16x3 /
// piper_hip_convtranspose1d_bf16x3 entry points. The arithmetic (conv_bf16x3.h): each operand a = a_hi + a_lo with
// a_hi = bf16(a), a_lo = bf16(a − a_hi); the contraction is W_lo·X_hi + W_hi·X_lo + W_hi·X_hi in one fp32 accumulator. Every
// product of two bf16 values is exact in fp32, the dropped lo·lo term is ≤ 2⁻¹⁶ relative, so per output
// |error| ≤ 3·2⁻¹⁶·Σ|w||x| plus fp32 accumulation — against 2·2⁻⁸·Σ|w||x| of single bf16.
//
// One block = 4 waves = a (row group, column block) of the implicit GEMM, as in conv_bf16.hip, on PLANAR hi/lo images:
//   1. both planes of the block's input window — every input channel × (columns + dilation reach) — are copied ONCE into LDS,
//      hi rows then lo rows, each plane with the 16-byte position stride that keeps ds_read_b128 conflict-free; the stored zero
//      halo of both planes is the conv's zero padding (0 = 0 + 0), so the hot loop has no bounds tests;
//   2. per (tap, 16 channels) a wave takes A_hi / A_lo (16 B per lane each, contiguous per wave) from L2 through two register
//      rings and B_hi / B_lo from the two window planes, and issues 3 · MTW · NTW MFMAs TERM-MAJOR: every tile's lo·hi, then
//      every tile's hi·lo, then every tile's hi·hi. Consecutive MFMAs then never wait on the accumulator just written (unless
//      the wave owns a single tile), and each tile's small terms enter before its large one. A step carries three times the
//      MFMA work of conv_bf16_kernel's, so the rings are half as deep in steps for the same latency cover and the doubled
//      fragments cost no more registers than there: no instance spills (profiles/bf16x3.md);
//   3. epilogue: conv_bf16_kernel's (bias, fp32 residual, MRF mean, fp32 store); the activation image of LeakyReLU(result) for
//      the next conv is split in registers and written to BOTH planes, zeros beyond the true length in both.
#include <algorithm>

#include "conv_bf16x3.h"

namespace ph {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBT = 256;  // 4 waves
constexpr size_t kLdsMax = 160 * 1024;

__device__ __forceinline__ unsigned pack2_bf16(float a, float b) {
  bf16x2 v = {(__bf16)a, (__bf16)b};  // v_cvt_pk_bf16_f32, round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
// (a, b) → packed hi pair; lo = the packed pair of the residuals a − float(a_hi), b − float(b_hi) (exact fp32 subtractions)
__device__ __forceinline__ unsigned split2_bf16(float a, float b, unsigned& lo) {
  const unsigned hi = pack2_bf16(a, b);
  lo = pack2_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
  return hi;
}
__device__ __forceinline__ void split8_bf16(const float (&v)[8], uint4& hi, uint4& lo) {
  hi.x = split2_bf16(v[0], v[1], lo.x); hi.y = split2_bf16(v[2], v[3], lo.y);
  hi.z = split2_bf16(v[4], v[5], lo.z); hi.w = split2_bf16(v[6], v[7], lo.w);
}
__device__ __forceinline__ float lrelu1(float v, float alpha) { return v >= 0.0f ? v : v * alpha; }

// ---------------------------------------------------------------- packing
// One thread per element of a fragment image (conv_bf16.hip's order): hi to out[i], lo to out[total + i]. Both pads are zero.
__device__ __forceinline__ void store_split(uint16_t* out, int64_t total, int64_t i, float v) {
  unsigned lo;
  const unsigned hi = split2_bf16(v, 0.0f, lo);
  out[i] = (uint16_t)(hi & 0xffffu);
  out[total + i] = (uint16_t)(lo & 0xffffu);
}

// conv: element e of lane l of step (tap, c16) of row tile mt  =  w[mt·32 + (l&31)][c16·16 + 8·(l>>5) + e][tap]
__global__ __launch_bounds__(kBT) void pack_conv_bf16x3_kernel(const float* __restrict__ w, int Cout, int Cin, int K,
                                                              uint16_t* __restrict__ out, int64_t total) {
  const int C16 = Cin >> 4;
  for (int64_t i = (int64_t)blockIdx.x * kBT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBT) {
    const int e = (int)(i & 7), l = (int)((i >> 3) & 63);
    int64_t st = i >> 9;
    const int c16 = (int)(st % C16); st /= C16;
    const int tap = (int)(st % K);
    const int64_t mt = st / K;
    const int64_t row = mt * 32 + (l & 31);
    const int ch = c16 * 16 + 8 * (l >> 5) + e;
    store_split(out, total, i, row < Cout ? w[(row * Cin + ch) * K + tap] : 0.0f);  // rows past Cout: tile padding and the ring's pad
  }
}

// convT: GEMM row R = ρ·Cout + co, tap j  ⇒  w[ci][co][(ρ+pad) mod s + s·j]
__global__ __launch_bounds__(kBT) void pack_convt_bf16x3_kernel(const float* __restrict__ w, int Cin, int Cout, int K, int stride,
                                                               int pad, uint16_t* __restrict__ out, int64_t total) {
  const int C16 = Cin >> 4, J = K / stride;
  for (int64_t i = (int64_t)blockIdx.x * kBT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBT) {
    const int e = (int)(i & 7), l = (int)((i >> 3) & 63);
    int64_t st = i >> 9;
    const int c16 = (int)(st % C16); st /= C16;
    const int j = (int)(st % J);
    const int64_t R = (st / J) * 32 + (l & 31);
    const int ci = c16 * 16 + 8 * (l >> 5) + e;
    const int64_t rho = R / Cout;
    const int co = (int)(R - rho * Cout);
    const int k = (int)((rho + pad) % stride) + stride * j;
    store_split(out, total, i, rho < stride ? w[((int64_t)ci * Cout + co) * K + k] : 0.0f);
  }
}

// fp32 [N][C][L] → both C8 planes of lrelu(x): one thread per (channel block, position) writes 16 bytes to each plane
__global__ __launch_bounds__(kBT) void pack_act_c8x2_kernel(const float* __restrict__ x, int C, int L, int64_t row, float alpha,
                                                           uint16_t* __restrict__ act, const int* __restrict__ len_ptr) {
  const int CB = (C + 7) >> 3;
  const int n = blockIdx.z, cb = blockIdx.y;
  const int Lv = len_ptr ? min(len_ptr[n], L) : L;
  if (len_ptr && Lv == 0) return;  // a row of length 0 is read by nobody (block-uniform)
  const float* xb = x + ((int64_t)n * C + cb * 8) * L;
  uint4* hi_p = (uint4*)act + ((int64_t)n * CB + cb) * row + kC8Halo;
  uint4* lo_p = hi_p + (int64_t)gridDim.z * CB * row;
  for (int pos = blockIdx.x * kBT + threadIdx.x; pos < L; pos += gridDim.x * kBT) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (cb * 8 + e < C && pos < Lv) ? lrelu1(xb[(int64_t)e * L + pos], alpha) : 0.0f;
    uint4 hi, lo;
    split8_bf16(v, hi, lo);
    hi_p[pos] = hi;
    lo_p[pos] = lo;
  }
}

// both C8 planes of lrelu(((a + b) + c) / 3): the MRF mean of three fp32 [N][C][L] tensors, C % 8 == 0; zeros past the true length
__global__ __launch_bounds__(kBT) void pack_mean3_c8x2_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int C,
                                                             int L, int64_t row, float alpha, uint16_t* __restrict__ act, const int* __restrict__ len_ptr,
                                                             int len_mul) {
  const int CB = C >> 3;
  const int n = blockIdx.z, cb = blockIdx.y;
  const int Lv = len_ptr ? min(len_ptr[n] * len_mul, L) : L;
  if (len_ptr && Lv == 0) return;  // a row of length 0 is read by nobody (block-uniform)
  const int64_t off = ((int64_t)n * C + cb * 8) * L;
  uint4* hi_p = (uint4*)act + ((int64_t)n * CB + cb) * row + kC8Halo;
  uint4* lo_p = hi_p + (int64_t)gridDim.z * CB * row;
  for (int pos = blockIdx.x * kBT + threadIdx.x; pos < L; pos += gridDim.x * kBT) {
    float va[8], vb[8], vc[8], v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int64_t i = off + (int64_t)e * L + pos;
      va[e] = a[i]; vb[e] = b[i]; vc[e] = c[i];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = pos < Lv ? lrelu1(((va[e] + vb[e]) + vc[e]) / 3.0f, alpha) : 0.0f;
    uint4 hi, lo;
    split8_bf16(v, hi, lo);
    hi_p[pos] = hi;
    lo_p[pos] = lo;
  }
}

// ---------------------------------------------------------------- the conv
// WM waves along rows × (4/WM) along columns; each wave MTW × NTW tiles of 32×32.
struct ConvBf16x3Multi {
  ConvBf16Args c[kBf16Multi];
};

template <int MTW, int NTW, int WM>
__global__ __launch_bounds__(kBT) void conv_bf16x3_kernel(const ConvBf16x3Multi multi, int batch) {
  extern __shared__ __attribute__((aligned(16))) uint4 win[];  // hi plane [Cin/8][W], lo plane [Cin/8][W], 1 dump slot
  const ConvBf16Args& p = multi.c[blockIdx.z / batch];  // wave-uniform: which of the launch's convs this block works on
  constexpr int WN = 4 / WM;
  constexpr int NBC = WN * NTW * 32;  // columns per block
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const bool ct = p.ct_stride > 0;
  const int taps = ct ? p.K / p.ct_stride : p.K;
  const int C16 = p.Cin >> 4, CB = p.Cin >> 3;
  const int n = blockIdx.z % batch;
  // a row of length 0 (batched streaming: a finished, dropped or pad item) is read by nobody: no work, no stores (block-uniform)
  if (p.len_ptr && p.len_ptr[n] == 0) return;
  const int nb0 = blockIdx.x * NBC;              // first column of the block
  const int mt0 = (blockIdx.y * WM + wm) * MTW;  // first row tile of this wave
  // window: input positions [nb0 + off_min, nb0 + NBC + off_max)
  const int off_min = ct ? -(taps - 1) : -p.padL;
  const int off_max = ct ? (p.ct_stride - 1 + p.ct_pad) / p.ct_stride : (p.K - 1) * p.dil - p.padL;
  const int W = NBC + off_max - off_min;
  const int PW = CB * W;     // LDS slots of one plane
  const int S = taps * C16;  // steps: (tap, 16 channels)
  const int rows_total = ct ? p.Cout * p.ct_stride : p.Cout;
  // weight fragments: one 1 KB wave-load per step, row tile and plane, through two kDA-deep register rings. Each image is
  // padded by kBf16WeightPad elements (≥ 16 steps), so the rings run past the last step without a clamp.
  constexpr int kDA = MTW == 1 ? 8 : 4;
  const int64_t wtile = (int64_t)S * 1024;  // bytes per row tile
  const int64_t wplane = (int64_t)((rows_total + 31) >> 5) * wtile + (int64_t)kBf16WeightPad * 2;  // bytes from the hi image to the lo image
  // uniform bases (SGPR pairs) + 32-bit lane offset: the loads take the saddr form, no 64-bit VALU adds per step
  const char* wa = (const char*)p.w + (int64_t)mt0 * wtile;
  const char* wl = wa + wplane;
  const unsigned lane16 = (unsigned)lane * 16u;
  uint4 ah[kDA][MTW], al[kDA][MTW];
  auto load_a = [&](int slot, int ahead) {
#pragma unroll
    for (int m = 0; m < MTW; m++) {
      ah[slot][m] = *(const uint4*)(wa + m * wtile + ahead * 1024 + lane16);
      al[slot][m] = *(const uint4*)(wl + m * wtile + ahead * 1024 + lane16);
    }
  };
#pragma unroll
  for (int d = 0; d < kDA - 1; d++) load_a(d, d);  // independent of the window: in flight before the staging round trips
  {
    // staging row R < CB is channel block R of the hi plane, R ≥ CB channel block R − CB of the lo plane; the LDS planes are
    // adjacent, so the destination is R·W + position for both. Rows by wave, 64 positions per wave instruction, kStage loads in
    // flight before the first LDS store. Every lane stores: lanes past the row end / rows past the window go to a dump slot
    // behind it, so the loads are not sunk into conditional blocks.
    const uint4* xb = (const uint4*)p.x + (int64_t)n * CB * p.x_row;
    const int64_t xplane = (int64_t)batch * CB * p.x_row;  // uint4 slots from the hi plane to the lo plane
    const int g0 = kC8Halo + nb0 + off_min;
    constexpr int kStage = 8;
    const int WCH = (W + 63) >> 6;
    const int R2 = 2 * CB;
    const int dump = 2 * PW;
    int row = wave, chunk = 0;
    while (row < R2) {
      uint4 t[kStage];
      int dst[kStage];
#pragma unroll
      for (int q = 0; q < kStage; q++) {
        const int rr = min(row, R2 - 1);
        const bool lo = rr >= CB;
        const int cb = lo ? rr - CB : rr;
        const int wpos = chunk * 64 + lane;
        const int gp = min(max(g0 + wpos, 0), p.x_row - 1);  // partial last block: clamped columns are masked at the store
        t[q] = xb[(lo ? xplane : 0) + (int64_t)cb * p.x_row + gp];
        dst[q] = (row < R2 && wpos < W) ? rr * W + wpos : dump;
        chunk++;
        const bool wrap = chunk == WCH;
        chunk = wrap ? 0 : chunk;
        row += wrap ? 4 : 0;
      }
#pragma unroll
      for (int q = 0; q < kStage; q++) win[dst[q]] = t[q];
    }
  }
  __syncthreads();

  f32x16 acc[MTW][NTW];
#pragma unroll
  for (int m = 0; m < MTW; m++)
#pragma unroll
    for (int j = 0; j < NTW; j++)
#pragma unroll
      for (int q = 0; q < 16; q++) acc[m][j][q] = 0.0f;

  // ConvTranspose: the wave's row tiles lie in one phase ρ when Cout % (32·MTW) == 0 (checked by the launcher)
  const int rho = ct ? (mt0 * 32) / p.Cout : 0;
  // window position read by tap t: conv t·dil − padL, convT ⌊(ρ+pad)/s⌋ − t  ⇒  off0 + t·dstep
  const int off0 = ct ? (rho + p.ct_pad) / p.ct_stride : -p.padL;
  const int dstep = ct ? -1 : p.dil;
  // LDS read base of this lane in the hi plane: channel block h, position r + wave's column offset; the lo plane is PW further
  const int lbase = h * W + wn * NTW * 32 + r - off_min + off0;

  // activation fragments: ds_read_b128 from both planes, kDB steps ahead of their MFMAs. The window index is a wave-uniform
  // part (2·c16·W + tap·dstep, advanced with scalar selects) plus the lane part; it stops advancing after the last step, so
  // the ring never reads outside the window. kDA is a multiple of kDB: the static slots line up across groups.
  constexpr int kDB = NTW == 4 ? 2 : 4;
  uint4 bh[kDB][NTW], bl[kDB][NTW];
  int sidx = 0, c_n = 0, left = S - 1;
  const int wrap_delta = dstep - 2 * W * (C16 - 1);
  auto read_b = [&](int slot) {
    const int idx = lbase + sidx;
#pragma unroll
    for (int j = 0; j < NTW; j++) {
      bh[slot][j] = win[idx + 32 * j];
      bl[slot][j] = win[idx + PW + 32 * j];
    }
    c_n++;
    const bool wrap = c_n == C16;
    c_n = wrap ? 0 : c_n;
    const int delta = wrap ? wrap_delta : 2 * W;
    sidx += left > 0 ? delta : 0;
    left--;
  };
  auto mfma = [&](const uint4& a, const uint4& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  };
  auto step = [&](int u) {  // u = static ring slot
    load_a((u + kDA - 1) % kDA, kDA - 1 + u);
    __builtin_amdgcn_sched_barrier(0);  // keep the rings' loads at the top of their step
    read_b((u + kDB - 1) % kDB);
    const int v = u % kDB;
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < NTW; j++) acc[m][j] = mfma(al[u][m], bh[v][j], acc[m][j]);  // W_lo · X_hi
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < NTW; j++) acc[m][j] = mfma(ah[u][m], bl[v][j], acc[m][j]);  // W_hi · X_lo
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < NTW; j++) acc[m][j] = mfma(ah[u][m], bh[v][j], acc[m][j]);  // W_hi · X_hi
  };
#pragma unroll
  for (int d = 0; d < kDB - 1; d++) read_b(d);
  // the rings' first loads were issued before the staging loop and have landed: an explicit vmcnt(0) gives the waitcnt pass a
  // clean state at the loop header
  __builtin_amdgcn_s_waitcnt(0x0F70);
  const int full = S / kDA;
  for (int g = 0; g < full; g++) {  // guard-free groups of kDA steps
#pragma unroll
    for (int u = 0; u < kDA; u++) step(u);
    wa += kDA * 1024;
    wl += kDA * 1024;
  }
  {
    const int rem = S - full * kDA;  // wave-uniform tail
#pragma unroll
    for (int u = 0; u < kDA - 1; u++)
      if (u < rem) step(u);
  }

  // ---- epilogue. accumulator register q of lane (r,h): row (q&3) + 8·(q>>2) + 4·h, column r.
  // All loads of a tile (bias, residual, MRF partners) are issued up front with clamped, always-valid indices; only the stores
  // are masked.
  const int ACB = p.Cout >> 3;
  const int64_t aplane = (int64_t)batch * ACB * p.act_row;  // uint4 slots from the hi plane of the output image to its lo plane
#pragma unroll
  for (int m = 0; m < MTW; m++) {
    const int row0 = (mt0 + m) * 32;
    if (row0 >= rows_total) continue;
    const int co0 = ct ? row0 - rho * p.Cout : row0;  // channel of tile row 0
    float bias_v[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int coc = min(co0 + (q & 3) + 8 * (q >> 2) + 4 * h, p.Cout - 1);
      bias_v[q] = p.bias ? p.bias[(int64_t)n * p.bias_batch_stride + coc] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NTW; j++) {
      const int col = nb0 + (wn * NTW + j) * 32 + r;
      const bool okc = col < p.Lout;
      const int colc = min(col, p.Lout - 1);
      const int pos = ct ? colc * p.ct_stride + rho : colc;
      int64_t yi[16];
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int coc = min(co0 + (q & 3) + 8 * (q >> 2) + 4 * h, p.Cout - 1);
        yi[q] = ((int64_t)n * p.Cout + coc) * p.y_len + pos;
        v[q] = acc[m][j][q] + bias_v[q];
      }
      if (p.res) {
        float t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = p.res[yi[q]];
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] += t[q];
      }
      if (p.mrf_a) {
        float ta[16], tb[16];
#pragma unroll
        for (int q = 0; q < 16; q++) { ta[q] = p.mrf_a[yi[q]]; tb[q] = p.mrf_b[yi[q]]; }
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = ((ta[q] + tb[q]) + v[q]) / 3.0f;
      }
      if (p.y) {
#pragma unroll
        for (int q = 0; q < 16; q++)
          if (okc && co0 + (q & 3) + 8 * (q >> 2) + 4 * h < p.Cout) p.y[yi[q]] = v[q];
      }
      if (p.act) {
        const bool live = !p.len_ptr || pos < p.len_ptr[n] * p.len_mul;  // past the true length both planes must hold zeros
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int cg = co0 + 8 * g + 4 * h;  // first of 4 consecutive channels
          uint2 oh, ol;
          oh.x = split2_bf16(lrelu1(v[4 * g], p.act_alpha), lrelu1(v[4 * g + 1], p.act_alpha), ol.x);
          oh.y = split2_bf16(lrelu1(v[4 * g + 2], p.act_alpha), lrelu1(v[4 * g + 3], p.act_alpha), ol.y);
          if (!live) oh = ol = make_uint2(0u, 0u);
          if (okc && cg < p.Cout) {
            uint4* slot = (uint4*)p.act + ((int64_t)n * ACB + (cg >> 3)) * p.act_row + kC8Halo + pos;
            *((uint2*)slot + ((cg >> 2) & 1)) = oh;
            *((uint2*)(slot + aplane) + ((cg >> 2) & 1)) = ol;
          }
        }
      }
    }
  }
}

template <int MTW, int NTW, int WM>
void raise_lds() {
  static bool done[kMaxDevices] = {};  // windows above the 64 KB default need the opt-in (160 KB per CU on gfx950), per device
  if (lds_optin_needed(done))
    (void)hipFuncSetAttribute((const void*)conv_bf16x3_kernel<MTW, NTW, WM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
}

int launch_cfg(hipStream_t s, const ConvBf16x3Multi& a, int batch, int MTW, int NTW, int WM, dim3 grid, size_t lds) {
#define PH_BF16X3_CASE(M, NT_, W_)                                                                    \
  if (MTW == M && NTW == NT_ && WM == W_) {                                                           \
    if (lds > 64 * 1024) raise_lds<M, NT_, W_>();                                                     \
    hipLaunchKernelGGL((conv_bf16x3_kernel<M, NT_, W_>), grid, dim3(kBT), lds, s, a, batch);          \
  } else
  PH_BF16X3_CASE(1, 1, 1) PH_BF16X3_CASE(1, 2, 1) PH_BF16X3_CASE(1, 4, 1)
  PH_BF16X3_CASE(1, 1, 2) PH_BF16X3_CASE(1, 2, 2) PH_BF16X3_CASE(1, 4, 2)
  // (no <2, ·, 2>: two waves along rows means the row-tile count is no multiple of 4, so no wave gets a second tile)
  PH_BF16X3_CASE(1, 1, 4) PH_BF16X3_CASE(1, 2, 4) PH_BF16X3_CASE(1, 4, 4)
  PH_BF16X3_CASE(2, 1, 4) PH_BF16X3_CASE(2, 2, 4) PH_BF16X3_CASE(2, 4, 4)
  PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "conv_bf16x3: no instance for MTW=%d NTW=%d WM=%d", MTW, NTW, WM);
#undef PH_BF16X3_CASE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "conv_bf16x3 launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

// waves along rows: as many of the 4 as the row-tile count allows (ConvTranspose: a wave's tiles stay in one phase)
int waves_along_rows(int per_phase) { return (per_phase % 4 == 0) ? 4 : (per_phase % 2 == 0) ? 2 : 1; }
// both planes of the window of a block of `cols` columns, and the dump slot
size_t lds_bytes(int Cin, int cols, int reach) { return (size_t)2 * (Cin / 8) * (cols + reach) * 16 + 16; }

template <class Kernel, class... Args>
int launch_pack(hipStream_t s, Kernel k, dim3 grid, Args... args) {
  hipLaunchKernelGGL(k, grid, dim3(kBT), 0, s, args...);
  return PIPER_HIP_OK;
}

}  // namespace

int pack_conv_weights_bf16x3(hipStream_t s, const float* w, int Cout, int Cin, int K, uint16_t* packed) {
  const int64_t total = (int64_t)packed_conv_bf16_elems(Cout, Cin, K);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(total, kBT), 4096));
  return launch_pack(s, pack_conv_bf16x3_kernel, grid, w, Cout, Cin, K, packed, total);
}
int pack_convt_weights_bf16x3(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, int pad, uint16_t* packed) {
  const int64_t total = (int64_t)packed_convt_bf16_elems(Cin, Cout, K, stride);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(total, kBT), 4096));
  return launch_pack(s, pack_convt_bf16x3_kernel, grid, w, Cin, Cout, K, stride, pad, packed, total);
}
int pack_act_c8x2(hipStream_t s, const float* x, int N, int C, int L, float alpha, uint16_t* act, int64_t row, const int* len_ptr) {
  if (N <= 0 || C <= 0 || L <= 0) return PIPER_HIP_OK;
  if (row <= 0) row = c8_row_len(L);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(L, kBT), 1024), (unsigned)((C + 7) / 8), (unsigned)N);  // gridDim.z = N: the plane offset
  return launch_pack(s, pack_act_c8x2_kernel, grid, x, C, L, row, alpha, act, len_ptr);
}
int pack_mean3_c8x2(hipStream_t s, const float* a, const float* b, const float* c, int N, int C, int L, float alpha, uint16_t* act, int64_t row,
                    const int* len_ptr, int len_mul) {
  if (N <= 0 || C <= 0 || L <= 0) return PIPER_HIP_OK;
  if (C & 7) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "pack_mean3_c8x2: %d channels (multiples of 8)", C);
  if (row <= 0) row = c8_row_len(L);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(L, kBT), 1024), (unsigned)(C / 8), (unsigned)N);  // gridDim.z = N: the plane offset
  return launch_pack(s, pack_mean3_c8x2_kernel, grid, a, b, c, C, L, row, alpha, act, len_ptr, len_mul);
}
bool conv_bf16x3_fits(int row_tiles, int Cin, int reach) { return lds_bytes(Cin, 4 / waves_along_rows(row_tiles) * 32, reach) <= kLdsMax; }

int launch_conv_bf16x3(piper_hip_ctx* ctx, hipStream_t s, const ConvBf16Args& a) { return launch_conv_bf16x3_multi(ctx, s, &a, 1); }

int launch_conv_bf16x3_multi(piper_hip_ctx* ctx, hipStream_t s, const ConvBf16Args* convs, int count) {
  if (count < 1 || count > kBf16Multi) PH_FAIL(PIPER_HIP_ERR_ARG, "conv_bf16x3: %d convs in one launch (1..%d)", count, kBf16Multi);
  const ConvBf16Args& a = convs[0];
  if (a.N <= 0 || a.Lout <= 0) return PIPER_HIP_OK;
  const bool ct = a.ct_stride > 0;
  const int rows = ct ? a.Cout * a.ct_stride : a.Cout;
  const int MT = (rows + 31) / 32;
  auto reach_of = [&](const ConvBf16Args& b) { return ct ? convt_reach(b.K, b.ct_stride, b.ct_pad) : conv_reach(b.K, b.dil); };
  int reach = reach_of(a);
  for (int i = 1; i < count; i++) {
    const ConvBf16Args& b = convs[i];
    if (b.N != a.N || b.Cin != a.Cin || b.Cout != a.Cout || b.Lout != a.Lout || b.ct_stride != a.ct_stride || b.x_row != a.x_row ||
        b.act_row != a.act_row)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "conv_bf16x3: convs of one launch must share N, Cin, Cout, Lout, row lengths and kind");
    reach = std::max(reach, reach_of(b));
  }
  const int per_phase = ct ? a.Cout / 32 : MT;
  const int WM = waves_along_rows(per_phase), WN = 4 / WM;
  int MTW = (per_phase % (2 * WM) == 0) ? 2 : 1;
  int NTW = 4;
  auto blocks = [&](int mtw, int ntw) { return ceil_div(MT, WM * mtw) * ceil_div(a.Lout, WN * ntw * 32) * a.N * count; };
  // the widest column block whose doubled window fits LDS; then narrower tiles until every CU has two blocks
  const int64_t want = 2 * (int64_t)ctx->num_cus;
  while (NTW > 1 && (blocks(MTW, NTW) < want || lds_bytes(a.Cin, WN * NTW * 32, reach) > kLdsMax)) NTW >>= 1;
  if (MTW == 2 && blocks(MTW, NTW) < want) MTW = 1;
  const size_t lds = lds_bytes(a.Cin, WN * NTW * 32, reach);
  if (lds > kLdsMax)
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "conv_bf16x3: both planes of the window, %zu bytes, do not fit LDS (Cin=%d reach=%d)", lds, a.Cin, reach);
  const dim3 grid((unsigned)ceil_div(a.Lout, WN * NTW * 32), (unsigned)ceil_div(MT, WM * MTW), (unsigned)(a.N * count));
  ConvBf16x3Multi multi;
  for (int i = 0; i < kBf16Multi; i++) multi.c[i] = convs[i < count ? i : 0];
  const int rc = launch_cfg(s, multi, a.N, MTW, NTW, WM, grid, lds);
  if (!rc)
    for (int i = 0; i < count; i++)
      PH_ROUTE(ctx, convs[i].Cout, convs[i].Cin, convs[i].Lout, convs[i].N, "bf16x3 K=%d MTW=%d NTW=%d WM=%d multi=%d %s", convs[i].K, MTW, NTW, WM,
               count, ct ? "convT" : "conv");
  return rc;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(conv_bf16x3, pack_conv_bf16x3_kernel); } }
