// conv_f16.hip — Conv1d / ConvTranspose1d with fp16 operands and fp32 accumulation on v_mfma_f32_32x32x16_f16.
//
// Role: the generator of the voice path at PIPER_HIP_PRECISION_F16 (voice.hip) and the op-level piper_hip_conv1d_f16 /
// piper_hip_convtranspose1d_f16 entry points. The arithmetic is conv_f16.h's contract: clamped, round-to-nearest-even fp16 activations,
// weights scaled by one power of two per output channel before they are rounded, the fp32 accumulator scaled back in the epilogue.
//
// One block = 4 waves = a (row group, column block) of the implicit GEMM  Y[rows, cols] = W[rows, Cin·K] · X[Cin·K, cols], WM waves
// along rows × 4/WM along columns, MTW × NTW tiles of 32×32 per wave, as in conv_bf16.hip:
//   1. the block's whole input window — every input channel × (columns + reach) — is staged ONCE from the C8 image into LDS; the stored
//      zero halo is the conv's zero padding, the hot loop has no bounds tests;
//   2. WEIGHTS. A step is (tap, 16 channels); its fragment is 1 KB per row tile. conv_bf16_kernel lets every wave stream its own
//      fragments from L2, so with WM = 1 the same kilobyte enters the CU four times. Here the block's RT = WM·MTW row tiles enter the CU
//      once, through a ring in LDS behind the window (wsrc=lds):
//        · the ring is two GROUPS of 16 KB; a group holds G = 16 / RT consecutive steps × RT row tiles, slot (step, tile) at
//          (step·RT + tile) KB, lane l's 16 bytes at 16·l: a wave reads its fragment with one conflict-free ds_read_b128, and with WM = 1
//          all four waves read the same slots;
//        · the copy is cooperative and register-staged: every thread carries 4 × 16 bytes (256 threads × 64 B = one group), wave w and
//          chunk c bring kilobyte 4·c + w of the group. The global loads of group g+1 are issued before the MFMAs of group g and
//          waited for (vmcnt) only behind them, at the LDS store;
//        · barrier discipline: group g lives in half g & 1. Producer phase of a half: the stores at the end of iteration g−1, closed by
//          that iteration's __syncthreads. Consumer phase: the ds_reads of iteration g, closed by ITS __syncthreads. The half is stored
//          again at the end of iteration g+1, behind the barrier that closed iteration g — so no slot is refilled before every wave of
//          the block has read it, and there is exactly one barrier per group. The window's barrier is the one that publishes group 0;
//        · the ring reads up to G − 1 steps past a row tile's last fragment (the last group is loaded whole): into the next row tile,
//          or, behind the last one, into the image's readable pad (kBf16WeightPad ≥ 16 steps). Those slots are never consumed.
//      The ring is taken from what the window leaves of the CU's 160 KB, and only where it does not cost the second resident block:
//      2 · (window + 32 KB) ≤ 160 KB. A lone block's barrier per group has no other block to hide behind, and there the instance keeps
//      conv_bf16_kernel's per-wave register ring from L2 (wsrc=l2): C_in = 512 at a dilated reach, or the wide column tiles of
//      C_in = 256. The route record says which path ran;
//   3. activation fragments: ds_read_b128 from the window, kDB steps ahead of their MFMA (conv_bf16.hip's ring);
//   4. epilogue: accumulator × 2^−e, bias, fp32 residual, MRF mean, fp32 store and/or the fp16 C8 image of LeakyReLU(result) (clamped;
//      zeros beyond the true length).
#include <algorithm>

#include "conv_f16.h"

namespace ph {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBT = 256;  // 4 waves
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kRingSlots = 2 * 1024;  // uint4 slots of the weight ring: two groups of 16 KB
constexpr size_t kRingBytes = (size_t)kRingSlots * 16;

__device__ __forceinline__ float clamp_f16(float v) { return __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }
__device__ __forceinline__ unsigned pack2_f16(float a, float b) {
  f16x2 v = {(_Float16)clamp_f16(a), (_Float16)clamp_f16(b)};  // plain casts: round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ uint4 pack8_f16(const float (&v)[8]) {
  uint4 o;
  o.x = pack2_f16(v[0], v[1]); o.y = pack2_f16(v[2], v[3]); o.z = pack2_f16(v[4], v[5]); o.w = pack2_f16(v[6], v[7]);
  return o;
}
__device__ __forceinline__ float lrelu1(float v, float alpha) { return v >= 0.0f ? v : v * alpha; }
// 2^e from scale = 2^−e (a normal power of two): the exponent field mirrored about the bias, exact
__device__ __forceinline__ float pow2_inverse(float scale) { return __uint_as_float((254u << 23) - __float_as_uint(scale)); }

// ---------------------------------------------------------------- packing
// scale[co] = 2^−e, e = 14 − ⌊log₂ max|w[co,·,·]|⌋ (0 for a zero row): one block per output channel.
// conv: w[co][Cin][K]; ConvTranspose (ct): w[Cin][co][K], the max over all Cin and K
__global__ __launch_bounds__(kBT) void row_scale_f16_kernel(const float* __restrict__ w, int Cout, int Cin, int K, int ct, float* __restrict__ scale) {
  __shared__ float red[kBT];
  const int co = blockIdx.x, n = Cin * K;
  float m = 0.0f;
  for (int i = threadIdx.x; i < n; i += kBT) {
    const int64_t idx = ct ? ((int64_t)(i / K) * Cout + co) * K + i % K : (int64_t)co * n + i;
    m = fmaxf(m, fabsf(w[idx]));
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int d = kBT / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + d]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int ex = 0;
    (void)frexpf(red[0], &ex);  // m = f · 2^ex, f ∈ [0.5, 1)  ⇒  ⌊log₂ m⌋ = ex − 1
    const int e = red[0] > 0.0f ? min(max(15 - ex, -126), 126) : 0;
    scale[co] = ldexpf(1.0f, -e);
  }
}

__device__ __forceinline__ uint16_t round_f16(float v) { return (uint16_t)(pack2_f16(v, 0.0f) & 0xffffu); }

// conv: element e of lane l of step (tap, c16) of row tile mt  =  w[mt·32 + (l&31)][c16·16 + 8·(l>>5) + e][tap] · 2^e_row
__global__ __launch_bounds__(kBT) void pack_conv_f16_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout, int Cin, int K,
                                                           uint16_t* __restrict__ out, int64_t total) {
  const int C16 = Cin >> 4;
  for (int64_t i = (int64_t)blockIdx.x * kBT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBT) {
    const int e = (int)(i & 7), l = (int)((i >> 3) & 63);
    int64_t st = i >> 9;
    const int c16 = (int)(st % C16); st /= C16;
    const int tap = (int)(st % K);
    const int64_t row = (st / K) * 32 + (l & 31);
    const int ch = c16 * 16 + 8 * (l >> 5) + e;
    out[i] = row < Cout ? round_f16(w[(row * Cin + ch) * K + tap] * pow2_inverse(scale[row])) : (uint16_t)0;  // rows past Cout: tile padding and the pad
  }
}

// convT: GEMM row R = ρ·Cout + co, tap j  ⇒  w[ci][co][(ρ+pad) mod s + s·j] · 2^e_co
__global__ __launch_bounds__(kBT) void pack_convt_f16_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cin, int Cout, int K,
                                                            int stride, int pad, uint16_t* __restrict__ out, int64_t total) {
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
    out[i] = rho < stride ? round_f16(w[((int64_t)ci * Cout + co) * K + k] * pow2_inverse(scale[co])) : (uint16_t)0;
  }
}

// fp32 [N][C][L] → fp16 C8 image of lrelu(x): one thread per (channel block, position) writes 16 bytes
__global__ __launch_bounds__(kBT) void pack_act_c8_f16_kernel(const float* __restrict__ x, int C, int L, int64_t row, float alpha,
                                                             uint16_t* __restrict__ act, const int* __restrict__ len_ptr) {
  const int CB = (C + 7) >> 3;
  const int n = blockIdx.z, cb = blockIdx.y;
  const int Lv = len_ptr ? min(len_ptr[n], L) : L;
  if (len_ptr && Lv == 0) return;  // a row of length 0 is read by nobody (block-uniform)
  const float* xb = x + ((int64_t)n * C + cb * 8) * L;
  uint4* ab = (uint4*)act + ((int64_t)n * CB + cb) * row + kC8Halo;
  for (int pos = blockIdx.x * kBT + threadIdx.x; pos < L; pos += gridDim.x * kBT) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (cb * 8 + e < C && pos < Lv) ? lrelu1(xb[(int64_t)e * L + pos], alpha) : 0.0f;
    ab[pos] = pack8_f16(v);
  }
}

// fp16 C8 image of lrelu(((a + b) + c) / 3, alpha): the MRF mean of three fp32 [N][C][L] tensors, C % 8 == 0; zeros past the true length
__global__ __launch_bounds__(kBT) void pack_mean3_c8_f16_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                               int C, int L, int64_t row, float alpha, uint16_t* __restrict__ act,
                                                               const int* __restrict__ len_ptr, int len_mul) {
  const int CB = C >> 3;
  const int n = blockIdx.z, cb = blockIdx.y;
  const int Lv = len_ptr ? min(len_ptr[n] * len_mul, L) : L;
  if (len_ptr && Lv == 0) return;  // a row of length 0 is read by nobody (block-uniform)
  const int64_t off = ((int64_t)n * C + cb * 8) * L;
  uint4* ab = (uint4*)act + ((int64_t)n * CB + cb) * row + kC8Halo;
  for (int pos = blockIdx.x * kBT + threadIdx.x; pos < L; pos += gridDim.x * kBT) {
    float va[8], vb[8], vc[8], v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int64_t i = off + (int64_t)e * L + pos;
      va[e] = a[i]; vb[e] = b[i]; vc[e] = c[i];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = pos < Lv ? lrelu1(((va[e] + vb[e]) + vc[e]) / 3.0f, alpha) : 0.0f;
    ab[pos] = pack8_f16(v);
  }
}

// ---------------------------------------------------------------- the conv
struct ConvF16Multi {
  ConvF16Args c[kBf16Multi];
};

// LDSW: weight fragments through the block's LDS ring (true) or through a per-wave register ring from L2 (false)
template <int MTW, int NTW, int WM, bool LDSW>
__global__ __launch_bounds__(kBT) void conv_f16_kernel(const ConvF16Multi multi, int batch) {
  extern __shared__ __attribute__((aligned(16))) uint4 win[];  // [Cin/8][W] positions of 8 channels, 1 dump slot, then the weight ring
  const ConvF16Args& p = multi.c[blockIdx.z / batch];  // wave-uniform: which of the launch's convs this block works on
  constexpr int WN = 4 / WM;
  constexpr int NBC = WN * NTW * 32;  // columns per block
  constexpr int RT = WM * MTW;        // row tiles per block
  constexpr int G = 16 / RT;          // steps per ring group
  static_assert(16 % RT == 0, "a ring group is a whole number of steps");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const bool ct = p.ct_stride > 0;
  const int taps = ct ? p.K / p.ct_stride : p.K;
  const int C16 = p.Cin >> 4, CB = p.Cin >> 3;
  const int n = blockIdx.z % batch;
  // a row of length 0 (batched streaming: a finished, dropped or pad item) is read by nobody: no work, no stores (block-uniform,
  // in front of every barrier)
  if (p.len_ptr && p.len_ptr[n] == 0) return;
  const int nb0 = blockIdx.x * NBC;              // first column of the block
  const int mt0 = (blockIdx.y * WM + wm) * MTW;  // first row tile of this wave
  // window: input positions [nb0 + off_min, nb0 + NBC + off_max)
  const int off_min = ct ? -(taps - 1) : -p.padL;
  const int off_max = ct ? (p.ct_stride - 1 + p.ct_pad) / p.ct_stride : (p.K - 1) * p.dil - p.padL;
  const int W = NBC + off_max - off_min;
  const int S = taps * C16;  // steps: (tap, 16 channels)
  const unsigned lane16 = (unsigned)lane * 16u;
  const int wtile = S * 1024;  // bytes per row tile (the launcher keeps a block's RT tiles within 32 bits)

  // ---- weight sources. Both read past a tile's last step into the next tile or the image's pad (kBf16WeightPad ≥ 16 steps).
  // LDS ring, producer side: chunk c of this wave is kilobyte kb = 4·c + wave of a group = (step kb / RT, tile kb % RT)
  uint4* const ring = win + CB * W + 1;
  const char* wblk = (const char*)p.w + (int64_t)blockIdx.y * RT * wtile;  // uniform base (SGPR pair) + 32-bit offsets
  uint4 stg0, stg1, stg2, stg3;  // (named, not an array: they live across the loop's back edge and must stay in registers)
  auto group_src = [&](int c, int g) {
    const int kb = 4 * c + wave;
    return *(const uint4*)(wblk + ((kb % RT) * wtile + (g * G + kb / RT) * 1024) + lane16);
  };
  auto load_group = [&](int g) {
    stg0 = group_src(0, g); stg1 = group_src(1, g); stg2 = group_src(2, g); stg3 = group_src(3, g);
  };
  auto store_group = [&](int half) {
    uint4* dst = ring + half * 1024 + threadIdx.x;
    dst[0] = stg0; dst[256] = stg1; dst[512] = stg2; dst[768] = stg3;
  };
  // L2 register ring (conv_bf16_kernel's): kDA steps deep per wave
  constexpr int kDA = LDSW ? 1 : (MTW == 1 ? 16 : 8);
  const char* wa = (const char*)p.w + (int64_t)mt0 * wtile;
  uint4 a[kDA][MTW];
  auto load_a = [&](int slot, int ahead) {
#pragma unroll
    for (int m = 0; m < MTW; m++) a[slot][m] = *(const uint4*)(wa + m * wtile + ahead * 1024 + lane16);
  };
  // independent of the window: in flight before the staging round trips
  if constexpr (LDSW) {
    load_group(0);
  } else {
#pragma unroll
    for (int d = 0; d < kDA - 1; d++) load_a(d, d);
  }
  {
    const uint4* xb = (const uint4*)p.x + (int64_t)n * CB * p.x_row;
    const int g0 = kC8Halo + nb0 + off_min;
    // rows of the window by wave, 64 positions per wave instruction; kStage loads in flight before the first LDS store. (row, chunk)
    // are wave-uniform counters. Every lane stores: lanes past the row end / rows past the window go to a dump slot behind it, so the
    // loads are not sunk into conditional blocks.
    constexpr int kStage = 8;
    const int WCH = (W + 63) >> 6;
    const int dump = CB * W;
    int row = wave, chunk = 0;
    while (row < CB) {
      uint4 t[kStage];
      int dst[kStage];
#pragma unroll
      for (int q = 0; q < kStage; q++) {
        const int rr = min(row, CB - 1);
        const int wpos = chunk * 64 + lane;
        const int gp = min(max(g0 + wpos, 0), p.x_row - 1);  // partial last block: clamped columns are masked at the store
        t[q] = xb[(int64_t)rr * p.x_row + gp];
        dst[q] = (row < CB && wpos < W) ? rr * W + wpos : dump;
        chunk++;
        const bool wrap = chunk == WCH;
        chunk = wrap ? 0 : chunk;
        row += wrap ? 4 : 0;
      }
#pragma unroll
      for (int q = 0; q < kStage; q++) win[dst[q]] = t[q];
    }
  }
  if constexpr (LDSW) store_group(0);
  __syncthreads();  // publishes the window and group 0

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
  // LDS read base of this lane: channel block h, position r + wave's column offset, relative to the window start
  const int lbase = h * W + wn * NTW * 32 + r - off_min + off0;

  // activation fragments, kDB steps ahead of their MFMA. The window index is a wave-uniform part (2·c16·W + tap·dstep, advanced with
  // scalar selects) plus the lane part; it stops advancing after the last step, so the ring never reads outside the window. Both G and
  // kDA are multiples of kDB: the static slots line up across groups.
  constexpr int kDB = (LDSW && G < 4) ? G : 4;
  uint4 b[kDB][NTW];
  int sidx = 0, c_n = 0, left = S - 1;
  const int wrap_delta = dstep - 2 * W * (C16 - 1);
  auto read_b = [&](int slot) {
    const int idx = lbase + sidx;
#pragma unroll
    for (int j = 0; j < NTW; j++) b[slot][j] = win[idx + 32 * j];
    c_n++;
    const bool wrap = c_n == C16;
    c_n = wrap ? 0 : c_n;
    const int delta = wrap ? wrap_delta : 2 * W;
    sidx += left > 0 ? delta : 0;
    left--;
  };
  auto mma = [&](const uint4 (&af)[MTW], int v) {
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
      for (int j = 0; j < NTW; j++)
        acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[m]), __builtin_bit_cast(f16x8, b[v][j]), acc[m][j], 0, 0, 0);
  };
#pragma unroll
  for (int d = 0; d < kDB - 1; d++) read_b(d);

  if constexpr (LDSW) {
    const uint4* mine = ring + (wm * MTW) * 64 + lane;  // this wave's tiles of step 0 of half 0
    auto step = [&](int half, int u) {
      uint4 af[MTW];
#pragma unroll
      for (int m = 0; m < MTW; m++) af[m] = mine[half * 1024 + (u * RT + m) * 64];
      read_b((u + kDB - 1) % kDB);
      mma(af, u % kDB);
    };
    const int groups = (S + G - 1) / G;
    for (int g = 0; g < groups; g++) {  // block-uniform trip count: every wave meets every barrier
      const bool more = g + 1 < groups;
      if (more) load_group(g + 1);
      const int half = g & 1;
      if (S - g * G >= G) {
#pragma unroll
        for (int u = 0; u < G; u++) step(half, u);
      } else {  // the last group, partial (wave-uniform)
        const int rem = S - g * G;
#pragma unroll
        for (int u = 0; u < G - 1; u++)
          if (u < rem) step(half, u);
      }
      if (more) store_group(half ^ 1);  // last read in iteration g − 1, whose barrier every wave has passed
      __syncthreads();
    }
  } else {
    auto step = [&](int u) {  // u = static ring slot
      load_a((u + kDA - 1) % kDA, kDA - 1 + u);
      __builtin_amdgcn_sched_barrier(0);  // keep the ring's load at the top of its step
      read_b((u + kDB - 1) % kDB);
      mma(a[u], u % kDB);
    };
    // the ring's first loads were issued before the staging loop and have landed: an explicit vmcnt(0) gives the waitcnt pass a clean
    // state at the loop header
    __builtin_amdgcn_s_waitcnt(0x0F70);
    const int full = S / kDA;
    for (int g = 0; g < full; g++) {  // guard-free groups of kDA steps
#pragma unroll
      for (int u = 0; u < kDA; u++) step(u);
      wa += kDA * 1024;
    }
    const int rem = S - full * kDA;  // wave-uniform tail
#pragma unroll
    for (int u = 0; u < kDA - 1; u++)
      if (u < rem) step(u);
  }

  // ---- epilogue. accumulator register q of lane (r,h): row (q&3) + 8·(q>>2) + 4·h, column r.
  // All loads of a tile (scale, bias, residual, MRF partners) are issued up front with clamped, always-valid indices; only the stores
  // are masked.
  const int rows_total = ct ? p.Cout * p.ct_stride : p.Cout;
  const int ACB = p.Cout >> 3;
#pragma unroll
  for (int m = 0; m < MTW; m++) {
    const int row0 = (mt0 + m) * 32;
    if (row0 >= rows_total) continue;
    const int co0 = ct ? row0 - rho * p.Cout : row0;  // channel of tile row 0
    float bias_v[16], scale_v[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int coc = min(co0 + (q & 3) + 8 * (q >> 2) + 4 * h, p.Cout - 1);
      scale_v[q] = p.wscale[coc];
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
        v[q] = acc[m][j][q] * scale_v[q] + bias_v[q];  // × 2^−e is exact; no contraction (-ffp-contract=off), and none would change it
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
        const bool live = !p.len_ptr || pos < p.len_ptr[n] * p.len_mul;  // past the true length the image must hold zeros
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int cg = co0 + 8 * g + 4 * h;  // first of 4 consecutive channels
          uint2 o;
          o.x = live ? pack2_f16(lrelu1(v[4 * g], p.act_alpha), lrelu1(v[4 * g + 1], p.act_alpha)) : 0u;
          o.y = live ? pack2_f16(lrelu1(v[4 * g + 2], p.act_alpha), lrelu1(v[4 * g + 3], p.act_alpha)) : 0u;
          if (okc && cg < p.Cout) {
            uint2* ap = (uint2*)((uint4*)p.act + ((int64_t)n * ACB + (cg >> 3)) * p.act_row + kC8Halo + pos) + ((cg >> 2) & 1);
            *ap = o;
          }
        }
      }
    }
  }
}

template <int MTW, int NTW, int WM, bool LDSW>
void launch_inst(hipStream_t s, const ConvF16Multi& a, int batch, dim3 grid, size_t lds) {
  static bool done[kMaxDevices] = {};  // more than the 64 KB default needs the opt-in (160 KB per CU on gfx950), per device
  if (lds > 64 * 1024 && lds_optin_needed(done))
    (void)hipFuncSetAttribute((const void*)conv_f16_kernel<MTW, NTW, WM, LDSW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
  hipLaunchKernelGGL((conv_f16_kernel<MTW, NTW, WM, LDSW>), grid, dim3(kBT), lds, s, a, batch);
}

int launch_cfg(hipStream_t s, const ConvF16Multi& a, int batch, int MTW, int NTW, int WM, bool ring, dim3 grid, size_t lds) {
#define PH_F16_CASE(M, NT_, W_)                                  \
  if (MTW == M && NTW == NT_ && WM == W_) {                      \
    if (ring) launch_inst<M, NT_, W_, true>(s, a, batch, grid, lds); \
    else launch_inst<M, NT_, W_, false>(s, a, batch, grid, lds); \
  } else
  PH_F16_CASE(1, 1, 1) PH_F16_CASE(1, 2, 1) PH_F16_CASE(1, 4, 1)
  PH_F16_CASE(1, 1, 2) PH_F16_CASE(1, 2, 2) PH_F16_CASE(1, 4, 2)
  // (no <2, ·, 2>: two waves along rows means the row-tile count is no multiple of 4, so no wave gets a second tile)
  PH_F16_CASE(1, 1, 4) PH_F16_CASE(1, 2, 4) PH_F16_CASE(1, 4, 4)
  PH_F16_CASE(2, 1, 4) PH_F16_CASE(2, 2, 4) PH_F16_CASE(2, 4, 4)
  PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "conv_f16: no instance for MTW=%d NTW=%d WM=%d", MTW, NTW, WM);
#undef PH_F16_CASE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "conv_f16 launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

// waves along rows: as many of the 4 as the row-tile count allows (ConvTranspose: a wave's tiles stay in one phase)
int waves_along_rows(int per_phase) { return (per_phase % 4 == 0) ? 4 : (per_phase % 2 == 0) ? 2 : 1; }
// the window of a block of `cols` columns and the dump slot
size_t window_bytes(int Cin, int cols, int reach) { return (size_t)(Cin / 8) * (cols + reach) * 16 + 16; }

int pack_weights(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, int pad, uint16_t* packed, float* scale) {
  const bool ct = stride > 0;
  const int64_t total = (int64_t)(ct ? packed_convt_bf16_elems(Cin, Cout, K, stride) : packed_conv_bf16_elems(Cout, Cin, K));
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(total, kBT), 4096));
  hipLaunchKernelGGL(row_scale_f16_kernel, dim3((unsigned)Cout), dim3(kBT), 0, s, w, Cout, Cin, K, ct ? 1 : 0, scale);
  if (ct)
    hipLaunchKernelGGL(pack_convt_f16_kernel, grid, dim3(kBT), 0, s, w, (const float*)scale, Cin, Cout, K, stride, pad, packed, total);
  else
    hipLaunchKernelGGL(pack_conv_f16_kernel, grid, dim3(kBT), 0, s, w, (const float*)scale, Cout, Cin, K, packed, total);
  return PIPER_HIP_OK;
}

}  // namespace

int pack_conv_weights_f16(hipStream_t s, const float* w, int Cout, int Cin, int K, uint16_t* packed, float* scale) {
  return pack_weights(s, w, Cin, Cout, K, 0, 0, packed, scale);
}
int pack_convt_weights_f16(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, int pad, uint16_t* packed, float* scale) {
  return pack_weights(s, w, Cin, Cout, K, stride, pad, packed, scale);
}
int pack_act_c8_f16(hipStream_t s, const float* x, int N, int C, int L, float alpha, uint16_t* act, int64_t row, const int* len_ptr) {
  if (N <= 0 || C <= 0 || L <= 0) return PIPER_HIP_OK;
  if (row <= 0) row = c8_row_len(L);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(L, kBT), 1024), (unsigned)((C + 7) / 8), (unsigned)N);
  hipLaunchKernelGGL(pack_act_c8_f16_kernel, grid, dim3(kBT), 0, s, x, C, L, row, alpha, act, len_ptr);
  return PIPER_HIP_OK;
}
int pack_mean3_c8_f16(hipStream_t s, const float* a, const float* b, const float* c, int N, int C, int L, float alpha, uint16_t* act, int64_t row,
                      const int* len_ptr, int len_mul) {
  if (N <= 0 || C <= 0 || L <= 0) return PIPER_HIP_OK;
  if (C & 7) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "pack_mean3_c8_f16: %d channels (multiples of 8)", C);
  if (row <= 0) row = c8_row_len(L);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(L, kBT), 1024), (unsigned)(C / 8), (unsigned)N);
  hipLaunchKernelGGL(pack_mean3_c8_f16_kernel, grid, dim3(kBT), 0, s, a, b, c, C, L, row, alpha, act, len_ptr, len_mul);
  return PIPER_HIP_OK;
}
bool conv_f16_fits(int row_tiles, int Cin, int reach) { return window_bytes(Cin, 4 / waves_along_rows(row_tiles) * 32, reach) <= kLdsMax; }

int launch_conv_f16(piper_hip_ctx* ctx, hipStream_t s, const ConvF16Args& a) { return launch_conv_f16_multi(ctx, s, &a, 1); }

int launch_conv_f16_multi(piper_hip_ctx* ctx, hipStream_t s, const ConvF16Args* convs, int count) {
  if (count < 1 || count > kBf16Multi) PH_FAIL(PIPER_HIP_ERR_ARG, "conv_f16: %d convs in one launch (1..%d)", count, kBf16Multi);
  const ConvF16Args& a = convs[0];
  if (a.N <= 0 || a.Lout <= 0) return PIPER_HIP_OK;
  const bool ct = a.ct_stride > 0;
  const int rows = ct ? a.Cout * a.ct_stride : a.Cout;
  const int MT = (rows + 31) / 32;
  auto reach_of = [&](const ConvF16Args& b) { return ct ? convt_reach(b.K, b.ct_stride, b.ct_pad) : conv_reach(b.K, b.dil); };
  int reach = 0;
  for (int i = 0; i < count; i++) {
    const ConvF16Args& b = convs[i];
    if (b.N != a.N || b.Cin != a.Cin || b.Cout != a.Cout || b.Lout != a.Lout || b.ct_stride != a.ct_stride || b.x_row != a.x_row)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "conv_f16: convs of one launch must share N, Cin, Cout, Lout, row length and kind");
    if (!b.wscale) PH_FAIL(PIPER_HIP_ERR_ARG, "conv_f16: a weight image without its scales");
    if ((int64_t)8 * (ct ? b.K / b.ct_stride : b.K) * (b.Cin / 16) * 1024 + 16 * 1024 > 0x7fffffff)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "conv_f16: a block's weight fragments exceed 32-bit offsets");
    reach = std::max(reach, reach_of(b));
  }
  const int per_phase = ct ? a.Cout / 32 : MT;
  const int WM = waves_along_rows(per_phase), WN = 4 / WM;
  int MTW = (per_phase % (2 * WM) == 0) ? 2 : 1;
  int NTW = 4;
  auto blocks = [&](int mtw, int ntw) { return ceil_div(MT, WM * mtw) * ceil_div(a.Lout, WN * ntw * 32) * a.N * count; };
  // the bf16 launcher's rule: the widest column block whose window fits LDS; then narrower tiles until every CU has two blocks
  const int64_t want = 2 * (int64_t)ctx->num_cus;
  while (NTW > 1 && (blocks(MTW, NTW) < want || window_bytes(a.Cin, WN * NTW * 32, reach) > kLdsMax)) NTW >>= 1;
  if (MTW == 2 && blocks(MTW, NTW) < want) MTW = 1;
  const size_t window = window_bytes(a.Cin, WN * NTW * 32, reach);
  if (window > kLdsMax) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "conv_f16: window of %zu bytes does not fit LDS (Cin=%d reach=%d)", window, a.Cin, reach);
  // the LDS weight ring where it leaves room for a second block on the CU; else the per-wave register ring from L2
  const bool ring = 2 * (window + kRingBytes) <= kLdsMax;
  const size_t lds = window + (ring ? kRingBytes : 0);
  const dim3 grid((unsigned)ceil_div(a.Lout, WN * NTW * 32), (unsigned)ceil_div(MT, WM * MTW), (unsigned)(a.N * count));
  ConvF16Multi multi;
  for (int i = 0; i < kBf16Multi; i++) multi.c[i] = convs[i < count ? i : 0];
  const int rc = launch_cfg(s, multi, a.N, MTW, NTW, WM, ring, grid, lds);
  if (!rc)
    for (int i = 0; i < count; i++)
      PH_ROUTE(ctx, convs[i].Cout, convs[i].Cin, convs[i].Lout, convs[i].N, "f16 K=%d MTW=%d NTW=%d WM=%d wsrc=%s multi=%d %s", convs[i].K, MTW, NTW, WM,
               ring ? "lds" : "l2", count, ct ? "convT" : "conv");
  return rc;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(conv_f16, pack_conv_f16_kernel); } }
