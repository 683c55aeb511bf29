// speaker.hip — the request-path kernel of a multi-speaker voice (piper_hip.h "Multi-speaker voices"; DESIGN.md §4 "Speakers").
//
// VITS conditions on g = emb_g[sid] through k = 1 convs whose input has length 1 in time (in the graph: Gather, Conv, Add —
// GraphExecutor.swift:653-666, 1739-1810, 741-779), so each of them is a [rows × gin] · [gin] product that yields one constant per item
// and channel. One launch computes them for all N items of a plan as the items' EFFECTIVE BIASES e = b_own + (bc + W·g), which the
// conditioned convs then read where they read their own bias (ConvArgs::bias_batch_stride).
//
// At N = 1 this is a GEMV over rows · gin · 4 bytes of weights (medium: 6 400 rows × 512 = 13.1 MB for the flow and generator rows) and
// nothing else: memory-bound. So: a wave owns RW rows and sweeps them with 16-byte loads along gin (a row is contiguous: 64 lanes × 16 B =
// 1 KB per load instruction, RW of them in flight per sweep step), g sits in LDS, the dot products end in a wave reduction, and the grid
// is rows / (4 waves · RW) blocks — 800 blocks of 256 threads for the medium voice, three per CU.
// For N > 1 the items are TILED: a block forms g for NI ≤ 8 items in LDS and every weight fragment it loads is used for all of them, so the
// weights are read once per tile of 8 items (once per launch up to N = 8; beyond that the re-reads come from the Infinity Cache, which
// holds all 13.5 MB). The tile is done on the vector ALU, not on MFMA: per 16 weight bytes a lane issues 4 FMAs per item, 32 at NI = 8 —
// 32 wave instructions per KB of weights, ≈ 32 clocks of a CU's four SIMDs, against ≈ 100 clocks for its share of HBM bandwidth (≈ 10 B/clk)
// to deliver that KB: the kernel stays memory-bound, and an MFMA formulation would need the [rows × gin] · [gin × N] operands in
// fragment layout for a product that is at most 8 columns wide.
// Measured (profiles/speakers.md, medium, gin 512): 7.8 µs at N = 1, 17.2 µs at N = 8, against 2.1 µs for one read of the weights at
// 6.3 TB/s — at this size the launch is bound by latency (launch, table → g, one sweep), not by bandwidth.
#include "speaker.h"

namespace ph {
namespace {

// one item's mix → float4 j4 of g. Accumulated in fp32 from 0.0f in ascending k, product rounded, then the sum (never contracted): with
// n = 1, w = 1.0 the result is the table row. n and the ids are clamped: no record can make the load leave the table.
__device__ __forceinline__ float4 mix_g(const piper_hip_speaker& sp, const float* __restrict__ emb, int S, int gin, int j4) {
  float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int n = min(max(sp.n, 0), 4);
  for (int k = 0; k < n; k++) {
    const int id = min(max(sp.ids[k], 0), S - 1);
    const float w = sp.weights[k];
    const float4 e = *(const float4*)(emb + (int64_t)id * gin + 4 * j4);
    g.x = __fadd_rn(g.x, __fmul_rn(w, e.x));
    g.y = __fadd_rn(g.y, __fmul_rn(w, e.y));
    g.z = __fadd_rn(g.z, __fmul_rn(w, e.z));
    g.w = __fadd_rn(g.w, __fmul_rn(w, e.w));
  }
  return g;
}

// grid (row groups of 4·RW, item tiles of NI), 256 threads; dynamic LDS: NI · gin floats
template <int NI, int RW>
__global__ __launch_bounds__(256) void speaker_rows_kernel(const SpeakerTables t, const piper_hip_speaker* __restrict__ spk, const int N,
                                                           const int row0, const int rows, float* __restrict__ g_out,
                                                           float* __restrict__ bias_out) {
  extern __shared__ __attribute__((aligned(16))) float gs[];  // [NI][gin]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gin = t.gin, q4 = gin >> 2;  // gin % 4 == 0
  const int item0 = blockIdx.y * NI;
  const int rbase = row0 + ((int)blockIdx.x * 4 + wave) * RW;  // wave-uniform
  const int rlast = row0 + rows - 1;
  const bool has_rows = rbase <= rlast;
  // The weights do not depend on g: the wave's first two sweep steps (all of a row at gin ≤ 512) and its bias entries are requested
  // BEFORE the block forms g, so the launch pays one memory round trip for table → g and weights together instead of one after the other.
  const float* wr[RW];
#pragma unroll
  for (int r = 0; r < RW; r++) wr[r] = t.w + (int64_t)min(max(rbase, row0) + r, rlast) * gin;  // (a row past the end repeats the last one; it is not stored)
  float4 wpre[2][RW];
  float b_own[RW], b_cond[RW];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int col = c * 256 + 4 * lane;
#pragma unroll
    for (int r = 0; r < RW; r++) wpre[c][r] = (has_rows && col < gin) ? *(const float4*)(wr[r] + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
#pragma unroll
  for (int r = 0; r < RW; r++) {
    const int row = min(max(rbase, row0) + r, rlast);
    b_own[r] = has_rows ? t.b_own[row] : 0.0f;
    b_cond[r] = has_rows ? t.bc[row] : 0.0f;
  }
  for (int idx = tid; idx < NI * q4; idx += 256) {
    const int i = idx / q4, j4 = idx - i * q4;
    const int it = item0 + i;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (it < N) {
      g = mix_g(spk[it], t.emb, t.S, gin, j4);
      if (g_out && blockIdx.x == 0) *(float4*)(g_out + (int64_t)it * gin + 4 * j4) = g;
    }
    *(float4*)(gs + i * gin + 4 * j4) = g;
  }
  __syncthreads();
  if (!has_rows) return;
  float acc[RW][NI];
#pragma unroll
  for (int r = 0; r < RW; r++)
#pragma unroll
    for (int i = 0; i < NI; i++) acc[r][i] = 0.0f;
  // one sweep step: 256 columns from c0 on, the wave's RW weight fragments against g of the NI items (a column past gin: weight 0, g[0])
  auto sweep = [&](const float4 (&wv)[RW], int c0) {
    const int col = c0 + 4 * lane;
    const int colc = col < gin ? col : 0;
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const float4 gv = *(const float4*)(gs + i * gin + colc);
#pragma unroll
      for (int r = 0; r < RW; r++) {
        float a = acc[r][i];
        a = __builtin_fmaf(wv[r].x, gv.x, a);
        a = __builtin_fmaf(wv[r].y, gv.y, a);
        a = __builtin_fmaf(wv[r].z, gv.z, a);
        a = __builtin_fmaf(wv[r].w, gv.w, a);
        acc[r][i] = a;
      }
    }
  };
  sweep(wpre[0], 0);
  if (gin > 256) sweep(wpre[1], 256);
  for (int c0 = 512; c0 < gin; c0 += 256) {
    const int col = c0 + 4 * lane;
    float4 wv[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) wv[r] = col < gin ? *(const float4*)(wr[r] + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    sweep(wv, c0);
  }
#pragma unroll
  for (int r = 0; r < RW; r++)
#pragma unroll
    for (int i = 0; i < NI; i++) {
      float a = acc[r][i];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
      acc[r][i] = a;
    }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RW; r++) {
      const int row = rbase + r;
      if (row > rlast) break;
#pragma unroll
      for (int i = 0; i < NI; i++)
        if (item0 + i < N) bias_out[(int64_t)(item0 + i) * t.Ctot + row] = __fadd_rn(b_own[r], __fadd_rn(b_cond[r], acc[r][i]));
    }
  }
}

template <int NI, int RW>
void launch_t(hipStream_t s, const SpeakerTables& t, const piper_hip_speaker* spk, int N, int row0, int rows, float* g_out, float* bias_out) {
  const dim3 grid((unsigned)ceil_div(rows, 4 * RW), (unsigned)ceil_div(N, NI));
  hipLaunchKernelGGL((speaker_rows_kernel<NI, RW>), grid, dim3(256), (size_t)NI * t.gin * sizeof(float), s, t, spk, N, row0, rows, g_out, bias_out);
}

}  // namespace

int launch_speaker_rows(hipStream_t s, const SpeakerTables& t, const piper_hip_speaker* spk, int N, int row0, int rows, float* g_out,
                        float* bias_out) {
  if (!t.emb || !t.w || !t.bc || !t.b_own || !spk || !bias_out) PH_FAIL(PIPER_HIP_ERR_ARG, "speaker rows: null argument");
  if (t.S < 1 || t.gin < 4 || t.gin > 1024 || (t.gin & 3) || N < 1 || N > 65535 || row0 < 0 || rows < 0 || row0 + rows > t.Ctot)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "speaker rows: S %d gin %d N %d rows [%d, %d) of %d", t.S, t.gin, N, row0, row0 + rows, t.Ctot);
  if (rows == 0) return PIPER_HIP_OK;
  // one item: two rows per wave, for twice the blocks; more: four rows per wave share every read of g
  if (N == 1) launch_t<1, 2>(s, t, spk, N, row0, rows, g_out, bias_out);
  else if (N == 2) launch_t<2, 4>(s, t, spk, N, row0, rows, g_out, bias_out);
  else if (N <= 4) launch_t<4, 4>(s, t, spk, N, row0, rows, g_out, bias_out);
  else launch_t<8, 4>(s, t, spk, N, row0, rows, g_out, bias_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "speaker rows launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

namespace { PH_WARM(speaker, (speaker_rows_kernel<1, 2>)); }

}  // namespace ph
