// eq.hip — the output equaliser: a cascade of up to four biquads in double, on the device (include/piper_hip.h "Equaliser").
//
// The cascade is a linear recurrence over a state of D = 2n doubles, so an item is cut into blocks of B = 64 samples anchored at sample
// 0, and the contract's block tree makes the parallel form exact: every block's start state is a fixed fold of aggregates that only
// depend on the block's absolute place. Whole items take three launches:
//   ends    one lane per block, 128 blocks per workgroup: the samples are staged through LDS with 16-byte loads, every lane runs its
//           block from zero state (E), then the workgroup builds tree levels 1 … 7 in LDS; every level goes to the work buffer
//   top     one workgroup per item builds the levels above a workgroup from the level-7 aggregates (skipped for items of one workgroup)
//   apply   every lane folds its block's start state from the levels (highest set bit first), runs its block again and writes y through
//           the same LDS tile, 16-byte stores
// Every sum runs in the contract's order and nothing is atomic: the same samples give the same bits, and the host twin
// (piper_hip_eq_from_f32) computes the same tree.
#include "eq.h"

#include <algorithm>
#include <cmath>
#include <memory>

#include "pcm16.h"

#pragma clang fp contract(off)

namespace ph {
namespace {

__host__ __device__ inline double eq_read(float v) {  // a non-finite sample reads as 0
  union { float f; uint32_t u; } c;
  c.f = v;
  return (c.u & 0x7f800000u) == 0x7f800000u ? 0.0 : (double)v;
}

// one sample through the cascade (st: D doubles)
template <int NS>
__host__ __device__ __forceinline__ double eq_sample(double* st, double v, const double (*co)[5]) {
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const double y = co[i][0] * v + st[2 * i];
    st[2 * i] = (co[i][1] * v - co[i][3] * y) + st[2 * i + 1];
    st[2 * i + 1] = co[i][2] * v - co[i][4] * y;
    v = y;
  }
  return v;
}

// out = P·S + T, the sums over ascending j from the j = 0 product (out may not alias S)
template <int D>
__host__ __device__ __forceinline__ void eq_mv(const double* __restrict__ P, const double* S, const double* T, double* out) {
#pragma unroll
  for (int i = 0; i < D; i++) {
    double s = P[i * kEqMaxD] * S[0];
#pragma unroll
    for (int j = 1; j < D; j++) s = s + P[i * kEqMaxD + j] * S[j];
    out[i] = s + T[i];
  }
}

__device__ __forceinline__ int64_t eq_item_len(const int* lensF, int F, int hop, int64_t n_flat, int b) {
  return lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
}

// The tile of workgroup g: samples [base, base + 128·64) of x into xs[block][kEqStride], zeros past n. 16-byte loads where x is aligned.
__device__ __forceinline__ void eq_stage(const float* __restrict__ x, int64_t base, int64_t n, float* xs) {
  const int tid = threadIdx.x;
  const int64_t have = std::min<int64_t>(kEqWgBlocks * kEqBlock, n - base);
  if (((uintptr_t)x & 15) == 0) {
    for (int q = tid; q < kEqWgBlocks * kEqBlock / 4; q += kEqWgBlocks) {
      const int i = q * 4;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (i + 4 <= have) {
        v = *(const float4*)(x + base + i);
      } else {
        if (i < have) v.x = x[base + i];
        if (i + 1 < have) v.y = x[base + i + 1];
        if (i + 2 < have) v.z = x[base + i + 2];
      }
      float* d = xs + (i >> 6) * kEqStride + (i & 63);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = tid; i < kEqWgBlocks * kEqBlock; i += kEqWgBlocks) xs[(i >> 6) * kEqStride + (i & 63)] = i < have ? x[base + i] : 0.0f;
  }
}

template <int NS>
__device__ __forceinline__ void eq_coeffs(const EqDesign* __restrict__ d, double (*co)[5]) {
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int c = 0; c < 5; c++) co[i][c] = d->co[i][c];
}

// launch 1: E of every block, levels 0 … 7 of the tree
template <int NS>
__global__ __launch_bounds__(kEqWgBlocks) void eq_ends_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F,
                                                              int hop, int64_t n_flat, const EqDesign* __restrict__ d, double* __restrict__ work,
                                                              int64_t work_row, int64_t Kmax) {
  constexpr int D = 2 * NS;
  __shared__ float xs[kEqWgBlocks * kEqStride];
  __shared__ double tl[2][kEqWgBlocks][D];
  const int b = blockIdx.y, r = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int64_t n = eq_item_len(lensF, F, hop, n_flat, b), K = eq_blocks(n);
  if (g * kEqWgBlocks >= K) return;  // (uniform)
  const float* x = audio + (int64_t)b * row;
  eq_stage(x, g * kEqWgBlocks * kEqBlock, n, xs);
  double co[NS][5];
  eq_coeffs<NS>(d, co);
  __syncthreads();
  const int64_t k = g * kEqWgBlocks + r;
  const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(kEqBlock, n - k * kEqBlock));
  double st[D];
#pragma unroll
  for (int j = 0; j < D; j++) st[j] = 0.0;
  for (int i = 0; i < cnt; i++) (void)eq_sample<NS>(st, eq_read(xs[r * kEqStride + i]), co);
  double* T = work + (int64_t)b * work_row;
#pragma unroll
  for (int j = 0; j < D; j++) tl[0][r][j] = st[j];
  if (k < K)
#pragma unroll
    for (int j = 0; j < D; j++) T[k * D + j] = st[j];
  __syncthreads();
  int64_t off = 0;  // entries before level l + 1
  for (int l = 0; l < kEqWgLevels; l++) {
    off += eq_level_count(Kmax, l);
    const int cur = l & 1, m = kEqWgBlocks >> (l + 1);
    if (r < m) {
      double o[D];
      eq_mv<D>(d->P[l], tl[cur][2 * r], tl[cur][2 * r + 1], o);
#pragma unroll
      for (int j = 0; j < D; j++) tl[cur ^ 1][r][j] = o[j];
      const int64_t gi = g * m + r;
      if (gi < eq_level_count(K, l + 1))
#pragma unroll
        for (int j = 0; j < D; j++) T[(off + gi) * D + j] = o[j];
    }
    __syncthreads();
  }
}

// launch 2: the levels above a workgroup, one workgroup per item; T_{l+1}[m] only where both halves exist (the only ones a fold reads)
template <int NS>
__global__ __launch_bounds__(kEqTopLanes) void eq_top_kernel(const int* __restrict__ lensF, int F, int hop, int64_t n_flat,
                                                             const EqDesign* __restrict__ d, double* __restrict__ work, int64_t work_row,
                                                             int64_t Kmax) {
  constexpr int D = 2 * NS;
  const int b = blockIdx.x;
  const int64_t K = eq_blocks(eq_item_len(lensF, F, hop, n_flat, b));
  double* T = work + (int64_t)b * work_row;
  int64_t off = 0;  // entries before level l
  for (int l = 0; l < kEqWgLevels; l++) off += eq_level_count(Kmax, l);
  for (int l = kEqWgLevels; l < kEqLevels; l++) {
    const int64_t half = eq_level_count(K, l) >> 1, next = off + eq_level_count(Kmax, l);
    if (half == 0) break;  // (uniform)
    for (int64_t m = threadIdx.x; m < half; m += kEqTopLanes) {
      double o[D];
      eq_mv<D>(d->P[l], T + (off + 2 * m) * D, T + (off + 2 * m + 1) * D, o);
#pragma unroll
      for (int j = 0; j < D; j++) T[(next + m) * D + j] = o[j];
    }
    __syncthreads();
    off = next;
  }
}

// launch 3: the start state of every block, the block from it, y through the tile
template <int NS>
__global__ __launch_bounds__(kEqWgBlocks) void eq_apply_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F,
                                                               int hop, int64_t n_flat, const EqDesign* __restrict__ d,
                                                               const double* __restrict__ work, int64_t work_row, int64_t Kmax,
                                                               float* __restrict__ out, int64_t out_row) {
  constexpr int D = 2 * NS;
  __shared__ float xs[kEqWgBlocks * kEqStride];
  const int b = blockIdx.y, r = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int64_t n = eq_item_len(lensF, F, hop, n_flat, b), K = eq_blocks(n);
  if (g * kEqWgBlocks >= K) return;  // (uniform)
  const float* x = audio + (int64_t)b * row;
  const int64_t base = g * kEqWgBlocks * kEqBlock;
  eq_stage(x, base, n, xs);
  double co[NS][5];
  eq_coeffs<NS>(d, co);
  const int64_t k = g * kEqWgBlocks + r;
  const double* T = work + (int64_t)b * work_row;
  double S[D];
#pragma unroll
  for (int j = 0; j < D; j++) S[j] = 0.0;
  // the levels a block of this item can need: the bits of K − 1; off walks down from the entries before level top + 1
  int top = 0;
  while (top + 1 < kEqLevels && ((K - 1) >> (top + 1)) != 0) top++;
  int64_t off = 0;
  for (int l = 0; l <= top; l++) off += eq_level_count(Kmax, l);
  for (int l = top; l >= 0; l--) {
    off -= eq_level_count(Kmax, l);
    if (k < K && ((k >> l) & 1)) {
      double o[D];
      eq_mv<D>(d->P[l], S, T + (off + (k >> l) - 1) * D, o);
#pragma unroll
      for (int j = 0; j < D; j++) S[j] = o[j];
    }
  }
  __syncthreads();
  const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(kEqBlock, n - k * kEqBlock));
  for (int i = 0; i < cnt; i++) {
    float* p = xs + r * kEqStride + i;
    *p = (float)eq_sample<NS>(S, eq_read(*p), co);
  }
  __syncthreads();
  float* y = out + (int64_t)b * out_row + base;
  const int64_t have = std::min<int64_t>(kEqWgBlocks * kEqBlock, n - base);
  if (((uintptr_t)y & 15) == 0) {
    for (int q = threadIdx.x; q < kEqWgBlocks * kEqBlock / 4; q += kEqWgBlocks) {
      const int i = q * 4;
      if (i >= have) break;
      const float* s = xs + (i >> 6) * kEqStride + (i & 63);
      if (i + 4 <= have) {
        *(float4*)(y + i) = make_float4(s[0], s[1], s[2], s[3]);
      } else {
        for (int c = 0; c < have - i; c++) y[i + c] = s[c];
      }
    }
  } else {
    for (int i = threadIdx.x; i < have; i += kEqWgBlocks) y[i] = xs[(i >> 6) * kEqStride + (i & 63)];
  }
}

template <int NS>
hipError_t eq_launch(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat, const EqDesign* d,
                     double* work, float* out, int64_t out_row) {
  const int64_t n_max = lensF ? (int64_t)F * hop : n_flat;
  if (n_max <= 0) return hipSuccess;
  const int64_t Kmax = ceil_div(n_max, kEqBlock), groups = ceil_div(Kmax, kEqWgBlocks), work_row = eq_work_row(n_max, 2 * NS);
  if (groups > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eq_ends_kernel<NS>, dim3((unsigned)groups, NB), dim3(kEqWgBlocks), 0, q, audio, row, lensF, F, hop, n_flat, d, work, work_row, Kmax);
  if (groups > 1) hipLaunchKernelGGL(eq_top_kernel<NS>, dim3(NB), dim3(kEqTopLanes), 0, q, lensF, F, hop, n_flat, d, work, work_row, Kmax);
  hipLaunchKernelGGL(eq_apply_kernel<NS>, dim3((unsigned)groups, NB), dim3(kEqWgBlocks), 0, q, audio, row, lensF, F, hop, n_flat, d,
                     (const double*)work, work_row, Kmax, out, out_row);
  return hipGetLastError();
}

// One stream step, one wave per generator row. The carry holds T_l[(k0 >> l) − 1] at every set bit l of the row's block count k0; a
// row at the start of its item (k0 = 0) reads none of it, so a pool row's new occupant never sees its predecessor's. Lanes run the
// chunk's blocks from zero state (E), then the first D lanes take the blocks in order as a binary counter — the start state of block
// k0 + j is the fold of the carry (highest level first), then E[j] is pushed, merging equal levels — and last every lane runs its
// blocks again from their start states. Every global read of the carry comes before any write of it.
template <int NS>
__global__ __launch_bounds__(64) void eq_step_kernel(const float* __restrict__ audio, int64_t row, const EqStepRow* __restrict__ desc,
                                                     const EqDesign* __restrict__ d, double* __restrict__ carry, double* __restrict__ scratch,
                                                     int blocks, float* __restrict__ out) {
  constexpr int D = 2 * NS;
  __shared__ double cs[kEqLevels + 1][kEqMaxD];
  __shared__ double sv[kEqMaxD], ov[kEqMaxD];
  const int r = blockIdx.x, tid = threadIdx.x;
  const EqStepRow dr = desc[r];
  const int n = min(max(dr.n, 0), blocks * kEqBlock);
  if (n == 0) return;  // (uniform)
  const float* x = audio + (int64_t)r * row + dr.skip;
  float* y = out + (int64_t)r * row + dr.skip;
  double* C = carry + (int64_t)r * kEqCarry;
  double* E = scratch + (int64_t)r * blocks * 2 * kEqMaxD;
  const int64_t k0 = dr.s / kEqBlock;
  const int nb = (n + kEqBlock - 1) / kEqBlock;
  double co[NS][5];
  eq_coeffs<NS>(d, co);
  for (int i = tid; i < kEqCarry; i += 64) {
    const int l = i / kEqMaxD;
    cs[l][i % kEqMaxD] = ((k0 >> l) & 1) ? C[i] : 0.0;
  }
  for (int j = tid; j < nb; j += 64) {
    double st[D];
#pragma unroll
    for (int c = 0; c < D; c++) st[c] = 0.0;
    const int cnt = min(kEqBlock, n - j * kEqBlock);
    for (int i = 0; i < cnt; i++) (void)eq_sample<NS>(st, eq_read(x[j * kEqBlock + i]), co);
#pragma unroll
    for (int c = 0; c < D; c++) E[j * 2 * kEqMaxD + c] = st[c];
  }
  __syncthreads();
  for (int j = 0; j < nb; j++) {
    const int64_t k = k0 + j;
    if (tid < D) sv[tid] = 0.0;
    __syncthreads();
    for (int l = kEqLevels - 1; l >= 0; l--) {  // (uniform) the fold, highest set bit first (blocks < 2^34)
      if (!((k >> l) & 1)) continue;
      double o = 0.0;
      if (tid < D) {
        const double* P = d->P[l];
        o = P[tid * kEqMaxD] * sv[0];
        for (int c = 1; c < D; c++) o = o + P[tid * kEqMaxD + c] * sv[c];
        o = o + cs[l][tid];
      }
      __syncthreads();
      if (tid < D) sv[tid] = o;
      __syncthreads();
    }
    if (tid < D) {
      E[j * 2 * kEqMaxD + kEqMaxD + tid] = sv[tid];
      ov[tid] = E[j * 2 * kEqMaxD + tid];
    }
    __syncthreads();
    int l = 0;
    for (; l < kEqLevels && ((k >> l) & 1); l++) {  // (uniform) the push: equal levels merge, the earlier aggregate on the left
      double o = 0.0;
      if (tid < D) {
        const double* P = d->P[l];
        o = P[tid * kEqMaxD] * cs[l][0];
        for (int c = 1; c < D; c++) o = o + P[tid * kEqMaxD + c] * cs[l][c];
        o = o + ov[tid];
      }
      __syncthreads();
      if (tid < D) ov[tid] = o;
      __syncthreads();
    }
    if (tid < D) cs[l][tid] = ov[tid];
    __syncthreads();
  }
  for (int i = tid; i < kEqCarry; i += 64) C[i] = cs[i / kEqMaxD][i % kEqMaxD];
  for (int j = tid; j < nb; j += 64) {
    double st[D];
#pragma unroll
    for (int c = 0; c < D; c++) st[c] = E[j * 2 * kEqMaxD + kEqMaxD + c];
    const int cnt = min(kEqBlock, n - j * kEqBlock);
    for (int i = 0; i < cnt; i++) y[j * kEqBlock + i] = (float)eq_sample<NS>(st, eq_read(x[j * kEqBlock + i]), co);
  }
}

void mat_mul(const double* a, const double* b, double* c, int D) {  // c = a·b at stride kEqMaxD, the contract's order
  double r[kEqMaxD * kEqMaxD] = {};
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) {
      double s = a[i * kEqMaxD] * b[j];
      for (int k = 1; k < D; k++) s = s + a[i * kEqMaxD + k] * b[k * kEqMaxD + j];
      r[i * kEqMaxD + j] = s;
    }
  memcpy(c, r, sizeof(r));
}

// the cascade's state after one sample, on the host at run-time n
double host_sample(double* st, double v, const EqDesign& d) {
  for (int i = 0; i < d.n; i++) {
    const double* c = d.co[i];
    const double y = c[0] * v + st[2 * i];
    st[2 * i] = (c[1] * v - c[3] * y) + st[2 * i + 1];
    st[2 * i + 1] = c[2] * v - c[4] * y;
    v = y;
  }
  return v;
}

void host_mv(const double* P, const double* S, const double* T, double* out, int D) {
  for (int i = 0; i < D; i++) {
    double s = P[i * kEqMaxD] * S[0];
    for (int j = 1; j < D; j++) s = s + P[i * kEqMaxD + j] * S[j];
    out[i] = s + T[i];
  }
}

PH_WARM(eq, eq_apply_kernel<4>);

}  // namespace

hipError_t launch_eq_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                           const EqDesign* d, int n, double* work, float* out, int64_t out_row) {
  if (NB < 1 || (!lensF && NB != 1)) return hipErrorInvalidValue;
  switch (n) {
    case 1: return eq_launch<1>(q, audio, row, lensF, F, hop, NB, n_flat, d, work, out, out_row);
    case 2: return eq_launch<2>(q, audio, row, lensF, F, hop, NB, n_flat, d, work, out, out_row);
    case 3: return eq_launch<3>(q, audio, row, lensF, F, hop, NB, n_flat, d, work, out, out_row);
    case 4: return eq_launch<4>(q, audio, row, lensF, F, hop, NB, n_flat, d, work, out, out_row);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_eq_step(hipStream_t q, int rows, int max_in, const float* audio, int64_t row, const EqStepRow* desc, const EqDesign* d, int n,
                          double* carry, double* scratch, float* out) {
  if (rows < 1 || max_in < 1) return hipErrorInvalidValue;
  const int blocks = (max_in + kEqBlock - 1) / kEqBlock;
  switch (n) {
    case 1: hipLaunchKernelGGL(eq_step_kernel<1>, dim3(rows), dim3(64), 0, q, audio, row, desc, d, carry, scratch, blocks, out); break;
    case 2: hipLaunchKernelGGL(eq_step_kernel<2>, dim3(rows), dim3(64), 0, q, audio, row, desc, d, carry, scratch, blocks, out); break;
    case 3: hipLaunchKernelGGL(eq_step_kernel<3>, dim3(rows), dim3(64), 0, q, audio, row, desc, d, carry, scratch, blocks, out); break;
    case 4: hipLaunchKernelGGL(eq_step_kernel<4>, dim3(rows), dim3(64), 0, q, audio, row, desc, d, carry, scratch, blocks, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

int eq_build(const piper_hip_eq* eq, int rate, EqDesign* out) {
  if (int rc = piper_hip_eq_check(eq, rate)) return rc;
  memset(out, 0, sizeof(*out));
  out->n = eq->n;
  if (int rc = piper_hip_eq_design(eq, rate, out->co)) return rc;
  const int D = 2 * eq->n;
  double A[kEqMaxD * kEqMaxD] = {};
  for (int j = 0; j < D; j++) {  // column j: unit state j, one sample without input
    double st[kEqMaxD] = {};
    st[j] = 1.0;
    (void)host_sample(st, 0.0, *out);
    for (int i = 0; i < D; i++) A[i * kEqMaxD + j] = st[i];
  }
  for (int i = 0; i < 6; i++) mat_mul(A, A, A, D);
  static_assert(kEqBlock == 64, "A^64 is six squarings");
  memcpy(out->P[0], A, sizeof(A));
  for (int l = 1; l < kEqLevels; l++) mat_mul(out->P[l - 1], out->P[l - 1], out->P[l], D);
  return PIPER_HIP_OK;
}

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_eq_check(const piper_hip_eq* eq, int32_t rate) {
  if (!eq) PH_FAIL(PIPER_HIP_ERR_ARG, "eq: null eq");
  if (!(rate >= 8000 && rate <= 48000)) PH_FAIL(PIPER_HIP_ERR_ARG, "eq: rate %d outside [8000, 48000]", (int)rate);
  if (eq->n < 1 || eq->n > kEqMaxSec) PH_FAIL(PIPER_HIP_ERR_ARG, "eq: n %d outside 1 … %d", (int)eq->n, kEqMaxSec);
  for (int i = 0; i < eq->n; i++) {
    const piper_hip_eq_section& s = eq->section[i];
    if (s.type < PIPER_HIP_EQ_LOWPASS || s.type > PIPER_HIP_EQ_HIGHSHELF)
      PH_FAIL(PIPER_HIP_ERR_ARG, "eq: section[%d].type %d outside 1 … 7", i, (int)s.type);
    if (!(std::isfinite(s.f0_hz) && (double)s.f0_hz >= 10.0 && (double)s.f0_hz <= 0.45 * (double)rate))
      PH_FAIL(PIPER_HIP_ERR_ARG, "eq: section[%d].f0_hz %g outside [10, %g]", i, (double)s.f0_hz, 0.45 * (double)rate);
    if (!(std::isfinite(s.q) && s.q >= 0.1f && s.q <= 30.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "eq: section[%d].q %g outside [0.1, 30]", i, (double)s.q);
    const bool gains = s.type == PIPER_HIP_EQ_PEAKING || s.type == PIPER_HIP_EQ_LOWSHELF || s.type == PIPER_HIP_EQ_HIGHSHELF;
    if (gains && !(std::isfinite(s.gain_db) && s.gain_db >= -30.0f && s.gain_db <= 30.0f))
      PH_FAIL(PIPER_HIP_ERR_ARG, "eq: section[%d].gain_db %g outside [-30, 30]", i, (double)s.gain_db);
    if (!gains && s.gain_db != 0.0f)
      PH_FAIL(PIPER_HIP_ERR_ARG, "eq: section[%d].gain_db %g: type %d takes no gain (exactly 0)", i, (double)s.gain_db, (int)s.type);
  }
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_eq_design(const piper_hip_eq* eq, int32_t rate, double coeffs[][5]) {
  if (int rc = piper_hip_eq_check(eq, rate)) return rc;
  if (!coeffs) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_design: null output");
  const double fs = (double)rate;
  for (int i = 0; i < eq->n; i++) {
    const piper_hip_eq_section& sec = eq->section[i];
    const double f0 = sec.f0_hz, Q = sec.q, g = sec.gain_db;
    const double w0 = 2.0 * M_PI * f0 / fs;
    const double c = std::cos(w0), s = std::sin(w0);
    const double alpha = s / (2.0 * Q);
    const double A = std::pow(10.0, g / 40.0);
    double b0, b1, b2, a0, a1, a2;
    switch (sec.type) {
      case PIPER_HIP_EQ_LOWPASS:
        b0 = (1.0 - c) / 2.0; b1 = 1.0 - c; b2 = (1.0 - c) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * c; a2 = 1.0 - alpha;
        break;
      case PIPER_HIP_EQ_HIGHPASS:
        b0 = (1.0 + c) / 2.0; b1 = -(1.0 + c); b2 = (1.0 + c) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * c; a2 = 1.0 - alpha;
        break;
      case PIPER_HIP_EQ_BANDPASS:
        b0 = alpha; b1 = 0.0; b2 = -alpha;
        a0 = 1.0 + alpha; a1 = -2.0 * c; a2 = 1.0 - alpha;
        break;
      case PIPER_HIP_EQ_NOTCH:
        b0 = 1.0; b1 = -2.0 * c; b2 = 1.0;
        a0 = 1.0 + alpha; a1 = -2.0 * c; a2 = 1.0 - alpha;
        break;
      case PIPER_HIP_EQ_PEAKING:
        b0 = 1.0 + alpha * A; b1 = -2.0 * c; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * c; a2 = 1.0 - alpha / A;
        break;
      case PIPER_HIP_EQ_LOWSHELF: {
        const double r = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) - (A - 1.0) * c + r);
        b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * c);
        b2 = A * ((A + 1.0) - (A - 1.0) * c - r);
        a0 = (A + 1.0) + (A - 1.0) * c + r;
        a1 = -2.0 * ((A - 1.0) + (A + 1.0) * c);
        a2 = (A + 1.0) + (A - 1.0) * c - r;
        break;
      }
      default: {  // PIPER_HIP_EQ_HIGHSHELF (the check admits nothing else)
        const double r = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) + (A - 1.0) * c + r);
        b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * c);
        b2 = A * ((A + 1.0) + (A - 1.0) * c - r);
        a0 = (A + 1.0) - (A - 1.0) * c + r;
        a1 = 2.0 * ((A - 1.0) - (A + 1.0) * c);
        a2 = (A + 1.0) - (A - 1.0) * c - r;
        break;
      }
    }
    coeffs[i][0] = b0 / a0; coeffs[i][1] = b1 / a0; coeffs[i][2] = b2 / a0; coeffs[i][3] = a1 / a0; coeffs[i][4] = a2 / a0;
  }
  return PIPER_HIP_OK;
}

// the host twin of the kernels: the same block tree, every operation in the same order
PH_EXPORT int piper_hip_eq_from_f32(const piper_hip_eq* eq, int32_t rate, const float* x, size_t n, float* y) {
  std::vector<EqDesign> hold(1);
  EqDesign& d = hold[0];
  if (int rc = eq_build(eq, rate, &d)) return rc;
  if ((!x || !y) && n) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_from_f32: null buffer");
  if (n > ((size_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "eq_from_f32: %zu samples", n);
  if (n == 0) return PIPER_HIP_OK;
  const int D = 2 * d.n;
  const int64_t K = ceil_div((int64_t)n, kEqBlock);
  std::vector<std::vector<double>> T(1, std::vector<double>((size_t)K * D, 0.0));
  for (int64_t k = 0; k < K; k++) {
    double* st = &T[0][(size_t)k * D];
    for (int64_t i = k * kEqBlock; i < std::min<int64_t>((int64_t)n, (k + 1) * kEqBlock); i++) (void)host_sample(st, eq_read(x[i]), d);
  }
  for (int l = 0; (int64_t)(T[l].size() / D) > 1; l++) {
    const int64_t half = (int64_t)(T[l].size() / D) / 2;
    std::vector<double> nx((size_t)half * D);
    for (int64_t m = 0; m < half; m++) host_mv(d.P[l], &T[l][(size_t)(2 * m) * D], &T[l][(size_t)(2 * m + 1) * D], &nx[(size_t)m * D], D);
    T.push_back(std::move(nx));
  }
  for (int64_t k = 0; k < K; k++) {
    double S[kEqMaxD] = {}, o[kEqMaxD];
    for (int l = (int)T.size() - 1; l >= 0; l--) {
      if (!((k >> l) & 1)) continue;
      host_mv(d.P[l], S, &T[l][(size_t)((k >> l) - 1) * D], o, D);
      memcpy(S, o, sizeof(S));
    }
    for (int64_t i = k * kEqBlock; i < std::min<int64_t>((int64_t)n, (k + 1) * kEqBlock); i++) y[i] = (float)host_sample(S, eq_read(x[i]), d);
  }
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_eq_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, const piper_hip_eq* eq, float** out,
                               piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_f32: null output pointer");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_f32: null input");
  if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_f32: the output buffer is not 4-byte aligned");
  if (((uintptr_t)x & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "eq_f32: the input buffer is not 4-byte aligned");
  if (count > ((size_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "eq_f32: %zu samples", count);
  auto built = std::make_unique<EqDesign>();
  int rc = eq_build(eq, rate, built.get());
  if (rc) return rc;
  if (!*out) {
    void* q = nullptr;
    if ((rc = ctx->pool.alloc(count * sizeof(float), &q))) return rc;
    *out = (float*)q;
  }
  if (count == 0) return PIPER_HIP_OK;
  void *dd = nullptr, *work = nullptr;
  if ((rc = ctx->pool.alloc(sizeof(EqDesign), &dd))) return rc;
  defer_free(ctx, dd);
  if ((rc = ctx->pool.alloc((size_t)eq_work_row((int64_t)count, 2 * eq->n) * sizeof(double), &work))) return rc;
  defer_free(ctx, work);
  StreamScope ss(ctx, stream);
  // the copy may read the host design after this call returns: it is freed by the stream itself once the copy has run
  EqDesign* src = built.release();
  hipError_t e = hipMemcpyAsync(dd, src, sizeof(EqDesign), hipMemcpyHostToDevice, ss.s);
  if (e == hipSuccess) e = hipLaunchHostFunc(ss.s, [](void* p) { delete (EqDesign*)p; }, src);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ss.s);
    delete src;
    PH_FAIL(PIPER_HIP_ERR_LAUNCH, "eq_f32: %s", hipGetErrorString(e));
  }
  (void)launch_eq_items(ss.s, x, 0, nullptr, 0, 1, 1, (int64_t)count, (const EqDesign*)dd, eq->n, (double*)work, *out, 0);
  return ss.finish("eq_f32");
}
