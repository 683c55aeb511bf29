// level.hip — look-ahead limiter: a drive, a ceiling and a short, known delay, on the device (include/piper_hip.h "Level control").
//
// The limiter is a contract, tested bit for bit against a numpy restatement (tests/level_ref.py). All arithmetic is fp32, every operation
// rounded on its own (the library is built with -ffp-contract=off):
//   u[n]    = x[n]·drive
//   p[k]    = max |u| over block k of B = 32 samples (NaN ignored; 0 past the item),  r[k] = p[k] > ceiling ? ceiling / p[k] : 1
//   m[k]    = min(r[k] … r[k + W]), W = 6;   G[k] = min(m[k], G[k − 1] + rel), G[−1] = 1;   node[k] = min(G[k − 1], G[k])
//   y[n]    = u[n]·(node[k] + (node[k + 1] − node[k])·(i / 32)),  k = n div 32, i = n mod 32
// Whole items run three launches: block peaks → r (16-byte loads, eight lanes per block), the G recursion (one wave per item: 64 blocks
// per pass, the chain of one add and one min per block runs on values broadcast lane by lane), apply (float4). A stream step is one launch,
// one block per generator row: the row's carry — the samples u the previous step could not finish yet, and the last final G — and the new
// chunk give the peaks of the new blocks in LDS, one wave runs the chain, all threads write the limited samples and then the new carry.
// Every global read of the carry happens before the first barrier and every write after the last, so one buffer serves.
// Nothing is atomic or order-dependent.
#include "level.h"

#include <algorithm>
#include <cmath>

#include "pcm16.h"

#pragma clang fp contract(off)

namespace ph {
namespace {

constexpr size_t kLvLdsMax = 64 << 10;

__device__ __forceinline__ float lv_abs(float u) {  // |u|, NaN counts as 0
  const float a = fabsf(u);
  return a != a ? 0.0f : a;
}
__device__ __forceinline__ float lv_ratio(float peak, float ceiling) { return peak > ceiling ? __fdiv_rn(ceiling, peak) : 1.0f; }

// 64 consecutive blocks of the recursion on one wave: lane i brings m of block (base + i); G enters as G[base − 1] and leaves as
// G[base + 63], the same value on every lane. *prev / *mine: G[k − 1] and G[k] of the lane's own block.
__device__ __forceinline__ void lv_chain64(float m, float rel, float& G, float* prev, float* mine) {
  const int lane = threadIdx.x & 63;
  float pv = 0.0f, mn = 0.0f;
#pragma unroll
  for (int i = 0; i < 64; i++) {
    const float mi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), i));
    const float Gn = fminf(mi, G + rel);
    if (lane == i) { pv = G; mn = Gn; }
    G = Gn;
  }
  *prev = pv;
  *mine = mn;
}

// phase 1: r[b][k] for the blocks of item b. Eight lanes share a block, one float4 each; a thread block covers 32 blocks per pass.
__global__ __launch_bounds__(256) void level_peaks_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                          int64_t n_flat, const LvParams p, float* __restrict__ r, int64_t KR) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  const int64_t K = (n + kLvBlock - 1) / kLvBlock;
  const float* x = audio + (int64_t)b * row;
  float* rr = r + (int64_t)b * KR;
  const bool vec = ((uintptr_t)x & 15) == 0;
  for (int64_t kb = (int64_t)blockIdx.x * 32; kb < K; kb += (int64_t)gridDim.x * 32) {  // (uniform over the thread block: every lane shuffles)
    const int64_t k = kb + (tid >> 3), at = k * kLvBlock + (tid & 7) * 4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec && at + 4 <= n) {
      v = *(const float4*)(x + at);
    } else {
      if (at < n) v.x = x[at];
      if (at + 1 < n) v.y = x[at + 1];
      if (at + 2 < n) v.z = x[at + 2];
      if (at + 3 < n) v.w = x[at + 3];
    }
    float a = fmaxf(fmaxf(lv_abs(v.x * p.drive), lv_abs(v.y * p.drive)), fmaxf(lv_abs(v.z * p.drive), lv_abs(v.w * p.drive)));
    a = fmaxf(a, __shfl_xor(a, 4));
    a = fmaxf(a, __shfl_xor(a, 2));
    a = fmaxf(a, __shfl_xor(a, 1));
    if ((tid & 7) == 0 && k < K) rr[k] = lv_ratio(a, p.ceiling);
  }
}

// phase 2: node[b][0 … K] of item b, one wave per item
__global__ __launch_bounds__(64) void level_gain_kernel(const int* __restrict__ lensF, int F, int hop, int64_t n_flat, const LvParams p,
                                                        const float* __restrict__ r, float* __restrict__ node, int64_t KR) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  const int64_t Kn = (n + kLvBlock - 1) / kLvBlock, K = Kn < KR ? Kn : KR;
  const float* rr = r + (int64_t)b * KR;
  float* nd = node + (int64_t)b * (KR + 1);
  float G = 1.0f;
  for (int64_t base = 0; base <= K; base += 64) {
    const int64_t k = base + lane;
    float m = 1.0f;
#pragma unroll
    for (int t = 0; t <= kLvAhead; t++) m = fminf(m, k + t < K ? rr[k + t] : 1.0f);
    float prev, mine;
    lv_chain64(m, p.rel, G, &prev, &mine);
    if (k <= K) nd[k] = fminf(prev, mine);
  }
}

// phase 3: y = u·g(n), four samples (of one block) per thread
__global__ __launch_bounds__(256) void level_apply_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                          int64_t n_flat, const LvParams p, const float* __restrict__ node, int64_t KR,
                                                          float* __restrict__ lim, int64_t lim_row) {
  const int b = blockIdx.y;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  const float* x = audio + (int64_t)b * row;
  float* y = lim + (int64_t)b * lim_row;
  const float* nd = node + (int64_t)b * (KR + 1);
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  for (int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; at < n; at += (int64_t)gridDim.x * 1024) {
    const int64_t k = at / kLvBlock;
    const int i0 = (int)(at - k * kLvBlock);
    const float n0 = nd[k], d = nd[k + 1] - n0;
    const bool full = vec && at + 4 <= n;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (full) {
      v = *(const float4*)(x + at);
    } else {
      v.x = x[at];
      if (at + 1 < n) v.y = x[at + 1];
      if (at + 2 < n) v.z = x[at + 2];
      if (at + 3 < n) v.w = x[at + 3];
    }
    float4 o;
    o.x = (v.x * p.drive) * (n0 + d * ((float)i0 * 0.03125f));
    o.y = (v.y * p.drive) * (n0 + d * ((float)(i0 + 1) * 0.03125f));
    o.z = (v.z * p.drive) * (n0 + d * ((float)(i0 + 2) * 0.03125f));
    o.w = (v.w * p.drive) * (n0 + d * ((float)(i0 + 3) * 0.03125f));
    if (full) {
      *(float4*)(y + at) = o;
    } else {
      y[at] = o.x;
      if (at + 1 < n) y[at + 1] = o.y;
      if (at + 2 < n) y[at + 2] = o.z;
      if (at + 3 < n) y[at + 3] = o.w;
    }
  }
}

// blocks of the LDS tables of a step whose rows take up to max_in input samples
__host__ __device__ inline int lv_step_blocks(int64_t max_in) { return (int)((max_in + kLvCarry - 1 + kLvBlock - 1) / kLvBlock); }

// One stream step, one block per generator row. LDS: the old carry [256], r [NBmax], node [NBmax + 1], the G the next step starts from.
__global__ __launch_bounds__(256) void level_step_kernel(const float* __restrict__ audio, int64_t row, const LvStepRow* __restrict__ desc,
                                                         float* __restrict__ carry, const LvParams p, int max_in, float* __restrict__ lim,
                                                         int64_t lim_row) {
  extern __shared__ float lv_lds[];
  const LvStepRow d = desc[blockIdx.x];
  const int tid = threadIdx.x;
  const int n_in = min(max(d.n_in, 0), max_in);
  if (n_in == 0) return;  // (a row without a chunk keeps no carry: a finished or dropped row never resumes, a new occupant starts from nothing)
  const int cn = min(max(d.carry_n, 0), kLvCarry - 1);
  const int total = cn + n_in, n_out = min(max(d.n_out, 0), total);
  const int NBmax = lv_step_blocks(max_in);
  float* cs = lv_lds;
  float* rs = cs + kLvCarry;
  float* nd = rs + NBmax;
  float* keep = nd + NBmax + 1;
  const float* x = audio + (int64_t)blockIdx.x * row + d.skip;
  float* cr = carry + (int64_t)blockIdx.x * kLvCarry;
  cs[tid] = tid < cn ? cr[tid] : 0.0f;
  float G = cn > 0 ? cr[kLvCarry - 1] : 1.0f;  // a row's first step sees nothing of the row's previous occupant
  __syncthreads();
  const int nblk = (total + kLvBlock - 1) / kLvBlock;
  for (int jb = 0; jb < nblk; jb += 8) {  // (uniform: every lane shuffles) 32 lanes per block
    const int j = jb + (tid >> 5), at = j * kLvBlock + (tid & 31);
    float a = 0.0f;
    if (at < total) a = lv_abs(at < cn ? cs[at] : x[at - cn] * p.drive);
    a = fmaxf(a, __shfl_xor(a, 16));
    a = fmaxf(a, __shfl_xor(a, 8));
    a = fmaxf(a, __shfl_xor(a, 4));
    a = fmaxf(a, __shfl_xor(a, 2));
    a = fmaxf(a, __shfl_xor(a, 1));
    if ((tid & 31) == 0 && j < nblk) rs[j] = lv_ratio(a, p.ceiling);
  }
  __syncthreads();
  const int jo = (n_out + kLvBlock - 1) / kLvBlock;  // nodes 0 … jo (jo ≤ nblk ≤ NBmax)
  if (tid < 64) {
    for (int base = 0; base <= jo; base += 64) {
      const int j = base + tid;
      float m = 1.0f;
#pragma unroll
      for (int t = 0; t <= kLvAhead; t++) m = fminf(m, j + t < nblk ? rs[j + t] : 1.0f);
      float prev, mine;
      lv_chain64(m, p.rel, G, &prev, &mine);
      if (j <= jo) nd[j] = fminf(prev, mine);
      if (j == jo) *keep = prev;  // G of the last block this step finishes
    }
  }
  __syncthreads();
  float* y = lim + (int64_t)blockIdx.x * lim_row;
  for (int at = tid; at < n_out; at += 256) {
    const int k = at >> 5, i = at & 31;
    const float u = at < cn ? cs[at] : x[at - cn] * p.drive;
    const float n0 = nd[k], dd = nd[k + 1] - n0;
    y[at] = u * (n0 + dd * ((float)i * 0.03125f));
  }
  const int left = min(total - n_out, kLvCarry - 1);
  if (tid < left) {
    const int at = n_out + tid;
    cr[tid] = at < cn ? cs[at] : x[at - cn] * p.drive;
  }
  if (tid == kLvCarry - 1) cr[tid] = *keep;
}

}  // namespace

size_t lv_scratch_floats(int NB, int64_t n_max) { return (size_t)NB * (2 * (size_t)ceil_div(std::max<int64_t>(n_max, 1), kLvBlock) + 1); }

hipError_t launch_level_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                              const LvParams& p, float* scratch, float* lim, int64_t lim_row) {
  if (NB < 1 || (!lensF && NB != 1)) return hipErrorInvalidValue;
  const int64_t n_max = lensF ? (int64_t)F * hop : n_flat;
  if (n_max <= 0) return hipSuccess;
  const int64_t KR = ceil_div(n_max, kLvBlock);
  float* r = scratch;
  float* node = scratch + (size_t)NB * KR;
  const unsigned gp = (unsigned)std::min<int64_t>(ceil_div(KR, 32), 1024), ga = (unsigned)std::min<int64_t>(ceil_div(n_max, 1024), 1024);
  hipLaunchKernelGGL(level_peaks_kernel, dim3(gp, NB), dim3(256), 0, q, audio, row, lensF, F, hop, n_flat, p, r, KR);
  hipLaunchKernelGGL(level_gain_kernel, dim3(NB), dim3(64), 0, q, lensF, F, hop, n_flat, p, r, node, KR);
  hipLaunchKernelGGL(level_apply_kernel, dim3(ga, NB), dim3(256), 0, q, audio, row, lensF, F, hop, n_flat, p, node, KR, lim, lim_row);
  return hipGetLastError();
}

size_t lv_step_lds(int64_t max_in) {
  if (max_in < 1 || max_in > ((int64_t)1 << 24)) return 0;
  const size_t bytes = ((size_t)kLvCarry + 2 * (size_t)lv_step_blocks(max_in) + 2) * sizeof(float);
  return bytes <= kLvLdsMax ? bytes : 0;
}

hipError_t launch_level_step(hipStream_t q, int NBg, int max_in, const float* audio, int64_t row, const LvStepRow* desc, float* carry,
                             const LvParams& p, float* lim_step, int64_t lim_row) {
  const size_t lds = lv_step_lds(max_in);
  if (NBg < 1 || lds == 0 || lim_row < lv_step_bound(max_in)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(level_step_kernel, dim3(NBg), dim3(256), lds, q, audio, row, desc, carry, p, max_in, lim_step, lim_row);
  return hipGetLastError();
}

namespace { PH_WARM(level, level_apply_kernel); }

int lv_resolve(const piper_hip_level* lv, int rate, LvParams* out) {
  piper_hip_level z{0.0f, 0.0f, 0.0f};
  if (!lv) lv = &z;
  if (int rc = piper_hip_level_check(lv)) return rc;
  if (rate <= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "level: rate %d", rate);
  const double ms = lv->release_ms == 0.0f ? 50.0 : (double)lv->release_ms;
  out->drive = lv->drive == 0.0f ? 1.0f : lv->drive;
  out->ceiling = lv->ceiling == 0.0f ? 1.0f : lv->ceiling;
  out->rel = (float)std::min(1.0, (double)kLvBlock * 1000.0 / ((double)rate * ms));
  return PIPER_HIP_OK;
}

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_level_check(const piper_hip_level* lv) {
  if (!lv) PH_FAIL(PIPER_HIP_ERR_ARG, "level: null level");
  if (lv->drive != 0.0f && !(std::isfinite(lv->drive) && lv->drive > 0.0f && lv->drive <= 1000.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "level: drive %g outside (0, 1000]", (double)lv->drive);
  if (lv->ceiling != 0.0f && !(lv->ceiling >= 0.001f && lv->ceiling <= 1.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "level: ceiling %g outside [0.001, 1]", (double)lv->ceiling);
  if (lv->release_ms != 0.0f && !(lv->release_ms >= 1.0f && lv->release_ms <= 10000.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "level: release_ms %g outside [1, 10000]", (double)lv->release_ms);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_level_info(const piper_hip_level* lv, int32_t rate, float* rel) {
  LvParams p;
  if (!lv) PH_FAIL(PIPER_HIP_ERR_ARG, "level_info: null level");
  if (int rc = lv_resolve(lv, rate, &p)) return rc;
  if (rel) *rel = p.rel;
  return PIPER_HIP_OK;
}

PH_EXPORT int64_t piper_hip_level_ready(int64_t e) {
  if (e < 0 || e > ((int64_t)1 << 50)) PH_FAIL(PIPER_HIP_ERR_ARG, "level_ready: %lld samples", (long long)e);
  return lv_ready(e);
}

PH_EXPORT int64_t piper_hip_level_step_bound(int64_t n_in) {
  if (n_in < 0 || n_in > ((int64_t)1 << 50)) PH_FAIL(PIPER_HIP_ERR_ARG, "level_step_bound: %lld input samples", (long long)n_in);
  return lv_step_bound(n_in);
}

// the host twin of the kernels: the same operations in the same order, every one rounded on its own
PH_EXPORT int piper_hip_level_from_f32(const piper_hip_level* lv, int32_t rate, const float* x, size_t n, float* y) {
  LvParams p;
  if (!lv) PH_FAIL(PIPER_HIP_ERR_ARG, "level_from_f32: null level");
  if (int rc = lv_resolve(lv, rate, &p)) return rc;
  if ((!x || !y) && n) PH_FAIL(PIPER_HIP_ERR_ARG, "level_from_f32: null buffer");
  if (n == 0) return PIPER_HIP_OK;
  const size_t K = (n + kLvBlock - 1) / kLvBlock;
  std::vector<float> r(K + kLvAhead + 1, 1.0f), node(K + 1);
  for (size_t k = 0; k < K; k++) {
    float peak = 0.0f;
    for (size_t i = k * kLvBlock; i < std::min(n, (k + 1) * kLvBlock); i++) {
      const float a = std::fabs(x[i] * p.drive);
      if (a > peak) peak = a;  // (false for NaN)
    }
    r[k] = peak > p.ceiling ? p.ceiling / peak : 1.0f;
  }
  float G = 1.0f;
  for (size_t k = 0; k <= K; k++) {
    float m = 1.0f;
    for (int t = 0; t <= kLvAhead; t++) m = std::min(m, r[k + t]);
    const float s = G + p.rel;
    const float Gn = std::min(m, s);
    node[k] = std::min(G, Gn);
    G = Gn;
  }
  for (size_t i = 0; i < n; i++) {
    const size_t k = i / kLvBlock;
    const float t = (float)(i - k * kLvBlock) * 0.03125f;
    const float d = node[k + 1] - node[k];
    const float dt = d * t;
    const float g = node[k] + dt;
    const float u = x[i] * p.drive;
    y[i] = u * g;
  }
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_level_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, const piper_hip_level* lv, float** out,
                                  piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "level_f32: null output pointer");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "level_f32: null input");
  if (!lv) PH_FAIL(PIPER_HIP_ERR_ARG, "level_f32: null level");
  if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "level_f32: the output buffer is not 4-byte aligned");
  if (count > ((size_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "level_f32: %zu samples", count);
  LvParams p;
  int rc = lv_resolve(lv, rate, &p);
  if (rc) return rc;
  if (!*out) {
    void* q = nullptr;
    if ((rc = ctx->pool.alloc(count * sizeof(float), &q))) return rc;
    *out = (float*)q;
  }
  if (count == 0) return PIPER_HIP_OK;
  void* scratch = nullptr;
  if ((rc = ctx->pool.alloc(lv_scratch_floats(1, (int64_t)count) * sizeof(float), &scratch))) return rc;
  defer_free(ctx, scratch);
  StreamScope ss(ctx, stream);
  (void)launch_level_items(ss.s, x, 0, nullptr, 0, 1, 1, (int64_t)count, p, (float*)scratch, *out, 0);
  return ss.finish("level_f32");
}
