// loudness.hip — ITU-R BS.1770 / EBU R128 integrated loudness of whole items on the device (include/piper_hip.h "Loudness").
//
// All of the measurement is in double. y = HP(shelf(x)) is a linear recurrence with a four-component state (two per biquad, transposed
// direct form II), so an item is cut into passes of 32 768 samples, one 512-lane workgroup each, and a pass into chunks of 64 samples,
// one per lane:
//   run      every lane runs its chunk from zero state (lane 0 from the state the pass starts in) and keeps the end state
//   scan     nine fixed steps over the lanes, v[t] += A^(64·2^k)·v[t − 2^k], leave in v[t] the true state behind chunk t
//   run      every lane runs its chunk again from v[t − 1] and sums y² into the (at most two) 100 ms segments the chunk touches
//   reduce   eight lanes per segment add the lanes' partials in a fixed order: the pass's share of each segment it touches
// The state a pass starts in: launch 1a runs every pass but the last from zero state (run, scan) and keeps its end state E, launch 1b
// chains S[c] = A^(64·512)·S[c − 1] + E[c − 1] on one lane, launch 1c is the four steps above. Items of one pass take launch 1c alone.
// Launch 2 (one wave per item) adds the shares of the one or two passes that touch a segment, forms the 400 ms block powers from four
// consecutive segments, applies both gates and writes {L, g}; launch 3 multiplies the item by g. Sums run in a fixed order and nothing
// is atomic: the same samples give the same bits.
#include "loudness.h"

#include <algorithm>
#include <cmath>

#include "pcm16.h"

#pragma clang fp contract(off)

namespace ph {
namespace {

static_assert(kLdSegs <= kLdLanes / 8, "eight lanes per segment of a pass");
static_assert(kLdChunk < 800, "a chunk touches at most two segments");

__host__ __device__ inline double ld_sample(float v) {  // a non-finite sample reads as 0
  union { float f; uint32_t u; } c;
  c.f = v;
  return (c.u & 0x7f800000u) == 0x7f800000u ? 0.0 : (double)v;
}

// The lane's chunk x[start, start + cnt) through the filter from state s. acc == nullptr: only the state moves on. Otherwise y² goes to
// acc[0] for samples below `split` and to acc[1] from there on.
__device__ __forceinline__ void ld_chunk(const float* __restrict__ x, int64_t start, int cnt, bool vec, LdState& s, const LdFilter& f,
                                         int64_t split, double* acc) {
  double a0 = 0.0, a1 = 0.0;
  if (vec && cnt == kLdChunk) {
    const float4* x4 = (const float4*)(x + start);
    for (int i = 0; i < kLdChunk / 4; i++) {
      const float4 v = x4[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const double y = ld_step(s, ld_sample(e[c]), f);
        if (start + i * 4 + c < split) a0 += y * y;
        else a1 += y * y;
      }
    }
  } else {
    for (int i = 0; i < cnt; i++) {
      const double y = ld_step(s, ld_sample(x[start + i]), f);
      if (start + i < split) a0 += y * y;
      else a1 += y * y;
    }
  }
  if (acc) { acc[0] = a0; acc[1] = a1; }
}

// The scan over the lanes of one pass: v comes in as the lane's end state (buffer 0 holds every lane's), and leaves as the state behind
// the lane's chunk given what the lanes before it contributed; the buffer kLdScan & 1 holds every lane's.
__device__ __forceinline__ void ld_scan(double (&st)[2][4][kLdLanes], int t, double (&v)[4], const LdFilter& f) {
#pragma unroll 1  // (one step's matrix in scalar registers at a time)
  for (int k = 0; k < kLdScan; k++) {
    const int cur = k & 1, d = 1 << k;
    if (t >= d) {
      const double u0 = st[cur][0][t - d], u1 = st[cur][1][t - d], u2 = st[cur][2][t - d], u3 = st[cur][3][t - d];
#pragma unroll
      for (int i = 0; i < 4; i++)
        v[i] = v[i] + (((f.M[k][i * 4] * u0 + f.M[k][i * 4 + 1] * u1) + f.M[k][i * 4 + 2] * u2) + f.M[k][i * 4 + 3] * u3);
    }
    st[cur ^ 1][0][t] = v[0]; st[cur ^ 1][1][t] = v[1]; st[cur ^ 1][2][t] = v[2]; st[cur ^ 1][3][t] = v[3];
    __syncthreads();
  }
}

// launch 1a, one workgroup per pass that another follows: the state the pass ends in when it starts from zero, E [passes][4]
__global__ __launch_bounds__(kLdLanes) void loud_ends_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F,
                                                             int hop, int64_t n_flat, const LdFilter f, double* __restrict__ work, int64_t work_row) {
  __shared__ double st[2][4][kLdLanes];
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kLdSuper;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  if (base + kLdSuper >= n) return;  // (uniform) the item's last pass, or none of it: nothing follows
  const float* x = audio + (int64_t)b * row;
  const bool vec = ((uintptr_t)x & 15) == 0;
  LdState s{0.0, 0.0, 0.0, 0.0};
  ld_chunk(x, base + (int64_t)t * kLdChunk, kLdChunk, vec, s, f, 0, nullptr);
  st[0][0][t] = s.s1; st[0][1][t] = s.s2; st[0][2][t] = s.t1; st[0][3][t] = s.t2;
  __syncthreads();
  double v[4] = {s.s1, s.s2, s.t1, s.t2};
  ld_scan(st, t, v, f);
  if (t == kLdLanes - 1) {
    double* E = work + (int64_t)b * work_row + 4 * c;
    E[0] = v[0]; E[1] = v[1]; E[2] = v[2]; E[3] = v[3];
  }
}

// launch 1b, one workgroup per item: the true state every pass starts from, S[0] = 0, S[c] = A^(64·512)·S[c − 1] + E[c − 1] — a serial
// chain on one lane, 256 passes at a time out of LDS
__global__ __launch_bounds__(256) void loud_carry_kernel(const int* __restrict__ lensF, int F, int hop, int64_t n_flat, const LdFilter f,
                                                         double* __restrict__ work, int64_t work_row, int64_t passes) {
  __shared__ double e[256][4], s[256][4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  const int64_t np = std::min<int64_t>((n + kLdSuper - 1) / kLdSuper, passes);
  const double* E = work + (int64_t)b * work_row;
  double* S = work + (int64_t)b * work_row + 4 * passes;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;  // (lane 0's: the state the tile starts from)
  for (int64_t at = 0; at < np; at += 256) {
    const int m = (int)std::min<int64_t>(256, np - at);
    // E[at + t − 1] moves S[at + t − 1] on to S[at + t]
    if (t < m && at + t > 0) { e[t][0] = E[4 * (at + t - 1)]; e[t][1] = E[4 * (at + t - 1) + 1]; e[t][2] = E[4 * (at + t - 1) + 2]; e[t][3] = E[4 * (at + t - 1) + 3]; }
    __syncthreads();
    if (t == 0) {
      for (int i = 0; i < m; i++) {
        if (at + i > 0) {
          const double n0 = (((f.Mp[0] * c0 + f.Mp[1] * c1) + f.Mp[2] * c2) + f.Mp[3] * c3) + e[i][0];
          const double n1 = (((f.Mp[4] * c0 + f.Mp[5] * c1) + f.Mp[6] * c2) + f.Mp[7] * c3) + e[i][1];
          const double n2 = (((f.Mp[8] * c0 + f.Mp[9] * c1) + f.Mp[10] * c2) + f.Mp[11] * c3) + e[i][2];
          const double n3 = (((f.Mp[12] * c0 + f.Mp[13] * c1) + f.Mp[14] * c2) + f.Mp[15] * c3) + e[i][3];
          c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        }
        s[i][0] = c0; s[i][1] = c1; s[i][2] = c2; s[i][3] = c3;
      }
    }
    __syncthreads();
    if (t < m) { S[4 * (at + t)] = s[t][0]; S[4 * (at + t) + 1] = s[t][1]; S[4 * (at + t) + 2] = s[t][2]; S[4 * (at + t) + 3] = s[t][3]; }
    __syncthreads();
  }
}

// launch 1c, one workgroup per pass: the pass from its true start state; part [passes][kLdSegs] = the pass's share of Σ y² of every
// segment it touches, segment g at g − (c·32768) div h
__global__ __launch_bounds__(kLdLanes) void loud_power_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F,
                                                              int hop, int64_t n_flat, const LdFilter f, double* __restrict__ work, int64_t work_row,
                                                              int64_t passes) {
  __shared__ double st[2][4][kLdLanes];  // the scan's two buffers, one array per state component
  __shared__ double pp[2][kLdLanes];     // the lanes' two partial sums
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kLdSuper;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  if (base >= n) return;  // (uniform)
  const int64_t h = f.h;
  const float* x = audio + (int64_t)b * row;
  const double* S = work + (int64_t)b * work_row + 4 * passes + 4 * c;
  double* part = work + (int64_t)b * work_row + 8 * passes + (int64_t)kLdSegs * c;
  const bool vec = ((uintptr_t)x & 15) == 0;
  const int64_t start = base + (int64_t)t * kLdChunk;
  const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(kLdChunk, n - start));
  LdState in{0.0, 0.0, 0.0, 0.0};  // (the first pass starts from zero and reads nothing: launch 1b is skipped for items of one pass)
  if (c > 0) in = LdState{S[0], S[1], S[2], S[3]};
  LdState s{0.0, 0.0, 0.0, 0.0};
  if (t == 0) s = in;
  ld_chunk(x, start, cnt, vec, s, f, 0, nullptr);
  st[0][0][t] = s.s1; st[0][1][t] = s.s2; st[0][2][t] = s.t1; st[0][3][t] = s.t2;
  __syncthreads();
  double v[4] = {s.s1, s.s2, s.t1, s.t2};
  ld_scan(st, t, v, f);
  constexpr int fin = kLdScan & 1;  // the buffer the last step wrote
  LdState s0 = in;
  if (t > 0) s0 = LdState{st[fin][0][t - 1], st[fin][1][t - 1], st[fin][2][t - 1], st[fin][3][t - 1]};
  const int64_t g0 = start / h;
  double acc[2];
  ld_chunk(x, start, cnt, vec, s0, f, (g0 + 1) * h, acc);
  pp[0][t] = acc[0];
  pp[1][t] = acc[1];
  __syncthreads();
  // the segments this pass touched, eight lanes each
  const int64_t end = std::min<int64_t>(base + kLdSuper, n);
  const int64_t gA = base / h, gB = (end - 1) / h;
  const int j = t >> 3, q = t & 7;
  const int64_t g = gA + j;
  double sum = 0.0;
  if (g <= gB) {
    const int64_t lo_s = std::max<int64_t>(g * h, base), hi_s = std::min<int64_t>((g + 1) * h, end);
    const int lo = (int)((lo_s - base) / kLdChunk), hi = (int)((hi_s - 1 - base) / kLdChunk);
    for (int l = lo + q; l <= hi; l += 8) sum += (base + (int64_t)l * kLdChunk >= g * h) ? pp[0][l] : pp[1][l];
  }
  sum += __shfl_xor(sum, 4);
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 1);
  if (g <= gB && q == 0 && j < kLdSegs) part[j] = sum;
}

__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// Σ y² of whole segment g of an item: the shares of the one or two passes that touch it, the earlier pass first
__device__ __forceinline__ double ld_segment(const double* __restrict__ part, int64_t g, int64_t h) {
  const int64_t c0 = (g * h) / kLdSuper, c1 = ((g + 1) * h - 1) / kLdSuper;
  double s = part[c0 * kLdSegs + (g - (c0 * kLdSuper) / h)];
  if (c1 != c0) s += part[c1 * kLdSegs + (g - (c1 * kLdSuper) / h)];
  return s;
}
// the power of 400 ms block j: four consecutive segments
__device__ __forceinline__ double ld_block(const double* __restrict__ part, int64_t j, int64_t h) {
  return (((ld_segment(part, j, h) + ld_segment(part, j + 1, h)) + ld_segment(part, j + 2, h)) + ld_segment(part, j + 3, h)) / (4.0 * (double)h);
}

// launch 2, one wave per item: block powers from four segments, the absolute and the relative gate, L and g
__global__ __launch_bounds__(64) void loud_gate_kernel(const int* __restrict__ lensF, int F, int hop, int64_t n_flat, int h,
                                                       const double* __restrict__ work, int64_t work_row, int64_t passes, const LdTarget tg,
                                                       float* __restrict__ rep) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t n = std::min<int64_t>(lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat, passes * kLdSuper);
  const int64_t S = n / h;  // whole segments
  const int64_t J = S >= 4 ? S - 3 : 0;
  const double* part = work + (int64_t)b * work_row + 8 * passes;
  double sum = 0.0, cnt = 0.0;
  for (int64_t j = lane; j < J; j += 64) {
    const double z = ld_block(part, j, h);
    const double l = -0.691 + 10.0 * log10(z);
    if (l > -70.0) { sum += z; cnt += 1.0; }
  }
  sum = ld_wave_sum(sum);
  cnt = ld_wave_sum(cnt);
  double L = -INFINITY;
  if (cnt > 0.0) {
    const double gate = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
    double sr = 0.0, cr = 0.0;
    for (int64_t j = lane; j < J; j += 64) {
      const double z = ld_block(part, j, h);
      const double l = -0.691 + 10.0 * log10(z);
      if (l > -70.0 && l > gate) { sr += z; cr += 1.0; }
    }
    sr = ld_wave_sum(sr);
    cr = ld_wave_sum(cr);
    if (cr > 0.0) L = -0.691 + 10.0 * log10(sr / cr);
  }
  const float Lf = (float)L;
  float g = 1.0f;
  if (tg.on && Lf > -INFINITY) {
    const double d = fmin(tg.target - (double)Lf, tg.max_gain);
    g = (float)pow(10.0, d / 20.0);
  }
  if (lane == 0) {
    rep[2 * b] = Lf;
    rep[2 * b + 1] = g;
  }
}

__global__ __launch_bounds__(256) void loud_gain_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                        const float* __restrict__ rep, float* __restrict__ out, int64_t out_row) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)clamp_len(lensF[b], F) * hop;
  const float g = rep[2 * b + 1];
  const float* x = audio + (int64_t)b * row;
  float* u = out + (int64_t)b * out_row;
  const bool vec = (((uintptr_t)x | (uintptr_t)u) & 15) == 0;
  for (int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; at < n; at += (int64_t)gridDim.x * 1024) {
    if (vec && at + 4 <= n) {
      const float4 v = *(const float4*)(x + at);
      *(float4*)(u + at) = make_float4(v.x * g, v.y * g, v.z * g, v.w * g);
    } else {
      for (int64_t i = at; i < std::min<int64_t>(at + 4, n); i++) u[i] = x[i] * g;
    }
  }
}

void mat4_mul(const double* a, const double* b, double* c) {
  double r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += a[i * 4 + k] * b[k * 4 + j];
      r[i * 4 + j] = s;
    }
  memcpy(c, r, sizeof(r));
}

PH_WARM(loudness, loud_gain_kernel);

}  // namespace

int ld_filter(int rate, LdFilter* out) {
  double sb[3], sa[3], hb[3], ha[3];
  if (int rc = piper_hip_loudness_coeffs(rate, sb, sa, hb, ha)) return rc;
  LdFilter& f = *out;
  f.sb0 = sb[0]; f.sb1 = sb[1]; f.sb2 = sb[2]; f.sa1 = sa[1]; f.sa2 = sa[2];
  f.ha1 = ha[1]; f.ha2 = ha[2];
  f.h = rate / 10;
  // A: one sample without input, column by column; then A^64 by six squarings and the scan's further powers
  double A[16];
  for (int j = 0; j < 4; j++) {
    LdState s{j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, j == 3 ? 1.0 : 0.0};
    (void)ld_step(s, 0.0, f);
    A[0 * 4 + j] = s.s1; A[1 * 4 + j] = s.s2; A[2 * 4 + j] = s.t1; A[3 * 4 + j] = s.t2;
  }
  for (int i = 0; i < 6; i++) mat4_mul(A, A, A);
  static_assert(kLdChunk == 64, "A^64 is six squarings");
  memcpy(f.M[0], A, sizeof(A));
  for (int k = 1; k < kLdScan; k++) mat4_mul(f.M[k - 1], f.M[k - 1], f.M[k]);
  mat4_mul(f.M[kLdScan - 1], f.M[kLdScan - 1], f.Mp);
  return PIPER_HIP_OK;
}

int ld_resolve(const piper_hip_loudness* ld, LdTarget* out) {
  out->on = 0; out->target = 0.0; out->max_gain = 0.0;
  if (!ld) return PIPER_HIP_OK;
  if (int rc = piper_hip_loudness_check(ld)) return rc;
  out->on = 1;
  out->target = ld->target_lufs == 0.0f ? -16.0 : (double)ld->target_lufs;
  out->max_gain = ld->max_gain_db == 0.0f ? 20.0 : (double)ld->max_gain_db;
  return PIPER_HIP_OK;
}

hipError_t launch_loudness_measure(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                                   const LdFilter& f, double* work) {
  if (NB < 1 || (!lensF && NB != 1) || f.h < 800) return hipErrorInvalidValue;
  const int64_t n_max = lensF ? (int64_t)F * hop : n_flat, passes = ld_passes(n_max), work_row = ld_work_row(n_max);
  if (n_max <= 0) return hipSuccess;
  if (passes > 0x7fffffff) return hipErrorInvalidValue;
  if (passes > 1) {
    hipLaunchKernelGGL(loud_ends_kernel, dim3((unsigned)passes - 1, NB), dim3(kLdLanes), 0, q, audio, row, lensF, F, hop, n_flat, f, work, work_row);
    hipLaunchKernelGGL(loud_carry_kernel, dim3(NB), dim3(256), 0, q, lensF, F, hop, n_flat, f, work, work_row, passes);
  }
  hipLaunchKernelGGL(loud_power_kernel, dim3((unsigned)passes, NB), dim3(kLdLanes), 0, q, audio, row, lensF, F, hop, n_flat, f, work, work_row, passes);
  return hipGetLastError();
}

hipError_t launch_loudness_gate(hipStream_t q, const int* lensF, int F, int hop, int NB, int64_t n_flat, int h, const double* work,
                                const LdTarget& t, float* rep) {
  if (NB < 1 || (!lensF && NB != 1) || h < 800) return hipErrorInvalidValue;
  const int64_t n_max = std::max<int64_t>(lensF ? (int64_t)F * hop : n_flat, 0);
  hipLaunchKernelGGL(loud_gate_kernel, dim3(NB), dim3(64), 0, q, lensF, F, hop, n_flat, h, work, ld_work_row(n_max), ld_passes(n_max), t, rep);
  return hipGetLastError();
}

hipError_t launch_loudness_gain(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, const float* rep,
                                float* out, int64_t out_row) {
  if (NB < 1 || !lensF) return hipErrorInvalidValue;
  const int64_t n_max = (int64_t)F * hop;
  if (n_max <= 0) return hipSuccess;
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(n_max, 1024), 1024);
  hipLaunchKernelGGL(loud_gain_kernel, dim3(gx, NB), dim3(256), 0, q, audio, row, lensF, F, hop, rep, out, out_row);
  return hipGetLastError();
}

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_loudness_check(const piper_hip_loudness* ld) {
  if (!ld) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness: null loudness");
  if (ld->target_lufs != 0.0f && !(ld->target_lufs >= -70.0f && ld->target_lufs <= -1.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "loudness: target_lufs %g outside [-70, -1]", (double)ld->target_lufs);
  if (ld->max_gain_db != 0.0f && !(ld->max_gain_db > 0.0f && ld->max_gain_db <= 60.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "loudness: max_gain_db %g outside (0, 60]", (double)ld->max_gain_db);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_loudness_coeffs(int32_t rate, double shelf_b[3], double shelf_a[3], double hp_b[3], double hp_a[3]) {
  static const int32_t rates[] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};
  if (std::find(std::begin(rates), std::end(rates), rate) == std::end(rates))
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "loudness: rate %d (supported: 8000, 16000, 22050, 24000, 32000, 44100, 48000)", (int)rate);
  if (!shelf_b || !shelf_a || !hp_b || !hp_a) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_coeffs: null output");
  const double pi = 3.14159265358979323846;
  {
    const double K = std::tan(pi * 1681.974450955533 / (double)rate), Q = 0.7071752369554196;
    const double Vh = std::pow(10.0, 3.999843853973347 / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    shelf_b[0] = (Vh + Vb * K / Q + K * K) / a0;
    shelf_b[1] = 2.0 * (K * K - Vh) / a0;
    shelf_b[2] = (Vh - Vb * K / Q + K * K) / a0;
    shelf_a[0] = 1.0;
    shelf_a[1] = 2.0 * (K * K - 1.0) / a0;
    shelf_a[2] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double K = std::tan(pi * 38.13547087602444 / (double)rate), Q = 0.5003270373238773;
    const double a0 = 1.0 + K / Q + K * K;
    hp_b[0] = 1.0; hp_b[1] = -2.0; hp_b[2] = 1.0;
    hp_a[0] = 1.0;
    hp_a[1] = 2.0 * (K * K - 1.0) / a0;
    hp_a[2] = (1.0 - K / Q + K * K) / a0;
  }
  return PIPER_HIP_OK;
}

// the sequential twin of the kernels: one recurrence over the item, segment sums, block powers from four segments, both gates
PH_EXPORT int piper_hip_loudness_from_f32(int32_t rate, const float* x, size_t n, float* lufs) {
  LdFilter f;
  if (int rc = ld_filter(rate, &f)) return rc;
  if (!lufs) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_from_f32: null output");
  if (!x && n) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_from_f32: null input");
  const size_t h = (size_t)f.h, S = n / h;
  *lufs = -INFINITY;
  if (S < 4) return PIPER_HIP_OK;
  std::vector<double> seg(S, 0.0);
  LdState s{0.0, 0.0, 0.0, 0.0};
  for (size_t k = 0; k < S; k++) {
    double a = 0.0;
    for (size_t i = k * h; i < (k + 1) * h; i++) {
      const double y = ld_step(s, ld_sample(x[i]), f);
      a += y * y;
    }
    seg[k] = a;
  }
  const size_t J = S - 3;
  const double len = 4.0 * (double)h;
  std::vector<double> z(J);
  double sum = 0.0, cnt = 0.0;
  for (size_t j = 0; j < J; j++) {
    z[j] = (((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) / len;
    if (-0.691 + 10.0 * std::log10(z[j]) > -70.0) { sum += z[j]; cnt += 1.0; }
  }
  if (cnt == 0.0) return PIPER_HIP_OK;
  const double gate = -0.691 + 10.0 * std::log10(sum / cnt) - 10.0;
  double sr = 0.0, cr = 0.0;
  for (size_t j = 0; j < J; j++) {
    const double l = -0.691 + 10.0 * std::log10(z[j]);
    if (l > -70.0 && l > gate) { sr += z[j]; cr += 1.0; }
  }
  if (cr > 0.0) *lufs = (float)(-0.691 + 10.0 * std::log10(sr / cr));
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_loudness_gain(const piper_hip_loudness* ld, float lufs, float* gain) {
  LdTarget t;
  if (!ld) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_gain: null loudness");
  if (!gain) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_gain: null output");
  if (int rc = ld_resolve(ld, &t)) return rc;
  if (lufs != lufs || lufs == INFINITY) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_gain: lufs %g", (double)lufs);
  *gain = 1.0f;  // an unmeasurable item
  if (lufs > -INFINITY) *gain = (float)std::pow(10.0, std::min(t.target - (double)lufs, t.max_gain) / 20.0);
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_loudness_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, float* lufs_host, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!lufs_host) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_f32: null output");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness_f32: null input");
  if (count > ((size_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "loudness_f32: %zu samples", count);
  LdFilter f;
  int rc = ld_filter(rate, &f);
  if (rc) return rc;
  *lufs_host = -INFINITY;
  if (count == 0) return PIPER_HIP_OK;
  void *work = nullptr, *rep = nullptr;
  if ((rc = ctx->pool.alloc((size_t)ld_work_row((int64_t)count) * sizeof(double), &work))) return rc;
  defer_free(ctx, work);
  if ((rc = ctx->pool.alloc(2 * sizeof(float), &rep))) return rc;
  defer_free(ctx, rep);
  StreamScope ss(ctx, stream);
  const LdTarget none{0, 0.0, 0.0};
  hipError_t e = launch_loudness_measure(ss.s, x, 0, nullptr, 0, 1, 1, (int64_t)count, f, (double*)work);
  if (e == hipSuccess) e = launch_loudness_gate(ss.s, nullptr, 0, 1, 1, (int64_t)count, f.h, (const double*)work, none, (float*)rep);
  if (e == hipSuccess) e = hipMemcpyAsync(lufs_host, rep, sizeof(float), hipMemcpyDeviceToHost, ss.s);
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "loudness_f32: %s", hipGetErrorString(e));
  return ss.finish("loudness_f32");
}
