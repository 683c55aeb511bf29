// prosody.hip — per-phoneme prosody (include/piper_hip.h "Per-phoneme prosody"): the host-side checks and the integer frame rule, and the
// three kernels a plan of a request with prosody runs in the place of dp_final_kernel (dp.hip), dp_paths_kernel and expand_noise_kernel
// (voice.hip). The reference has no counterpart: its `scales` input carries three scalars per utterance (PiperMetalRuntime.swift:62-80).
//   * dp_final_prosody_kernel: logw → w0 = exp(logw)·length_scale (kept: the "dp.w" tap) → ·length[t] → ceil → ceiling → floor.
//   * dp_paths_prosody_kernel: generate_path with the fit step: scan in LDS, rescale in 64-bit integers when the total exceeds the bound and
//     the item asked for it, scan again; the totals before and after reach the host through the mapped report area.
//   * expand_noise_prosody_kernel: the latent expansion with a noise multiplier per id, read through frame2id.
// All three are short-row, latency-bound launches (a few blocks): every thread requests the operands of its column in one burst before it
// uses any of them.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "dp_scalars.h"
#include "rng.h"

namespace ph {
namespace {

__global__ __launch_bounds__(256) void dp_final_prosody_kernel(const float* __restrict__ z, const float* __restrict__ m, const float* __restrict__ logs,
                                                               const DpScalars* __restrict__ sc, const float* __restrict__ len,
                                                               const int32_t* __restrict__ minf, const int32_t* __restrict__ maxf,
                                                               float* __restrict__ logw, float* __restrict__ w0_out, int32_t* __restrict__ dur, int T,
                                                               const int* __restrict__ len_ptr) {
  const int n = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int64_t i = (int64_t)n * T + t;
  // one burst: nothing below is used before all of it has been requested
  const float zv = z[(int64_t)n * 2 * T + t];
  const float lm = len[i];
  const int32_t mn = minf[i], mx = maxf[i];
  const float m0 = m[0], lg0 = logs[0], ls = sc[n].length_scale;
  const int Tv = len_ptr ? min(len_ptr[n], T) : T;
  float lw = 0.0f, w0 = 0.0f;
  int32_t d = 0;
  if (t < Tv) {
    lw = (zv - m0) * expf(-lg0);
    w0 = expf(lw) * ls;  // what dp_final_kernel computes
    const float w1 = w0 * lm;
    const float c = ceilf(w1);
    const int32_t d0 = c > 0.0f ? (c < 1e6f ? (int32_t)c : 1000000) : 0;  // NaN → 0, as there
    const int32_t d1 = mx > 0 ? min(d0, mx) : d0;
    d = max(d1, mn);
  }
  logw[i] = lw;
  w0_out[i] = w0;
  dur[i] = d;
}

// Inclusive scan of the block's per-thread sums in place (256 entries); every thread returns the sum of the threads before it.
__device__ __forceinline__ long long scan256(long long* part, int tid, long long mine) {
  part[tid] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const long long v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  return tid ? part[tid - 1] : 0;
}

// dp_paths_kernel (voice.hip) with the fit step. One block per item, the ids of a thread consecutive, the cumulative sums in LDS. The
// sums are carried in 64 bits (4096 ids of up to 10^6 frames pass 2^31) and saturate at INT_MAX where they are stored: every frame
// index compared against them is below the bucket's length. `fit` [n]: ≠ 0 = compress the item to `cap` when its total exceeds it:
// d ← ⌊d · cap / S⌋ in int64. rep (host-mapped): [n] the frame counts the rest of the route sees (after fitting, before clamping),
// [n][T] the durations used, [n] fitted flags, [n][2] the total before fitting as two 32-bit halves (low first).
__global__ __launch_bounds__(256) void dp_paths_prosody_kernel(const int32_t* __restrict__ dur, const int* __restrict__ lensT, const int32_t* __restrict__ fit,
                                                               int T, int F, int cap, int32_t* __restrict__ frame2id, int* __restrict__ lensF,
                                                               int32_t* __restrict__ rep, int n) {
  __shared__ int cum[4096];
  __shared__ long long part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = min(lensT[b], T);
  const int per = (T + 255) / 256;  // ≤ 16 ids per thread, consecutive
  const int t0 = tid * per;
  int32_t d[16];
  const int32_t want_fit = fit[b];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int t = t0 + i;
    d[i] = (i < per && t < Tb) ? max(dur[(size_t)b * T + t], 0) : 0;
  }
  long long sum = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) sum += d[i];
  long long base = scan256(part, tid, sum);
  const long long S = part[255];
  const bool fitted = want_fit != 0 && S > (long long)cap;
  __syncthreads();  // part is written again below
  if (fitted) {
    sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      d[i] = (int32_t)((long long)d[i] * cap / S);
      sum += d[i];
    }
    base = scan256(part, tid, sum);
  }
  const long long total = part[255];
  long long run = base;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int t = t0 + i;
    run += d[i];
    if (i < per && t < T) {
      cum[t] = (int)min(run, (long long)INT_MAX);
      rep[n + (size_t)b * T + t] = d[i];
    }
  }
  __syncthreads();
  const int want = (int)min(max(total, 1LL), (long long)INT_MAX);  // an all-zero prediction still yields one frame (of id 0)
  const int Fv = min(min(want, cap), F);
  if (tid == 0) {
    lensF[b] = Fv;
    rep[b] = want;
    if (total < 1) rep[n + (size_t)b * T] = 1;
    int32_t* tail = rep + n + (size_t)n * T;
    tail[b] = fitted ? 1 : 0;
    tail[n + 2 * b] = (int32_t)(unsigned)(S & 0xffffffffLL);
    tail[n + 2 * b + 1] = (int32_t)(S >> 32);
  }
  for (int f = tid; f < F; f += 256) {
    int id = 0;
    if (f < Fv && (long long)f < total) {  // smallest t with cum[t] > f
      int lo = 0, hi = Tb - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > f) hi = mid; else lo = mid + 1;
      }
      id = lo;
    }
    frame2id[(size_t)b * F + f] = id;
  }
}

// expand_noise_kernel (voice.hip) with ns[t] = fl(noise_scale · noise[t]) in the place of noise_scale:
// z_p[c][f] = m_p[c][t(f)] + fl(fl(nz[c][f] · exp(logs_p[c][t(f)])) · ns[t(f)]).
__global__ __launch_bounds__(256) void expand_noise_prosody_kernel(const float* __restrict__ stats, const int32_t* __restrict__ frame2id,
                                                                   const float* __restrict__ noise, const float* __restrict__ id_noise,
                                                                   float* __restrict__ zp, float* __restrict__ zp_tap, int I, int T, int F,
                                                                   const float* __restrict__ noise_scale_dev, const unsigned* __restrict__ rng_dev,
                                                                   const int* __restrict__ lensF) {
  const int nb = blockIdx.y;  // batch item
  stats += (int64_t)nb * 2 * I * T;
  frame2id += (int64_t)nb * F;
  noise += (int64_t)nb * I * F;
  id_noise += (int64_t)nb * T;
  zp += (int64_t)nb * I * F;
  zp_tap += (int64_t)nb * I * F;
  const float noise_scale = noise_scale_dev[nb];
  const bool gen = rng_dev[2 * nb] != 0u;
  const unsigned seed = rng_dev[2 * nb + 1];
  const int Fv = lensF ? min(lensF[nb], F) : F;
  const int64_t total = (int64_t)I * F;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / F), f = (int)(i - (int64_t)c * F);
    const int t = frame2id[f];
    // the three operands of the column and the injected noise in one burst
    const float m = stats[(int64_t)c * T + t];
    const float lg = stats[(int64_t)(I + c) * T + t];
    const float pn = id_noise[t];
    const float nin = gen ? 0.0f : noise[i];
    const float nz = gen ? (f < Fv ? rnl_normal(seed, (unsigned)(c * Fv + f)) : 0.0f) : nin;
    const float ns = noise_scale * pn;
    const float r = m + (nz * expf(lg)) * ns;
    zp[i] = r;
    zp_tap[i] = r;
  }
}

const char* check_fields(const piper_hip_prosody* p, char* msg, size_t cap) {
  if (p->t < 1) { snprintf(msg, cap, "t = %d (at least 1)", p->t); return msg; }
  for (int i = 0; i < p->t; i++) {
    if (p->length && !(std::isfinite(p->length[i]) && p->length[i] >= 0.0f && p->length[i] <= 1000.0f)) {
      snprintf(msg, cap, "length[%d] = %g outside [0, 1000]", i, (double)p->length[i]);
      return msg;
    }
    if (p->noise && !(std::isfinite(p->noise[i]) && p->noise[i] >= 0.0f && p->noise[i] <= 1000.0f)) {
      snprintf(msg, cap, "noise[%d] = %g outside [0, 1000]", i, (double)p->noise[i]);
      return msg;
    }
    if (p->min_frames && (p->min_frames[i] < 0 || p->min_frames[i] > 1000000)) {
      snprintf(msg, cap, "min_frames[%d] = %d outside [0, 1000000]", i, p->min_frames[i]);
      return msg;
    }
    if (p->max_frames && (p->max_frames[i] < 0 || p->max_frames[i] > 1000000)) {
      snprintf(msg, cap, "max_frames[%d] = %d outside [0, 1000000]", i, p->max_frames[i]);
      return msg;
    }
    if (p->max_frames && p->min_frames && p->max_frames[i] != 0 && p->min_frames[i] > p->max_frames[i]) {
      snprintf(msg, cap, "min_frames[%d] = %d above max_frames[%d] = %d", i, p->min_frames[i], i, p->max_frames[i]);
      return msg;
    }
  }
  return nullptr;
}

}  // namespace

// What piper_hip_prosody_check and piper_hip_voice_slot_prosody run on entry `item` (−1: a lone record): status + message.
int prosody_check_item(const piper_hip_prosody* p, int item) {
  char msg[160];
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "prosody: null record");
  if (const char* why = check_fields(p, msg, sizeof msg)) {
    if (item >= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "prosody %d: %s", item, why);
    PH_FAIL(PIPER_HIP_ERR_ARG, "prosody: %s", why);
  }
  return PIPER_HIP_OK;
}

int launch_dp_final_prosody(hipStream_t s, const float* z, const float* m, const float* logs, const void* scalars, const float* len, const int32_t* minf,
                            const int32_t* maxf, float* logw, float* w0, int32_t* dur, int N, int T, const int* len_ptr) {
  const dim3 grid((unsigned)ceil_div(T, 256), (unsigned)N);
  hipLaunchKernelGGL(dp_final_prosody_kernel, grid, dim3(256), 0, s, z, m, logs, (const DpScalars*)scalars, len, minf, maxf, logw, w0, dur, T, len_ptr);
  return PIPER_HIP_OK;
}

// rep holds n + n·T + 3·n entries (prosody_report_entries)
size_t prosody_report_entries(int n, int T) { return (size_t)n + (size_t)n * T + 3 * (size_t)n; }

int launch_dp_paths_prosody(hipStream_t s, const int32_t* dur, const int* lensT, const int32_t* fit, int T, int F, int cap, int32_t* frame2id, int* lensF,
                            int32_t* rep, int n) {
  if (T > 4096 || !rep) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "dp_paths_prosody: %d ids per row (at most 4096) or no report area", T);
  hipLaunchKernelGGL(dp_paths_prosody_kernel, dim3(n), dim3(256), 0, s, dur, lensT, fit, T, F, cap, frame2id, lensF, rep, n);
  return PIPER_HIP_OK;
}

int launch_expand_noise_prosody(hipStream_t s, const float* stats, const int32_t* frame2id, const float* noise, const float* id_noise, float* zp,
                                float* zp_tap, int NB, int I, int T, int F, const float* noise_scale, const unsigned* rng, const int* lensF) {
  const int grid = (int)std::min<int64_t>(ceil_div((int64_t)I * F, 256), 4096);
  hipLaunchKernelGGL(expand_noise_prosody_kernel, dim3(grid, NB), dim3(256), 0, s, stats, frame2id, noise, id_noise, zp, zp_tap, I, T, F, noise_scale, rng,
                     lensF);
  return PIPER_HIP_OK;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(prosody, dp_final_prosody_kernel); } }

using namespace ph;

PH_EXPORT int piper_hip_prosody_check(const piper_hip_prosody* p) { return prosody_check_item(p, -1); }

// The integer rule of the header, from w0 on: host arithmetic in the order the kernels carry it out.
PH_EXPORT int piper_hip_prosody_frames(const piper_hip_prosody* p, const float* w0, int32_t t, int64_t cap, int32_t* frames_out, int64_t* wanted) {
  if (!w0 || !frames_out) PH_FAIL(PIPER_HIP_ERR_ARG, "prosody_frames: null argument");
  if (t < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "prosody_frames: t = %d (at least 1)", t);
  if (p) {
    if (int rc = prosody_check_item(p, -1)) return rc;
    if (p->t != t) PH_FAIL(PIPER_HIP_ERR_SHAPE, "prosody_frames: the prosody has %d entries, the utterance %d ids", p->t, t);
  }
  int64_t S = 0;
  for (int i = 0; i < t; i++) {
    const float w1 = w0[i] * ((p && p->length) ? p->length[i] : 1.0f);  // one fp32 multiply (the build evaluates float in float)
    const float c = ceilf(w1);
    const int32_t d0 = c > 0.0f ? (c < 1e6f ? (int32_t)c : 1000000) : 0;
    const int32_t mx = (p && p->max_frames) ? p->max_frames[i] : 0, mn = (p && p->min_frames) ? p->min_frames[i] : 0;
    const int32_t d1 = mx > 0 ? std::min(d0, mx) : d0;
    frames_out[i] = std::max(d1, mn);
    S += frames_out[i];
  }
  if (p && p->fit && cap > 0 && S > cap)
    for (int i = 0; i < t; i++) frames_out[i] = (int32_t)((int64_t)frames_out[i] * cap / S);
  if (wanted) *wanted = S;
  return PIPER_HIP_OK;
}
