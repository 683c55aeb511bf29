// pitch.hip — per-item semitone shift of fp32 audio on the device (include/piper_hip.h "Pitch").
//
// To raise the pitch by ρ the voice synthesises ρ times slower (length_scale, on the device already) and this stage plays the result ρ
// times faster: a variable-ratio resampler, nothing else. The conversion is a contract, tested bit for bit against a numpy restatement
// (tests/pitch_ref.py):
//   step      Q = floor(2^(st/12)·2^32 + 0.5), 32.32 fixed point; output j sits at input position u = j·Q: n = u >> 32, frac = u & (2^32 − 1).
//   filter    Kaiser-windowed sinc at 128 phases (129 rows), P = 2·⌈24·max(Q, 2^32) / 2^32⌉ taps, cutoff 0.93·min(1, 2^32 / Q), β = 9; designed
//             in double, every row divided by its own sum, rounded once to fp32: the table c[129][P] (pt_design below).
//   sample    p = frac >> 25, α = ((frac >> 1) & 0xffffff)·2^−24; y0 = Σ_t c[p][t]·x[n − (P/2 − 1) + t], y1 the same with c[p + 1], x = 0 outside
//             [0, N), fp32 in ascending t from 0.0f, each product rounded, then each sum; y[j] = y0 + α·(y1 − y0), each operation rounded.
//
// The kernel is the sibling of resample_items_kernel: a block is one item by a tile of consecutive outputs. The item's table (at most
// 49 536 bytes) is staged into LDS once per block, the tile's input span once per tile, by 16-byte loads where the source is aligned and
// zeros outside the item resolved while staging; a thread runs the two P-term sums of four adjacent outputs out of LDS and stores them as
// 16 bytes where all four belong to the row. Lengths come from device memory, so plain, ragged and bounded slots take the same launch,
// which also writes the zero tail up to the frame boundary and the pitched frame count. Nothing is atomic or order-dependent.
#include "pitch.h"

#include <algorithm>
#include <cmath>
#include <memory>

#include "pcm16.h"

namespace ph {
namespace {

constexpr int kPtTile = 1024;  // outputs per tile: one quad per thread
static_assert(kPtTile == 4 * 256, "a tile is one quad of outputs per thread of the block");

__host__ __device__ inline int pt_tab_floats(int P) { return ((kPtPhases + 1) * P + 3) & ~3; }
// floats of the staged input span of a tile: ⌊(tile − 1)·Q / 2^32⌋ + 1 samples between the first and the last centre, P around them, up
// to 3 in front for the 16-byte alignment, rounded up to whole float4s
inline size_t pt_span_floats(uint64_t q_max, int p_max) { return (size_t)((((uint64_t)kPtTile * q_max) >> 32) + 1 + p_max + 3 + 3) & ~(size_t)3; }

__device__ __forceinline__ float pt_at(const float* x, int64_t n, int64_t g) { return g >= 0 && g < n ? x[g] : 0.0f; }

__global__ __launch_bounds__(256) void pitch_items_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                          int64_t n_flat, const PtItem* __restrict__ items, const PtItem one,
                                                          float* __restrict__ out, int64_t out_row, int* __restrict__ lensF_out) {
  extern __shared__ float4 pt_lds[];
  float* lds = (float*)pt_lds;
  const int b = blockIdx.y, tid = threadIdx.x;
  const PtItem it = items ? items[b] : one;
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  const float* x = audio + (int64_t)b * row;
  float* y = out + (int64_t)b * out_row;
  const int64_t n_out = it.Q == kPtOne ? n : pt_count(n, it.Q);
  int64_t n_row = n_out;  // what the block's row receives: the samples, then zeros up to the frame boundary
  if (lensF) {
    const int64_t Fp = (n_out + hop - 1) / hop;
    n_row = min(Fp * hop, out_row);  // (the launch sizes out_row for the least step of the batch: never the smaller)
    if (lensF_out && blockIdx.x == 0 && tid == 0) lensF_out[b] = (int)(n_row / hop);
  }
  if (it.Q == kPtOne) {  // not a filter: the item passes bit for bit (n_row == n: whole frames)
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n_row; i += (int64_t)gridDim.x * 256) y[i] = i < n ? x[i] : 0.0f;
    return;
  }
  if (n_row <= 0) return;  // (the whole block: an empty item)
  const int P = it.P, half = P >> 1;
  float* xs = lds + pt_tab_floats(P);
  for (int i = tid; i < ((kPtPhases + 1) * P) >> 1; i += 256) ((float2*)lds)[i] = ((const float2*)it.taps)[i];  // (the first tile's barrier covers it)
  const int lead = (int)(((uintptr_t)y >> 2) & 3);  // outputs are numbered v = j + lead: v % 4 == 0 is a 16-byte-aligned address
  const int64_t vend = n_row + lead;
  for (int64_t v0 = (int64_t)blockIdx.x * kPtTile; v0 < vend; v0 += (int64_t)gridDim.x * kPtTile) {
    const int64_t ja = v0 > lead ? v0 - lead : 0;
    const int64_t jb = min((v0 + kPtTile < vend ? v0 + kPtTile : vend) - lead, n_out);  // the tile's filtered outputs [ja, jb)
    int64_t na = 0, g0 = 0;
    __syncthreads();  // the previous tile has been read
    if (ja < jb) {
      na = (int64_t)(((uint64_t)ja * it.Q) >> 32);
      const int64_t nb = (int64_t)(((uint64_t)(jb - 1) * it.Q) >> 32);
      // the samples the tile reads are [na − (half − 1), nb + half]; the staged span starts up to 3 earlier, where x is 16-byte aligned
      g0 = na - (half - 1);
      g0 -= ((int64_t)((uintptr_t)x >> 2) + g0) & 3;
      const int span = (int)(nb + half - g0) + 1;
      for (int q = tid; q < (span + 3) >> 2; q += 256) {
        const int64_t g = g0 + 4 * q;
        float4 v;
        if (g >= 0 && g + 4 <= n) {
          v = *(const float4*)(x + g);
        } else {
          v.x = pt_at(x, n, g); v.y = pt_at(x, n, g + 1); v.z = pt_at(x, n, g + 2); v.w = pt_at(x, n, g + 3);
        }
        *(float4*)(xs + 4 * q) = v;
      }
    }
    __syncthreads();
    for (int q = tid; q < kPtTile / 4; q += 256) {
      const int64_t v = v0 + 4 * q;
      float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        ok[k] = v + k >= lead && v + k < vend;
        const int64_t j = v + k - lead;
        if (!ok[k] || j >= n_out) continue;  // (past N': the zero tail)
        const uint64_t u = (uint64_t)j * it.Q;
        const unsigned frac = (unsigned)u;
        const int p = (int)(frac >> 25);
        const float alpha = (float)((frac >> 1) & 0xffffffu) * 5.9604644775390625e-08f;  // 2^−24; the product is exact
        const float* xp = xs + (int)((int64_t)(u >> 32) - (half - 1) - g0);
        const float* c0 = lds + p * P;
        const float* c1 = c0 + P;
        float y0 = 0.0f, y1 = 0.0f;
        for (int t = 0; t < P; t += 2) {  // P is even; ascending t, product and sum rounded separately
          const float2 a = *(const float2*)(c0 + t), c = *(const float2*)(c1 + t);
          const float s0 = xp[t], s1 = xp[t + 1];
          y0 = y0 + a.x * s0;
          y1 = y1 + c.x * s0;
          y0 = y0 + a.y * s1;
          y1 = y1 + c.y * s1;
        }
        const float d = y1 - y0;
        const float e = alpha * d;
        r[k] = y0 + e;
      }
      const int64_t o = v - lead;  // index of the thread's first sample in the row
      if (ok[0] && ok[3]) {        // (the outputs are a range: first and last inside means all inside)
        *(float4*)(y + o) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (ok[k]) y[o + k] = r[k];
      }
    }
  }
}

// ---- filter design (host, double)

double pt_bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

}  // namespace

int pt_step(const char* who, float semitones, uint64_t* Q) {
  if (!std::isfinite(semitones) || semitones < -12.0f || semitones > 12.0f)
    PH_FAIL(PIPER_HIP_ERR_ARG, "%s: semitones %g is not finite or outside [-12, 12]", who, (double)semitones);
  const double rho = std::exp2((double)semitones / 12.0);
  *Q = (uint64_t)std::floor(rho * 4294967296.0 + 0.5);
  return PIPER_HIP_OK;
}

int pt_design(uint64_t Q, const PtDesign** out) {
  if (Q < (kPtOne >> 1) || Q > (kPtOne << 1)) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch: step %llu outside [2^31, 2^33]", (unsigned long long)Q);
  static std::mutex mu;
  static std::map<uint64_t, std::unique_ptr<PtDesign>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto& slot = cache[Q];
  if (!slot) {
    std::unique_ptr<PtDesign> d(new PtDesign());
    const int P = pt_taps(Q);
    d->Q = Q; d->P = P;
    d->taps.resize((size_t)(kPtPhases + 1) * P);
    const double pi = 3.14159265358979323846, rq = (double)Q / 4294967296.0, fc = 0.93 * std::min(1.0, 1.0 / rq), half = (double)(P / 2);
    const double i0b = pt_bessel_i0(9.0);
    std::vector<double> c((size_t)P);
    for (int p = 0; p <= kPtPhases; p++) {
      double sum = 0.0;
      for (int t = 0; t < P; t++) {
        const double tau = (double)(t - (P / 2 - 1)) - (double)p / 128.0;
        const double a = fc * tau;
        const double h = fc * (a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a));
        const double r = tau / half;
        const double w = std::fabs(tau) < half ? pt_bessel_i0(9.0 * std::sqrt(1.0 - r * r)) / i0b : 0.0;
        c[t] = h * w;
        sum += c[t];
      }
      for (int t = 0; t < P; t++) d->taps[(size_t)p * P + t] = (float)(c[t] / sum);
    }
    slot = std::move(d);
  }
  *out = slot.get();
  return PIPER_HIP_OK;
}

void pt_apply_host(const PtDesign& d, const float* x, int64_t n, float* y) {
  const int P = d.P, half = P / 2;
  const int64_t n_out = pt_count(n, d.Q);
  for (int64_t j = 0; j < n_out; j++) {
    const uint64_t u = (uint64_t)j * d.Q;
    const unsigned frac = (unsigned)u;
    const int p = (int)(frac >> 25);
    const float alpha = (float)((frac >> 1) & 0xffffffu) * 5.9604644775390625e-08f;
    const int64_t base = (int64_t)(u >> 32) - (half - 1);
    const float* c0 = d.taps.data() + (size_t)p * P;
    const float* c1 = c0 + P;
    float y0 = 0.0f, y1 = 0.0f;
    for (int t = 0; t < P; t++) {
      const int64_t g = base + t;
      const float s = g >= 0 && g < n ? x[g] : 0.0f;
      y0 = y0 + c0[t] * s;
      y1 = y1 + c1[t] * s;
    }
    const float dd = y1 - y0;
    const float e = alpha * dd;
    y[j] = y0 + e;
  }
}

hipError_t launch_pitch_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                              const PtItem* items, PtItem one, uint64_t q_min, uint64_t q_max, int p_max, float* out, int64_t out_row,
                              int* lensF_out) {
  if (NB < 1 || hop < 1 || (!lensF && NB != 1) || (lensF && !items)) return hipErrorInvalidValue;
  if (q_min < (kPtOne >> 1) || q_max > (kPtOne << 1) || q_min > q_max || p_max < 2 || p_max > kPtMaxTaps) return hipErrorInvalidValue;
  const int64_t n_max = lensF ? (int64_t)F * hop : n_flat;
  if (n_max < 0 || n_max >= kPtMaxSamples) return hipErrorInvalidValue;
  const int64_t outs = lensF ? ceil_div(pt_count(n_max, q_min), hop) * hop : pt_count(n_max, q_min);
  if (lensF && out_row < outs) return hipErrorInvalidValue;  // a row holds the longest item the batch's least step can make
  const size_t lds = ((size_t)pt_tab_floats(p_max) + pt_span_floats(q_max, p_max)) * sizeof(float);
  const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(outs + 3, kPtTile), 1), 128), NB);
  hipLaunchKernelGGL(pitch_items_kernel, grid, dim3(256), lds, q, audio, row, lensF, F, hop, n_flat, items, one, out, out_row, lensF_out);
  return hipGetLastError();
}

namespace { PH_WARM(pitch, pitch_items_kernel); }

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_pitch_check(const piper_hip_pitch* pitch) {
  if (!pitch) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_check: null pitch");
  uint64_t Q;
  if (int rc = pt_step("pitch_check", pitch->semitones, &Q)) return rc;
  if (pitch->keep_tempo != 0 && pitch->keep_tempo != 1) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_check: keep_tempo %d (0 or 1)", pitch->keep_tempo);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_pitch_info(float semitones, uint64_t* step, int32_t* taps, float* length_factor) {
  uint64_t Q;
  if (int rc = pt_step("pitch_info", semitones, &Q)) return rc;
  if (step) *step = Q;
  if (taps) *taps = pt_taps(Q);
  if (length_factor) *length_factor = (float)((double)Q / 4294967296.0);
  return PIPER_HIP_OK;
}

PH_EXPORT int64_t piper_hip_pitch_count(float semitones, int64_t n_in) {
  uint64_t Q;
  if (int rc = pt_step("pitch_count", semitones, &Q)) return rc;
  if (n_in < 0 || n_in >= kPtMaxSamples) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_count: %lld input samples (0 … 2^30 − 1)", (long long)n_in);
  return pt_count(n_in, Q);
}

PH_EXPORT int piper_hip_pitch_taps(float semitones, float* table, size_t max_floats) {
  uint64_t Q;
  if (int rc = pt_step("pitch_taps", semitones, &Q)) return rc;
  const PtDesign* d = nullptr;
  if (int rc = pt_design(Q, &d)) return rc;
  if (!table) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_taps: null table");
  if (max_floats < d->taps.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "pitch_taps: buffer holds %zu < %zu floats", max_floats, d->taps.size());
  memcpy(table, d->taps.data(), d->taps.size() * sizeof(float));
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_pitch_from_f32(float semitones, const float* x, size_t n, float* y, size_t max_out, size_t* n_out) {
  uint64_t Q;
  if (int rc = pt_step("pitch_from_f32", semitones, &Q)) return rc;
  if (n >= (size_t)kPtMaxSamples) PH_FAIL(PIPER_HIP_ERR_SHAPE, "pitch_from_f32: %zu samples (below 2^30)", n);
  if ((!x && n) || (!y && n)) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_from_f32: null buffer");
  const size_t count = Q == kPtOne ? n : (size_t)pt_count((int64_t)n, Q);
  if (max_out < count) PH_FAIL(PIPER_HIP_ERR_SHAPE, "pitch_from_f32: buffer holds %zu < %zu samples", max_out, count);
  if (n_out) *n_out = count;
  if (Q == kPtOne) {  // not a filter
    if (n) memmove(y, x, n * sizeof(float));
    return PIPER_HIP_OK;
  }
  const PtDesign* d = nullptr;
  if (int rc = pt_design(Q, &d)) return rc;
  pt_apply_host(*d, x, (int64_t)n, y);
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_pitch_f32(piper_hip_ctx* ctx, const float* x, size_t count, float semitones, float** out, size_t* out_count,
                                  piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_f32: null output pointer");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_f32: null input");
  if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "pitch_f32: the output buffer is not 4-byte aligned");
  if (count >= (size_t)kPtMaxSamples) PH_FAIL(PIPER_HIP_ERR_SHAPE, "pitch_f32: %zu samples (below 2^30)", count);
  uint64_t Q;
  int rc = pt_step("pitch_f32", semitones, &Q);
  if (rc) return rc;
  const size_t n_out = Q == kPtOne ? count : (size_t)pt_count((int64_t)count, Q);
  if (!*out) {
    void* p = nullptr;
    if ((rc = ctx->pool.alloc(n_out * sizeof(float), &p))) return rc;
    *out = (float*)p;
  }
  if (out_count) *out_count = n_out;
  if (n_out == 0) return PIPER_HIP_OK;
  StreamScope ss(ctx, stream);
  if (Q == kPtOne) {  // not a filter: a copy
    PH_HIP(hipMemcpyAsync(*out, x, count * sizeof(float), hipMemcpyDeviceToDevice, ss.s), PIPER_HIP_ERR_LAUNCH);
    return ss.finish("pitch_f32");
  }
  const PtDesign* d = nullptr;
  if ((rc = pt_design(Q, &d))) return rc;
  void* tab = nullptr;
  if ((rc = ctx->pool.alloc(d->taps.size() * sizeof(float), &tab))) return rc;
  defer_free(ctx, tab);
  PH_HIP(hipMemcpyAsync(tab, d->taps.data(), d->taps.size() * sizeof(float), hipMemcpyHostToDevice, ss.s), PIPER_HIP_ERR_LAUNCH);
  const PtItem one{(const float*)tab, Q, d->P, 0};
  PH_HIP(launch_pitch_items(ss.s, x, 0, nullptr, 0, 1, 1, (int64_t)count, nullptr, one, Q, Q, d->P, *out, 0, nullptr), PIPER_HIP_ERR_LAUNCH);
  return ss.finish("pitch_f32");
}
