// volume.hip — per-phoneme volume: one gain per id, ramped linearly between frame centres (include/piper_hip.h "Per-phoneme volume").
//
// The envelope is a contract, tested bit for bit against a numpy restatement (tests/volume_ref.py). All arithmetic is fp32, every operation
// rounded on its own:
//   gf[f]  = gain[t(f)], the gain of the id frame f belongs to (frame2id)           f in [0, F)
//   c      = hop div 2;  m = n − c;  k = floor(m / hop);  i = m − k·hop
//   e(n)   = gf[max(k, 0)] + (gf[min(k + 1, F − 1)] − gf[max(k, 0)])·((float)i / (float)hop)
//   v[n]   = x[n]·e(n)
// One launch, one read and one write per sample: a thread takes four consecutive samples. With hop % 8 == 0 the centre offset c is a
// multiple of four, so an aligned group of four never crosses a frame centre: it shares both gains and moves as one 16-byte load and one
// 16-byte store where the rows are aligned. Any other hop, and unaligned rows, take the scalar path. blockIdx.y is the item; lengths are
// read from device memory, so a bounded slot takes the same launch. A stream step is the same routine over the chunk of every generator
// row (VolStepRow: the chunk's absolute place in its item and the row's gains per frame), one launch for all rows; a row without a volume
// has its chunk copied, so the stages behind read one buffer.
#include "volume.h"

#include <algorithm>
#include <cmath>

#include "pcm16.h"

#pragma clang fp contract(off)

namespace ph {
namespace {

// the gain of frame f of a row of F ≥ 1 frames: the row's own gf, or the id's gain through frame2id
struct VolGains {
  const float* gf;       // [F] per frame, or null
  const int32_t* f2i;    // [F] frame → id
  const float* gain;     // [T] per id
  int T;
  __device__ __forceinline__ float at(int64_t f) const {
    if (gf) return gf[f];
    // (no producer of frame2id writes an id outside [0, T): prepare stages ids below the item's t, the path kernels bisect over T entries.
    // The clamp keeps the read inside the row's gains whatever the map holds; it is not part of the contract.)
    return gain[min(max(f2i[f], 0), T - 1)];
  }
};

// (float)i / (float)hop, correctly rounded: hop a power of two → the product with 1 / hop is that quotient exactly
__device__ __forceinline__ float vol_w(int i, float hopf, float inv, bool pow2) { return pow2 ? (float)i * inv : __fdiv_rn((float)i, hopf); }

__device__ __forceinline__ float vol_env(float a, float d, float w) { return a + d * w; }

// Samples [base, base + n) of an item of Fb frames, x[0] and y[0] being sample `base` (a whole item: base 0, n = Fb·hop; a stream step: the
// chunk, base and n multiples of hop) → y, the envelope of gains g: the grid's x dimension strides over groups of four samples
__device__ __forceinline__ void vol_row(const float* __restrict__ x, float* __restrict__ y, int64_t base, int64_t n, int64_t Fb, int hop,
                                        const VolGains& g) {
  const int c = hop >> 1;
  const float hopf = (float)hop, inv = 1.0f / hopf;
  const bool pow2 = (hop & (hop - 1)) == 0;
  const bool vec = (hop & 7) == 0 && ((base | n) & 7) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;  // (every group of four is whole)
  for (int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; at < n; at += (int64_t)gridDim.x * 1024) {
    if (vec) {
      const int64_t m = base + at - c;  // a multiple of four, like c and hop: i … i + 3 stay inside one hop
      const int64_t k = m < 0 ? -1 : m / hop;
      const int i = (int)(m - k * hop);
      const float a = g.at(k < 0 ? 0 : k), b = g.at(k + 1 < Fb ? k + 1 : Fb - 1), d = b - a;
      const float4 v = *(const float4*)(x + at);
      float4 o;
      o.x = v.x * vol_env(a, d, vol_w(i, hopf, inv, pow2));
      o.y = v.y * vol_env(a, d, vol_w(i + 1, hopf, inv, pow2));
      o.z = v.z * vol_env(a, d, vol_w(i + 2, hopf, inv, pow2));
      o.w = v.w * vol_env(a, d, vol_w(i + 3, hopf, inv, pow2));
      *(float4*)(y + at) = o;
    } else {
      const int64_t end = at + 4 < n ? at + 4 : n;
      for (int64_t s = at; s < end; s++) {
        const int64_t m = base + s - c;
        const int64_t k = m < 0 ? -1 : m / hop;
        const int i = (int)(m - k * hop);
        const float a = g.at(k < 0 ? 0 : k), b = g.at(k + 1 < Fb ? k + 1 : Fb - 1), d = b - a;
        y[s] = x[s] * vol_env(a, d, vol_w(i, hopf, inv, pow2));
      }
    }
  }
}

// whole items of a plan: item b = blockIdx.y over its true length
__global__ __launch_bounds__(256) void volume_items_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                           const int32_t* __restrict__ frame2id, int64_t f2i_row, const float* __restrict__ gain,
                                                           int T, float* __restrict__ shaped, int64_t out_row) {
  const int b = blockIdx.y;
  const int Fb = clamp_len(lensF[b], F);
  if (Fb < 1 || (int64_t)blockIdx.x * 1024 >= (int64_t)Fb * hop) return;  // (uniform) past the item's length
  const VolGains g{nullptr, frame2id + (int64_t)b * f2i_row, gain + (int64_t)b * T, T};
  vol_row(audio + (int64_t)b * row, shaped + (int64_t)b * out_row, 0, (int64_t)Fb * hop, Fb, hop, g);
}

// one flat item whose gains are given per frame
__global__ __launch_bounds__(256) void volume_flat_kernel(const float* __restrict__ x, const float* __restrict__ frame_gain, int64_t frames, int hop,
                                                          float* __restrict__ y) {
  const VolGains g{frame_gain, nullptr, nullptr, 0};
  vol_row(x, y, 0, frames * hop, frames, hop, g);
}

// one stream step: row r = blockIdx.y of the window plan's audio [rows][row] → the same place in `out`, the chunk alone
__global__ __launch_bounds__(256) void volume_step_kernel(const float* __restrict__ audio, int64_t row, const VolStepRow* __restrict__ desc, int hop,
                                                          float* __restrict__ out) {
  const VolStepRow d = desc[blockIdx.y];
  const int64_t n = d.n;
  if (n <= 0 || (int64_t)blockIdx.x * 1024 >= n) return;  // (uniform) a row without a chunk, or past it
  const float* x = audio + (int64_t)blockIdx.y * row + d.skip;
  float* y = out + (int64_t)blockIdx.y * row + d.skip;
  if (!d.gf) {  // a row without a volume: its chunk as it is, 16 bytes at a time where the chunk allows
    const bool vec = (n & 3) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    for (int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; at < n; at += (int64_t)gridDim.x * 1024) {
      if (vec) *(float4*)(y + at) = *(const float4*)(x + at);
      else for (int64_t s = at; s < at + 4 && s < n; s++) y[s] = x[s];
    }
    return;
  }
  const VolGains g{d.gf, nullptr, nullptr, 0};
  vol_row(x, y, d.n0, n, d.F, hop, g);
}

// gf [NB][F] of the items: the "vol.gain" tap
__global__ __launch_bounds__(256) void volume_frame_gains_kernel(const int* __restrict__ lensF, int F, const int32_t* __restrict__ frame2id,
                                                                 int64_t f2i_row, const float* __restrict__ gain, int T, float* __restrict__ gf) {
  const int b = blockIdx.y;
  const int Fb = clamp_len(lensF[b], F);
  const VolGains g{nullptr, frame2id + (int64_t)b * f2i_row, gain + (int64_t)b * T, T};
  for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) gf[(int64_t)b * F + f] = f < Fb ? g.at(f) : 0.0f;
}

// blocks along x for rows of at most n samples, `rows` rows: four samples per thread, at most ≈ 2048 blocks in all (the rest strides)
unsigned vol_grid(int64_t n, int rows) {
  const int64_t want = ceil_div(n, (int64_t)1024), cap = std::max<int64_t>(2048 / std::max(rows, 1), 8);
  return (unsigned)std::max<int64_t>(std::min(want, cap), 1);
}

const char* vol_check_fields(const piper_hip_volume* v, char* msg, size_t cap) {
  if (v->t < 1) { snprintf(msg, cap, "t = %d (at least 1)", v->t); return msg; }
  for (int i = 0; v->gain && i < v->t; i++)
    if (!(std::isfinite(v->gain[i]) && v->gain[i] >= 0.0f && v->gain[i] <= 16.0f)) {
      snprintf(msg, cap, "gain[%d] = %g outside [0, 16]", i, (double)v->gain[i]);
      return msg;
    }
  return nullptr;
}

}  // namespace

int volume_check_item(const piper_hip_volume* v, int item) {
  char msg[160];
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "volume: null record");
  if (const char* why = vol_check_fields(v, msg, sizeof msg)) {
    if (item >= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "volume %d: %s", item, why);
    PH_FAIL(PIPER_HIP_ERR_ARG, "volume: %s", why);
  }
  return PIPER_HIP_OK;
}

hipError_t launch_volume_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, const int32_t* frame2id,
                               int64_t f2i_row, const float* gain, int T, float* shaped, int64_t out_row) {
  if (NB < 1 || F < 1 || hop < 1 || T < 1 || !lensF || !frame2id || !gain) return hipErrorInvalidValue;
  hipLaunchKernelGGL(volume_items_kernel, dim3(vol_grid((int64_t)F * hop, NB), NB), dim3(256), 0, q, audio, row, lensF, F, hop, frame2id, f2i_row, gain, T,
                     shaped, out_row);
  return hipGetLastError();
}

hipError_t launch_volume_flat(hipStream_t q, const float* x, const float* frame_gain, int64_t frames, int hop, float* y) {
  if (frames < 0 || hop < 1) return hipErrorInvalidValue;
  if (frames == 0) return hipSuccess;
  hipLaunchKernelGGL(volume_flat_kernel, dim3(vol_grid(frames * hop, 1)), dim3(256), 0, q, x, frame_gain, frames, hop, y);
  return hipGetLastError();
}

hipError_t launch_volume_step(hipStream_t q, int rows, int64_t max_n, const float* audio, int64_t row, const VolStepRow* desc, int hop, float* out) {
  if (rows < 1 || hop < 1 || max_n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(volume_step_kernel, dim3(vol_grid(max_n, rows), rows), dim3(256), 0, q, audio, row, desc, hop, out);
  return hipGetLastError();
}

hipError_t launch_volume_frame_gains(hipStream_t q, const int* lensF, int F, int NB, const int32_t* frame2id, int64_t f2i_row, const float* gain, int T,
                                     float* gf) {
  if (NB < 1 || F < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(volume_frame_gains_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(F, 256), 64), NB), dim3(256), 0, q, lensF, F, frame2id, f2i_row,
                     gain, T, gf);
  return hipGetLastError();
}

namespace { PH_WARM(volume, volume_items_kernel); }

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_volume_check(const piper_hip_volume* v) { return volume_check_item(v, -1); }

PH_EXPORT int piper_hip_volume_frames(const piper_hip_volume* v, const int32_t* durations, int32_t t, float* frame_gain, int64_t max_frames,
                                      int64_t* frames) {
  if (!durations) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_frames: null durations");
  if (t < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_frames: t = %d (at least 1)", t);
  if (v) {
    if (int rc = piper_hip_volume_check(v)) return rc;
    if (v->t != t) PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume_frames: the volume has %d entries, the utterance %d ids", v->t, t);
  }
  int64_t sum = 0;
  for (int i = 0; i < t; i++) {
    if (durations[i] < 0) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_frames: durations[%d] = %d is negative", i, durations[i]);
    sum += durations[i];
  }
  const int64_t F = std::max<int64_t>(sum, 1);
  if (frames) *frames = F;
  if (!frame_gain) return PIPER_HIP_OK;
  if (max_frames < F) PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume_frames: buffer holds %lld < %lld frames", (long long)max_frames, (long long)F);
  const float* gain = v ? v->gain : nullptr;
  if (sum == 0) {  // the single frame of an all-zero row belongs to id 0
    frame_gain[0] = gain ? gain[0] : 1.0f;
    return PIPER_HIP_OK;
  }
  int64_t f = 0;
  for (int i = 0; i < t; i++)
    for (int j = 0; j < durations[i]; j++) frame_gain[f++] = gain ? gain[i] : 1.0f;
  return PIPER_HIP_OK;
}

// the host twin of the kernels: the same operations in the same order, every one rounded on its own
PH_EXPORT int piper_hip_volume_from_f32(const float* frame_gain, int64_t frames, int32_t hop, const float* x, size_t n, float* y) {
  if (hop < 1 || hop > 65536) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_from_f32: hop %d outside [1, 65536]", hop);
  if (frames < 0 || frames > ((int64_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume_from_f32: %lld frames", (long long)frames);
  if ((uint64_t)frames * (uint64_t)hop != (uint64_t)n)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume_from_f32: %zu samples are not %lld frames of %d", n, (long long)frames, hop);
  if (n && (!frame_gain || !x || !y)) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_from_f32: null buffer");
  const int64_t c = hop / 2;
  const float hopf = (float)hop;
  for (int64_t s = 0; s < (int64_t)n; s++) {
    const int64_t m = s - c;
    const int64_t k = m < 0 ? -1 : m / hop;
    const int64_t i = m - k * hop;
    const float a = frame_gain[k < 0 ? 0 : k], b = frame_gain[k + 1 < frames ? k + 1 : frames - 1];
    const float w = (float)i / hopf;
    const float d = b - a;
    const float dw = d * w;
    const float e = a + dw;
    y[s] = x[s] * e;
  }
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_volume_f32(piper_hip_ctx* ctx, const float* x, size_t count, const float* frame_gain, int64_t frames, int32_t hop, float** out,
                                   piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_f32: null output pointer");
  if (hop < 1 || hop > 65536) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_f32: hop %d outside [1, 65536]", hop);
  if (frames < 0 || frames > ((int64_t)1 << 40) || count > ((size_t)1 << 40) || (uint64_t)frames * (uint64_t)hop != (uint64_t)count)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume_f32: %zu samples are not %lld frames of %d", count, (long long)frames, hop);
  if ((!x || !frame_gain) && count) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_f32: null input");
  if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "volume_f32: the output buffer is not 4-byte aligned");
  if (!*out) {
    void* q = nullptr;
    if (int rc = ctx->pool.alloc(count * sizeof(float), &q)) return rc;
    *out = (float*)q;
  }
  if (count == 0) return PIPER_HIP_OK;
  StreamScope ss(ctx, stream);
  (void)launch_volume_flat(ss.s, x, frame_gain, frames, hop, *out);
  return ss.finish("volume_f32");
}
