// pcm16.hip — fp32 waveform → 16-bit PCM on the device: the last hop before the bus (include/piper_hip.h "16-bit PCM straight from the device").
//
// The arithmetic is a contract, tested bit for bit against the host's piper_hip_pcm16_from_f32 (audio_io.cpp) and a numpy restatement:
//   reference mode   y = x·gain (fp32; ·1.0f is the identity on every non-NaN float), NaN → 0, clamp to [−1, 1], ×32767.0 in DOUBLE, truncate
//                    toward zero. The multiply is f64 because x·32767 in fp32 can round UP across an integer boundary and the sample would
//                    then be one more than the host's; one v_mul_f64 per sample is free in a kernel that waits for memory.
//   peak mode        Piper's audio_float_to_int16 in float32: v = x·scale_b, v·gain, NaN → 0, clamp to [−32767, 32767], truncate; scale_b =
//                    fp32(32767 / max(0.01, peak_b)), the quotient taken in double and rounded once (= the correctly rounded fp32 quotient).
// The library is built with -ffp-contract=off; none of the products below is followed by an add anyway.
//
// Memory: every kernel here moves each sample once — 16-byte loads, one 16-byte (8 samples) or 8-byte (4 samples) store where source and
// destination are aligned (with hop = 256 every item of a voice path is), scalar otherwise and for the tail. The destination may be a
// page-locked host buffer seen through its device mapping: the stores then ARE the transfer.
//
// G.711 (include/piper_hip.h "G.711 output"): the same kernels with a one-byte sink — the sample type is their template parameter, the law
// travels in PcmCvt. 16 samples leave as one 16-byte store where source and destination are aligned, four as one dword behind a head of
// up to three byte stores otherwise; no store covers a byte outside the span, because the neighbouring bytes of a packed output belong to
// another item whose block writes them at the same time.
#include "pcm16.h"

#include <algorithm>
#include <cmath>

namespace ph {
namespace {

// Plan audio [NB][row] → the items back to back at their true lengths. blockIdx.y = item; the item's offset is the sum of the lengths
// before it (NB ≤ 256 = one per thread), so plain, ragged and bounded slots — whose lengths only the device knows — take the same launch.
// T: int16_t, or uint8_t for G.711 by `law`.
template <class T>
__global__ __launch_bounds__(256) void pcm16_pack_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                         float gain, const float* __restrict__ peaks, float* __restrict__ peaks_host,
                                                         T* __restrict__ out, int law) {
  __shared__ int part[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  int before = tid < b ? clamp_len(lensF[tid], F) : 0;
  for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off);
  if ((tid & 63) == 0) part[tid >> 6] = before;
  __syncthreads();
  const int64_t at = (int64_t)(part[0] + part[1] + part[2] + part[3]) * hop;
  const int64_t n = (int64_t)clamp_len(lensF[b], F) * hop;
  PcmCvt c;
  c.gain = gain; c.scale = 1.0f; c.norm = 0; c.law = law;
  if (peaks) {
    const float peak = peaks[b];
    c.scale = (float)(32767.0 / (double)fmaxf(0.01f, peak));
    c.norm = 1;
    if (peaks_host && blockIdx.x == 0 && tid == 0) peaks_host[b] = peak;
  }
  pcm_span(audio + (int64_t)b * row, out + at, n, (int64_t)blockIdx.x * 256 + tid, (int64_t)gridDim.x * 256, c);
}

// peaks[b] = max |x| of item b (zeroed before the launch). Max is exact in any order, and the bit patterns of non-negative floats order
// like unsigned integers, so one vector atomic max per block is deterministic. fmaxf drops a NaN operand.
__global__ __launch_bounds__(256) void pcm16_peak_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F, int hop,
                                                         float* __restrict__ peaks) {
  __shared__ float part[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = (int64_t)clamp_len(lensF[b], F) * hop;
  const float* src = audio + (int64_t)b * row;
  const int64_t gt = (int64_t)blockIdx.x * 256 + tid, nth = (int64_t)gridDim.x * 256;
  float m = 0.0f;
  int64_t done = 0;
  if (((uintptr_t)src & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = gt; i < n4; i += nth) {
      const float4 a = ((const float4*)src)[i];
      m = fmaxf(fmaxf(m, fabsf(a.x)), fmaxf(fabsf(a.y), fmaxf(fabsf(a.z), fabsf(a.w))));
    }
    done = n4 << 2;
  }
  for (int64_t i = done + gt; i < n; i += nth) m = fmaxf(m, fabsf(src[i]));
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
  if ((tid & 63) == 0) part[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    if (m > 0.0f) atomicMax((unsigned*)peaks + b, __float_as_uint(m));  // (a block past the item's end has nothing to add)
  }
}

template <class T>
__global__ __launch_bounds__(256) void pcm16_flat_kernel(const float* __restrict__ x, int64_t n, float gain, T* __restrict__ out, int law) {
  PcmCvt c;
  c.gain = gain; c.scale = 1.0f; c.norm = 0; c.law = law;
  pcm_span(x, out, n, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256, c);
}

// stream_chunk_pack_kernel (voice.hip) with int16 or G.711 output: each active row's chunk out of the generator plan's audio [NBg][row], the
// halo samples dropped, packed back to back at the descriptor's offsets.
template <class T>
__global__ __launch_bounds__(256) void stream_chunk_pack_pcm16_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ desc,
                                                                      float gain, T* __restrict__ out, int law) {
  const int* d = desc + blockIdx.y * kDescInts;
  const int n = d[kDescN];
  if (n == 0) return;
  PcmCvt c;
  c.gain = gain; c.scale = 1.0f; c.norm = 0; c.law = law;
  pcm_span(audio + (int64_t)blockIdx.y * row + d[kDescSkip], out + d[kDescOff], n, (int64_t)blockIdx.x * 256 + threadIdx.x,
           (int64_t)gridDim.x * 256, c);
}

// blocks along an item: 8 samples per thread and pass, at most 1024 blocks (copy_out_kernel's bound in voice.hip)
int span_blocks(int64_t samples, int per_thread) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(samples, (int64_t)256 * per_thread), 1), 1024); }

}  // namespace

hipError_t launch_pcm16_pack(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float gain,
                             const float* peaks, float* peaks_host, void* out, int law) {
  if (NB < 1 || NB > 256) return hipErrorInvalidValue;  // the offset of an item is summed by one block of 256 threads
  if (law)
    hipLaunchKernelGGL(pcm16_pack_kernel<uint8_t>, dim3(span_blocks((int64_t)F * hop, 16), NB), dim3(256), 0, q, audio, row, lensF, F, hop, gain,
                       peaks, peaks_host, (uint8_t*)out, law);
  else
    hipLaunchKernelGGL(pcm16_pack_kernel<int16_t>, dim3(span_blocks((int64_t)F * hop, 8), NB), dim3(256), 0, q, audio, row, lensF, F, hop, gain,
                       peaks, peaks_host, (int16_t*)out, 0);
  return hipGetLastError();
}

hipError_t launch_pcm16_peak(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float* peaks) {
  if (NB < 1 || NB > 256) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(peaks, 0, (size_t)NB * sizeof(float), q);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pcm16_peak_kernel, dim3(span_blocks((int64_t)F * hop, 16), NB), dim3(256), 0, q, audio, row, lensF, F, hop, peaks);
  return hipGetLastError();
}

hipError_t launch_pcm16_flat(hipStream_t q, const float* x, int64_t n, float gain, void* out, int law, int num_cus) {
  const int64_t cap = (int64_t)num_cus * 8;
  const int grid = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256 * (law ? 16 : 8)), 1), cap);
  if (law) hipLaunchKernelGGL(pcm16_flat_kernel<uint8_t>, dim3(grid), dim3(256), 0, q, x, n, gain, (uint8_t*)out, law);
  else hipLaunchKernelGGL(pcm16_flat_kernel<int16_t>, dim3(grid), dim3(256), 0, q, x, n, gain, (int16_t*)out, 0);
  return hipGetLastError();
}

hipError_t launch_stream_chunk_pack_pcm16(hipStream_t q, int px, int NBg, const float* audio, int64_t row, const int* desc, float gain,
                                          void* out, int law) {
  if (law) hipLaunchKernelGGL(stream_chunk_pack_pcm16_kernel<uint8_t>, dim3(px, NBg), dim3(256), 0, q, audio, row, desc, gain, (uint8_t*)out, law);
  else hipLaunchKernelGGL(stream_chunk_pack_pcm16_kernel<int16_t>, dim3(px, NBg), dim3(256), 0, q, audio, row, desc, gain, (int16_t*)out, 0);
  return hipGetLastError();
}

namespace { PH_WARM(pcm16, pcm16_pack_kernel<int16_t>); }

}  // namespace ph

using namespace ph;

PH_EXPORT int piper_hip_pcm16_f32(piper_hip_ctx* ctx, const float* x, size_t count, float gain, int16_t** out, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched (tests/test_pcm16_ref.py)
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16_f32: null output pointer");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16_f32: null input");
  if (!(gain >= 0.0f) || !std::isfinite(gain)) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16_f32: gain %g is negative or not finite", (double)gain);
  if (((uintptr_t)*out & 1) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16_f32: the output buffer is not 2-byte aligned");
  if (!*out) {
    void* p = nullptr;
    const int rc = ctx->pool.alloc(count * sizeof(int16_t), &p);
    if (rc) return rc;
    *out = (int16_t*)p;
  }
  if (count == 0) return PIPER_HIP_OK;
  StreamScope ss(ctx, stream);
  (void)launch_pcm16_flat(ss.s, x, (int64_t)count, gain == 0.0f ? 1.0f : gain, *out, 0, ctx->num_cus);
  return ss.finish("pcm16_f32");
}
