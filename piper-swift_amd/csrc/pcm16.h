// pcm16.h — fp32 waveform → 16-bit PCM on the device (pcm16.hip); launched from voice.hip behind a plan's graph, never captured into it.
#pragma once
#include "common.h"

namespace ph {

// The per-step descriptor of a batched stream (voice.hip builds it, stream_chunk_pack_kernel and its int16 sibling read it): one row of
// kDescInts per generator row — source item, window start a, window length Fc (0: finished, dropped or pad row), halo skip (f0 − a)·hop,
// samples of the chunk, offset of the chunk in the packed output (in samples, whatever the sample type).
enum { kDescSrc = 0, kDescA, kDescFc, kDescSkip, kDescN, kDescOff, kDescInts };

// The conversion of one sample (pcm16.hip tells the contract), shared with the resampling kernels (resample.hip): norm == 0 is the reference
// mode on x·gain, norm == 1 the peak mode with `scale` = fp32(32767 / max(0.01, peak)). law: the G.711 law of a kernel whose sink is one
// byte per sample (PIPER_HIP_G711_MULAW / _ALAW, uniform per launch); the int16 and fp32 sinks do not read it.
struct PcmCvt {
  float gain, scale;
  int norm;
  int law;
};

__device__ __forceinline__ int pcm_cvt(float x, const PcmCvt c) {
  if (c.norm) {
    float v = x * c.scale;
    v = v * c.gain;
    v = v != v ? 0.0f : fminf(fmaxf(v, -32767.0f), 32767.0f);
    return (int)v;  // v_cvt_i32_f32 truncates toward zero
  }
  double d = (double)(x * c.gain);
  d = d != d ? 0.0 : fmin(fmax(d, -1.0), 1.0);
  return (int)(d * 32767.0);  // v_cvt_i32_f64 truncates toward zero
}

__device__ __forceinline__ unsigned pcm_pair(float lo, float hi, const PcmCvt c) {
  return ((unsigned)pcm_cvt(lo, c) & 0xffffu) | ((unsigned)pcm_cvt(hi, c) << 16);  // little-endian: the first sample in the low half
}

// int16 sample → G.711 byte (include/piper_hip.h "G.711 output": the Sun g711.c definition), branch-free. The segment is the bit length of
// the biased magnitude instead of a table search: μ-law m = min(|s >> 2|, 8159) + 33 lies in [33, 8192], seg = ⌊log2 m⌋ − 5, and seg 8
// (m = 8192 only) yields 0x80, which the min turns into the clip code 0x7F; A-law m = s >> 3 with the sign's bits flipped (−v − 1) lies in
// [0, 4095], seg = max(0, bitlen(m) − 5), the mantissa shift is max(seg, 1). The sign is bit 7 of the mask.
__device__ __forceinline__ unsigned g711_cvt(int s, int law) {
  const bool alaw = law == PIPER_HIP_G711_ALAW;
  const int v = s >> (alaw ? 3 : 2);
  const int sgn = v >> 31;  // 0 or −1
  const int m = alaw ? (v ^ sgn) : min((v ^ sgn) - sgn, 8159) + 33;
  const int bl = 32 - __clz(m | 1);  // bit length (m | 1: 0 counts as one bit, every other m is unchanged in length)
  const int seg = alaw ? max(bl - 5, 0) : bl - 6;
  const int sh = alaw ? max(seg, 1) : seg + 1;
  const int code = min((seg << 4) | ((m >> sh) & 15), 0x7F);
  return (unsigned)(code ^ (alaw ? 0xD5 : 0xFF) ^ (sgn & 0x80));
}

// four samples → four bytes, the first in the low byte (little-endian)
__device__ __forceinline__ unsigned g711_quad(float a, float b, float c2, float d, const PcmCvt c) {
  return g711_cvt(pcm_cvt(a, c), c.law) | (g711_cvt(pcm_cvt(b, c), c.law) << 8) | (g711_cvt(pcm_cvt(c2, c), c.law) << 16) |
         (g711_cvt(pcm_cvt(d, c), c.law) << 24);
}

// frames of an item as the device reports them, clamped to the plan's row
__device__ __forceinline__ int clamp_len(int len, int F) { return min(max(len, 0), F); }

// n samples src → dst, shared among `nth` threads of which this is `tid`
__device__ __forceinline__ void pcm_span(const float* __restrict__ src, int16_t* __restrict__ dst, int64_t n, int64_t tid, int64_t nth,
                                         const PcmCvt c) {
  const bool src16 = ((uintptr_t)src & 15) == 0;
  int64_t done = 0;
  if (src16 && ((uintptr_t)dst & 15) == 0) {
    const int64_t n8 = n >> 3;
    for (int64_t i = tid; i < n8; i += nth) {
      const float4 a = ((const float4*)src)[2 * i], b = ((const float4*)src)[2 * i + 1];
      uint4 o;
      o.x = pcm_pair(a.x, a.y, c); o.y = pcm_pair(a.z, a.w, c); o.z = pcm_pair(b.x, b.y, c); o.w = pcm_pair(b.z, b.w, c);
      ((uint4*)dst)[i] = o;
    }
    done = n8 << 3;
  } else if (src16 && ((uintptr_t)dst & 7) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 a = ((const float4*)src)[i];
      uint2 o;
      o.x = pcm_pair(a.x, a.y, c); o.y = pcm_pair(a.z, a.w, c);
      ((uint2*)dst)[i] = o;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) dst[i] = (int16_t)pcm_cvt(src[i], c);
}

// the same with one G.711 byte per sample (c.law), dst at any byte address
__device__ __forceinline__ void pcm_span(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t n, int64_t tid, int64_t nth,
                                         const PcmCvt c) {
  const int64_t head = min(n, (int64_t)((4 - ((uintptr_t)dst & 3)) & 3));  // byte stores up to the first 4-byte-aligned address
  for (int64_t i = tid; i < head; i += nth) dst[i] = (uint8_t)g711_cvt(pcm_cvt(src[i], c), c.law);
  const float* s = src + head;
  uint8_t* d = dst + head;
  const int64_t m = n - head;
  const bool src16 = ((uintptr_t)s & 15) == 0;
  int64_t done = 0;
  if (src16 && ((uintptr_t)d & 15) == 0) {
    const int64_t n16 = m >> 4;
    for (int64_t i = tid; i < n16; i += nth) {
      const float4 a = ((const float4*)s)[4 * i], b = ((const float4*)s)[4 * i + 1], e = ((const float4*)s)[4 * i + 2], f = ((const float4*)s)[4 * i + 3];
      uint4 o;
      o.x = g711_quad(a.x, a.y, a.z, a.w, c); o.y = g711_quad(b.x, b.y, b.z, b.w, c);
      o.z = g711_quad(e.x, e.y, e.z, e.w, c); o.w = g711_quad(f.x, f.y, f.z, f.w, c);
      ((uint4*)d)[i] = o;
    }
    done = n16 << 4;
  } else {
    const int64_t n4 = m >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 a;
      if (src16) a = ((const float4*)s)[i];
      else { a.x = s[4 * i]; a.y = s[4 * i + 1]; a.z = s[4 * i + 2]; a.w = s[4 * i + 3]; }
      ((unsigned*)d)[i] = g711_quad(a.x, a.y, a.z, a.w, c);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < m; i += nth) d[i] = (uint8_t)g711_cvt(pcm_cvt(s[i], c), c.law);
}

// the same with a float sink: the chunk itself (a mixed stream step's F32 row at the voice's rate)
__device__ __forceinline__ void pcm_span(const float* __restrict__ src, float* __restrict__ dst, int64_t n, int64_t tid, int64_t nth, const PcmCvt) {
  int64_t done = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) ((float4*)dst)[i] = ((const float4*)src)[i];
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) dst[i] = src[i];
}

// Items of plan audio [NB][row] → back to back at their true lengths lensF[b]·hop in `out` (device memory or a page-locked host mapping),
// item b at hop·Σ_{i<b} lensF[i]; lengths are read from device memory and clamped to F, so at most NB·F·hop samples are written.
// peaks == nullptr: the reference conversion of x·gain. peaks != nullptr ([NB], from launch_pcm16_peak): peak normalisation per item;
// peaks_host (optional, host mapping) then receives a copy of the peaks. NB ≤ 256.
// law (here and below): 0 = `out` is int16_t*; PIPER_HIP_G711_MULAW / _ALAW = `out` is uint8_t*, one byte per sample, at any byte address.
hipError_t launch_pcm16_pack(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float gain,
                             const float* peaks, float* peaks_host, void* out, int law);
// peaks[b] = max |x| over item b's true samples (NaN ignored, 0 for an empty item). Zeroes `peaks` first (stream-ordered).
hipError_t launch_pcm16_peak(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float* peaks);
// n contiguous samples, the reference conversion of x·gain
hipError_t launch_pcm16_flat(hipStream_t q, const float* x, int64_t n, float gain, void* out, int law, int num_cus);
// stream_chunk_pack_kernel with int16 or G.711 output: same descriptor, same grid
hipError_t launch_stream_chunk_pack_pcm16(hipStream_t q, int px, int NBg, const float* audio, int64_t row, const int* desc, float gain,
                                          void* out, int law);

}  // namespace ph
