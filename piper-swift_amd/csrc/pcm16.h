// pcm16.h — fp32 waveform → 16-bit PCM on the device (pcm16.hip); launched from voice.hip behind a plan's graph, never captured into it.
#pragma once
#include "common.h"

namespace ph {

// The per-step descriptor of a batched stream (voice.hip builds it, stream_chunk_pack_kernel and its int16 sibling read it): one row of
// kDescInts per generator row — source item, window start a, window length Fc (0: finished, dropped or pad row), halo skip (f0 − a)·hop,
// samples of the chunk, offset of the chunk in the packed output (in samples, whatever the sample type).
enum { kDescSrc = 0, kDescA, kDescFc, kDescSkip, kDescN, kDescOff, kDescInts };

// The conversion of one sample (pcm16.hip tells the contract), shared with the resampling kernels (resample.hip): norm == 0 is the reference
// mode on x·gain, norm == 1 the peak mode with `scale` = fp32(32767 / max(0.01, peak)).
struct PcmCvt {
  float gain, scale;
  int norm;
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

// frames of an item as the device reports them, clamped to the plan's row
__device__ __forceinline__ int clamp_len(int len, int F) { return min(max(len, 0), F); }

// Items of plan audio [NB][row] → back to back at their true lengths lensF[b]·hop in `out` (device memory or a page-locked host mapping),
// item b at hop·Σ_{i<b} lensF[i]; lengths are read from device memory and clamped to F, so at most NB·F·hop samples are written.
// peaks == nullptr: the reference conversion of x·gain. peaks != nullptr ([NB], from launch_pcm16_peak): peak normalisation per item;
// peaks_host (optional, host mapping) then receives a copy of the peaks. NB ≤ 256.
hipError_t launch_pcm16_pack(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float gain,
                             const float* peaks, float* peaks_host, int16_t* out);
// peaks[b] = max |x| over item b's true samples (NaN ignored, 0 for an empty item). Zeroes `peaks` first (stream-ordered).
hipError_t launch_pcm16_peak(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, float* peaks);
// n contiguous samples, the reference conversion of x·gain
hipError_t launch_pcm16_flat(hipStream_t q, const float* x, int64_t n, float gain, int16_t* out, int num_cus);
// stream_chunk_pack_kernel with int16 output: same descriptor, same grid
hipError_t launch_stream_chunk_pack_pcm16(hipStream_t q, int px, int NBg, const float* audio, int64_t row, const int* desc, float gain,
                                          int16_t* out);

}  // namespace ph
