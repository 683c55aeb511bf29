// pitch.h — per-item semitone shift: a variable-ratio resampler on the device (pitch.hip); launched from voice.hip behind a plan's graph,
// never captured into it. The arithmetic is the contract of include/piper_hip.h "Pitch".
#pragma once
#include <algorithm>

#include "common.h"

namespace ph {

constexpr uint64_t kPtOne = (uint64_t)1 << 32;  // the step of an item without a pitch: not a filter
constexpr int kPtPhases = 128;                  // rows 0 … 128 inclusive: row p + 1 is read next to row p
constexpr int kPtMaxTaps = 96;                  // P at +12 semitones
constexpr int64_t kPtMaxSamples = (int64_t)1 << 30;  // N below this: j·Q stays inside 64 bits

// The filter of one step Q, designed in double on the host once per process (pt_design) and kept for its life.
struct PtDesign {
  uint64_t Q = 0;
  int P = 0;
  std::vector<float> taps;  // [129][P]
};

// Q of a shift; PIPER_HIP_ERR_ARG (message with `who` and the field) for a value that is not finite or outside [−12, 12]
int pt_step(const char* who, float semitones, uint64_t* Q);
inline int pt_taps(uint64_t Q) { return 2 * (int)((24 * std::max(Q, kPtOne) + kPtOne - 1) >> 32); }
__host__ __device__ inline int64_t pt_count(int64_t n, uint64_t Q) { return (int64_t)((((uint64_t)n << 32) + Q - 1) / Q); }  // N', n < 2^30
int pt_design(uint64_t Q, const PtDesign** out);
// the sequential twin of the kernel: x[n] → y[pt_count(n, Q)]
void pt_apply_host(const PtDesign& d, const float* x, int64_t n, float* y);

// One item as the kernel takes it: its step and its [129][P] table in device memory (Q == kPtOne: no table, the item is copied).
struct PtItem {
  const float* taps;
  uint64_t Q;
  int P, pad;
};

// Items of audio [NB][row], item b over its true length lensF[b]·hop (read from device memory, clamped to F) → out [NB][out_row]: the N'
// samples of the contract, then +0.0f up to F'·hop, F' = ceil(N' / hop), which goes to lensF_out[b]. items: [NB] in device memory.
// q_min / p_max: the least step and the most taps of the batch (they size the grid and the LDS). lensF == nullptr: one item of n_flat
// samples described by `one`, no tail and no lensF_out (the per-op entry point). out_row ≥ ceil(pt_count(F·hop, q_min) / hop)·hop.
hipError_t launch_pitch_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                              const PtItem* items, PtItem one, uint64_t q_min, uint64_t q_max, int p_max, float* out, int64_t out_row,
                              int* lensF_out);

}  // namespace ph
