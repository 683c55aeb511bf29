// loudness.h — BS.1770 integrated loudness on the device (loudness.hip); launched from voice.hip behind a plan's graph, never captured
// into it. The arithmetic is the contract of include/piper_hip.h "Loudness".
#pragma once
#include "common.h"

namespace ph {

constexpr int kLdChunk = 64;                    // samples a lane filters on its own
constexpr int kLdLanes = 512;                   // lanes of the workgroup that filters one pass
constexpr int kLdSuper = kLdChunk * kLdLanes;   // samples of one pass: what one workgroup filters
constexpr int kLdSegs = kLdSuper / 800 + 2;     // 100 ms segments a pass can touch, at the shortest segment (8000 Hz)
constexpr int kLdScan = 9;                      // scan steps over the lanes: 2^9 = kLdLanes
static_assert((1 << kLdScan) == kLdLanes, "the scan covers every lane");

// The K-weighting of one rate as the kernels take it. State of the cascade: (s1, s2) of the shelf, (t1, t2) of the high-pass, both in
// transposed direct form II; with no input one sample maps the state by a 4×4 matrix A; M[k] = A^(64·2^k) and Mp = A^(64·512), row-major.
struct LdFilter {
  double sb0, sb1, sb2, sa1, sa2;  // shelf
  double ha1, ha2;                 // high-pass (b = [1, −2, 1])
  double M[kLdScan][16];
  double Mp[16];                   // from one pass to the next
  int h;                           // samples of 100 ms
};
struct LdState {
  double s1, s2, t1, t2;
};
// one sample through shelf and high-pass
__host__ __device__ inline double ld_step(LdState& s, double x, const LdFilter& f) {
  const double y1 = f.sb0 * x + s.s1;
  s.s1 = f.sb1 * x - f.sa1 * y1 + s.s2;
  s.s2 = f.sb2 * x - f.sa2 * y1;
  const double y = y1 + s.t1;
  s.t1 = -2.0 * y1 - f.ha1 * y + s.t2;
  s.t2 = y1 - f.ha2 * y;
  return y;
}
// PIPER_HIP_ERR_UNSUPPORTED for a rate outside the contract
int ld_filter(int rate, LdFilter* out);

// A target as the gate kernel takes it: checked, defaults resolved. on = 0: measure only, g = 1.
struct LdTarget {
  int on;
  double target, max_gain;
};
int ld_resolve(const piper_hip_loudness* ld, LdTarget* out);

// Passes of items of at most n_max samples, and the doubles of an item's row of the measurement's work buffer: per pass the end state
// from zero state [4], then per pass the true start state [4], then per pass its share of every segment it touches [kLdSegs].
inline int64_t ld_passes(int64_t n_max) { return std::max<int64_t>(1, ceil_div(n_max, kLdSuper)); }
inline int64_t ld_work_row(int64_t n_max) { return ld_passes(n_max) * (8 + kLdSegs); }

// Items [NB][row] → per pass Σ y² of the 100 ms segments it touches, work [NB][ld_work_row(n_max)], item b over its true length
// lensF[b]·hop (read from device memory, clamped to F), n_max = F·hop. lensF == nullptr: one item of n_flat = n_max contiguous samples (NB = 1).
hipError_t launch_loudness_measure(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                                   const LdFilter& f, double* work);
// work → rep [NB][2] = {L rounded to fp32, g}: segment powers from the passes' shares, both gates, then the gain of the target
hipError_t launch_loudness_gate(hipStream_t q, const int* lensF, int F, int hop, int NB, int64_t n_flat, int h, const double* work,
                                const LdTarget& t, float* rep);
// u = x·g_b over each item's true length, out [NB][out_row]
hipError_t launch_loudness_gain(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, const float* rep,
                                float* out, int64_t out_row);

}  // namespace ph
