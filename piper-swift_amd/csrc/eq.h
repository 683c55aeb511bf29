// eq.h — the output equaliser on the device (eq.hip); launched from voice.hip behind a plan's graph, never captured into it.
// The arithmetic is the contract of include/piper_hip.h "Equaliser".
#pragma once
#include "common.h"

namespace ph {

constexpr int kEqBlock = PIPER_HIP_EQ_BLOCK;          // B: samples per block of the tree
constexpr int kEqMaxSec = PIPER_HIP_EQ_MAX_SECTIONS;  // sections of a cascade
constexpr int kEqMaxD = 2 * kEqMaxSec;                // doubles of the state; the stride of a row of P
constexpr int kEqWgBlocks = 128;                      // blocks per workgroup: one lane runs one block
constexpr int kEqWgLevels = 7;                        // tree levels built in LDS inside a workgroup: 2^7 = kEqWgBlocks
constexpr int kEqStride = kEqBlock + 1;               // floats per block in the LDS tile (padded: one bank per lane)
constexpr int kEqTopLanes = 256;                      // lanes of the workgroup that builds the levels above a workgroup
constexpr int kEqLevels = 34;                         // P_0 … P_33: items of up to 2^40 samples (2^34 blocks)
static_assert((1 << kEqWgLevels) == kEqWgBlocks, "the LDS tree ends in one aggregate per workgroup");

// A design as the kernels take it: the coefficients {b0, b1, b2, a1, a2} of n sections and P_l = A^(64·2^l) [D][D], row-major at
// stride kEqMaxD. Built on the host (eq_build), uploaded whole.
struct EqDesign {
  int n;
  double co[kEqMaxSec][5];
  double P[kEqLevels][kEqMaxD * kEqMaxD];
};
// piper_hip_eq_check, the design, the transition and its powers
int eq_build(const piper_hip_eq* eq, int rate, EqDesign* out);

// blocks of n samples
__host__ __device__ inline int64_t eq_blocks(int64_t n) { return n > 0 ? (n + kEqBlock - 1) / kEqBlock : 0; }
// Entries of tree level l for K blocks, and the doubles of an item's row of the work buffer for items of at most Kmax blocks
__host__ __device__ inline int64_t eq_level_count(int64_t K, int l) { return K > 0 ? ((K - 1) >> l) + 1 : 0; }
inline int64_t eq_work_row(int64_t n_max, int D) {
  const int64_t K = ceil_div(std::max<int64_t>(n_max, 1), kEqBlock);
  int64_t e = 0;
  for (int l = 0; l <= kEqLevels; l++) e += eq_level_count(K, l);
  return e * D;
}

// Items of plan audio [NB][row] → out [NB][out_row], item b over its true length lensF[b]·hop (read from device memory, clamped to F).
// lensF == nullptr: one item of n_flat contiguous samples (NB = 1). d: the design in device memory, n its sections; work:
// [NB][eq_work_row(n_max, 2n)] doubles.
hipError_t launch_eq_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                           const EqDesign* d, int n, double* work, float* out, int64_t out_row);

// One generator row of an EQ'd stream step (voice.hip fills it, eq_step_kernel reads it): the chunk is the n samples behind the skip of the
// row's window audio, and its first sample is sample s of the item (a multiple of 64: hop % 64 == 0). n == 0: the row has nothing.
struct EqStepRow {
  int64_t s;
  int skip, n;
};
// doubles of a row's carry: one aggregate per level, the levels of the set bits of the row's block count
constexpr int kEqCarry = (kEqLevels + 1) * kEqMaxD;
// One stream step: row r of audio [rows][row] → the same place of out [rows][row]; carry [rows][kEqCarry] read, then rewritten;
// scratch [rows][blocks][2·kEqMaxD], blocks = ceil(max_in / 64).
hipError_t launch_eq_step(hipStream_t q, int rows, int max_in, const float* audio, int64_t row, const EqStepRow* desc, const EqDesign* d, int n,
                          double* carry, double* scratch, float* out);

}  // namespace ph
