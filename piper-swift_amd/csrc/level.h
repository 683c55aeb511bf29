// level.h — look-ahead limiter on the device (level.hip); launched from voice.hip behind a plan's graph, never captured into it.
// The arithmetic is the contract of include/piper_hip.h "Level control".
#pragma once
#include "common.h"

namespace ph {

constexpr int kLvBlock = PIPER_HIP_LEVEL_BLOCK;      // B: samples per block
constexpr int kLvAhead = PIPER_HIP_LEVEL_LOOKAHEAD;  // W: blocks of look-ahead
constexpr int kLvCarry = 256;                        // floats of a stream row's carry: up to 255 samples u, then the last final G
static_assert(kLvBlock == 32 && kLvBlock * (kLvAhead + 2) - 1 == kLvCarry - 1, "a step keeps at most 32·(W + 2) − 1 = 255 samples back");

// A level as the kernels take it: checked, defaults resolved, rel for the rate of the samples being limited.
struct LvParams {
  float drive, ceiling, rel;
};
// piper_hip_level_check, then the resolved values (lv == nullptr or all zero: {1, 1, 50 ms})
int lv_resolve(const piper_hip_level* lv, int rate, LvParams* out);
// y is final on [0, lv_ready(e)) when samples [0, e) are known and more follow
inline int64_t lv_ready(int64_t e) { return std::max<int64_t>(0, (int64_t)kLvBlock * (e / kLvBlock - (kLvAhead + 1))); }
// limited samples one row can deliver in a step over n_in input samples
inline int64_t lv_step_bound(int64_t n_in) { return n_in + kLvCarry - 1; }
// floats of the scratch of launch_level_items for NB rows of at most n_max samples
size_t lv_scratch_floats(int NB, int64_t n_max);

// Items of plan audio [NB][row] → lim [NB][row], item b over its true length lensF[b]·hop (read from device memory, clamped to F).
// lensF == nullptr: one item of n_flat contiguous samples (NB = 1). scratch: lv_scratch_floats(NB, F·hop or n_flat) floats.
hipError_t launch_level_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                              const LvParams& p, float* scratch, float* lim, int64_t lim_row);

// One generator row of a limiting stream step (voice.hip fills it, level_step_kernel reads it): the chunk is the n_in samples behind the
// halo skip of the row's plan audio; carry_n samples before it are in the row's carry (0 on a row's first step, which starts from
// G[−1] = 1 and reads nothing of the carry); the step writes the limited samples [lo, lo + n_out) to the row of lim_step.
// n_in == 0: the row has nothing in this step.
struct LvStepRow {
  int skip, n_in, carry_n, n_out;
};
// Dynamic LDS of a step whose rows take up to max_in input samples; 0 when that exceeds what a block may hold
size_t lv_step_lds(int64_t max_in);
// One stream step: row r of audio [NBg][row] → row r of lim_step [NBg][lim_row], carry [NBg][kLvCarry] read and rewritten.
hipError_t launch_level_step(hipStream_t q, int NBg, int max_in, const float* audio, int64_t row, const LvStepRow* desc, float* carry,
                             const LvParams& p, float* lim_step, int64_t lim_row);

}  // namespace ph
