// resample.h — rational sample-rate conversion fused into the 16-bit PCM conversion (resample.hip); launched from voice.hip behind a
// plan's graph, never captured into it. The arithmetic is the contract of include/piper_hip.h "Output rate".
#pragma once
#include "common.h"

namespace ph {

// The filter of one (in, out) pair, designed in double on the host once per process (rs_design) and kept for its life.
struct RsDesign {
  int in = 0, out = 0, L = 0, M = 0, P = 0;  // out / gcd, in / gcd, taps per phase
  std::vector<float> taps;                   // [L][P]
};
// PIPER_HIP_ERR_UNSUPPORTED for a pair outside the contract (output rate not in the list, L > 640 or P > 256), PIPER_HIP_ERR_ARG for a rate ≤ 0.
int rs_design(int in_rate, int out_rate, const RsDesign** out);
inline int64_t rs_count(const RsDesign& d, int64_t n_in) { return ceil_div(n_in * d.L, d.M); }  // J(n_in)
// the first output a stream step may NOT emit yet when the item's samples [0, e) are known and more follow: ⌈(e − P/2)·L / M⌉, at least 0
inline int64_t rs_ready(const RsDesign& d, int64_t e) { return e <= d.P / 2 ? 0 : ceil_div((e - d.P / 2) * d.L, d.M); }
// outputs one row can deliver in a step over n_in input samples
inline int64_t rs_step_bound(const RsDesign& d, int64_t n_in) { return ceil_div(n_in * d.L, d.M) + ceil_div((int64_t)(d.P / 2) * d.L, d.M) + 1; }

// The filter as the kernels take it: the [L][P] table in device memory.
struct RsFilter {
  const float* taps;
  int L, M, P;
};

// Samples of a stream row the next step reads before its chunk: the last kRsHist true samples of the previous chunk (P − 1 ≤ 255 are needed).
constexpr int kRsHist = 256;

// One generator row of a resampling stream step (voice.hip fills it, resample_step_kernel reads it): the chunk is the n_in samples behind
// the halo skip of the row's plan audio, input samples [s, s + n_in) of the item; the step emits outputs [j0, j0 + count) at `off` samples
// into the packed output. n_in == 0: the row has nothing in this step.
struct RsStepRow {
  int64_t s, j0;
  int skip, n_in, count, off;
};

// One generator row of a mixed-format stream step (include/piper_hip.h "Mixed formats"; voice.hip fills it, mixed_step_kernel reads it):
// RsStepRow with a BYTE offset into the packed output (a multiple of 4), plus the row's own format — its filter (L == 0: the voice's own
// rate, not a filter: the chunk goes through the chunk-pack body and no history is read or written), the bytes of an output (4 fp32,
// 2 int16, 1 G.711 by `law`), the gain, and the tile of rs_geometry for that filter (mix_step_plan fills it). n_in == 0: nothing in this step.
struct MixStepRow {
  int64_t s, j0, off;
  const float* taps;
  int skip, n_in, count;
  int L, M, P;
  int elem, law;
  float gain;
  int tile;
};

// Items of plan audio [NB][row] → back to back at J(lensF[b]·hop) samples each (lengths read from device memory and clamped to F), item b
// at Σ_{i<b} J(·). elem = bytes of a sample of `out`: 4 the fp32 y; 2 int16 through the PCM contract — gain, and peak normalisation per
// item when peaks != nullptr, as launch_pcm16_pack; 1 the G.711 byte of that int16 by `law` (PIPER_HIP_G711_*), `out` at any byte address.
// lensF == nullptr: one item of n_flat contiguous samples (NB = 1). NB ≤ 256.
hipError_t launch_resample_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                                 const RsFilter& f, float gain, const float* peaks, float* peaks_host, void* out, int elem, int law);
// One stream step: every row's outputs packed at the descriptor's offsets as int16 (law 0) or G.711 bytes; hist_old / hist_new are
// [NBg][kRsHist] (read / written).
hipError_t launch_resample_step(hipStream_t q, int NBg, int max_count, const float* audio, int64_t row, const RsStepRow* desc,
                                const float* hist_old, float* hist_new, const RsFilter& f, float gain, void* out, int law);
// One mixed-format stream step. mix_step_plan sets `tile` of every row of the host table that delivers through a filter and returns the
// launch's geometry: grid.x covers the row that needs the most tiles (pack_blocks: what the rows at the voice's rate want), the dynamic
// LDS is the largest any delivering row's filter needs. launch_mixed_step then takes the uploaded table; one launch whatever the formats.
void mix_step_plan(MixStepRow* rows, int NBg, int pack_blocks, int* grid_x, size_t* lds_bytes);
hipError_t launch_mixed_step(hipStream_t q, int NBg, int grid_x, size_t lds_bytes, const float* audio, int64_t row, const MixStepRow* desc,
                             const float* hist_old, float* hist_new, void* out);

}  // namespace ph
