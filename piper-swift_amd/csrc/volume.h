// volume.h — per-phoneme volume: a gain envelope on the device (volume.hip); launched from voice.hip behind a plan's graph, never captured
// into it. The arithmetic is the contract of include/piper_hip.h "Per-phoneme volume".
#pragma once
#include "common.h"

namespace ph {

// piper_hip_volume_check with the item's index in the message (item < 0: none)
int volume_check_item(const piper_hip_volume* v, int item);

// Items of plan audio [NB][row] → shaped [NB][out_row], item b over its true length lensF[b]·hop (read from device memory, clamped to F).
// The gain of frame f of item b is gain[b·T + frame2id[b·f2i_row + f]] (an id outside [0, T) reads as its nearest end).
hipError_t launch_volume_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, const int32_t* frame2id,
                               int64_t f2i_row, const float* gain, int T, float* shaped, int64_t out_row);

// One item of `frames` frames whose gains are given per frame: x [frames·hop] → y [frames·hop]; the pointers need no alignment.
hipError_t launch_volume_flat(hipStream_t q, const float* x, const float* frame_gain, int64_t frames, int hop, float* y);

// gf [NB][F]: the gain of every frame of every item (0 past an item's true length) — the "vol.gain" tap
hipError_t launch_volume_frame_gains(hipStream_t q, const int* lensF, int F, int NB, const int32_t* frame2id, int64_t f2i_row, const float* gain, int T,
                                     float* gf);

// One generator row of a stream step (voice.hip fills it, volume_step_kernel reads it): the chunk is the n samples behind the halo skip of
// the row's window audio, sample n0 of an item of F frames whose gains per frame are gf (null: the row has no volume, its chunk is copied).
// n0, n and skip are multiples of hop. n == 0: the row has nothing in this step.
struct VolStepRow {
  const float* gf;
  int64_t n0;
  int F, skip, n, pad;
};
// One stream step: the chunk of row r of audio [rows][row] → the same place of out [rows][row]; max_n: the longest chunk.
hipError_t launch_volume_step(hipStream_t q, int rows, int64_t max_n, const float* audio, int64_t row, const VolStepRow* desc, int hop, float* out);

}  // namespace ph
