// dp_scalars.h — the duration predictor's per-item scalars in device memory, one record per batch item: written by dp_scalars_fill
// (dp.hip), read by the predictor's kernels in dp.hip and prosody.hip.
#pragma once

namespace ph {

struct DpScalars {
  float noise_w, length_scale;
  unsigned gen, seed;  // gen ≠ 0: draw the `dp` RandomNormalLike tensor on the device
};

}  // namespace ph
