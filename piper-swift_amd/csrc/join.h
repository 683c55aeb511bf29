// join.h — the join of a batch into one programme on the device (join.hip); launched from voice.hip behind a plan's graph, never
// captured into it. The arithmetic is the contract of include/piper_hip.h "Join".
#pragma once
#include <cmath>

#include "common.h"

namespace ph {

constexpr int kJoinMaxItems = PIPER_HIP_JOIN_MAX_ITEMS;  // one item per thread of the plan kernel's block

// A join as the kernels take it: the S() counts at the rate of the samples and the gap behind every item. Built on the host
// (join_build), uploaded whole.
struct JoinParams {
  int64_t lead, tail, pad, fade;
  float threshold;
  int trim;
  int64_t gap[kJoinMaxItems];  // gap[i] behind item i (the one behind the last item is never read)
};
// piper_hip_join_check, then the counts at `rate`
int join_build(const piper_hip_join* join, const float* gaps, int n_gaps, int rate, JoinParams* out);
// S(ms) at `rate`
inline int64_t join_samples(float ms, int rate) { return (int64_t)std::floor((double)ms * (double)rate / 1000.0 + 0.5); }
// the no-trim bound on total for `n` items of `sum` samples together
inline int64_t join_bound(const JoinParams& p, int n, int64_t sum) {
  int64_t c = p.lead + p.tail + sum;
  for (int i = 0; i + 1 < n; i++) c += p.gap[i];
  return c;
}

// Where the items are: plan audio [NB][row] with the true lengths lensF[b]·hop read from device memory and clamped to F, or — lensF ==
// nullptr — item b at x[off[b] … + len[b]) with both tables in device memory.
struct JoinSrc {
  const float* x;
  int64_t row;
  const int* lensF;
  int F, hop;
  const int64_t* off;
  const int64_t* len;
};

// One item of the programme as the plan kernel leaves it for the write kernel: the kept samples x[src … + len) go to dst, behind
// `zb` zeros (the lead, item 0 only) and in front of `za` (the item's gap, or the tail); cut bit 0: the head was cut, bit 1: the tail.
struct JoinRow {
  int64_t src, dst, len, zb, za;
  int cut, pad_;
};

// ints of the report: total, then start[NB], then len[NB]
constexpr int kJoinReport = 1 + 2 * kJoinMaxItems;

// The three launches on q. p, edges [2·NB] ints, rows [NB], total (one int: the length the sinks read as lensF of one item at hop 1),
// report [kJoinReport] int64 in device memory; report_host (optional): the host mapping of a page-locked copy of the report.
// n_max bounds every item's length, z_max every silence; out holds join_bound() samples. NB in 1 … 256.
hipError_t launch_join(hipStream_t q, const JoinSrc& src, int NB, int64_t n_max, int64_t z_max, const JoinParams* p, bool trim, int* edges,
                       JoinRow* rows, int* total, int64_t* report, int64_t* report_host, float* out);

}  // namespace ph
