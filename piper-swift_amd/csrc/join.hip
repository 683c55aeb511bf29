// join.hip — the items of a batch → ONE programme on the device: trimmed, faded, with silences (include/piper_hip.h "Join").
//
// The arithmetic is a contract, tested bit for bit against the host twin piper_hip_join_from_f32 below and a numpy restatement
// (tests/join_ref.py): the compare fabsf(x) > threshold in fp32 (false for NaN), the ramp (float)((double)(k + 1) / (double)(Fd + 1)),
// one fp32 product per ramp (head first, then tail), every other kept sample moved bit for bit, +0.0f in the silences.
//
// Three launches, all memory-bound:
//   edges   (trim only) one pass over every item: per thread the first and the last index above the threshold, a wave reduction, and one
//           vector atomicMin / atomicMax per block on the item's two words — min and max of ints are order-independent, so the words hold
//           the same bits every run (pcm16_peak_kernel is the precedent). 16-byte loads where the item starts on a 16-byte line.
//   plan    one block, thread b = item b: edges → [s, t), a shuffle + LDS prefix sum over len + gap → where it goes (pcm16_pack_kernel's
//           idiom), the JoinRow table, the total and the report.
//   write   grid (tiles, NB): block row b owns the region [dst − zb, dst + len + za) of the programme — its lead, its kept samples, its
//           gap or the tail — and nothing else. The regions tile the programme, and their starts have any of the four 4-byte phases of a
//           16-byte line: whole 16-byte stores on the destination side between a scalar head and tail, the shifted source read with
//           dword loads that neighbouring lanes coalesce. No store touches a sample outside the block's own region.
#include "join.h"

#include <algorithm>
#include <climits>
#include <cmath>

#include "pcm16.h"

namespace ph {
namespace {

__device__ __forceinline__ void join_item(const JoinSrc& s, int b, int64_t* off, int64_t* n) {
  if (s.lensF) {
    *off = (int64_t)b * s.row;
    *n = (int64_t)clamp_len(s.lensF[b], s.F) * s.hop;
  } else {
    *off = s.off[b];
    *n = s.len[b];
  }
}

__global__ __launch_bounds__(256) void join_edges_kernel(const JoinSrc s, const JoinParams* __restrict__ p, int* __restrict__ edges) {
  __shared__ int lo[4], hi[4];
  const int b = blockIdx.y, NB = gridDim.y, tid = threadIdx.x;
  int64_t off, n;
  join_item(s, b, &off, &n);
  const float* __restrict__ x = s.x + off;
  const float thr = p->threshold;
  const int64_t gt = (int64_t)blockIdx.x * 256 + tid, nth = (int64_t)gridDim.x * 256;
  int first = INT_MAX, last = -1;
  const auto mark = [&](float v, int64_t i) {
    if (fabsf(v) > thr) {  // (false for NaN)
      first = min(first, (int)i);
      last = max(last, (int)i);
    }
  };
  int64_t done = 0;
  if (((uintptr_t)x & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = gt; i < n4; i += nth) {
      const float4 a = ((const float4*)x)[i];
      mark(a.x, 4 * i); mark(a.y, 4 * i + 1); mark(a.z, 4 * i + 2); mark(a.w, 4 * i + 3);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + gt; i < n; i += nth) mark(x[i], i);
  for (int o = 32; o > 0; o >>= 1) {
    first = min(first, __shfl_down(first, o));
    last = max(last, __shfl_down(last, o));
  }
  if ((tid & 63) == 0) { lo[tid >> 6] = first; hi[tid >> 6] = last; }
  __syncthreads();
  if (tid == 0) {
    first = min(min(lo[0], lo[1]), min(lo[2], lo[3]));
    last = max(max(hi[0], hi[1]), max(hi[2], hi[3]));
    if (last >= 0) {  // (a block that met no loud sample has nothing to add)
      atomicMin(edges + b, first);
      atomicMax(edges + NB + b, last);
    }
  }
}

__global__ __launch_bounds__(256) void join_plan_kernel(const JoinSrc s, int NB, const JoinParams* __restrict__ p, const int* __restrict__ edges,
                                                        JoinRow* __restrict__ rows, int* __restrict__ total, int64_t* __restrict__ report,
                                                        int64_t* __restrict__ report_host) {
  __shared__ long long wave_sum[4];
  const int b = threadIdx.x, lane = b & 63, w = b >> 6;
  int64_t off = 0, n = 0, s0 = 0, t0 = 0, za = 0;
  if (b < NB) {
    join_item(s, b, &off, &n);
    n = max(n, (int64_t)0);
    t0 = n;
    if (p->trim) {
      const int a = edges[b], e = edges[NB + b];
      if (e < 0) {
        s0 = t0 = 0;
      } else {
        s0 = max((int64_t)0, (int64_t)a - p->pad);
        t0 = min(n, (int64_t)e + 1 + p->pad);
      }
    }
    za = b < NB - 1 ? p->gap[b] : p->tail;
  }
  const long long mine = (t0 - s0) + za;
  long long inc = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wave_sum[w] = inc;
  __syncthreads();
  long long before = p->lead;
  for (int i = 0; i < w; i++) before += wave_sum[i];
  const int64_t dst = before + inc - mine;
  if (b < NB) {
    JoinRow r;
    r.src = off + s0; r.dst = dst; r.len = t0 - s0; r.zb = b == 0 ? p->lead : 0; r.za = za;
    r.cut = (s0 > 0 ? 1 : 0) | (t0 < n ? 2 : 0);
    r.pad_ = 0;
    rows[b] = r;
    report[1 + b] = dst;
    report[1 + NB + b] = t0 - s0;
    if (report_host) { report_host[1 + b] = dst; report_host[1 + NB + b] = t0 - s0; }
  }
  if (b == 0) {
    const long long tot = p->lead + wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    *total = (int)tot;
    report[0] = tot;
    if (report_host) report_host[0] = tot;
  }
}

__global__ __launch_bounds__(256) void join_write_kernel(const float* __restrict__ x, const JoinRow* __restrict__ rows,
                                                         const JoinParams* __restrict__ p, float* __restrict__ out) {
  const JoinRow r = rows[blockIdx.y];
  const int64_t Fd = p->fade;
  const int64_t fe = min(Fd, r.len);  // samples under the ramp of a cut edge
  const int64_t hn = (r.cut & 1) ? fe : 0, tn = (r.cut & 2) ? fe : 0;
  const double den = (double)(Fd + 1);
  const float* __restrict__ src = x + r.src;
  float* __restrict__ dst = out + (r.dst - r.zb);
  const int64_t R = r.zb + r.len + r.za;  // the block row's own region
  const auto val = [&](int64_t j) -> float {
    const int64_t k = j - r.zb;
    if (k < 0 || k >= r.len) return 0.0f;
    float v = src[k];
    if (k < hn) v = v * (float)((double)(k + 1) / den);
    const int64_t kt = r.len - 1 - k;
    if (kt < tn) v = v * (float)((double)(kt + 1) / den);
    return v;
  };
  const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t head = min(R, (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2));  // scalar stores up to the first 16-byte line
  for (int64_t i = gt; i < head; i += nth) dst[i] = val(i);
  const int64_t n4 = (R - head) >> 2;
  float4* __restrict__ d4 = (float4*)(dst + head);
  const int64_t plain0 = r.zb + hn, plain1 = r.zb + r.len - tn;  // [plain0, plain1): kept samples under no ramp
  for (int64_t i = gt; i < n4; i += nth) {
    const int64_t j = head + 4 * i;
    float4 o;
    if (j >= plain0 && j + 4 <= plain1) {
      const float* q = src + (j - r.zb);
      o.x = q[0]; o.y = q[1]; o.z = q[2]; o.w = q[3];
    } else {
      o.x = val(j); o.y = val(j + 1); o.z = val(j + 2); o.w = val(j + 3);
    }
    d4[i] = o;
  }
  for (int64_t i = head + (n4 << 2) + gt; i < R; i += nth) dst[i] = val(i);
}

// blocks along an item: 4 samples per thread and pass, at most 1024 blocks (pcm16.hip's bound)
int join_blocks(int64_t samples) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(samples, (int64_t)256 * 4), 1), 1024); }

bool ms_ok(float ms, float hi) { return std::isfinite(ms) && ms >= 0.0f && ms <= hi; }

}  // namespace

int join_build(const piper_hip_join* join, const float* gaps, int n_gaps, int rate, JoinParams* out) {
  if (int rc = piper_hip_join_check(join, gaps, n_gaps)) return rc;
  if (rate < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "join: rate %d", rate);
  out->lead = join_samples(join->lead_ms, rate);
  out->tail = join_samples(join->tail_ms, rate);
  out->pad = join_samples(join->trim_pad_ms, rate);
  out->fade = join_samples(join->fade_ms, rate);
  out->threshold = join->trim_threshold;
  out->trim = join->trim;
  const int64_t g = join_samples(join->gap_ms, rate);
  for (int i = 0; i < kJoinMaxItems; i++) out->gap[i] = i < n_gaps ? join_samples(gaps[i], rate) : g;
  return PIPER_HIP_OK;
}

hipError_t launch_join(hipStream_t q, const JoinSrc& src, int NB, int64_t n_max, int64_t z_max, const JoinParams* p, bool trim, int* edges,
                       JoinRow* rows, int* total, int64_t* report, int64_t* report_host, float* out) {
  if (NB < 1 || NB > kJoinMaxItems) return hipErrorInvalidValue;  // one item per thread of the plan kernel's block
  if (trim) {
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)edges, INT_MAX, (size_t)NB, q);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(edges + NB), -1, (size_t)NB, q);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(join_edges_kernel, dim3(join_blocks(n_max), NB), dim3(256), 0, q, src, p, edges);
  }
  hipLaunchKernelGGL(join_plan_kernel, dim3(1), dim3(256), 0, q, src, NB, p, edges, rows, total, report, report_host);
  hipLaunchKernelGGL(join_write_kernel, dim3(join_blocks(n_max + z_max), NB), dim3(256), 0, q, src.x, rows, p, out);
  return hipGetLastError();
}

namespace { PH_WARM(join, join_write_kernel); }

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_join_check(const piper_hip_join* join, const float* gaps, int n) {
  if (!join) PH_FAIL(PIPER_HIP_ERR_ARG, "join: null join");
  if (!ms_ok(join->lead_ms, 10000.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: lead_ms %g outside [0, 10000]", (double)join->lead_ms);
  if (!ms_ok(join->gap_ms, 10000.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: gap_ms %g outside [0, 10000]", (double)join->gap_ms);
  if (!ms_ok(join->tail_ms, 10000.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: tail_ms %g outside [0, 10000]", (double)join->tail_ms);
  if (join->trim != 0 && join->trim != 1) PH_FAIL(PIPER_HIP_ERR_ARG, "join: trim %d is neither 0 nor 1", (int)join->trim);
  if (!(std::isfinite(join->trim_threshold) && join->trim_threshold >= 0.0f))
    PH_FAIL(PIPER_HIP_ERR_ARG, "join: trim_threshold %g is negative or not finite", (double)join->trim_threshold);
  if (!ms_ok(join->trim_pad_ms, 1000.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: trim_pad_ms %g outside [0, 1000]", (double)join->trim_pad_ms);
  if (!ms_ok(join->fade_ms, 100.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: fade_ms %g outside [0, 100]", (double)join->fade_ms);
  if (n < 0 || n > kJoinMaxItems) PH_FAIL(PIPER_HIP_ERR_ARG, "join: %d gaps outside 0 … %d", n, kJoinMaxItems);
  if (n > 0 && !gaps) PH_FAIL(PIPER_HIP_ERR_ARG, "join: null gaps");
  for (int i = 0; i < n; i++)
    if (!ms_ok(gaps[i], 10000.0f)) PH_FAIL(PIPER_HIP_ERR_ARG, "join: gaps[%d] %g outside [0, 10000]", i, (double)gaps[i]);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_join_counts(const piper_hip_join* join, int32_t rate, int64_t* lead, int64_t* gap, int64_t* tail, int64_t* pad,
                                    int64_t* fade) {
  JoinParams p;
  if (int rc = join_build(join, nullptr, 0, rate, &p)) return rc;
  if (lead) *lead = p.lead;
  if (gap) *gap = p.gap[0];
  if (tail) *tail = p.tail;
  if (pad) *pad = p.pad;
  if (fade) *fade = p.fade;
  return PIPER_HIP_OK;
}

namespace {
int join_items_check(const char* who, const int64_t* item_len, int n_items, int64_t* sum) {
  if (n_items < 1 || n_items > kJoinMaxItems) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: %d items outside 1 … %d", who, n_items, kJoinMaxItems);
  if (!item_len) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: null item lengths", who);
  *sum = 0;
  for (int i = 0; i < n_items; i++) {
    if (item_len[i] < 0 || item_len[i] > INT_MAX) PH_FAIL(PIPER_HIP_ERR_SHAPE, "%s: item %d has %lld samples", who, i, (long long)item_len[i]);
    *sum += item_len[i];
  }
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_join_capacity(const piper_hip_join* join, const float* gaps, int n_gaps, int32_t rate, const int64_t* item_samples,
                                      int n_items, int64_t* samples) {
  JoinParams p;
  if (int rc = join_build(join, gaps, n_gaps, rate, &p)) return rc;
  int64_t sum;
  if (int rc = join_items_check("join_capacity", item_samples, n_items, &sum)) return rc;
  if (!samples) PH_FAIL(PIPER_HIP_ERR_ARG, "join_capacity: null output");
  *samples = join_bound(p, n_items, sum);
  return PIPER_HIP_OK;
}

// the host twin of the kernels
PH_EXPORT int piper_hip_join_from_f32(const piper_hip_join* join, const float* gaps, int n_gaps, int32_t rate, const float* x,
                                      const int64_t* item_off, const int64_t* item_len, int n_items, float* y, int64_t max, int64_t* start,
                                      int64_t* len, int64_t* total) {
  JoinParams p;
  if (int rc = join_build(join, gaps, n_gaps, rate, &p)) return rc;
  int64_t sum;
  if (int rc = join_items_check("join_from_f32", item_len, n_items, &sum)) return rc;
  if (!item_off || (!x && sum) || !total) PH_FAIL(PIPER_HIP_ERR_ARG, "join_from_f32: null argument");
  // the kept ranges first: nothing is written into a buffer that turns out too short
  std::vector<int64_t> s0(n_items), t0(n_items);
  int64_t tot = p.lead + p.tail;
  for (int i = 0; i < n_items; i++) {
    const float* xi = x + item_off[i];
    const int64_t n = item_len[i];
    s0[i] = 0; t0[i] = n;
    if (p.trim) {
      int64_t a = -1, e = -1;
      for (int64_t k = 0; k < n; k++)
        if (std::fabs(xi[k]) > p.threshold) { if (a < 0) a = k; e = k; }
      if (e < 0) s0[i] = t0[i] = 0;
      else { s0[i] = std::max<int64_t>(0, a - p.pad); t0[i] = std::min(n, e + 1 + p.pad); }
    }
    tot += t0[i] - s0[i] + (i + 1 < n_items ? p.gap[i] : 0);
  }
  if (max < tot) PH_FAIL(PIPER_HIP_ERR_SHAPE, "join_from_f32: buffer holds %lld < %lld samples", (long long)max, (long long)tot);
  if (!y && tot) PH_FAIL(PIPER_HIP_ERR_ARG, "join_from_f32: null output");
  int64_t at = 0;
  for (int64_t k = 0; k < p.lead; k++) y[at++] = 0.0f;
  const double den = (double)(p.fade + 1);
  for (int i = 0; i < n_items; i++) {
    const float* xi = x + item_off[i];
    const int64_t n = item_len[i], L = t0[i] - s0[i], fe = std::min(p.fade, L);
    if (start) start[i] = at;
    if (len) len[i] = L;
    float* yi = y + at;
    if (L) memcpy(yi, xi + s0[i], (size_t)L * sizeof(float));
    if (s0[i] > 0)
      for (int64_t k = 0; k < fe; k++) yi[k] = yi[k] * (float)((double)(k + 1) / den);
    if (t0[i] < n)
      for (int64_t k = 0; k < fe; k++) yi[L - 1 - k] = yi[L - 1 - k] * (float)((double)(k + 1) / den);
    at += L;
    const int64_t z = i + 1 < n_items ? p.gap[i] : p.tail;
    for (int64_t k = 0; k < z; k++) y[at++] = 0.0f;
  }
  *total = tot;
  return PIPER_HIP_OK;
}

// ---- per-op

PH_EXPORT int piper_hip_join_f32(piper_hip_ctx* ctx, const float* x, const int64_t* item_off, const int64_t* item_len, int n_items, int32_t rate,
                                 const piper_hip_join* join, const float* gaps, int n_gaps, float** out, int64_t* start_host, int64_t* len_host,
                                 int64_t* total_host, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "join_f32: null output pointer");
  if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "join_f32: the output buffer is not 4-byte aligned");
  if (((uintptr_t)x & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "join_f32: the input buffer is not 4-byte aligned");
  std::vector<JoinParams> hold(1);
  JoinParams& p = hold[0];
  int rc = join_build(join, gaps, n_gaps, rate, &p);
  if (rc) return rc;
  int64_t sum;
  if ((rc = join_items_check("join_f32", item_len, n_items, &sum))) return rc;
  if (!item_off || (!x && sum) || !total_host) PH_FAIL(PIPER_HIP_ERR_ARG, "join_f32: null argument");
  for (int i = 0; i < n_items; i++)
    if (item_off[i] < 0) PH_FAIL(PIPER_HIP_ERR_ARG, "join_f32: item_off[%d] is negative", i);
  const int64_t cap = join_bound(p, n_items, sum);
  if (cap > INT_MAX) PH_FAIL(PIPER_HIP_ERR_SHAPE, "join_f32: a programme of up to %lld samples does not fit an int", (long long)cap);
  if (!*out) {
    void* q = nullptr;
    if ((rc = ctx->pool.alloc((size_t)std::max<int64_t>(cap, 1) * sizeof(float), &q))) return rc;
    *out = (float*)q;
  }
  // one device block for everything the launches read and leave: params | off, len | report | rows | edges, total
  const size_t o_tab = sizeof(JoinParams), o_rep = o_tab + 2 * (size_t)n_items * sizeof(int64_t);
  const size_t o_rows = o_rep + (size_t)kJoinReport * sizeof(int64_t), o_edges = o_rows + (size_t)n_items * sizeof(JoinRow);
  const size_t bytes = o_edges + (2 * (size_t)n_items + 1) * sizeof(int);
  void* blk = nullptr;
  if ((rc = ctx->pool.alloc(bytes, &blk))) return rc;
  char* d = (char*)blk;
  std::vector<int64_t> tab(2 * (size_t)n_items), rep(1 + 2 * (size_t)n_items);
  int64_t n_max = 0, z_gap = p.tail;
  for (int i = 0; i < n_items; i++) {
    tab[i] = item_off[i];
    tab[n_items + i] = item_len[i];
    n_max = std::max(n_max, item_len[i]);
    if (i + 1 < n_items) z_gap = std::max(z_gap, p.gap[i]);
  }
  StreamScope ss(ctx, stream);
  hipError_t e = hipMemcpyAsync(d, &p, sizeof(JoinParams), hipMemcpyHostToDevice, ss.s);
  if (e == hipSuccess) e = hipMemcpyAsync(d + o_tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, ss.s);
  JoinSrc src{x, 0, nullptr, 0, 1, (const int64_t*)(d + o_tab), (const int64_t*)(d + o_tab) + n_items};
  int* edges = (int*)(d + o_edges);
  if (e == hipSuccess)
    e = launch_join(ss.s, src, n_items, n_max, p.lead + z_gap, (const JoinParams*)d, p.trim != 0, edges,
                    (JoinRow*)(d + o_rows), edges + 2 * n_items, (int64_t*)(d + o_rep), nullptr, *out);
  if (e == hipSuccess) e = hipMemcpyAsync(rep.data(), d + o_rep, rep.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ss.s);
  // the report is the call's answer: it waits whatever `stream` is (and the host tables above outlive the copies that read them)
  const hipError_t w = hipStreamSynchronize(ss.s);
  (void)ctx->pool.release(blk);
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "join_f32: %s", hipGetErrorString(e));
  *total_host = rep[0];
  for (int i = 0; i < n_items; i++) {
    if (start_host) start_host[i] = rep[1 + i];
    if (len_host) len_host[i] = rep[1 + n_items + i];
  }
  return ss.finish("join_f32");
}
