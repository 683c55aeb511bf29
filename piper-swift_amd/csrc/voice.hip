// voice.hip — whole-utterance VITS forward pass as a static schedule of fused launches, replayed as a HIP graph.
//
// Stands where PiperMetalRuntime.synthesize → GraphExecutor.executeOutput stands in the reference
// (PiperMetalRuntime.swift:62-80, GraphExecutor.swift:156-327), but instead of interpreting 2 755 ONNX nodes with a
// fresh buffer, a string-keyed table lookup and (in the unbatched mode) a blocking commit per node, the voice is
// compiled once into 80 launches (medium voice) over a preplanned arena:
//   encoder layer = qkv conv · rel-attention · o conv · add+LayerNorm · ffn1(+ReLU) · ffn2 · add+LayerNorm
//   flow coupling = pre conv (Flip/Split folded into channel maps) · 4×[in conv + tanh·sigmoid gate, res/skip conv
//                   writing x and skip in place] · post conv with x1 ← x1 − m in place (Concat folded)
//   generator     = conv_pre · per stage [LeakyReLU(+MRF mean)→ConvTranspose, 3 ResBlocks with LeakyReLU and residual
//                   fused into each conv] · LeakyReLU+MRF mean→conv_post→tanh
// Weights stay resident (packed once into MFMA fragment order); nothing is decoded or uploaded per call
// (the reference re-decodes 401 initializers and re-uploads every Conv weight per synthesize: GraphExecutor.swift:187-189,
// 1774-1780).  Utterances are independent, so a voice has several slots (stream + arena + graph) that overlap on the GPU.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <climits>
#include <functional>
#include <memory>

#include "../../include/piper_hip_voice_layout.h"
#include "conv.h"
#include "conv_bf16.h"
#include "conv_win.h"
#include "eq.h"
#include "join.h"
#include "pitch.h"
#include "level.h"
#include "loudness.h"
#include "volume.h"
#include "pcm16.h"
#include "resample.h"
#include "rng.h"
#include "speaker.h"

namespace ph {
int validate_config(const piper_hip_voice_config* c);
int validate_speaker_config(const piper_hip_voice_config* cfg, const piper_hip_speaker_config* sc);
int launch_rel_attention(piper_hip_ctx* ctx, hipStream_t s, const float* q, const float* k, const float* v, const float* ek,
                         const float* ev, float* out, int N, int H, int d, int T, int w, int64_t in_batch_stride,
                         int64_t out_batch_stride, const int* len_ptr);
int rel_attention_split_parts(piper_hip_ctx* ctx, int N, int H, int d, int T, int w);
int launch_rel_attention_split(piper_hip_ctx* ctx, hipStream_t s, const float* q, const float* k, const float* v, const float* ek,
                               const float* ev, float* out, int N, int H, int d, int T, int w, int64_t in_batch_stride,
                               int64_t out_batch_stride, const int* len_ptr, int nsplit, float* part_o, float* part_ml);
size_t dp_scalars_bytes(int n);
void dp_scalars_fill(void* host, int i, float noise_w, float length_scale, unsigned gen, unsigned seed);
bool flow_seam_eligible(int H, int half);
int launch_flow_seam(piper_hip_ctx* ctx, hipStream_t s, const float* skip, float* zp, float* h, const float* post16, const float* post_b, const float* pre16,
                     const float* pre_b, int N, int H, int half, int F, int post_steps, int pre_steps, int ob, int os, const int* len_ptr);
bool dds_layer_eligible(int H, int K);
int launch_dds_layer(piper_hip_ctx* ctx, hipStream_t s, const float* x, const float* dw_w, const float* dw_b, const float* g1, const float* b1,
                     const float* pw16, const float* pw_b, const float* g2, const float* b2, float* out, int N, int H, int T, int K, int dil,
                     int pw_steps, const int* len_ptr, float eps);
int launch_dp_init(hipStream_t s, const float* noise, const void* scalars, float* z, int N, int T, const int* len_ptr);
int launch_dp_spline(hipStream_t s, const float* h, float* z, int N, int T, int bins, float tail_bound, float filter_channels, const int* len_ptr);
int launch_dp_final(hipStream_t s, const float* z, const float* m, const float* logs, const void* scalars, float* logw, int32_t* dur, int N, int T,
                    const int* len_ptr);
// prosody.hip: the checks of one prosody record, and the three kernels a plan of a request with prosody runs in the place of dp_final_kernel,
// dp_paths_kernel and expand_noise_kernel
int prosody_check_item(const piper_hip_prosody* p, int item);
size_t prosody_report_entries(int n, int T);
int launch_dp_final_prosody(hipStream_t s, const float* z, const float* m, const float* logs, const void* scalars, const float* len, const int32_t* minf,
                            const int32_t* maxf, float* logw, float* w0, int32_t* dur, int N, int T, const int* len_ptr);
int launch_dp_paths_prosody(hipStream_t s, const int32_t* dur, const int* lensT, const int32_t* fit, int T, int F, int cap, int32_t* frame2id, int* lensF,
                            int32_t* rep, int n);
int launch_expand_noise_prosody(hipStream_t s, const float* stats, const int32_t* frame2id, const float* noise, const float* id_noise, float* zp,
                                float* zp_tap, int NB, int I, int T, int F, const float* noise_scale, const unsigned* rng, const int* lensF);
bool attention_block_eligible(int H, int d, int w, int T);
bool attention_block_wanted();
int launch_attention_block(piper_hip_ctx* ctx, hipStream_t s, const float* q, const float* k, const float* v, const float* ek, const float* ev,
                           const float* wo16, const float* bo, const float* xres, const float* gamma, const float* beta, float* out, int N,
                           int H, int d, int T, int w, int64_t in_batch_stride, int64_t x_batch_stride, const int* len_ptr, int o_nsteps,
                           float eps);
}  // namespace ph

using namespace ph;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxSlots = 16;

// x[c][t] = emb[ids[t]][c] * sqrt(H): Gather + Mul + Transpose of the graph head (GraphExecutor.swift:653-666)
__global__ __launch_bounds__(kBlock) void embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb,
                                                       float* __restrict__ x, int H, int T, int n_vocab, float scale) {
  ids += (int64_t)blockIdx.y * T;  // batch item
  x += (int64_t)blockIdx.y * H * T;
  const int total = H * T;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
    const int c = i / T, t = i - c * T;
    int64_t id = ids[t];
    if (id < 0) id += n_vocab;  // gather_axis0_f32_2d (gather.metal:54-57): negative ids wrap once, …
    x[i] = (id < 0 || id >= n_vocab) ? 0.0f * scale : emb[id * H + c] * scale;  // … what is still out of range gathers 0.0
  }
}

// z_p[c][f] = m_p[c][t(f)] + (noise[c][f] * exp(logs_p[c][t(f)])) * noise_scale.
// m_p/logs_p expansion by the one-hot path matrix (MatMul [1,F,T]×[1,T,I], GraphExecutor.swift:1862-1915) is a row
// gather: frame f copies phoneme t(f); bit-identical to the matmul (every other product is an exact ±0 add).
__global__ __launch_bounds__(kBlock) void expand_noise_kernel(const float* __restrict__ stats, const int32_t* __restrict__ frame2id,
                                                              const float* __restrict__ noise, float* __restrict__ zp, float* __restrict__ zp_tap,
                                                              int I, int T, int F, const float* __restrict__ noise_scale_dev,
                                                              const unsigned* __restrict__ rng_dev, const int* __restrict__ lensF) {
  const int nb = blockIdx.y;  // batch item
  stats += (int64_t)nb * 2 * I * T;
  frame2id += (int64_t)nb * F;
  noise += (int64_t)nb * I * F;
  zp += (int64_t)nb * I * F;
  zp_tap += (int64_t)nb * I * F;
  const float noise_scale = noise_scale_dev[nb];  // per-utterance scalar lives in device memory so a replayed graph sees it
  // RandomNormalLike on the device (random_normal_like_f32, elementwise.metal:139-163): element index = flat index of the
  // item's [1, I, F] tensor; rng_dev[2nb] = generate?, rng_dev[2nb+1] = seed. Otherwise the injected tensor is read.
  const bool gen = rng_dev[2 * nb] != 0u;
  const unsigned seed = rng_dev[2 * nb + 1];
  const int Fv = lensF ? min(lensF[nb], F) : F;  // RandomNormalLike mirrors the item's TRUE [1, I, Fv] shape, not the bucket
  const int64_t total = (int64_t)I * F;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int c = (int)(i / F), f = (int)(i - (int64_t)c * F);
    const int t = frame2id[f];
    const float m = stats[(int64_t)c * T + t];
    const float lg = stats[(int64_t)(I + c) * T + t];
    const float nz = gen ? (f < Fv ? rnl_normal(seed, (unsigned)(c * Fv + f)) : 0.0f) : noise[i];
    const float r = m + (nz * expf(lg)) * noise_scale;
    zp[i] = r;      // updated in place by the flow couplings
    zp_tap[i] = r;  // pristine copy for the "z_p" debug tap
  }
}

// HiFi-GAN multi-receptive-field mean + the LeakyReLU that follows it: y = lrelu(((a + b) + c) / 3, alpha).
// Done once per element here instead of inside the consumer conv, which re-reads every input element
// (row tiles × taps) times — the in-conv form paid 3 loads and one IEEE division per re-read.
__global__ __launch_bounds__(kBlock) void mrf_mean_lrelu_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const float* __restrict__ c, float* __restrict__ y, int64_t n,
                                                                float alpha) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i],
                 vc = reinterpret_cast<const float4*>(c)[i];
    float4 r;
    r.x = ((va.x + vb.x) + vc.x) / 3.0f; r.y = ((va.y + vb.y) + vc.y) / 3.0f;
    r.z = ((va.z + vb.z) + vc.z) / 3.0f; r.w = ((va.w + vb.w) + vc.w) / 3.0f;
    r.x = r.x >= 0.0f ? r.x : alpha * r.x; r.y = r.y >= 0.0f ? r.y : alpha * r.y;
    r.z = r.z >= 0.0f ? r.z : alpha * r.z; r.w = r.w >= 0.0f ? r.w : alpha * r.w;
    reinterpret_cast<float4*>(y)[i] = r;
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const float v = ((a[i] + b[i]) + c[i]) / 3.0f;
    y[i] = v >= 0.0f ? v : alpha * v;
  }
}

__global__ __launch_bounds__(kBlock) void flip_channels_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int L) {
  x += (int64_t)blockIdx.y * C * L;  // batch item
  y += (int64_t)blockIdx.y * C * L;
  const int64_t total = (int64_t)C * L;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int c = (int)(i / L), l = (int)(i - (int64_t)c * L);
    y[i] = x[(int64_t)(C - 1 - c) * L + l];
  }
}

// keeps the GPU busy for `ticks` of the 100 MHz realtime counter: lets the host queue a whole profiled pass ahead of the
// GPU, so the per-launch event deltas contain the ~1.7 µs kernel boundary but not host launch latency
__global__ void empty_kernel() {}
// lensT / lensF of a fresh plan = the bucket's own lengths (a kernel, not a copy from a host vector: see stream_wait below — nothing on the
// request path hands PAGEABLE host memory to an asynchronous copy)
__global__ void fill_lens_kernel(int* __restrict__ lensT, int* __restrict__ lensF, int T, int F, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { lensT[i] = T; lensF[i] = F; }
}

__global__ void spin_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// Wait for a stream on the request path. hipStreamSynchronize parks the thread on an interrupt; on the GPU boxes of this pool a wake-up is
// now and then 25 … 35 ms late (r3, tools/probe/request_max.py: the same ~26 ms in whichever synchronisation of a request it hits — arena
// initialisation, prepare, collect — on requests whose GPU work is 1 ms). A request is short: poll the stream for up to 5 ms, then park.
hipError_t stream_wait(hipStream_t q) {
  static const bool park = getenv("PIPER_HIP_NO_SPIN_WAIT") != nullptr;
  if (!park) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(q);
      if (e != hipErrorNotReady) return e;
      (void)hipGetLastError();  // "not ready" must not show up as the sticky error of a later launch check
      if (clk::now() - t0 > std::chrono::milliseconds(5)) break;
      for (int i = 0; i < 16; i++) __builtin_ia32_pause();
    }
  }
  return hipStreamSynchronize(q);
}

struct Step {
  std::string name;
  std::function<int(hipStream_t)> run;
  double flops = 0, bytes = 0;
  std::string tag;  // kernel family ("conv_mfma", "conv_small", "rel_attention", …) for piper_hip_voice_time_subset
  int lane = 0;  // 0 = the slot's stream; 1, 2 = side streams between a FORK and a JOIN (independent ResBlocks of one stage)
  enum Kind { LAUNCH, FORK, JOIN } kind = LAUNCH;
  // route records of the most recent enqueue, eager or under capture (a captured graph replays the same kernels): empty unless the
  // context was armed then (piper_hip_routes_arm)
  piper_hip_ctx* ctx = nullptr;
  std::string routes;
  int enqueue(hipStream_t q) {
    if (__builtin_expect(!ctx->routes_on, 1)) return run(q);
    routes.clear();
    ctx->route_sink = &routes;
    const int rc = run(q);
    ctx->route_sink = nullptr;
    return rc;
  }
};

struct ConvW {  // one resident conv: packed (MFMA) or raw (direct) weights + bias pointer into the resident blob
  const float* w = nullptr;
  const float* w16 = nullptr;  // 16-wide fragment image (short-utterance geometry)
  const float* w16g = nullptr; // the same for a gated conv: 8 tanh rows + their 8 sigmoid rows per tile
  const float* w8 = nullptr;   // 8-row fragment image (the FFN's second conv: 768 → 192)
  const float* w4 = nullptr;   // conv_win_kernel fragment image (generator convs: long rows)
  const float* w5 = nullptr;   // conv_pipe_kernel fragment image (chunk-major step order; Cin % 32 == 0)
  const float* bias = nullptr;
  int Cout = 0, Cin = 0, K = 1;
  bool mfma = false;
};

// A plan's streams and events: the main stream with the timing events ev0 / ev1 (create_set), and the two side streams of schedules with
// parallel branches with their fork / join events (ensure_side_streams, created on first use). A plan holds one while it is attached.
struct StreamSet {
  hipStream_t stream = nullptr, side[2] = {nullptr, nullptr};
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
};

// What a plan computes. PLAN_PREDICT then PLAN_FROM_STATS is a whole utterance with predicted durations that runs the encoder once.
enum PlanKind : int {
  PLAN_WHOLE = 0,       // whole utterance: text encoder, flow, generator
  PLAN_GENERATOR = 1,   // generator only, over a window of the latent (streaming)
  PLAN_PREDICT = 2,     // text encoder + projection + duration predictor
  PLAN_FROM_STATS = 3,  // everything AFTER the text encoder (expansion, flow, generator), from an m_p / logs_p tensor copied in from a PLAN_PREDICT plan
};

// A row's output format on a mixed slot (include/piper_hip.h "Mixed formats"), as checked: rate 0 = the voice's own, gain never 0.
struct RowFormat {
  int rate = 0, enc = PIPER_HIP_ENC_S16;
  float gain = 1.0f;
};

// One row of a stream on the host, the same record for a single stream, an item of a group and a row of a pool (Stream::rows):
// the item's frames, its next frame, and whether the next step decodes a chunk of it (false: finished, dropped, or a pool row never taken).
struct StreamRow {
  int F = 0, next = 0;
  bool active = false;
  // A group's item after stream_drop: it delivers nothing (active = false), but until the frame where its stream would have ended its window
  // still counts when a step chooses its plan, so the other items run the plans — and receive the samples, bit for bit — that they would
  // have without the drop. A pool's rows are never ghosts: a dropped row is free for the next join at once.
  bool ghost = false;
  RowFormat fmt;  // read on a mixed slot only; set by stream_item_formats (group) or the join that took the row (pool)
  const float* gf = nullptr;  // the gains per frame [F] of an item with a volume, in device memory (piper_hip.h "Per-phoneme volume"); null: none
  int64_t lim_lo = 0;  // read on a slot with a level only: where the row's previous step ended, in limited samples (a step at next == 0 starts it at 0)
};

// The level of a stream — single, group or pool (piper_hip_voice_stream_set_level; include/piper_hip.h "Level control"): per generator row
// a carry in device memory (the samples u a step could not finish yet and the last final G), the step's LvStepRow table, and the limited
// samples of one step, lim [rows][row], which the output kernels then read in place of the window plan's audio.
struct StreamLevel {
  bool on = false;
  piper_hip_level lv{};       // as stream_level reports it: defaults resolved
  LvParams p{};
  int rows = 0;               // generator rows the buffers below hold
  int64_t row = 0;            // floats of a row of `lim`
  float* carry = nullptr;     // device [rows][kLvCarry]
  float* lim = nullptr;       // device [rows][row]
  LvStepRow* desc = nullptr;  // device [rows]
};

// The equaliser of a stream — single, group or pool (piper_hip_voice_stream_set_eq; include/piper_hip.h "Equaliser"): the design in device
// memory, per generator row a carry (the aggregates of the set bits of the row's block count), the step's EqStepRow table and scratch,
// and the EQ'd chunks of one step in the layout of the window plan's audio, which the later stages read in place of it.
struct StreamEq {
  bool on = false;
  piper_hip_eq eq{};
  int rows = 0;               // generator rows carry, scratch and desc hold
  int blocks = 0;             // scratch blocks per row
  EqDesign* dev = nullptr;    // device
  double* carry = nullptr;    // device [rows][kEqCarry]
  double* scratch = nullptr;  // device [rows][blocks][2·kEqMaxD]
  EqStepRow* desc = nullptr;  // device [rows]
  float* out = nullptr;       // device, out_bytes: the EQ'd chunks of one step
  size_t out_bytes = 0;
};

// The output rate of a stream — single, group or pool (piper_hip_voice_stream_set_rate): 0 is the voice's own rate. A resampling stream
// keeps, per generator row, the last kRsHist samples of the previous chunk in device memory, in two buffers that change roles every step
// (one launch reads the old history and writes the new one), and uploads a descriptor of its own per step.
struct StreamRate {
  int rate = 0;
  bool started = false;       // a step has run (a pool: or a session has joined): the rate can no longer change
  int parity = 0;             // which history buffer the next step reads
  int rows = 0;               // generator rows the buffers below hold
  float* hist = nullptr;      // device [2][rows][kRsHist]
  RsStepRow* desc = nullptr;  // device [rows]
  // Mixed formats (piper_hip_voice_stream_set_mixed): every row brings its own rate, encoding and gain (StreamRow::fmt); `rate` stays 0.
  // The history is the one above, used by the rows that have a filter; the step's descriptor is a MixStepRow table of its own.
  bool mixed = false;
  int mix_rows = 0;             // generator rows `mdesc` holds
  MixStepRow* mdesc = nullptr;  // device [mix_rows]
};

// A stream in progress, whoever holds it: a plan (Slot::stream — a single stream or a group) or a streaming pool (StreamPool::st).
// `rows` empty: no stream. The device buffers come from stream_alloc and belong to `plan`, or to the context pool for a streaming pool.
struct Slot;
struct Stream {
  int chunk = 0, halo = 0, NBg = 1;  // frames; the generator's batch (1 for a single stream), fixed for the life of the stream
  bool single = false;               // stream_begin's: one row that stream_next steps, not a group of one
  std::vector<StreamRow> rows;       // one per item / pool row
  int* d_desc = nullptr;             // device: [NBg][kDescInts] descriptor of a batched step (one upload per step)
  void* pack = nullptr;              // device: the packed chunks of one batched step
  size_t pack_bytes = 0;             // of `pack`
  StreamRate rs;                     // output rate of the stream
  StreamLevel lv;                    // level of the stream
  StreamEq eq;                       // equaliser of the stream
  // Per-phoneme volume: the shaped chunks of one step in the layout of the window plan's audio, and the step's VolStepRow table; both
  // allocated by the first step that has a row with a volume
  float* vol = nullptr;
  size_t vol_bytes = 0;
  VolStepRow* vol_desc = nullptr;    // device [NBg]
  Slot* plan = nullptr;              // owner of the device buffers; nullptr = the context pool (a streaming pool)
  int items() const { return (int)rows.size(); }
};

// A device buffer of a plan's output chain (in the plan's `owned`) that knows its own size: plan_ensure allocates it on first use and
// replaces it where it is too small, plan_release gives it back.
struct PlanBuf {
  void* p = nullptr;
  size_t bytes = 0;
  template <class T> T* as() const { return (T*)p; }
};

// Page-locked host memory of a slot id's staging (piper_hip_voice::Staging), the host twin of PlanBuf: the pointer and its capacity in
// elements. THE INVARIANT of every one of them: a slot id's staging is regrown or rewritten only after that slot id's stream has been
// waited for (both prepares wait before their first ensure; every stream step and every collect ends with a wait).
template <typename Tp>
struct PinnedBuf {
  Tp* p = nullptr;
  size_t cap = 0;
  operator Tp*() const { return p; }
  // Room for `need` elements: nothing to do where there is, otherwise freed and allocated again (contents dropped) at `min_cap` elements
  // or a power of two times that. On failure p is null and cap 0.
  int ensure(size_t need, size_t min_cap = 1024) {
    if (cap >= need) return PIPER_HIP_OK;
    release();
    size_t c = min_cap;
    while (c < need) c <<= 1;
    PH_HIP(hipHostMalloc((void**)&p, c * sizeof(Tp)), PIPER_HIP_ERR_ALLOC);
    cap = c;
    return PIPER_HIP_OK;
  }
  // The device's view of the memory, or null: none allocated, or no mapping on this system (the runtime's sticky error is cleared then,
  // and nothing else happens: a caller that refuses says so in its own words).
  Tp* mapped() const {
    Tp* d = nullptr;
    if (p && hipHostGetDevicePointer((void**)&d, p, 0) != hipSuccess) { d = nullptr; (void)hipGetLastError(); }
    return d;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
  }
};

// The output chain of a whole-item plan: what the stages between the plan's graph and the sinks — volume, pitch, EQ, loudness, level,
// join, and the peaks of a normalising PCM collect — keep with the plan. chain_walk runs the stages in that order; every stage reads
// the rows its predecessor hands on and writes rows of its own, in the layout of the plan's audio. The plan's audio stays raw.
struct OutputChain {
  // What was computed from the audio of the latest launch. chain_invalidate clears all of it where the plan's audio is new or about to be.
  bool shaped_ok = false;         // shaped holds the latest launch
  bool pitched_ok = false;        // pitched and pt_lensF do
  bool eq_ok = false;             // eqd does, under eq_held
  bool loud_ok = false;           // loud_seg does, measured behind eq_held
  std::vector<float> h_peaks;     // [NB] max |x| per item of a normalising collect_pcm16 (empty: none since the last launch)
  std::vector<int64_t> h_jrep;    // {total, start[NB], len[NB]} of the latest joined collect (empty: none since the last launch)
  // volume (the staged gains are the plan's vol_gain)
  PlanBuf shaped;                 // float [NB][n_samples] the items under their envelopes
  // pitch (piper_hip_voice_slot_pitch), as the plan's latest staging left it (stage_pitch)
  bool pt_on = false;             // the staging carried a pitch: pt_q holds the items' steps, pt_dev their tables
  std::vector<uint64_t> pt_q;     // [NB] the 32.32 step per item (kPtOne: the item has no pitch)
  uint64_t pt_qmin = kPtOne, pt_qmax = kPtOne;  // over the batch, items without a pitch included
  int pt_pmax = 0;                // the most taps of the batch
  PlanBuf pt_dev;                 // PtItem [NB] | the [129][P] tables, one per distinct step of the batch
  PlanBuf pitched;                // float [NB][F'cap·hop] the pitched items, each zero from N' up to its F'·hop
  PlanBuf pt_lensF;               // int [NB] F' per item, as the kernel wrote them
  // The row (samples, frames) the buffers of the stages behind the pitch (row_sized) were allocated for: a staging with a lower pitch
  // makes longer rows, and the walk then gives them all back to be allocated again by the stage that next needs one.
  int64_t row = 0;
  int F = 0;
  // EQ (piper_hip_voice_slot_eq)
  PlanBuf eqd;                    // float [NB][row] the EQ'd items
  PlanBuf eq_work;                // double [NB][eq_work_row(F·hop, kEqMaxD)] the block tree
  PlanBuf eq_dev;                 // EqDesign: the design eqd was filtered with
  bool eq_on = false;             // the EQ the chain last read the items through: eq_held, or none (the loudness measured behind it too)
  piper_hip_eq eq_held{};
  bool eq_dev_ok = false;         // eq_dev holds the design of eq_dev_eq
  piper_hip_eq eq_dev_eq{};
  // loudness (piper_hip_voice_slot_loudness, piper_hip_voice_loudness)
  PlanBuf loud_seg;               // double [NB][ld_work_row(F·hop)] the passes' shares of Σ y² per 100 ms segment
  PlanBuf loud_rep;               // float [NB][2] {L, g} as the gate kernel last wrote them
  PlanBuf gained;                 // float [NB][row] the items times their loudness gain
  // level (piper_hip_voice_slot_level)
  PlanBuf lim;                    // float [NB][row] the limited items
  PlanBuf lim_scratch;            // float lv_scratch_floats(NB, F·hop)
  // join (piper_hip_voice_slot_join)
  PlanBuf jn_buf;                 // float: the programme
  PlanBuf jn_dev;                 // JoinParams | report [kJoinReport] | rows [kJoinMaxItems] | edges [2·kJoinMaxItems], total
  uint64_t jn_gen = 0;            // the slot_join call whose params jn_dev holds (0: none)
  // normalize = 1
  PlanBuf peaks;                  // float [NB] max |x| per item
  std::array<PlanBuf*, 6> row_sized() { return {&eqd, &eq_work, &gained, &loud_seg, &lim, &lim_scratch}; }
};

// The plan's audio is new, or about to be (a launch, a staging): everything computed from the old audio is stale.
void chain_invalidate(OutputChain& ch) {
  ch.h_peaks.clear();
  ch.loud_ok = false;
  ch.shaped_ok = false;
  ch.pitched_ok = false;
  ch.eq_ok = false;
  ch.h_jrep.clear();
}

struct Slot {
  StreamSet set;  // empty (set.stream == nullptr) while the plan is idle: slot_init takes one, give_back_set returns it
  // A Slot is a PLAN: schedule + arena + graph for one bucket (kind, T, F, NB). T and F are the bucket's row lengths; the
  // true lengths of the NB batch items live in device memory (lensT / lensF) where every length-aware kernel reads them, so
  // one captured graph serves every utterance that fits the bucket — exactly (positions past a true length read as zero
  // padding, attention excludes keys past it), not approximately.
  PlanKind kind = PLAN_WHOLE;
  int T = -1, F = -1, NB = 1;
  int prec = 0;            // generator precision the schedule was built for
  bool in_use = false;     // attached to a user slot id
  bool built = false;      // schedule + arena exist; `exec` (the captured graph) follows after the plan's FIRST run, which goes out eagerly
  uint64_t last_use = 0;   // voice-wide clock value of the last attach (LRU)
  size_t arena_bytes = 0;
  int* lensT = nullptr;    // [NB] device: true phoneme count per item
  int* lensF = nullptr;    // [NB] device: true frame count per item
  std::vector<int> h_T, h_F;   // the same on the host (collect / tap / streaming)
  // duration-predictor plan (PLAN_PREDICT): encoder + predictor → frames per id
  float* dp_noise = nullptr;   // [NB][2][T] injected `dp` RandomNormalLike tensor
  void* dp_scalars = nullptr;  // [NB] DpScalars (device)
  int32_t* dp_dur = nullptr;   // [NB][T] predicted frames per id
  std::vector<int32_t> h_dur;  // predicted durations of the attached request, per item back to back (host)
  // PLAN_FROM_STATS prepared by piper_hip_voice_prepare_batch_bounded: the frame counts are decided on the device and reach the host with the
  // waveform (collect). Until then h_F holds the bucket's capacity.
  bool bounded_pending = false;
  int bounded_cap = 0;         // max_frames the caller allowed
  hipEvent_t ev_in = nullptr;  // PLAN_FROM_STATS: "the copy of the predictor plan's projection has been read" (that plan's stream waits for it)
  float* stats = nullptr;      // [NB][2·inter][T] encoder projection (m_p ; logs_p): output of PLAN_WHOLE / PLAN_PREDICT, INPUT of PLAN_FROM_STATS
  // device buffers
  std::vector<void*> owned;
  int64_t* ids = nullptr;
  int32_t* frame2id = nullptr;
  float* noise = nullptr;
  float* noise_scale = nullptr;  // [NB] device
  unsigned* rng = nullptr;       // [NB][2] device: {generate noise on the device?, seed}
  // a voice with a speaker table (null otherwise): the items' speakers, a plan input staged like ids and lengths; what the plan's
  // "spk.rows" step makes of them — g [NB][gin] and the speaker rows [NB][Ctot], of which this plan computes its own part. A generator
  // window plan has no step: spk_bias is [NB][up_initial], the conv_pre rows that travel with the rows' latents.
  piper_hip_speaker* spk_in = nullptr;
  float* spk_g = nullptr;
  float* spk_bias = nullptr;
  // A plan of requests that carry prosody (piper_hip.h "Per-phoneme prosody") is a plan kind of its own: `pro` is part of its cache key
  // next to (kind, T, F, NB), its schedule runs the _prosody steps and it owns the per-id inputs below, staged with the ids. A plan
  // without (pro = false) has none of them. Predictor plan: pro_len, pro_min, pro_max [NB][T] and dp_w [NB][T] (the "dp.w" tap); the
  // others: pro_noise [NB][T] and pro_fit [NB] (read by the bounded route's generate_path).
  bool pro = false;
  float *pro_len = nullptr, *pro_noise = nullptr, *dp_w = nullptr;
  int32_t *pro_min = nullptr, *pro_max = nullptr, *pro_fit = nullptr;
  std::vector<int64_t> h_wanted;  // per item: Σ d of the frame rule before fitting (piper_hip_voice_prosody_report), where h_dur answers
  std::vector<int32_t> h_fitted;  // per item: the bounded route compressed it to its bound
  const Slot* ran_predict = nullptr;  // the predictor plan the latest prepare_batch on this plan ran (null: none) — only ever compared
                                      // against the plans in the cache ("predict:" selectors), never dereferenced
  float* audio = nullptr;
  int64_t n_samples = 0;
  std::vector<Step> steps;
  struct Tap {  // a named intermediate: [NB] items of [C][row] floats, of which the first len_b (T or F of item b) are real
    const float* p;
    int C, row, unit;  // unit: 0 = phonemes (T), k ≥ 1 = k positions per frame (1: frames; a generator stage: its upsampling so far)
    size_t batch_stride;
  };
  std::map<std::string, Tap> taps;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool timed = false;
  bool parallel = false;  // capture FORK/JOIN lanes as parallel graph branches (set by the schedule builder)
  float* zin = nullptr;   // generator-only schedule (streaming): the latent window [inter, F] it decodes
  const float* z_out = nullptr;  // full schedule: where the flow leaves z
  // streaming state of a full-schedule slot (piper_hip_voice_stream_*)
  hipGraph_t front_graph = nullptr;
  hipGraphExec_t front_exec = nullptr;  // encoder + flow only
  // the stream of a full-schedule slot, single (piper_hip_voice_stream_begin) or a group (_stream_begin_batch: one row per item, F copied
  // from h_F); its device buffers are in `owned`, kept across streams and released with the plan
  Stream stream;
  // 16-bit PCM output (piper_hip_voice_collect_pcm16 / stream_next_pcm16): a device buffer of this plan (in `owned`), allocated on first use
  void* pcm = nullptr;        // the items back to back, as they travel to the host (int16, or one G.711 byte per sample)
  size_t pcm_cap = 0;         // bytes
  // Per-phoneme volume (piper_hip_voice_slot_volume): plan inputs staged with the ids, read by the output chain and by the streams alike
  bool vol_on = false;           // the plan's latest staging carried a volume: vol_gain holds its gains
  float* vol_gain = nullptr;     // [NB][T] the gain per id (1.0 where an item or an id has none)
  float* vol_gf = nullptr;       // [NB][F] the gain per frame, written for the "vol.gain" tap
  OutputChain chain;             // everything the whole-item stages between the plan's graph and the sinks keep
};

// No stream, single or batched, is in progress on the plan any more (a prepare, a detach, a release).
void reset_stream_state(Slot& s) {
  s.stream.rows.clear();
  s.stream.single = false;
  StreamRate& rs = s.stream.rs;
  rs.rate = 0; rs.started = false; rs.parity = 0; rs.mixed = false;  // (a new stream starts at the voice's own rate; the buffers stay with the plan)
  s.stream.lv.on = false;                                            // (and without a level)
  s.stream.eq.on = false;                                            // (and without an EQ)
}

// Streaming pool (piper_hip_voice_stream_pool_*): `capacity` generator rows on one slot id that sessions enter (join) and leave (last chunk
// or stream_drop) while the stream runs. It belongs to the voice per slot id, not to a plan — a pool has no single front plan: every join
// runs encoder + flow on a work slot's plan and moves the latents into the rows' own stores. A row is a group's StreamRow plus its store;
// the stream's buffers come from the context pool and go back in pool_close.
struct PoolRowRef {  // device table entry: where row r's latent [inter][stride] lives
  const float* z;
  int64_t stride;
};
struct PoolJoinEnt {  // per-join table entry of stream_adopt_kernel
  int src, row, F, pad;
};
struct StreamPool {
  Stream st;               // rows.size() = the pool's capacity; a row with active = false is free (never taken, finished or dropped)
  struct Row {             // what only a pool's row has, parallel to st.rows
    float* z = nullptr;    // [inter][stride] row store (context pool), kept while the pool lives, regrown for a longer utterance
    size_t cap = 0;        // floats
    float* gf = nullptr;   // [gf_cap] the gains per frame of an occupant with a volume (context pool), written behind the join's adopt
    size_t gf_cap = 0;     // floats
    int stride = 0;        // bucket_f(F) of the item in the row
    // stream_pool_join_bounded: the row is taken (active) but its F is still on the device until pool_resolve has read the adopt's report
    bool pending = false;
    bool held = false;     // F is the length of the row's latest occupant (stream_pool_item_samples)
    int over_want = 0, over_cap = 0;  // over_want > 0: the latest bounded occupant wanted more frames than its join allowed and never ran
  };
  std::vector<Row> ext;
  struct BoundedJoin {  // a bounded join that pool_resolve has not seen yet: its event (one of ev_pending) and the work slot's prepare
    hipEvent_t ev;
    int work_slot;
    const Slot* plan;
    uint64_t prepared;  // the plan's last_use at the join: the same value later = the work slot has not been prepared again
  };
  std::vector<BoundedJoin> bounded;
  PinnedBuf<int32_t> h_rep;       // page-locked [capacity][2]: {wanted frames, allowed frames} per row, written by stream_adopt_bounded_kernel
  int32_t* d_rep = nullptr;       // its device mapping
  PoolRowRef* d_rows = nullptr;   // device: [NBg] row table, then the [capacity] PoolJoinEnt table of the latest join (one upload per join)
  std::vector<hipEvent_t> ev_free, ev_pending;  // ev_pending: "the adopt of a join since the last step has run", one per join
  float* spk_rows = nullptr;     // device: [capacity][up_initial] conv_pre rows of the sessions in the rows (a voice with speakers; else null)
};

// What the latest stream step of a slot id ran (the "window:" selector of piper_hip_voice_tap): the generator window plan, its last_use
// stamp of that step — another value later = someone else has run the plan since — and the window length Fc of every generator row
// (one for a single stream; 0: a finished, dropped, free or pad row). Host bookkeeping only; plan == nullptr: no step has run.
struct WindowRecord {
  const Slot* plan = nullptr;
  uint64_t stamp = 0;
  std::vector<int> Fc;
};

}  // namespace

struct piper_hip_voice {
  piper_hip_ctx* ctx = nullptr;
  piper_hip_voice_config cfg{};
  float* blob = nullptr;    // resident copy of the fp32 blob (biases, embeddings, LayerNorm, raw weights)
  float* packed = nullptr;  // MFMA fragment images
  size_t blob_floats = 0, packed_floats = 0;
  std::map<std::string, piper_tensor_desc> index;
  // compiled weights
  struct EncLayer {
    ConvW qkv, o, f1, f2;
    const float *ek, *ev, *g1, *b1, *g2, *b2;
    float* qkv_bias;
  };
  std::vector<EncLayer> enc;
  ConvW proj;
  struct Coupling {
    ConvW pre, post;
    std::vector<ConvW> in, rs;
    // the linear tail (last res_skip, post, x1 − m, Flip, the next coupling's pre) as one matrix: fold_flow_tail, null when not folded
    const float *tail_w = nullptr, *tail_b = nullptr;
  };
  std::vector<Coupling> flows;
  ConvW conv_pre, conv_post;
  struct DdsLayer {
    const float *dw_w, *dw_b, *g1, *b1, *g2, *b2;
    ConvW pw;  // 1×1 conv: the 16-wide fragment image (w16) is what dds_layer_kernel reads
  };
  struct DpBlock {  // the predictor's own stack (flow = 0) or one ConvFlow
    int flow = 0;
    ConvW pre, proj;
    std::vector<DdsLayer> dds;
  };
  std::vector<DpBlock> dp;  // [0] main, then the ConvFlows in EXECUTION order (module indices 7, 5, 3)
  const float *dp_m = nullptr, *dp_logs = nullptr;
  struct Stage {
    ConvW up;  // packed ConvTranspose (rows = Cout·stride)
    int Cin, Cout, K, stride, pad;
    std::vector<std::vector<ConvW>> rb;  // [n_rb][n_dil or 2·n_dil]
  };
  std::vector<Stage> stages;
  // bf16 generator (PIPER_HIP_PRECISION_BF16): fragment images of the same decoder convs, built by set_precision
  struct ConvWB {
    const uint16_t* w = nullptr;
    const float* bias = nullptr;
    int Cout = 0, Cin = 0, K = 0;
  };
  int precision = PIPER_HIP_PRECISION_F32;
  ConvWB conv_pre_b;
  std::vector<ConvWB> up_b;                             // [stage]
  std::vector<std::vector<std::vector<ConvWB>>> rb_b;   // [stage][rb][conv]
  std::vector<void*> owned;
  // Plans are cached voice-wide, least-recently-used first out; a user slot id is a handle on one of them. A TTS server sees
  // a new (T, F) almost every call: with buckets the plan for it usually exists already (prepare = input upload only).
  std::vector<std::unique_ptr<Slot>> plans;
  std::vector<StreamSet> free_sets;  // sets of idle plans and those voice_create made, for the next plan attached (a HIP stream costs ≈ 3 ms to create)
  double last_build_ms[6] = {0, 0, 0, 0, 0, 0};  // the latest plan build: stream/events, schedule + arena, arena init, 0 (ABI), capture, instantiate
  size_t plan_cache_max = 128, plan_cache_bytes = (size_t)24 << 30;
  // Page-locked staging of a slot id's inputs and of its (short) waveform: it belongs to the SLOT ID, not to the plan attached to it —
  // a new bucket then costs no hipHostMalloc (≈ 0.3–1 ms each). Every buffer is a PinnedBuf (its invariant is told there), listed in
  // each(): what is freed with the voice.
  struct Staging {
    PinnedBuf<int64_t> h_ids;
    PinnedBuf<int32_t> h_f2i;
    PinnedBuf<int> h_lens;
    PinnedBuf<float> h_audio;
    // the whole-plan scalars of a request (RequestScalars) and, on the bounded route, the predictor's scalars behind them
    PinnedBuf<char> h_misc;
    // bounded prepare (durations predicted, no host round trip): the predictor's noise, and what the device reports back (frames per
    // item, durations) — written by a kernel through the host mapping
    PinnedBuf<float> h_dpn;
    PinnedBuf<int32_t> h_res;
    PinnedBuf<float> h_noise;  // the caller's noise tensors, laid out in bucket rows (prepare_batch)
    PinnedBuf<int> h_desc;     // batched stream: the step's descriptor table (one H2D per step)
    PinnedBuf<float> h_peaks;  // collect_pcm16 with normalize = 1: the items' peaks, written by the pack kernel through the host mapping
    PinnedBuf<float> h_loud;   // piper_hip_voice_loudness: {L, g} per item as the gate kernel reported them
    std::vector<hipEvent_t> chunk_ev;  // collect, 1 … 16 MB waveforms: one event per 1 MB chunk landed in h_audio
    PinnedBuf<piper_hip_speaker> h_spk;  // the items' speakers of a prepare (a voice with a speaker table): kMaxGroup records
    PinnedBuf<int32_t> h_pro;  // the per-id prosody arrays of a prepare in bucket rows: noise [n][T], fit [n], then (bounded) length, min, max [n][T] each
    PinnedBuf<float> h_vol;    // the per-id gains of a prepare in bucket rows [n][T] (a request with a volume)
    PinnedBuf<VolStepRow> h_vstep;  // a stream step's VolStepRow table (one H2D per step that shapes)
    PinnedBuf<EqDesign> h_eq;  // the design of the slot id's EQ on its way to a plan (one H2D when the EQ or the plan changes)
    hipEvent_t eq_ev = nullptr;  // recorded behind the latest copy from h_eq
    PinnedBuf<EqStepRow> h_estep;  // a stream step's EqStepRow table (one H2D per step of a stream with an EQ)
    PinnedBuf<JoinParams> h_join;  // the params of the slot id's join on their way to a plan (one H2D when the join or the plan changes)
    hipEvent_t join_ev = nullptr;  // recorded behind the latest copy from h_join
    PinnedBuf<int64_t> h_jrep;     // the report of a joined collect: written by the plan kernel through the mapping, or by a D2H behind it
    PinnedBuf<char> h_pt;          // the PtItem table and the filter tables of a prepare with a pitch, as they go to the plan's pt_dev
    template <class Fn>
    void each(Fn f) {
      f(h_ids), f(h_f2i), f(h_lens), f(h_audio), f(h_misc), f(h_dpn), f(h_res), f(h_noise), f(h_desc), f(h_peaks), f(h_loud), f(h_eq), f(h_estep),
          f(h_join), f(h_jrep), f(h_spk), f(h_pro), f(h_vol), f(h_pt), f(h_vstep);
    }
  } staging[kMaxSlots];
  // The prosody of a slot id's NEXT staging call (piper_hip_voice_slot_prosody): owned copies of the caller's arrays, an empty array = the
  // field was NULL. The staging call takes the assignment (take_controls) whether or not it succeeds.
  struct Prosody {
    std::vector<float> length, noise;
    std::vector<int32_t> min_frames, max_frames;
    int t = 0, fit = 0;
  };
  std::vector<Prosody> slot_pro[kMaxSlots];
  // The volume of a slot id's NEXT staging call (piper_hip_voice_slot_volume), with the same lifecycle: owned copies of the caller's gains,
  // an empty array = the field was NULL.
  struct Volume {
    std::vector<float> gain;
    int t = 0;
  };
  std::vector<Volume> slot_vol[kMaxSlots];
  // The pitch of a slot id's NEXT staging call (piper_hip_voice_slot_pitch), with the same lifecycle; checked when it was given.
  std::vector<piper_hip_pitch> slot_pt[kMaxSlots];
  // Speaker table of a multi-speaker voice (piper_hip_voice_attach_speakers; spk.S == 0: none): the device tables of speaker.hip, where an
  // item's speaker row keeps the dp.pre rows [0, spk_dp_rows), the flow's from there and the conv_pre rows from spk_pre_off, and each
  // slot id's assignment (empty: speaker 0 alone; items past the end take the last entry).
  SpeakerTables spk;
  int spk_dp_rows = 0, spk_pre_off = 0;
  std::vector<piper_hip_speaker> slot_spk[kMaxSlots];
  // The level of each slot id's whole-item collects (piper_hip_voice_slot_level), as given; on = false: none.
  struct SlotLevel { bool on = false; piper_hip_level lv{}; } slot_lv[kMaxSlots];
  // The loudness target of each slot id's whole-item collects (piper_hip_voice_slot_loudness), as given; on = false: none.
  struct SlotLoudness { bool on = false; piper_hip_loudness ld{}; } slot_ld[kMaxSlots];
  // The equaliser of each slot id's whole-item collects (piper_hip_voice_slot_eq), as given and checked; on = false: none.
  struct SlotEq { bool on = false; piper_hip_eq eq{}; } slot_eq[kMaxSlots];
  // The join of each slot id's whole-item collects (piper_hip_voice_slot_join), checked and counted at the voice's rate; on = false:
  // none. gen numbers the slot_join calls voice-wide: a plan knows by it whether its device copy of the params is this one.
  struct SlotJoin { bool on = false; uint64_t gen = 0; JoinParams p{}; } slot_jn[kMaxSlots];
  uint64_t join_clock = 0;
  bool planned = false;  // a plan has been asked for: the voice's schedules are fixed (no attach_speakers any more)
  Slot* attached[kMaxSlots] = {};
  std::unique_ptr<StreamPool> pools[kMaxSlots];  // the streaming pool a slot id holds (then attached[slot] is null)
  Slot* attached_dp[kMaxSlots] = {};  // bounded prepare: the encoder + predictor plan this slot id holds until its next prepare / detach
  WindowRecord windows[kMaxSlots];    // the latest stream step of each slot id (single stream, group or pool)
  uint64_t use_clock = 0;
  int hop = 1;
  // Output rates used so far: the filter of (cfg.sample_rate → rate) and its table in device memory (context pool), freed with the voice.
  struct RateTable { const RsDesign* d = nullptr; float* taps = nullptr; };
  std::map<int, RateTable> rate_tables;
};

namespace {

struct IndexOut {
  std::map<std::string, piper_tensor_desc>* m;
};
void index_visit(const piper_tensor_desc* d, void* user) { (*((IndexOut*)user)->m)[d->name] = *d; }

const float* tensor(const piper_hip_voice* v, const std::string& name) {
  auto it = v->index.find(name);
  if (it == v->index.end()) return nullptr;
  return v->blob + it->second.offset;
}

struct Packer {  // bump allocator over the packed-weights allocation
  piper_hip_voice* v;
  size_t off = 0;
  hipStream_t s;
  float* take(size_t n) {
    float* p = v->packed ? v->packed + off : nullptr;
    off += (n + 63) & ~(size_t)63;
    return p;
  }
};

// Registers one conv. dry = true only measures the packed size.
ConvW make_conv(Packer& pk, bool dry, const std::string& prefix, int Cout, int Cin, int K, bool has_bias = true, bool win = false, bool gated = false, bool rows8 = false) {
  ConvW c;
  c.Cout = Cout; c.Cin = Cin; c.K = K;
  c.mfma = conv_mfma_eligible(Cout, Cin, K, 1, 1);
  const float* w = dry ? nullptr : tensor(pk.v, prefix + ".weight");
  c.bias = (dry || !has_bias) ? nullptr : tensor(pk.v, prefix + ".bias");
  if (c.mfma) {
    float* p = pk.take(packed_conv_floats(Cout, Cin, K));
    if (!dry) pack_conv_weights(pk.s, w, Cout, Cin, K, p);
    c.w = p;
    float* p16 = pk.take(packed_conv_floats(Cout, Cin, K, 16));
    if (!dry) pack_conv_weights(pk.s, w, Cout, Cin, K, p16, 16);
    c.w16 = p16;
    if (rows8 && Cin % 32 == 0) {  // 8-row tiles for a conv with many input channels and few output rows (conv_lean.hip)
      float* p8 = pk.take(packed_conv_rows8_floats(Cout, Cin, K));
      if (!dry) pack_conv_weights_rows8(pk.s, w, Cout, Cin, K, p8);
      c.w8 = p8;
    }
    if (gated && Cout % 16 == 0) {  // tanh / sigmoid rows interleaved per 16-row tile (conv_short.hip)
      float* pg = pk.take(packed_conv_floats(Cout, Cin, K, 16));
      if (!dry) pack_conv_weights_gate16(pk.s, w, Cout, Cin, K, pg);
      c.w16g = pg;
    }
    if (win) {
      float* p4 = pk.take(packed_conv_win_floats(Cout, Cin, K));
      if (!dry) pack_conv_weights_win(pk.s, w, Cout, Cin, K, p4);
      c.w4 = p4;
      if (Cin % 32 == 0 && K * (Cin / 32) >= 2) {
        float* p5 = pk.take(packed_conv_pipe_floats(Cout, Cin, K));
        if (!dry) pack_conv_weights_pipe(pk.s, w, Cout, Cin, K, p5);
        c.w5 = p5;
      }
    }
  } else {
    c.w = w;
  }
  return c;
}

int compile_weights(piper_hip_voice* v, Packer& pk, bool dry, const std::vector<float*>* qkv_bias) {
  const piper_hip_voice_config& c = v->cfg;
  const int H = c.hidden, I = c.inter;
  char nm[128];
  v->enc.clear(); v->flows.clear(); v->stages.clear();
  for (int l = 0; l < c.n_layers; l++) {
    piper_hip_voice::EncLayer L{};
    L.qkv_bias = qkv_bias ? (*qkv_bias)[l] : nullptr;
    // q,k,v as one 3H-row conv: the packed image is [row tile][step][64], so three H-row images concatenate
    L.qkv.Cout = 3 * H; L.qkv.Cin = H; L.qkv.K = 1; L.qkv.mfma = true;
    float* p = pk.take(3 * packed_conv_floats(H, H, 1));
    float* p16 = pk.take(3 * packed_conv_floats(H, H, 1, 16));
    L.qkv.w = p;
    L.qkv.w16 = p16;
    if (!dry) {
      static const char* qkv[3] = {"conv_q", "conv_k", "conv_v"};
      for (int j = 0; j < 3; j++) {
        snprintf(nm, sizeof nm, "enc_p.encoder.attn_layers.%d.%s", l, qkv[j]);
        pack_conv_weights(pk.s, tensor(v, std::string(nm) + ".weight"), H, H, 1, p + j * packed_conv_floats(H, H, 1));
        pack_conv_weights(pk.s, tensor(v, std::string(nm) + ".weight"), H, H, 1, p16 + j * packed_conv_floats(H, H, 1, 16), 16);
        PH_HIP(hipMemcpyAsync(L.qkv_bias + j * H, tensor(v, std::string(nm) + ".bias"), H * sizeof(float),
                              hipMemcpyDeviceToDevice, pk.s), PIPER_HIP_ERR_LAUNCH);
      }
      L.qkv.bias = L.qkv_bias;
    }
    snprintf(nm, sizeof nm, "enc_p.encoder.attn_layers.%d.conv_o", l);
    L.o = make_conv(pk, dry, nm, H, H, 1);
    snprintf(nm, sizeof nm, "enc_p.encoder.ffn_layers.%d.conv_1", l);
    L.f1 = make_conv(pk, dry, nm, c.ffn, H, c.ffn_kernel);
    snprintf(nm, sizeof nm, "enc_p.encoder.ffn_layers.%d.conv_2", l);
    L.f2 = make_conv(pk, dry, nm, H, c.ffn, c.ffn_kernel, true, false, false, true);
    if (!dry) {
      snprintf(nm, sizeof nm, "enc_p.encoder.attn_layers.%d.emb_rel_k", l); L.ek = tensor(v, nm);
      snprintf(nm, sizeof nm, "enc_p.encoder.attn_layers.%d.emb_rel_v", l); L.ev = tensor(v, nm);
      snprintf(nm, sizeof nm, "enc_p.encoder.norm_layers_1.%d.gamma", l); L.g1 = tensor(v, nm);
      snprintf(nm, sizeof nm, "enc_p.encoder.norm_layers_1.%d.beta", l); L.b1 = tensor(v, nm);
      snprintf(nm, sizeof nm, "enc_p.encoder.norm_layers_2.%d.gamma", l); L.g2 = tensor(v, nm);
      snprintf(nm, sizeof nm, "enc_p.encoder.norm_layers_2.%d.beta", l); L.b2 = tensor(v, nm);
    }
    v->enc.push_back(L);
  }
  v->proj = make_conv(pk, dry, "enc_p.proj", 2 * I, H, 1);
  for (int f = 0; f < c.n_flows; f++) {
    piper_hip_voice::Coupling C;
    snprintf(nm, sizeof nm, "flow.flows.%d.pre", 2 * f);
    C.pre = make_conv(pk, dry, nm, H, I / 2, 1);
    for (int i = 0; i < c.wn_layers; i++) {
      snprintf(nm, sizeof nm, "flow.flows.%d.enc.in_layers.%d", 2 * f, i);
      C.in.push_back(make_conv(pk, dry, nm, 2 * H, H, c.wn_kernel, true, false, true));
      snprintf(nm, sizeof nm, "flow.flows.%d.enc.res_skip_layers.%d", 2 * f, i);
      C.rs.push_back(make_conv(pk, dry, nm, (i + 1 < c.wn_layers) ? 2 * H : H, H, 1));
    }
    snprintf(nm, sizeof nm, "flow.flows.%d.post", 2 * f);
    C.post = make_conv(pk, dry, nm, I / 2, H, 1);
    v->flows.push_back(C);
  }
  // The folded tails (conv.h: FlowTailArgs). Coupling f's tail ends in the pre of coupling f − 1, the next one the reverse flow runs;
  // coupling 0's ends at x1new. The reverse pass flips before every coupling, so coupling f sees its x1 through a reversed channel
  // map exactly when n_flows − f is odd.
  if (flow_tail_shape_ok(H, I / 2) && I % 2 == 0 && c.wn_layers >= 2 && c.n_flows >= 1) {
    const int half = I / 2;
    double* scratch = (double*)pk.take(2 * flow_tail_scratch_doubles(H, half));
    for (int f = 0; f < c.n_flows; f++) {
      auto& C = v->flows[f];
      const int seam = f > 0;
      float* img = pk.take(flow_tail_image_floats(H, half, seam));
      float* tb = pk.take((size_t)half + (seam ? H : 0));
      if (dry) continue;
      auto raw = [&](const char* what, int g) {
        snprintf(nm, sizeof nm, "flow.flows.%d.%s", 2 * g, what);
        return std::string(nm);
      };
      const std::string rs = raw("enc.res_skip_layers.", f) + std::to_string(c.wn_layers - 1), post = raw("post", f), pre = raw("pre", std::max(f - 1, 0));
      const int rc = fold_flow_tail(pk.s, tensor(v, rs + ".weight"), tensor(v, rs + ".bias"), tensor(v, post + ".weight"), tensor(v, post + ".bias"),
                                    seam ? tensor(v, pre + ".weight") : nullptr, seam ? tensor(v, pre + ".bias") : nullptr, H, half,
                                    (c.n_flows - f) % 2 ? -1 : 1, scratch, img, tb);
      if (rc) return rc;
      C.tail_w = img; C.tail_b = tb;
    }
  }
  v->conv_pre = make_conv(pk, dry, "dec.conv_pre", c.up_initial, I, 7);
  int ch = c.up_initial;
  for (int u = 0; u < c.n_ups; u++) {
    piper_hip_voice::Stage S;
    S.Cin = ch; S.Cout = ch / 2; S.K = c.up_kernels[u]; S.stride = c.up_rates[u]; S.pad = (S.K - S.stride) / 2;
    const int J = (S.K + S.stride - 1) / S.stride;
    S.up.Cout = S.Cout * S.stride; S.up.Cin = S.Cin; S.up.K = J; S.up.mfma = true;
    float* p = pk.take(packed_convt_floats(S.Cin, S.Cout, S.K, S.stride));
    float* p16 = pk.take(packed_convt_floats(S.Cin, S.Cout, S.K, S.stride, 16));
    S.up.w = p;
    S.up.w16 = p16;
    const bool ct_win = convt_win_eligible(S.Cin, S.Cout, S.K, S.stride, S.pad, 4);
    float* p4 = ct_win ? pk.take(packed_convt_win_floats(S.Cin, S.Cout, S.K, S.stride)) : nullptr;
    S.up.w4 = ct_win ? p4 : nullptr;
    const bool ct_pipe = convt_pipe_eligible(S.Cin, S.Cout, S.K, S.stride, S.pad, 4);
    float* p5 = ct_pipe ? pk.take(packed_convt_pipe_floats(S.Cin, S.Cout, S.K, S.stride)) : nullptr;
    S.up.w5 = p5;
    if (!dry) {
      snprintf(nm, sizeof nm, "dec.ups.%d", u);
      if (ct_win) pack_convt_weights_win(pk.s, tensor(v, std::string(nm) + ".weight"), S.Cin, S.Cout, S.K, S.stride, S.pad, p4);
      if (ct_pipe) pack_convt_weights_pipe(pk.s, tensor(v, std::string(nm) + ".weight"), S.Cin, S.Cout, S.K, S.stride, S.pad, p5);
      pack_convt_weights(pk.s, tensor(v, std::string(nm) + ".weight"), S.Cin, S.Cout, S.K, S.stride, p);
      pack_convt_weights(pk.s, tensor(v, std::string(nm) + ".weight"), S.Cin, S.Cout, S.K, S.stride, p16, 16);
      S.up.bias = tensor(v, std::string(nm) + ".bias");
    }
    ch /= 2;
    for (int j = 0; j < c.n_rb; j++) {
      std::vector<ConvW> convs;
      const int rb = u * c.n_rb + j;
      for (int d = 0; d < c.rb_n_dil; d++) {
        if (c.resblock_type == 1) {
          snprintf(nm, sizeof nm, "dec.resblocks.%d.convs1.%d", rb, d);
          convs.push_back(make_conv(pk, dry, nm, ch, ch, c.rb_kernels[j], true, true));
          snprintf(nm, sizeof nm, "dec.resblocks.%d.convs2.%d", rb, d);
          convs.push_back(make_conv(pk, dry, nm, ch, ch, c.rb_kernels[j], true, true));
        } else {
          snprintf(nm, sizeof nm, "dec.resblocks.%d.convs.%d", rb, d);
          convs.push_back(make_conv(pk, dry, nm, ch, ch, c.rb_kernels[j], true, true));
        }
      }
      S.rb.push_back(convs);
    }
    v->stages.push_back(S);
  }
  v->conv_post = make_conv(pk, dry, "dec.conv_post", 1, ch, 7, false);
  v->dp.clear();
  if (c.dp_present) {
    auto dds_of = [&](const std::string& base) {
      std::vector<piper_hip_voice::DdsLayer> out;
      for (int i = 0; i < c.dp_dds_layers; i++) {
        piper_hip_voice::DdsLayer d{};
        const std::string sep = base + ".convs.convs_sep." + std::to_string(i), n1 = base + ".convs.norms_1." + std::to_string(i),
                          n2 = base + ".convs.norms_2." + std::to_string(i);
        d.pw = make_conv(pk, dry, base + ".convs.convs_1x1." + std::to_string(i), H, H, 1);
        if (!dry) {
          d.dw_w = tensor(v, sep + ".weight"); d.dw_b = tensor(v, sep + ".bias");
          d.g1 = tensor(v, n1 + ".gamma"); d.b1 = tensor(v, n1 + ".beta");
          d.g2 = tensor(v, n2 + ".gamma"); d.b2 = tensor(v, n2 + ".beta");
        }
        out.push_back(d);
      }
      return out;
    };
    piper_hip_voice::DpBlock m;
    m.flow = 0;
    m.pre = make_conv(pk, dry, "dp.pre", H, H, 1);
    m.proj = make_conv(pk, dry, "dp.proj", H, H, 1);
    m.dds = dds_of("dp");
    v->dp.push_back(m);
    for (int f = 2 * c.dp_n_flows - 1; f > 1; f -= 2) {
      piper_hip_voice::DpBlock b;
      const std::string base = "dp.flows." + std::to_string(f);
      b.flow = f;
      b.pre = make_conv(pk, dry, base + ".pre", H, 1, 1);             // 1 → H: direct kernel
      b.proj = make_conv(pk, dry, base + ".proj", 3 * c.dp_bins - 1, H, 1);
      b.dds = dds_of(base);
      v->dp.push_back(b);
    }
    if (!dry) { v->dp_m = tensor(v, "dp.flows.0.m"); v->dp_logs = tensor(v, "dp.flows.0.logs"); }
  }
  return PIPER_HIP_OK;
}

// ---- stream sets: created by create_set, taken by slot_init, given back by give_back_set, destroyed with the voice -------------

// The first device → host copy a STREAM hands to the copy engine costs 7 … 17 ms (r3, tools/probe/first_run.py with PIPER_HIP_COLLECT_DMA=1:
// 8.1 ms in collect for 1.0 ms of GPU work; warming another stream of the process did not help). Every stream a plan will use gets that copy
// out of the way when it is created — while the voice loads for the four it pre-creates.
void warm_stream_copies(piper_hip_voice* v, hipStream_t q) {
  void* hp = nullptr;
  const size_t nb = std::min<size_t>((size_t)2 << 20, v->blob_floats * sizeof(float));  // large enough for the copy ENGINE (small ones are blitted)
  if (!v->blob || hipHostMalloc(&hp, nb) != hipSuccess) { (void)hipGetLastError(); return; }
  hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, q);  // as in a request: the copy waits for a kernel of the same stream
  (void)hipMemcpyAsync(hp, v->blob, nb, hipMemcpyDeviceToHost, q);
  (void)hipStreamSynchronize(q);
  (void)hipHostFree(hp);
  (void)hipGetLastError();
}

void destroy_set(StreamSet& st) {
  for (hipEvent_t e : {st.ev0, st.ev1, st.ev_fork, st.ev_join[0], st.ev_join[1]})
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t q : {st.side[0], st.side[1], st.stream})
    if (q) (void)hipStreamDestroy(q);
  st = {};
}

// A new set: the main stream and its timing events, with the stream's first copy made. On failure nothing is left behind.
// r3 (tools/probe/cold_prepare.py): creating the three streams of a plan was 8.6–10 ms of an 11 ms plan build. The two side streams are only
// for schedules with parallel branches (ensure_side_streams), so a set starts with one.
int create_set(piper_hip_voice* v, StreamSet& st) {
  st = {};
  hipError_t e = hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&st.ev0);
  if (e == hipSuccess) e = hipEventCreate(&st.ev1);
  if (e != hipSuccess) {
    destroy_set(st);
    PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream set: creation failed: %s", hipGetErrorString(e));
  }
  warm_stream_copies(v, st.stream);
  return PIPER_HIP_OK;
}

// An idle plan needs no stream: its set goes to the next plan that is attached (usually the one replacing it on the same slot id), so that
// after a slot id's first request no prepare creates a stream again (≈ 3 ms each, r3). The caller has synchronised the stream.
void give_back_set(piper_hip_voice* v, Slot& s) {
  if (s.set.stream) v->free_sets.push_back(s.set);
  s.set = {};
}

// `count` sets on the free list while the voice loads (voice_create). Not fatal: slot_init creates what is missing. Returns the first
// set's stream, or null if none could be created.
hipStream_t precreate_sets(piper_hip_voice* v, int count) {
  for (int i = 0; i < count; i++) {
    StreamSet st;
    if (create_set(v, st)) {
      (void)hipGetLastError();
      break;
    }
    v->free_sets.push_back(st);
  }
  return v->free_sets.empty() ? nullptr : v->free_sets[0].stream;
}

// A set for the plan: one given back earlier if there is one, a new one otherwise.
int slot_init(piper_hip_voice* v, Slot& s) {
  if (s.set.stream) return PIPER_HIP_OK;
  if (v->free_sets.empty()) return create_set(v, s.set);
  s.set = v->free_sets.back();
  v->free_sets.pop_back();
  return PIPER_HIP_OK;
}

int ensure_side_streams(Slot& s) {
  StreamSet& st = s.set;
  for (int i = 0; i < 2; i++) {
    if (!st.side[i]) PH_HIP(hipStreamCreateWithFlags(&st.side[i], hipStreamNonBlocking), PIPER_HIP_ERR_LAUNCH);
    if (!st.ev_join[i]) PH_HIP(hipEventCreateWithFlags(&st.ev_join[i], hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
  }
  if (!st.ev_fork) PH_HIP(hipEventCreateWithFlags(&st.ev_fork, hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// The end of a plan: no Slot is used again after it (its callers erase it, or clear the cache).
void slot_release(piper_hip_voice* v, Slot& s) {
  if (s.exec) { (void)hipGraphExecDestroy(s.exec); s.exec = nullptr; }
  if (s.graph) { (void)hipGraphDestroy(s.graph); s.graph = nullptr; }
  if (s.front_exec) { (void)hipGraphExecDestroy(s.front_exec); s.front_exec = nullptr; }
  if (s.front_graph) { (void)hipGraphDestroy(s.front_graph); s.front_graph = nullptr; }
  s.stream = Stream();  // (no stream any more; its device buffers — descriptor, packed chunks, history, tables — are in `owned`)
  s.zin = nullptr; s.z_out = nullptr;
  s.pcm = nullptr; s.pcm_cap = 0;  // (these too)
  s.vol_on = false; s.vol_gain = nullptr; s.vol_gf = nullptr;
  s.chain = OutputChain();
  s.dp_noise = nullptr; s.dp_scalars = nullptr; s.dp_dur = nullptr;
  s.spk_in = nullptr; s.spk_g = nullptr; s.spk_bias = nullptr;
  s.pro = false; s.pro_len = s.pro_noise = s.dp_w = nullptr; s.pro_min = s.pro_max = s.pro_fit = nullptr;
  for (void* p : s.owned) (void)v->ctx->pool.release(p);
  s.owned.clear();
  s.steps.clear();
  s.taps.clear();
  s.T = s.F = -1;
  s.built = false;
  // (the pinned staging buffers are the slot id's: piper_hip_voice::staging)
  if (s.ev_in) (void)hipEventDestroy(s.ev_in);
  s.ev_in = nullptr;
  give_back_set(v, s);  // piper_hip_voice_destroy destroys the sets
}

// Closes the streaming pool of slot id `slot`, if it holds one: waits for the adopts still queued (they write the row stores), then gives
// the row stores and tables back to the context pool.
void pool_close(piper_hip_voice* v, int slot) {
  StreamPool* P = v->pools[slot].get();
  if (!P) return;
  for (hipEvent_t e : P->ev_pending) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
  for (hipEvent_t e : P->ev_free) (void)hipEventDestroy(e);
  for (auto& r : P->ext)
    if (r.z) (void)v->ctx->pool.release(r.z);
  for (auto& r : P->ext)
    if (r.gf) (void)v->ctx->pool.release(r.gf);
  if (P->st.vol) (void)v->ctx->pool.release(P->st.vol);
  if (P->st.vol_desc) (void)v->ctx->pool.release(P->st.vol_desc);
  if (P->d_rows) (void)v->ctx->pool.release(P->d_rows);
  const StreamRate& rs = P->st.rs;
  const StreamLevel& lv = P->st.lv;
  const StreamEq& sq = P->st.eq;
  for (void* p : {(void*)sq.dev, (void*)sq.carry, (void*)sq.scratch, (void*)sq.desc, (void*)sq.out})
    if (p) (void)v->ctx->pool.release(p);
  for (void* p : {(void*)P->st.d_desc, P->st.pack, (void*)rs.hist, (void*)rs.desc, (void*)rs.mdesc, (void*)lv.carry, (void*)lv.lim, (void*)lv.desc})
    if (p) (void)v->ctx->pool.release(p);
  if (P->spk_rows) (void)v->ctx->pool.release(P->spk_rows);
  P->h_rep.release();  // (the adopts that write it have run: waited for above)
  v->pools[slot].reset();
}

struct Arena {
  piper_hip_voice* v;
  Slot* s;
  int rc = PIPER_HIP_OK;
  float* f32(size_t n) {
    void* p = nullptr;
    if (rc) return nullptr;
    rc = v->ctx->pool.alloc((n ? n : 1) * sizeof(float), &p);
    if (!rc) { s->owned.push_back(p); s->arena_bytes += (n ? n : 1) * sizeof(float); }
    return (float*)p;
  }
  void* raw(size_t bytes) {
    void* p = nullptr;
    if (rc) return nullptr;
    rc = v->ctx->pool.alloc(bytes ? bytes : 1, &p);
    if (!rc) { s->owned.push_back(p); s->arena_bytes += bytes ? bytes : 1; }
    return p;
  }
};

double conv_bytes(int Cin, int Cout, int K, int64_t L) { return 4.0 * ((double)Cin * L + (double)Cout * L + (double)Cout * Cin * K + Cout); }

// what a bf16 conv moves: the bf16 input image and weights, the bf16 output image, the fp32 result / residual / MRF operands
double conv_bf16_bytes(const ConvBf16Args& a) {
  const double cols = (double)a.N * a.Lout, out_cols = a.ct_stride > 0 ? cols * a.ct_stride : cols;
  return 2.0 * (a.Cin * cols + (double)a.Cout * a.Cin * a.K) + (a.act ? 2.0 : 0.0) * a.Cout * out_cols +
         ((a.y ? 4.0 : 0.0) + (a.res ? 4.0 : 0.0) + (a.mrf_a ? 8.0 : 0.0)) * a.Cout * out_cols;
}

// What the schedule builders work on: the voice, the plan being built and its arena, the bucket (T, F, NB), the device arrays of the
// items' true lengths, and the lane of the steps added next. Every step, fork, join and tap of a plan is appended here.
struct Builder {
  piper_hip_voice* v;
  Slot& s;
  Arena ar;
  const int T, F, NB;
  const int *lensT = nullptr, *lensF = nullptr;
  int lane = 0;  // given to the steps added next (Step::lane): the ResBlock loops of the per-conv generators move it
  Builder(piper_hip_voice* v_, Slot& s_, int T_, int F_, int NB_) : v(v_), s(s_), ar{v_, &s_}, T(T_), F(F_), NB(NB_) {}
  Builder(const Builder&) = delete;  // a step's closure copies the few values its launch needs, never the builder

  void step(const std::string& name, const char* tag, double flops, double bytes, std::function<int(hipStream_t)> run) {
    Step st;
    st.name = name;
    st.tag = tag;
    st.flops = flops; st.bytes = bytes;
    st.lane = lane;
    st.run = std::move(run);
    st.ctx = v->ctx;
    s.steps.push_back(std::move(st));
  }
  void mark(const std::string& name, Step::Kind kind) {
    Step st;
    st.name = name;
    st.kind = kind;
    s.steps.push_back(std::move(st));
  }
  void fork(const std::string& name) { mark(name, Step::FORK); }
  void join(const std::string& name) { mark(name, Step::JOIN); }
  // a named intermediate: [NB] items of [C][row] floats, batch_stride apart (0 ⇒ dense: C · row)
  void tap(const std::string& name, const float* p, int C, int row, int unit, size_t batch_stride = 0) {
    s.taps[name] = {p, C, row, unit, batch_stride ? batch_stride : (size_t)C * row};
  }

  // lens = the per-item true lengths the rows of this conv are measured in (phonemes or frames), mul = positions per unit
  ConvArgs plain(const float* in, float* out, int Cin_, int Cout_, int L, const int* lens, int mul = 1) const {
    ConvArgs a;
    a.x = in; a.y = out; a.N = NB; a.Lin = L; a.Lout = L; a.x_batch_stride = (int64_t)Cin_ * L; a.y_batch_stride = (int64_t)Cout_ * L;
    a.y_len = L;
    a.len_ptr = lens; a.len_mul = mul;
    return a;
  }

  // A voice with a speaker table: the conv whose rows start at `row` of the speaker row (a main or predictor plan), or conv_pre of a
  // generator window plan (row < 0), reads each item's effective bias. A voice without: nothing changes (the conv's own bias, stride 0).
  template <class Args>
  void speaker_bias(Args& a, int row) const {
    if (!v->spk.S || !s.spk_bias) return;
    a.bias = row < 0 ? s.spk_bias : s.spk_bias + row;
    a.bias_batch_stride = row < 0 ? v->cfg.up_initial : v->spk.Ctot;
  }

  // conv step over a resident ConvW
  void conv(const std::string& name, const ConvW& w, ConvArgs a, int64_t Lout_for_work) {
    a.w = w.w;
    a.w16 = w.w16;
    a.w16g = w.w16g;
    a.w8 = w.w8;
    if (!a.bias) a.bias = w.bias;  // (a speaker-conditioned conv comes with its items' effective biases: speaker_bias)
    a.Cin = w.Cin; a.Cout = w.Cout; a.K = w.K;
    piper_hip_ctx* ctx = v->ctx;
    const bool mfma = w.mfma;
    step(name, mfma ? "conv_mfma" : "conv_small", a.N * conv_flops(w.Cout, w.Cin, w.K, Lout_for_work),
         a.N * conv_bytes(w.Cin, a.gate ? w.Cout / 2 : w.Cout, w.K, Lout_for_work),
         [ctx, a, mfma](hipStream_t q) { return mfma ? launch_conv_mfma(ctx, q, a) : launch_conv_direct(ctx, q, a); });
  }

  // conv step over a bf16 fragment image
  void conv_bf16(const std::string& name, const piper_hip_voice::ConvWB& w, ConvBf16Args a, double flops) {
    a.w = w.w; a.Cin = w.Cin; a.Cout = w.Cout; a.K = w.K;
    if (!a.bias) a.bias = w.bias;  // (conv_pre of a voice with speakers comes with its items' effective biases)
    piper_hip_ctx* ctx = v->ctx;
    step(name, "conv_bf16", flops, conv_bf16_bytes(a), [ctx, a](hipStream_t q) { return launch_conv_bf16(ctx, q, a); });
  }

  // several same-shape bf16 convs (the stage's ResBlocks) as one launch
  void conv_bf16_multi(const std::string& name, const piper_hip_voice::ConvWB* const* ws, const ConvBf16Args* args, int count, double flops) {
    struct Pack { ConvBf16Args a[kBf16Multi]; } pk;
    double bytes = 0;
    for (int i = 0; i < count; i++) {
      ConvBf16Args& a = pk.a[i] = args[i];
      const auto& w = *ws[i];
      a.w = w.w; a.bias = w.bias; a.Cin = w.Cin; a.Cout = w.Cout; a.K = w.K;
      bytes += conv_bf16_bytes(a);
    }
    piper_hip_ctx* ctx = v->ctx;
    step(name, "conv_bf16", flops, bytes, [ctx, pk, count](hipStream_t q) { return launch_conv_bf16_multi(ctx, q, pk.a, count); });
  }
};

// ---- A/B switches of the generator builders. Each is parsed in one place, and looked up (ph::tuning_getenv records the ones that are
// set, piper_hip_config_string() reports them) the first time a builder that honours it asks.
bool no_merged_rb() { static const bool on = getenv("PIPER_HIP_NO_MERGED_RB") != nullptr; return on; }  // both precisions: one launch per conv
bool no_rb_pair() { static const bool on = getenv("PIPER_HIP_NO_RB_PAIR") != nullptr; return on; }      // both precisions: no two-conv launches

struct GenF32Switches {
  const bool parallel_rb = getenv("PIPER_HIP_PARALLEL_RB") != nullptr;
  const bool use_win = getenv("PIPER_HIP_NO_WIN") == nullptr;  // window kernel for the generator's long rows
  // PIPER_HIP_NO_PIPE=1 keeps round 1's one-tile-per-block window kernel.
  // conv_pipe (persistent, chunk-pipelined) wins once a launch holds enough work to amortise its prologue and tail — the
  // high voice's 128/256-channel stages: 89 vs 73 TFLOP/s — and loses to the one-tile-per-block window kernel on the medium
  // voice at factor 8 (48 vs 46 µs per merged launch). Threshold on the launch's FLOPs; PIPER_HIP_PIPE_MIN_GFLOP overrides.
  const bool no_pipe = getenv("PIPER_HIP_NO_PIPE") != nullptr;
  const double pipe_min_flops = [] { const char* e = getenv("PIPER_HIP_PIPE_MIN_GFLOP"); return (e ? atof(e) : 5.0) * 1e9; }();
  // r2f (factor 64): as a single-conv launch it also loses at 32 / 64 channels (135 vs 114 µs, 105 vs 100 µs: one chunk per
  // tile leaves nothing to pipeline, and 2 blocks per CU hide less than the window kernel's 4) and wins from 128 channels up.
  // ConvTranspose: it won (112 vs 145 µs) until the window kernel staged narrow windows with a flat index and kept the phases
  // of a column range in one block; since then the window kernel wins at every size measured (factor 64: 126 / 121 vs
  // 187 / 204 µs, 8 × factor 8: 111 / 119 vs 181 / 201 µs, high voice factor 32: 215 vs 312 µs) — never by default,
  // PIPER_HIP_PIPE_CT_MIN_GFLOP=g brings it back for launches of ≥ g GFLOP.
  const double pipe_ct_min_flops = [] { const char* e = getenv("PIPER_HIP_PIPE_CT_MIN_GFLOP"); return e ? atof(e) * 1e9 : 1e30; }();
  bool pipe_pays(double launch_flops, int Cin, bool ct) const {
    return !no_pipe && launch_flops >= (ct ? pipe_ct_min_flops : pipe_min_flops) && (ct || Cin >= 128);
  }
};
const GenF32Switches& gen_f32_switches() {
  static const GenF32Switches sw;
  return sw;
}

// ---- generator pieces that more than one builder schedules

// window-kernel arguments of a 'same'-padded stride-1 conv on lrelu(x, 0.1) over rows of L positions; mrf_a / mrf_b: the MRF mean
// ((mrf_a + mrf_b) + result) / 3 and the LeakyReLU(out_alpha) after it, folded into the epilogue
ConvWinArgs win_args(const Builder& b, const ConvW& w, const float* x, const float* res, float* y, int dil, int L, const float* mrf_a = nullptr,
                     const float* mrf_b = nullptr, float out_alpha = 1.0f) {
  ConvWinArgs wa;
  wa.x = x; wa.w4 = w.w4; wa.bias = w.bias; wa.res = res; wa.y = y;
  wa.pro_alpha = 0.1f;
  if (mrf_a) { wa.mrf_a = mrf_a; wa.mrf_b = mrf_b; wa.out_alpha = out_alpha; }
  wa.N = b.NB; wa.Cin = w.Cin; wa.Cout = w.Cout; wa.K = w.K; wa.dil = dil; wa.padL = (w.K * dil - dil) / 2;
  wa.Lin = L; wa.Lout = L; wa.y_len = L;
  wa.len_ptr = b.lensF; wa.len_mul = L / b.F;
  return wa;
}

// fp32 ConvTranspose of stage S, rows of L → L · stride positions, on lrelu(input, pro_alpha) — input = cur[0] (pro_alpha 1: its producer
// applied the LeakyReLU already) or, with cur[1] and cur[2] set, the MRF mean of the three. Pipe, window or streaming kernel.
void add_convt_f32(Builder& b, const std::string& name, const piper_hip_voice::Stage& S, const float* const cur[3], float pro_alpha, float* up,
                   int L) {
  const GenF32Switches& sw = gen_f32_switches();
  piper_hip_ctx* ctx = b.v->ctx;
  const int NB = b.NB, Lo = L * S.stride;
  const double flops = NB * 2.0 * S.Cin * S.Cout * (double)S.K * L;  // convT(Cin,Cout,K,s,Lin)
  const double bytes = NB * 4.0 * ((double)S.Cin * L * (cur[1] ? 3 : 1) + (double)S.Cout * Lo + (double)S.Cin * S.Cout * S.K + S.Cout);
  const bool pipe = sw.use_win && sw.pipe_pays(flops, S.Cin, true) && S.up.w5 && convt_pipe_eligible(S.Cin, S.Cout, S.K, S.stride, S.pad, L);
  if (pipe || (sw.use_win && S.up.w4 && convt_win_eligible(S.Cin, S.Cout, S.K, S.stride, S.pad, L))) {
    ConvWinArgs wa;
    wa.x = cur[0]; wa.x2 = cur[1]; wa.x3 = cur[2]; wa.w4 = pipe ? S.up.w5 : S.up.w4; wa.bias = S.up.bias; wa.y = up;
    wa.pro_alpha = pro_alpha;
    wa.N = NB; wa.Cin = S.Cin; wa.Cout = S.Cout; wa.K = S.K; wa.Lin = L; wa.Lout = L; wa.y_len = Lo;
    wa.ct_stride = S.stride; wa.ct_pad = S.pad;
    wa.len_ptr = b.lensF; wa.len_mul = L / b.F;
    if (pipe) b.step(name, "conv_mfma", flops, bytes, [ctx, wa](hipStream_t q) { return launch_conv_pipe_multi(ctx, q, &wa, 1); });
    else b.step(name, "conv_mfma", flops, bytes, [ctx, wa](hipStream_t q) { return launch_conv_win(ctx, q, wa); });
    return;
  }
  ConvArgs a;
  a.x = cur[0]; a.x2 = cur[1]; a.x3 = cur[2];
  a.prologue = cur[1] ? PRO_AVG3_LRELU : pro_alpha == 1.0f ? PRO_NONE : PRO_LRELU;
  a.alpha = 0.1f;
  a.y = up; a.N = NB; a.dil = -1; a.padL = 0; a.Lin = L; a.Lout = (Lo - 1 + S.pad) / S.stride + 1;
  a.len_ptr = b.lensF; a.len_mul = L / b.F;
  a.x_batch_stride = (int64_t)S.Cin * L; a.y_batch_stride = (int64_t)S.Cout * Lo; a.y_len = Lo;
  a.epilogue = EPI_CONVT; a.ct_stride = S.stride; a.ct_padL = S.pad; a.ct_Lout = Lo;
  a.w = S.up.w; a.w16 = S.up.w16; a.bias = S.up.bias; a.Cin = S.up.Cin; a.Cout = S.up.Cout; a.K = S.up.K;
  b.step(name, "conv_mfma", flops, bytes, [ctx, a](hipStream_t q) { return launch_conv_mfma(ctx, q, a); });
}

// y = lrelu(((r0 + r1) + r2) / 3, alpha) over cnt floats, as a launch of its own
void add_mrf_mean(Builder& b, const std::string& name, const float* r0, const float* r1, const float* r2, float* y, int64_t cnt, float alpha) {
  b.step(name, "", 0, 0, [=](hipStream_t q) {
    const int grid = (int)std::min<int64_t>(ceil_div(cnt, (int64_t)kBlock * 4), 2048);
    hipLaunchKernelGGL(mrf_mean_lrelu_kernel, dim3(grid), dim3(kBlock), 0, q, r0, r1, r2, y, cnt, alpha);
    return PIPER_HIP_OK;
  });
}

// The waveform: conv_post (→ 1 channel, k7: thread-per-output fp32 kernel) + tanh over rows of L samples. `prologue` says what its input still
// needs: PRO_NONE — x is lrelu(MRF mean, 0.01) already; PRO_LRELU — x is the MRF mean; PRO_AVG3_LRELU — x, x2, x3 are the ResBlock outputs
// to average (0.01 = F.leaky_relu's default slope before conv_post).
int add_conv_post(Builder& b, const std::string& name, const float* x, const float* x2, const float* x3, int prologue, int L) {
  Slot& s = b.s;
  s.n_samples = L;
  s.audio = b.ar.f32((size_t)b.NB * L);
  if (b.ar.rc) return b.ar.rc;
  b.tap("audio", s.audio, 1, L, L / b.F);  // the waveform rows (a window plan: before the chunk is cut out of them)
  ConvArgs a;
  a.x = x; a.x2 = x2; a.x3 = x3;
  a.prologue = prologue;
  if (prologue != PRO_NONE) a.alpha = 0.01f;
  a.y = s.audio; a.N = b.NB; a.padL = 3; a.Lin = L; a.Lout = L;
  a.len_ptr = b.lensF; a.len_mul = L / b.F;
  a.x_batch_stride = (int64_t)b.v->conv_post.Cin * L; a.y_batch_stride = L; a.y_len = L;
  a.epilogue = EPI_TANH;
  b.conv(name, b.v->conv_post, a, L);
  return PIPER_HIP_OK;
}

// arguments of a 'same'-padded ResBlock conv (kernel K, dilation dil) over rows of Lo positions: fp32 on lrelu(in, 0.1) …
ConvArgs rb_args_f32(const Builder& b, const float* in, const float* res, float* out, int C, int K, int dil, int Lo) {
  ConvArgs a = b.plain(in, out, C, C, Lo, b.lensF, Lo / b.F);
  a.dil = dil; a.padL = (K * dil - dil) / 2; a.prologue = PRO_LRELU; a.alpha = 0.1f; a.res = res;
  return a;
}
// … and bf16 on the C8 image `in` (row positions per channel block) that its producer wrote as lrelu(·, 0.1)
ConvBf16Args rb_args_bf16(const Builder& b, const uint16_t* in, int K, int dil, int Lo, int row) {
  ConvBf16Args a;
  a.x = in; a.N = b.NB; a.dil = dil; a.padL = (K * dil - dil) / 2; a.Lout = Lo; a.x_row = row; a.act_row = row; a.y_len = Lo;
  a.act_alpha = 0.1f;
  a.len_ptr = b.lensF; a.len_mul = Lo / b.F;
  return a;
}

// HiFi-GAN generator with bf16 contraction operands. Same graph as the fp32 generators below;
// what changes is the data each conv READS: the C8 bf16 image of LeakyReLU(x) written by its producer's epilogue
// (conv_bf16.h). The residual stream, the bias adds and the MRF mean stay fp32, so rounding enters only through the
// operands of each contraction and does not accumulate along the residual chain.
int build_generator_bf16(Builder& b, const float* z, float* dec0) {
  piper_hip_voice* v = b.v;
  Slot& s = b.s;
  Arena& ar = b.ar;
  const int F = b.F, NB = b.NB;
  const piper_hip_voice_config& c = v->cfg;
  piper_hip_ctx* ctx = v->ctx;
  const int I = c.inter;
  const size_t B = (size_t)NB;
  hipStream_t zs = s.set.stream;
  static const bool no_par = getenv("PIPER_HIP_BF16_SERIAL_RB") != nullptr;
  const bool no_merge = no_merged_rb();
  // short utterances / small batches: the three ResBlocks advance in one launch; otherwise one launch per conv, as parallel
  // graph branches for the 18-conv ResBlock1 stages (+10 %; the 6-conv ResBlock2 stages do not gain)
  const bool merged = !no_merge && c.n_rb == 3 && (int64_t)NB * F <= 1536;
  s.parallel = !merged && !no_par && c.resblock_type == 1;
  auto image = [&](int C, int L) -> uint16_t* {  // zeroed once per build: kernels write the interior only
    const size_t bytes = (size_t)c8_elems(NB, C, L) * 2;
    void* p = ar.raw(bytes);
    if (p && hipMemsetAsync(p, 0, bytes, zs) != hipSuccess) ar.rc = PIPER_HIP_ERR_LAUNCH;
    return (uint16_t*)p;
  };
  uint16_t* zc8 = image(I, F);
  uint16_t* a_in = image(c.up_initial, F);
  if (ar.rc) return ar.rc;
  {
    const int* lf = b.lensF;
    b.step("dec.z_to_bf16", "", 0, 0, [=](hipStream_t q) { return pack_act_c8(q, z, NB, I, F, 1.0f, zc8, 0, lf); });
  }
  {
    ConvBf16Args a;
    a.x = zc8; a.y = dec0; a.act = a_in; a.act_alpha = 0.1f;  // the first stage's ConvTranspose reads lrelu(conv_pre)
    a.N = NB; a.dil = 1; a.padL = 3; a.Lout = F; a.x_row = (int)c8_row_len(F); a.act_row = (int)c8_row_len(F); a.y_len = F;
    a.len_ptr = b.lensF; a.len_mul = 1;
    b.speaker_bias(a, s.kind == PLAN_GENERATOR ? -1 : v->spk_pre_off);  // x = dec.conv_pre(z) + dec.cond(g), the bias stays fp32
    b.conv_bf16("dec.conv_pre", v->conv_pre_b, a, NB * conv_flops(c.up_initial, I, 7, F));
  }
  b.tap("dec_pre", dec0, c.up_initial, F, 1);
  int L = F;
  const float* mean = nullptr;
  for (int u = 0; u < c.n_ups; u++) {
    const auto& S = v->stages[u];
    const bool last_stage = u + 1 == c.n_ups;
    const int Lo = L * S.stride;
    const int row = (int)c8_row_len(Lo);
    float* up = ar.f32(B * S.Cout * Lo);
    uint16_t* a_up = image(S.Cout, Lo);
    uint16_t* a_next = last_stage ? nullptr : image(S.Cout, Lo);  // lrelu(MRF mean): the next stage's input
    float* m = last_stage ? ar.f32(B * S.Cout * Lo) : nullptr;    // conv_post reads the fp32 mean
    float* r[PIPER_HIP_MAX_RB];
    float* tmp[PIPER_HIP_MAX_RB][2];
    uint16_t* act[PIPER_HIP_MAX_RB][2];
    uint16_t* mid[PIPER_HIP_MAX_RB];
    for (int j = 0; j < c.n_rb; j++) {
      r[j] = ar.f32(B * S.Cout * Lo);
      for (int i = 0; i < 2; i++) {
        tmp[j][i] = ar.f32(B * S.Cout * Lo);
        act[j][i] = image(S.Cout, Lo);
      }
      mid[j] = c.resblock_type == 1 ? image(S.Cout, Lo) : nullptr;
    }
    if (ar.rc) return ar.rc;
    const std::string p = "dec.s" + std::to_string(u) + ".";
    // Read-only taps on the stage's fp32 tensors (tests/test_gpu_bf16_exact.py): names only — no launch, no copy, no buffer. A dilation
    // step that is not the ResBlock's last lands in tmp[j][d & 1] and is registered when no later step overwrites it: the last two
    // of them (every step of the presets' three). The closing step of the last ResBlock has no fp32 tensor of its own on the schedules
    // that fold the MRF mean into its epilogue: there only the mean exists (fp32 in the last stage: "dec.mean"; else the next image).
    auto tap_f32 = [&](const std::string& name, const float* ptr) {
      if (ptr) b.tap(name, ptr, S.Cout, Lo, Lo / F);
    };
    auto tap_step = [&](int j, int di, const float* ptr) {
      if (di + 3 >= c.rb_n_dil) tap_f32(p + "rb" + std::to_string(j) + ".c" + std::to_string(di), ptr);
    };
    tap_f32(p + "up", up);
    if (last_stage) tap_f32("dec.mean", m);
    // the bf16 image of lrelu(MRF mean) that the next stage reads, as raw bits: row cb holds positions × 8 channels × bf16 = 4 floats per position
    if (a_next) b.tap(p + "mean_act", (const float*)a_next + kC8Halo * 4, S.Cout / 8, row * 4, Lo / F * 4);
    {
      ConvBf16Args a;
      a.x = a_in; a.y = up; a.act = a_up; a.act_alpha = 0.1f;
      a.N = NB; a.Lout = L; a.x_row = (int)c8_row_len(L); a.act_row = row; a.y_len = Lo;
      a.ct_stride = S.stride; a.ct_pad = S.pad;
      a.len_ptr = b.lensF; a.len_mul = Lo / F;
      b.conv_bf16(p + "lrelu_convT", v->up_b[u], a, NB * 2.0 * S.Cin * S.Cout * (double)S.K * L);
    }
    if (merged) {
      // conv i of rb0, rb1, rb2 have the same shape and no dependence on each other: one launch advances all three. Only the
      // very last conv of rb2 runs alone, after the others, because its epilogue folds the MRF mean over r0, r1.
      const float* src[3] = {up, up, up};
      const uint16_t* src_act[3] = {a_up, a_up, a_up};
      for (int di = 0; di < c.rb_n_dil; di++) {
        const bool lastd = di + 1 == c.rb_n_dil;
        const std::string nm = p + "rb012.c" + std::to_string(di);
        ConvBf16Args aa[3], bb[3];
        const piper_hip_voice::ConvWB *wa[3], *wb[3];
        double fl[3];
        for (int j = 0; j < 3; j++) {
          const int K = c.rb_kernels[j], dl = c.rb_dilations[j][di];
          fl[j] = NB * conv_flops(S.Cout, S.Cout, K, Lo);
          float* dst = lastd ? (j == 2 ? m : r[j]) : tmp[j][di & 1];
          uint16_t* dst_act = lastd ? (j == 2 ? a_next : nullptr) : act[j][di & 1];
          ConvBf16Args fin = rb_args_bf16(b, c.resblock_type == 1 ? mid[j] : src_act[j], K, c.resblock_type == 1 ? 1 : dl, Lo, row);
          fin.res = src[j]; fin.y = dst; fin.act = dst_act;
          if (lastd && j == 2) { fin.mrf_a = r[0]; fin.mrf_b = r[1]; }
          bb[j] = fin;
          wb[j] = c.resblock_type == 1 ? &v->rb_b[u][j][2 * di + 1] : &v->rb_b[u][j][di];
          if (c.resblock_type == 1) {
            aa[j] = rb_args_bf16(b, src_act[j], K, dl, Lo, row);
            aa[j].act = mid[j];
            wa[j] = &v->rb_b[u][j][2 * di];
          }
          src[j] = dst;
          src_act[j] = dst_act;
          if (!(lastd && j == 2)) tap_step(j, di, dst);
        }
        // ResBlock1 pairs that are not the stage's last: both convs in one launch, intermediate in LDS (rb_pair_bf16.hip)
        const bool no_pair = no_rb_pair();
        if (c.resblock_type == 1 && !no_pair) {
          struct Pack { RbPairBf16Args a[3]; } pk;
          bool ok = true;
          for (int j = 0; j < 3 && ok; j++) {
            RbPairBf16Args& q = pk.a[j];
            q.x = bb[j].res; q.y = bb[j].y;
            // fused pairs stage from the fp32 stream themselves; the stage's last pair writes the next stage's input image, and a
            // pair in front of an UNFUSED one writes the image that one reads
            const bool next_fused = !lastd && rb_pair_bf16_eligible(S.Cout, c.rb_kernels[j], c.rb_dilations[j][di + 1], c.rb_kernels[j], 1, Lo);
            q.act = (lastd || !next_fused) ? bb[j].act : nullptr;
            q.mrf_a = bb[j].mrf_a; q.mrf_b = bb[j].mrf_b;
            q.act_row = row;
            q.wa = wa[j]->w; q.ba = wa[j]->bias; q.wb = wb[j]->w; q.bb = wb[j]->bias;
            q.Ka = wa[j]->K; q.dila = aa[j].dil; q.Kb = wb[j]->K; q.dilb = 1; q.alpha = 0.1f;
            q.N = NB; q.C = S.Cout; q.L = Lo; q.len_ptr = b.lensF; q.len_mul = Lo / F;
            ok = q.x && (q.y || q.act) && q.wa && q.wb && q.ba && q.bb && wa[j]->Cin == S.Cout && wa[j]->Cout == S.Cout && wb[j]->Cin == S.Cout && wb[j]->Cout == S.Cout &&
                 rb_pair_bf16_eligible(S.Cout, q.Ka, q.dila, q.Kb, q.dilb, Lo);
          }
          if (ok) {
            if (lastd) {
              // all three last pairs in one launch (rb2 writes its own fp32 output), then the MRF mean as a small elementwise
              // launch: a single pair of a 128-channel stage is 96 blocks for 256 CUs (52 µs; r3h), the mean 8 µs
              pk.a[2].y = r[2]; pk.a[2].act = nullptr; pk.a[2].mrf_a = nullptr; pk.a[2].mrf_b = nullptr;
              tap_step(2, di, r[2]);
            }
            b.step(nm + "ab_lrelu_conv_lrelu_conv_res_x3", "conv_bf16", 2.0 * (fl[0] + fl[1] + fl[2]), NB * 3 * (2.0 * 4.0 * S.Cout * (double)Lo),
                   [ctx, pk](hipStream_t q) { return launch_rb_pair_bf16_multi(ctx, q, pk.a, 3); });
            if (lastd) {
              const std::string mn = p + "mrf_mean" + (last_stage ? "" : "_lrelu_to_bf16");
              const float *r0 = r[0], *r1 = r[1], *r2 = r[2];
              const int* lf = b.lensF;
              const int Cc = S.Cout, lm = Lo / F;
              if (last_stage)  // conv_post applies its LeakyReLU(0.01) itself: slope 1 here
                add_mrf_mean(b, mn, r0, r1, r2, m, (int64_t)NB * S.Cout * Lo, 1.0f);
              else
                b.step(mn, "", 0, 0, [=](hipStream_t q) { return pack_mean3_c8(q, r0, r1, r2, NB, Cc, Lo, 0.1f, a_next, row, lf, lm); });
            }
            continue;
          }
        }
        if (c.resblock_type == 1) b.conv_bf16_multi(nm + "a_lrelu_conv_x3", wa, aa, 3, fl[0] + fl[1] + fl[2]);
        const std::string bn = c.resblock_type == 1 ? "b" : "";
        if (!lastd) {
          b.conv_bf16_multi(nm + bn + "_lrelu_conv_res_x3", wb, bb, 3, fl[0] + fl[1] + fl[2]);
        } else {
          b.conv_bf16_multi(nm + bn + "_lrelu_conv_res_x2", wb, bb, 2, fl[0] + fl[1]);
          b.conv_bf16_multi(nm + bn + "_lrelu_conv_res_mrfmean", wb + 2, bb + 2, 1, fl[2]);
        }
      }
      a_in = a_next;
      mean = m;
      L = Lo;
      continue;
    }
    // The stage's three ResBlocks are independent chains of short, latency-bound launches that leave most CUs idle:
    // rb0 / rb1 run as side branches of the graph, rb2 on the main lane, joined before rb2's last conv (which folds the
    // MRF mean over all three).
    if (s.parallel) b.fork(p + "fork");
    for (int j = 0; j < c.n_rb; j++) {
      const int K = c.rb_kernels[j];
      const float* src = up;
      const uint16_t* src_act = a_up;
      b.lane = (j + 1 == c.n_rb) ? 0 : j + 1;
      for (int di = 0; di < c.rb_n_dil; di++) {
        const int dil = c.rb_dilations[j][di];
        const bool lastd = di + 1 == c.rb_n_dil;
        const bool fuse_mean = lastd && j + 1 == c.n_rb;  // r0, r1 are complete: fold (r0+r1+r2)/3 into this epilogue
        float* dst = lastd ? (fuse_mean ? m : r[j]) : tmp[j][di & 1];
        uint16_t* dst_act = lastd ? (fuse_mean ? a_next : nullptr) : act[j][di & 1];
        const std::string nm = p + "rb" + std::to_string(j) + ".c" + std::to_string(di);
        auto finish = [&](ConvBf16Args a) {  // the conv that closes the residual: x ← x + conv(…)
          a.res = src; a.y = dst; a.act = dst_act;
          if (fuse_mean) { a.mrf_a = r[0]; a.mrf_b = r[1]; }
          return a;
        };
        const double fl = NB * conv_flops(S.Cout, S.Cout, K, Lo);
        auto join = [&]() {
          if (fuse_mean && s.parallel) b.join(p + "join");
        };
        if (c.resblock_type == 1) {
          ConvBf16Args a1 = rb_args_bf16(b, src_act, K, dil, Lo, row);
          a1.act = mid[j];
          b.conv_bf16(nm + "a_lrelu_conv", v->rb_b[u][j][2 * di], a1, fl);
          join();
          b.conv_bf16(nm + (fuse_mean ? "b_lrelu_conv_res_mrfmean" : "b_lrelu_conv_res"), v->rb_b[u][j][2 * di + 1],
                      finish(rb_args_bf16(b, mid[j], K, 1, Lo, row)), fl);
        } else {
          join();
          b.conv_bf16(nm + (fuse_mean ? "_lrelu_conv_res_mrfmean" : "_lrelu_conv_res"), v->rb_b[u][j][di],
                      finish(rb_args_bf16(b, src_act, K, dil, Lo, row)), fl);
        }
        if (!fuse_mean) tap_step(j, di, dst);
        src = dst;
        src_act = dst_act;
      }
    }
    b.lane = 0;
    a_in = a_next;
    mean = m;
    L = Lo;
  }
  // LeakyReLU(0.01) on the fp32 mean as conv_post's prologue
  return add_conv_post(b, "dec.conv_post_tanh", mean, nullptr, nullptr, PRO_LRELU, L);
}

// fp32 HiFi-GAN generator with the stage's three ResBlocks advanced together: conv i of rb0, rb1, rb2 are independent and
// have the same shape (they differ in kernel size, dilation, weights, buffers), so they run as ONE window-kernel launch
// (launch_conv_win_multi). The MRF mean (r0+r1+r2)/3 is folded into the consumer's staging (ConvTranspose of the next
// stage / conv_post). Medium voice: 23 → 11 generator launches; high: 77 → 29. Returns UNSUPPORTED (nothing scheduled)
// when a conv falls outside the window kernel's geometry, and the caller schedules the per-conv path instead.
int build_generator_merged(Builder& b, float* dec0) {
  piper_hip_voice* v = b.v;
  Arena& ar = b.ar;
  const int F = b.F, NB = b.NB;
  const piper_hip_voice_config& c = v->cfg;
  piper_hip_ctx* ctx = v->ctx;
  const size_t B = (size_t)NB;
  if (c.n_rb != kWinMulti) return PIPER_HIP_ERR_UNSUPPORTED;
  const GenF32Switches& sw = gen_f32_switches();
  {
    int L = F;
    for (int u = 0; u < c.n_ups; u++) {
      const auto& S = v->stages[u];
      const int Lo = L * S.stride;
      for (int j = 0; j < c.n_rb; j++)
        for (const ConvW& w : S.rb[j]) {
          int dmax = 1;
          for (int di = 0; di < c.rb_n_dil; di++) dmax = std::max(dmax, (int)c.rb_dilations[j][di]);
          if (!w.w4 || !conv_win_eligible(w.Cout, w.Cin, w.K, dmax, (w.K * dmax - dmax) / 2, Lo, Lo)) return PIPER_HIP_ERR_UNSUPPORTED;
        }
      L = Lo;
    }
  }
  const float* cur[3] = {dec0, nullptr, nullptr};  // stage input: one tensor, or the three ResBlock outputs to average
  int L = F;
  for (int u = 0; u < c.n_ups; u++) {
    const auto& S = v->stages[u];
    const int Lo = L * S.stride;
    float* up = ar.f32(B * S.Cout * Lo);
    float* buf[kWinMulti][2];
    float* mid[kWinMulti];
    for (int j = 0; j < c.n_rb; j++) {
      buf[j][0] = ar.f32(B * S.Cout * Lo);
      buf[j][1] = ar.f32(B * S.Cout * Lo);
      mid[j] = c.resblock_type == 1 ? ar.f32(B * S.Cout * Lo) : nullptr;
    }
    if (ar.rc) return ar.rc;
    const std::string p = "dec.s" + std::to_string(u) + ".";
    // Read-only taps (tests/test_gpu_f32_exact.py), under the names of build_generator_bf16: names only — no launch, no copy, no buffer.
    // The ping-pong buffers keep the last two ResBlock steps; held[j][i] is the step whose output buf[j][i] holds when the stage has run.
    // A step fused inside a pair launch (ResBlock2: the first of the two) has no tensor and therefore no name.
    auto tap_f32 = [&](const std::string& name, const float* ptr) { b.tap(name, ptr, S.Cout, Lo, Lo / F); };
    int held[kWinMulti][2] = {{-1, -1}, {-1, -1}, {-1, -1}};
    auto holds = [&](float* const y[kWinMulti], int di) {
      for (int j = 0; j < kWinMulti; j++) held[j][y[j] == buf[j][1]] = di;
    };
    tap_f32(p + "up", up);
    // ConvTranspose on lrelu(input) — input = conv_pre output, or the mean of the previous stage's ResBlocks
    add_convt_f32(b, p + (cur[1] ? "mrfmean_lrelu_convT" : "lrelu_convT"), S, cur, 0.1f, up, L);
    const float* src[kWinMulti] = {up, up, up};
    auto add_multi = [&](const std::string& name, const ConvW* ws[kWinMulti], const float* const x[kWinMulti],
                         const float* const res[kWinMulti], float* const y[kWinMulti], const int dil[kWinMulti]) {
      struct Pack { ConvWinArgs a[kWinMulti]; } pk;
      double fl = 0, by = 0;
      double launch_fl = 0;
      for (int j = 0; j < kWinMulti; j++) launch_fl += NB * conv_flops(ws[j]->Cout, ws[j]->Cin, ws[j]->K, Lo);
      bool pipe = sw.pipe_pays(launch_fl, ws[0]->Cin, false);
      for (int j = 0; j < kWinMulti; j++)
        pipe = pipe && ws[j]->w5 && conv_pipe_eligible(ws[j]->Cout, ws[j]->Cin, ws[j]->K, dil[j], (ws[j]->K * dil[j] - dil[j]) / 2, Lo, Lo);
      for (int j = 0; j < kWinMulti; j++) {
        const ConvW& w = *ws[j];
        pk.a[j] = win_args(b, w, x[j], res[j], y[j], dil[j], Lo);
        if (pipe) pk.a[j].w4 = w.w5;
        fl += NB * conv_flops(w.Cout, w.Cin, w.K, Lo);
        by += NB * conv_bytes(w.Cin, w.Cout, w.K, Lo);
      }
      if (pipe) b.step(name, "conv_mfma", fl, by, [ctx, pk](hipStream_t q) { return launch_conv_pipe_multi(ctx, q, pk.a, kWinMulti); });
      else b.step(name, "conv_mfma", fl, by, [ctx, pk](hipStream_t q) { return launch_conv_win_multi(ctx, q, pk.a, kWinMulti); });
    };
    // two chained convs per launch, intermediate in LDS (rb_pair.hip): ResBlock1 — (convs1[di], convs2[di]); ResBlock2 —
    // steps (di, di+1). PIPER_HIP_NO_RB_PAIR=1 keeps the conv-by-conv schedule (A/B). Very short utterances (under 128 frames in the
    // launch: factors 1 and 2) leave the pair kernel's 256-column tiles too few blocks — 41 at factor 1 — and run conv by conv
    // (r2: factor 1 0.649 → 0.620 ms, factor 2 0.670 → 0.659; from factor 4 on the pair kernel wins). PIPER_HIP_RB_PAIR_MIN_F moves it.
    const bool no_pair_env = no_rb_pair();
    static const int64_t pair_min_f = [] { const char* e = getenv("PIPER_HIP_RB_PAIR_MIN_F"); return e ? atoll(e) : 128ll; }();
    const bool no_pair = no_pair_env || (int64_t)F * NB < pair_min_f;
    auto add_pair = [&](const std::string& name, int ia, int ib, const int da[kWinMulti], const int db[kWinMulti], bool res_a, bool res_b_x,
                        const float* const x[kWinMulti], float* const y[kWinMulti]) {
      struct Pack { RbPairArgs a[kWinMulti]; } pk;
      double fl = 0, by = 0;
      for (int j = 0; j < kWinMulti; j++) {
        const ConvW &wa = S.rb[j][ia], &wb = S.rb[j][ib];
        if (no_pair || !wa.w4 || !wb.w4 || !wa.bias || !wb.bias || wa.Cin != wa.Cout || wa.Cin != wb.Cin || wb.Cin != wb.Cout ||
            !rb_pair_eligible(wa.Cin, wa.K, da[j], wb.K, db[j], Lo))
          return false;
        RbPairArgs& a = pk.a[j];
        a.x = x[j]; a.y = y[j]; a.wa4 = wa.w4; a.ba = wa.bias; a.wb4 = wb.w4; a.bb = wb.bias;
        a.Ka = wa.K; a.dila = da[j]; a.Kb = wb.K; a.dilb = db[j]; a.res_a = res_a; a.res_b_x = res_b_x; a.alpha = 0.1f;
        a.N = NB; a.C = wa.Cin; a.L = Lo; a.len_ptr = b.lensF; a.len_mul = Lo / F;
        fl += NB * (conv_flops(wa.Cout, wa.Cin, wa.K, Lo) + conv_flops(wb.Cout, wb.Cin, wb.K, Lo));
        by += NB * 4.0 * (2.0 * wa.Cin * (double)Lo + (double)wa.Cin * wa.Cin * (wa.K + wb.K) + 2.0 * wa.Cin);  // x in, y out, weights
      }
      b.step(name, "conv_mfma", fl, by, [ctx, pk](hipStream_t q) { return launch_rb_pair_multi(ctx, q, pk.a, kWinMulti); });
      return true;
    };
    for (int di = 0; di < c.rb_n_dil; di++) {
      float* dst[kWinMulti];
      int dil[kWinMulti], one[kWinMulti] = {1, 1, 1};
      const float* none[kWinMulti] = {nullptr, nullptr, nullptr};
      for (int j = 0; j < kWinMulti; j++) { dst[j] = src[j] == buf[j][0] ? buf[j][1] : buf[j][0]; dil[j] = c.rb_dilations[j][di]; }  // never the buffer being read
      const std::string nm = p + "rb012.c" + std::to_string(di);
      if (c.resblock_type == 1 && add_pair(nm + "ab_lrelu_conv_lrelu_conv_res_x3", 2 * di, 2 * di + 1, dil, one, false, true, src, dst)) {
        for (int j = 0; j < kWinMulti; j++) src[j] = dst[j];
        holds(dst, di);
        continue;
      }
      if (c.resblock_type == 2 && di + 1 < c.rb_n_dil) {
        int dil2[kWinMulti];
        for (int j = 0; j < kWinMulti; j++) dil2[j] = c.rb_dilations[j][di + 1];
        if (add_pair(p + "rb012.c" + std::to_string(di) + std::to_string(di + 1) + "_lrelu_conv_res_pair_x3", di, di + 1, dil, dil2, true, false, src, dst)) {
          for (int j = 0; j < kWinMulti; j++) src[j] = dst[j];
          di++;
          holds(dst, di);
          continue;
        }
      }
      if (c.resblock_type == 1) {
        const ConvW* wa[kWinMulti] = {&S.rb[0][2 * di], &S.rb[1][2 * di], &S.rb[2][2 * di]};
        const ConvW* wb[kWinMulti] = {&S.rb[0][2 * di + 1], &S.rb[1][2 * di + 1], &S.rb[2][2 * di + 1]};
        const float* midc[kWinMulti] = {mid[0], mid[1], mid[2]};
        add_multi(nm + "a_lrelu_conv_x3", wa, src, none, mid, dil);
        add_multi(nm + "b_lrelu_conv_res_x3", wb, midc, src, dst, one);
      } else {
        const ConvW* w[kWinMulti] = {&S.rb[0][di], &S.rb[1][di], &S.rb[2][di]};
        add_multi(nm + "_lrelu_conv_res_x3", w, src, src, dst, dil);
      }
      for (int j = 0; j < kWinMulti; j++) src[j] = dst[j];
      holds(dst, di);
    }
    for (int j = 0; j < kWinMulti; j++)
      for (int i = 0; i < 2; i++)
        if (held[j][i] >= 0) tap_f32(p + "rb" + std::to_string(j) + ".c" + std::to_string(held[j][i]), buf[j][i]);
    for (int j = 0; j < kWinMulti; j++) cur[j] = src[j];
    L = Lo;
  }
  return add_conv_post(b, "dec.mrfmean_conv_post_tanh", cur[0], cur[1], cur[2], PRO_AVG3_LRELU, L);
}

// fp32 HiFi-GAN generator conv by conv: the stage's ResBlocks as three lanes between a fork and a join, the MRF mean + LeakyReLU folded
// into the stage's very last conv (PIPER_HIP_PARALLEL_RB: a launch of its own after the join).
int build_generator_f32_per_conv(Builder& b, float* dec0) {
  piper_hip_voice* v = b.v;
  Arena& ar = b.ar;
  const int F = b.F, NB = b.NB;
  const piper_hip_voice_config& c = v->cfg;
  piper_hip_ctx* ctx = v->ctx;
  const size_t B = (size_t)NB;
  const GenF32Switches& sw = gen_f32_switches();
  const float* cur[3] = {dec0, nullptr, nullptr};
  bool cur_is_mrf = false;
  int L = F;
  for (int u = 0; u < c.n_ups; u++) {
    const auto& S = v->stages[u];
    const int Lo = L * S.stride;  // (L−1)s − 2·pad + K = L·s for the even (K−s) the config check enforces
    float* up = ar.f32(B * S.Cout * Lo);
    float* r[PIPER_HIP_MAX_RB];
    float* tmp[PIPER_HIP_MAX_RB];
    float* tmp2[PIPER_HIP_MAX_RB];
    float* mid[PIPER_HIP_MAX_RB];
    for (int j = 0; j < c.n_rb; j++) {
      r[j] = ar.f32(B * S.Cout * Lo);
      tmp[j] = ar.f32(B * S.Cout * Lo);
      tmp2[j] = c.rb_n_dil > 2 ? ar.f32(B * S.Cout * Lo) : nullptr;
      mid[j] = c.resblock_type == 1 ? ar.f32(B * S.Cout * Lo) : nullptr;
    }
    if (ar.rc) return ar.rc;
    const std::string p = "dec.s" + std::to_string(u) + ".";
    // the MRF mean kernel already applied LeakyReLU(0.1): slope 1 here
    add_convt_f32(b, p + "lrelu_convT", S, cur, cur_is_mrf ? 1.0f : 0.1f, up, L);
    b.fork(p + "fork");  // the stage's ResBlocks read the same `up` and write disjoint buffers: run them as parallel graph branches
    float* m = ar.f32(B * S.Cout * Lo);  // lrelu(mean of the three ResBlock outputs): input of the next stage
    if (ar.rc) return ar.rc;
    const float mean_alpha = (u + 1 == c.n_ups) ? 0.01f : 0.1f;  // F.leaky_relu default slope before conv_post
    // Read-only taps (tests/test_gpu_f32_exact.py): names only. Every step has a buffer of its own here, except the closing step of the
    // last ResBlock where the mean is folded into its epilogue; "mean_lrelu" is what the next stage (or conv_post) reads:
    // lrelu(MRF mean, 0.1), in the last stage lrelu(MRF mean, 0.01).
    auto tap_f32 = [&](const std::string& name, const float* ptr) { b.tap(name, ptr, S.Cout, Lo, Lo / F); };
    tap_f32(p + "up", up);
    tap_f32(p + "mean_lrelu", m);
    for (int j = 0; j < c.n_rb; j++) {
      b.lane = j < 3 ? j : 0;
      const int K = c.rb_kernels[j];
      const float* src = up;
      for (int di = 0; di < c.rb_n_dil; di++) {
        const int dil = c.rb_dilations[j][di];
        const bool lastd = di + 1 == c.rb_n_dil;
        // the very last conv of the stage folds the MRF mean + LeakyReLU into its epilogue (r0, r1 are complete by then)
        const bool fuse_mean = lastd && j + 1 == c.n_rb && !sw.parallel_rb;
        float* dst = lastd ? (fuse_mean ? m : r[j]) : ((di & 1) ? tmp2[j] : tmp[j]);
        const std::string nm = p + "rb" + std::to_string(j) + ".c" + std::to_string(di);
        if (!fuse_mean && di + 3 >= c.rb_n_dil) tap_f32(nm, dst);  // (tmp / tmp2 keep the last two steps before the closing one)
        auto with_mean = [&](ConvArgs a) {
          if (fuse_mean) {
            a.epilogue = EPI_MRF_MEAN;
            a.mrf_a = r[0]; a.mrf_b = r[1]; a.alpha2 = mean_alpha;
          }
          return a;
        };
        // long rows: the window kernel (conv_win.hip), or the pipe kernel where it pays; otherwise the streaming kernel
        auto add_rb = [&](const std::string& name, const ConvW& w, const ConvArgs& a) {
          if (!(sw.use_win && w.w4 && conv_win_eligible(w.Cout, w.Cin, w.K, a.dil, a.padL, Lo, Lo))) {
            b.conv(name, w, a, Lo);
            return;
          }
          ConvWinArgs wa = win_args(b, w, a.x, a.res, a.y, a.dil, Lo, a.epilogue == EPI_MRF_MEAN ? a.mrf_a : nullptr, a.mrf_b, a.alpha2);
          const double flops = NB * conv_flops(w.Cout, w.Cin, w.K, Lo), bytes = NB * conv_bytes(w.Cin, w.Cout, w.K, Lo);
          if (sw.pipe_pays(flops, w.Cin, false) && w.w5 && conv_pipe_eligible(w.Cout, w.Cin, w.K, a.dil, a.padL, Lo, Lo)) {
            wa.w4 = w.w5;
            b.step(name, "conv_mfma", flops, bytes, [ctx, wa](hipStream_t q) { return launch_conv_pipe_multi(ctx, q, &wa, 1); });
          } else {
            b.step(name, "conv_mfma", flops, bytes, [ctx, wa](hipStream_t q) { return launch_conv_win(ctx, q, wa); });
          }
        };
        if (c.resblock_type == 1) {
          add_rb(nm + "a_lrelu_conv", S.rb[j][2 * di], rb_args_f32(b, src, nullptr, mid[j], S.Cout, K, dil, Lo));
          add_rb(nm + (fuse_mean ? "b_lrelu_conv_res_mrfmean" : "b_lrelu_conv_res"), S.rb[j][2 * di + 1],
                 with_mean(rb_args_f32(b, mid[j], src, dst, S.Cout, K, 1, Lo)));
        } else {
          add_rb(nm + (fuse_mean ? "_lrelu_conv_res_mrfmean" : "_lrelu_conv_res"), S.rb[j][di],
                 with_mean(rb_args_f32(b, src, src, dst, S.Cout, K, dil, Lo)));
        }
        src = dst;
      }
    }
    b.lane = 0;
    b.join(p + "join");
    if (sw.parallel_rb)  // branches finish independently: the mean needs its own launch after the join
      add_mrf_mean(b, p + "mrf_mean_lrelu", r[0], r[1], r[2], m, (int64_t)NB * S.Cout * Lo, mean_alpha);
    cur[0] = m; cur[1] = nullptr; cur[2] = nullptr;
    cur_is_mrf = true;
    L = Lo;
  }
  // LeakyReLU(0.01) of the MRF mean was applied by the mean kernel
  return add_conv_post(b, "dec.conv_post_tanh", cur[0], nullptr, nullptr, PRO_NONE, L);
}

// arena buffers of everything in front of the generator (planned by build_schedule)
struct FrontBuffers {
  float *x, *x1, *qkv, *att, *att_po, *att_pml, *y, *ff, *stats, *zp, *zflip, *zp_tap, *h, *acts, *skip;
  int att_parts;
};

// ---------------- text encoder: embed, the layers, and the projection to m_p / logs_p. for_predictor: the encoder output x must exist in
// memory (the duration predictor reads it), so a LayerNorm folded into its consumer is materialised.
int build_encoder(Builder& b, const FrontBuffers& fb, bool for_predictor) {
  piper_hip_voice* v = b.v;
  Arena& ar = b.ar;
  const int T = b.T, NB = b.NB;
  const int* lensT = b.lensT;
  const piper_hip_voice_config& c = v->cfg;
  piper_hip_ctx* ctx = v->ctx;
  const int H = c.hidden, I = c.inter, d = H / c.n_heads;
  const size_t B = (size_t)NB;
  float *x = fb.x, *x1 = fb.x1, *qkv = fb.qkv, *att = fb.att, *att_po = fb.att_po, *att_pml = fb.att_pml, *y = fb.y, *ff = fb.ff, *stats = fb.stats;
  const int att_parts = fb.att_parts;
  {
    const int64_t* ids = b.s.ids;
    const float* emb = tensor(v, "enc_p.emb.weight");
    const int nv = c.n_vocab;
    const float scale = sqrtf((float)H);
    b.step("embed", "", 0, 0, [=](hipStream_t q) {
      const int grid = (int)std::min<int64_t>(ceil_div((int64_t)H * T, kBlock), 2048);
      hipLaunchKernelGGL(embed_kernel, dim3(grid, NB), dim3(kBlock), 0, q, ids, emb, x, H, T, nv, scale);
      return PIPER_HIP_OK;
    });
  }
  const int kf = c.ffn_kernel;
  // LayerNorms without launches of their own: the conv BEFORE a LayerNorm adds the residual and leaves per-column partial
  // sums (stats_out), the conv AFTER it normalises its input on load (PRO_LN) and writes the normalised tensor once.
  // PIPER_HIP_NO_LN_FUSE=1 keeps the add+LayerNorm kernels (A/B).
  // Above ≈ 640 columns (r2: factor 64 and 8 × factor 8, T·NB = 896: 3.07–3.09 vs 3.10 ms, 2.87 vs 2.90 ms) the normalisation
  // inside the consumers' K loops costs more than the twelve launches it saves; up to T·NB = 448 the fused form wins (factor 8:
  // 0.853 vs 0.879 ms). PIPER_HIP_LN_FUSE_MAX_T moves the crossover.
  static const bool ln_fuse = getenv("PIPER_HIP_NO_LN_FUSE") == nullptr;
  static const int64_t ln_fuse_max_t = [] { const char* e = getenv("PIPER_HIP_LN_FUSE_MAX_T"); return e ? atoll(e) : 640ll; }();
  const bool ln_ok = ln_fuse && (kf == 1 || kf == 3) && v->proj.mfma && H <= 256 && (int64_t)T * NB <= ln_fuse_max_t;
  float* st1 = ln_ok ? ar.f32(B * (size_t)ceil_div(H, 16) * T * 2) : nullptr;
  float* st2 = ln_ok ? ar.f32(B * (size_t)ceil_div(H, 16) * T * 2) : nullptr;
  if (ar.rc) return ar.rc;
  // Round 3: where conv_lean.hip takes all three consumers (qkv, ffn1, proj of one utterance: a block holds every channel of its
  // columns), the CONSUMER computes the LayerNorm statistics of its own operand (ConvArgs::ln_self) and the producers are plain
  // residual adds — no statistics tensor crosses the kernel boundary.
  const bool ln_self = ln_ok && !for_predictor && conv_lean_ln_self_ok(ctx, H, 3 * H, 1, 0, T, NB) && conv_lean_ln_self_ok(ctx, H, c.ffn, kf, (kf - 1) / 2, T, NB) &&
                       conv_lean_ln_self_ok(ctx, H, 2 * I, 1, 0, T, NB);
  auto with_ln = [&](ConvArgs a, const float* stats, const float* g, const float* be, float* normalised) {
    a.prologue = PRO_LN;
    a.ln_stats = ln_self ? nullptr : stats; a.ln_self = ln_self ? 1 : 0;
    a.ln_gamma = g; a.ln_beta = be; a.ln_out = normalised; a.ln_eps = 1e-5f;
    return a;
  };
  auto add_ln = [&](const std::string& nm, const float* a, const float* a2, const float* g, const float* be, float* out) {
    b.step(nm, "add_layernorm", 0, 0, [=](hipStream_t q) {
      float* o = out;
      return piper_hip_add_layernorm_f32(ctx, a, a2, g, be, NB, H, T, 1e-5f, &o, (piper_hip_stream)q);
    });
  };
  for (int l = 0; l < c.n_layers; l++) {
    const auto& L = v->enc[l];
    const std::string p = "enc" + std::to_string(l) + ".";
    if (ln_ok && l > 0)  // x = LN2 of the previous layer, applied to y = x1 + ffn2(…) on load; materialised into x
      b.conv(p + "ln2_qkv", L.qkv, with_ln(b.plain(y, qkv, H, 3 * H, T, lensT), st2, v->enc[l - 1].g2, v->enc[l - 1].b2, x), T);
    else
      b.conv(p + "qkv", L.qkv, b.plain(x, qkv, H, 3 * H, T, lensT), T);
    bool ln1_pending = false;  // LN1 still to be applied by ffn1's prologue (y holds x + conv_o(att), st1 its statistics)
    // mm(2,T,T,96) ×2 + mm(2,T,2T−1,96) ×2
    const double att_flops = NB * 2.0 * c.n_heads * ((double)T * T * d * 2 + (double)T * (2 * T - 1) * d * 2);
    const double att_bytes = NB * 4.0 * c.n_heads * (2.0 * ((double)T * d + (double)d * T + (double)T * T) + 2.0 * ((double)T * d + (double)d * (2 * T - 1) + (double)T * (2 * T - 1)));
    const float *ek = L.ek, *ev = L.ev;
    const int nh = c.n_heads, w = c.window;
    if (L.o.w16 && attention_block_wanted() && attention_block_eligible(c.n_heads, d, c.window, T)) {
      // attention + conv_o + Add + LayerNorm in one launch: the block owns every channel of its 16 columns
      const float *wo = L.o.w16, *bo = L.o.bias, *g1 = L.g1, *b1 = L.b1;
      const int o_nsteps = (int)(packed_conv_floats(H, H, 1, 16) / ((size_t)ceil_div(H, 16) * 64));
      b.step(p + "attention_o_add_ln1", "attention_block", att_flops + NB * conv_flops(H, H, 1, T), att_bytes + NB * conv_bytes(H, H, 1, T),
             [=](hipStream_t q) {
               return launch_attention_block(ctx, q, qkv, qkv + (size_t)H * T, qkv + (size_t)2 * H * T, ek, ev, wo, bo, x, g1, b1, x1, NB, nh, d, T, w,
                                             (int64_t)3 * H * T, (int64_t)H * T, lensT, o_nsteps, 1e-5f);
             });
    } else {
      b.step(p + "rel_attention", "rel_attention", att_flops, att_bytes, [=](hipStream_t q) {
        if (att_parts > 1)
          return launch_rel_attention_split(ctx, q, qkv, qkv + (size_t)H * T, qkv + (size_t)2 * H * T, ek, ev, att, NB, nh, d, T, w,
                                            (int64_t)3 * H * T, (int64_t)H * T, lensT, att_parts, att_po, att_pml);
        return launch_rel_attention(ctx, q, qkv, qkv + (size_t)H * T, qkv + (size_t)2 * H * T, ek, ev, att, NB, nh, d, T, w,
                                    (int64_t)3 * H * T, (int64_t)H * T, lensT);
      });
      if (ln_ok) {  // y = x + conv_o(att) with its LayerNorm statistics; the normalisation itself happens in ffn1's prologue
        ConvArgs a = b.plain(att, y, H, H, T, lensT);
        a.res = x; a.stats_out = ln_self ? nullptr : st1;
        b.conv(p + (ln_self ? "o_add" : "o_add_stats"), L.o, a, T);
        ln1_pending = true;
      } else {
        b.conv(p + "o", L.o, b.plain(att, y, H, H, T, lensT), T);
        add_ln(p + "add_ln1", x, y, L.g1, L.b1, x1);
      }
    }
    {
      ConvArgs a = b.plain(ln1_pending ? y : x1, ff, H, c.ffn, T, lensT);
      a.padL = (kf - 1) / 2;
      if (ln1_pending) a = with_ln(a, st1, L.g1, L.b1, x1);
      a.epilogue = EPI_RELU;
      b.conv(p + (ln1_pending ? "ln1_ffn1_relu" : "ffn1_relu"), L.f1, a, T);
      ConvArgs a2 = b.plain(ff, y, c.ffn, H, T, lensT);
      a2.padL = (kf - 1) / 2;
      if (ln_ok) { a2.res = x1; a2.stats_out = ln_self ? nullptr : st2; }
      b.conv(p + (ln_self ? "ffn2_add" : ln_ok ? "ffn2_add_stats" : "ffn2"), L.f2, a2, T);
    }
    if (!ln_ok) add_ln(p + "add_ln2", x1, y, L.g2, L.b2, x);
  }
  b.tap("enc_out", x, H, T, 0);
  const bool ln2_pending = ln_ok && c.n_layers > 0;  // the last layer's LN2 is still to be applied to y
  if (ln2_pending && for_predictor) add_ln("enc.ln2_final", y, nullptr, v->enc[c.n_layers - 1].g2, v->enc[c.n_layers - 1].b2, x);
  if (ln2_pending && !for_predictor)
    b.conv("enc.ln2_proj", v->proj, with_ln(b.plain(y, stats, H, 2 * I, T, lensT), st2, v->enc[c.n_layers - 1].g2, v->enc[c.n_layers - 1].b2, x), T);
  else
    b.conv("enc.proj", v->proj, b.plain(x, stats, H, 2 * I, T, lensT), T);  // (for the predictor: kept for the plan that continues from here)
  return PIPER_HIP_OK;
}

// ---------------- expansion of m_p / logs_p to frames with the noise, and the flow (reverse). Returns where it leaves z.
const float* build_flow(Builder& b, const FrontBuffers& fb) {
  piper_hip_voice* v = b.v;
  Slot& s = b.s;
  const int T = b.T, F = b.F, NB = b.NB;
  const int* lensF = b.lensF;
  const piper_hip_voice_config& c = v->cfg;
  const int H = c.hidden, I = c.inter;
  float *stats = fb.stats, *zp = fb.zp, *zflip = fb.zflip, *zp_tap = fb.zp_tap, *h = fb.h, *acts = fb.acts, *skip = fb.skip;
  {
    const int32_t* f2i = s.frame2id;
    const float* nz = s.noise;
    const float* nsd = s.noise_scale;
    const unsigned* rngd = s.rng;
    // path expansion counted as the reference's two MatMuls mm(1,F,192,T)
    if (s.pro) {  // a plan of requests with prosody: the noise multiplier per id, read through frame2id (prosody.hip)
      const float* idn = s.pro_noise;
      b.step("expand_noise_prosody", "", NB * 2.0 * 2.0 * F * (double)I * T, NB * 2.0 * 4.0 * ((double)F * T + (double)T * I + (double)F * I),
             [=](hipStream_t q) { return launch_expand_noise_prosody(q, stats, f2i, nz, idn, zp, zp_tap, NB, I, T, F, nsd, rngd, lensF); });
    } else
    b.step("expand_noise", "", NB * 2.0 * 2.0 * F * (double)I * T, NB * 2.0 * 4.0 * ((double)F * T + (double)T * I + (double)F * I), [=](hipStream_t q) {
      const int grid = (int)std::min<int64_t>(ceil_div((int64_t)I * F, kBlock), 4096);
      hipLaunchKernelGGL(expand_noise_kernel, dim3(grid, NB), dim3(kBlock), 0, q, stats, f2i, nz, zp, zp_tap, I, T, F, nsd, rngd, lensF);
      return PIPER_HIP_OK;
    });
  }
  b.tap("z_p", zp_tap, I, F, 1);
  bool flipped = false;
  const int half = I / 2;
  // post of a coupling + x1 − m + Flip + pre of the next one in ONE launch (flow_seam.hip); PIPER_HIP_NO_FLOW_SEAM=1 keeps them apart
  static const bool no_seam = getenv("PIPER_HIP_NO_FLOW_SEAM") != nullptr;
  auto seam_ok = [&](const piper_hip_voice::Coupling& A, const piper_hip_voice::Coupling& B) {
    return !no_seam && I == 2 * half && flow_seam_eligible(H, half) && A.post.w16 && B.pre.w16 && A.post.bias && B.pre.bias && A.post.K == 1 && B.pre.K == 1 &&
           A.post.Cin == H && A.post.Cout == half && B.pre.Cin == half && B.pre.Cout == H;
  };
  // … and with the last WaveNet layer's res_skip conv in front of them multiplied into the same matrix when the voice was created: one
  // lean k = 1 launch per coupling (conv.h: FlowTailArgs). PIPER_HIP_NO_FLOW_FOLD=1 keeps the schedule above.
  static const bool no_fold = getenv("PIPER_HIP_NO_FLOW_FOLD") != nullptr;
  bool fold = !no_fold && c.wn_layers >= 2 && flow_tail_plan_ok(v->ctx, H, half, F, NB);
  for (int f = 0; f < c.n_flows && fold; f++)
    fold = v->flows[f].tail_w && v->flows[f].tail_b && (f == 0 || seam_ok(v->flows[f], v->flows[f - 1]));
  // A folded seam's other row tiles read the old x1 as an operand, so it writes x1new to the OTHER of zp / zflip: the two halves of z
  // (physical channels [0, half) and [half, I)) travel separately. zloc[k] is the buffer half k was last written to.
  float* zloc[2] = {zp, zp};
  for (int f = c.n_flows - 1; f >= 0; f--) {
    flipped = !flipped;
    const auto& C = v->flows[f];
    const std::string p = "flow" + std::to_string(f) + ".";
    const bool pre_done = f + 1 < c.n_flows && (fold || seam_ok(v->flows[f + 1], C));  // the previous (f + 1) coupling's seam already wrote h
    if (!pre_done) {
      ConvArgs a = b.plain(zp, h, I, H, F, lensF);
      a.in_ch_base = flipped ? I - 1 : 0;
      a.in_ch_sign = flipped ? -1 : 1;
      b.conv(p + "pre", C.pre, a, F);
    }
    for (int i = 0; i < c.wn_layers; i++) {
      const bool last = i + 1 == c.wn_layers;
      ConvArgs a = b.plain(h, acts, H, H, F, lensF);
      a.padL = (c.wn_kernel - 1) / 2;
      a.gate = 1;
      b.speaker_bias(a, v->spk_dp_rows + (f * c.wn_layers + i) * 2 * H);  // acts = tanh(a + g_l[:H]) · sigmoid(b + g_l[H:])
      b.conv(p + "wn" + std::to_string(i) + ".in_gate", C.in[i], a, F);
      if (last && fold) break;
      ConvArgs a2 = b.plain(acts, h, H, H, F, lensF);
      a2.y2 = skip; a2.y2_batch_stride = (int64_t)H * F;
      a2.skip = i == 0 ? nullptr : skip;
      if (last) a2.epilogue = EPI_WN_SKIP_LAST;
      else { a2.epilogue = EPI_WN_RES_SKIP; a2.wn_c = H; a2.res = h; }
      b.conv(p + "wn" + std::to_string(i) + ".res_skip", C.rs[i], a2, F);
    }
    const int ob = flipped ? I - 1 - half : half, os = flipped ? -1 : 1;
    // what the graph ops behind a seam / a post_sub cost (the folded launch reports the ops it replaces, not its own matrix)
    const double seam_flops = NB * (conv_flops(half, H, 1, F) + conv_flops(H, half, 1, F));
    const double seam_bytes = NB * 4.0 * ((double)H * F + 2.0 * half * F + (double)H * F + 2.0 * half * H);
    if (fold) {
      const int xh = flipped ? 0 : 1;  // the half of z this coupling's x1 is
      FlowTailArgs t;
      t.acts = acts; t.skip = skip; t.zin = zloc[xh]; t.h = h; t.w = C.tail_w; t.bias = C.tail_b; t.len_ptr = lensF;
      t.N = NB; t.H = H; t.half = half; t.F = F; t.seam = f > 0; t.out_ch_base = ob; t.out_ch_sign = os;
      // a seam: the other buffer. The last coupling reads x1 in its epilogue only: it finishes where the other half already is.
      t.zout = f > 0 ? (zloc[xh] == zp ? zflip : zp) : zloc[1 - xh];
      zloc[xh] = t.zout;
      piper_hip_ctx* ctx = v->ctx;
      const std::string rs = p + "wn" + std::to_string(c.wn_layers - 1) + ".res_skip_";
      const double rs_flops = NB * conv_flops(H, H, 1, F), rs_bytes = NB * conv_bytes(H, H, 1, F);
      if (f > 0) b.step(rs + "post_sub_flip_pre" + std::to_string(f - 1), "conv_mfma", rs_flops + seam_flops, rs_bytes + seam_bytes, [=](hipStream_t q) { return launch_flow_tail(ctx, q, t); });
      else b.step(rs + "post_sub", "conv_mfma", rs_flops + NB * conv_flops(half, H, 1, F), rs_bytes + NB * conv_bytes(H, half, 1, F), [=](hipStream_t q) { return launch_flow_tail(ctx, q, t); });
    } else if (f > 0 && seam_ok(C, v->flows[f - 1])) {
      const auto& Nx = v->flows[f - 1];
      const float *p16 = C.post.w16, *pb = C.post.bias, *q16 = Nx.pre.w16, *qb = Nx.pre.bias;
      const int ps = (int)(packed_conv_floats(half, H, 1, 16) / ((size_t)ceil_div(half, 16) * 64));
      const int qs = (int)(packed_conv_floats(H, half, 1, 16) / ((size_t)ceil_div(H, 16) * 64));
      piper_hip_ctx* ctx = v->ctx;
      b.step(p + "post_sub_flip_pre" + std::to_string(f - 1), "conv_mfma", seam_flops, seam_bytes,
             [=](hipStream_t q) { return launch_flow_seam(ctx, q, skip, zp, h, p16, pb, q16, qb, NB, H, half, F, ps, qs, ob, os, lensF); });
    } else {
      ConvArgs a = b.plain(skip, zp, H, I, F, lensF);
      a.epilogue = EPI_RSUB;
      a.res = zp;
      a.out_ch_base = ob;
      a.out_ch_sign = os;
      b.conv(p + "post_sub", C.post, a, F);
    }
  }
  float *z = zloc[0], *zother = z == zp ? zflip : zp;  // (both halves end in one buffer: the last coupling saw to that)
  if (!flipped) return z;
  // odd number of couplings: materialise the last Flip once
  b.step("flow.final_flip", "", 0, 0, [=](hipStream_t q) {
    const int grid = (int)std::min<int64_t>(ceil_div((int64_t)I * F, kBlock), 4096);
    hipLaunchKernelGGL(flip_channels_kernel, dim3(grid, NB), dim3(kBlock), 0, q, z, zother, I, F);
    return PIPER_HIP_OK;
  });
  return zother;
}

// the duration predictor on the encoder output x [NB][H][T]: → s.dp_dur / "logw" tap
int build_duration_predictor(Builder& b, const float* x) {
  piper_hip_voice* v = b.v;
  Slot& s = b.s;
  Arena& ar = b.ar;
  const int T = b.T, NB = b.NB;
  const piper_hip_voice_config& c = v->cfg;
  piper_hip_ctx* ctx = v->ctx;
  const int H = c.hidden, nbins = c.dp_bins, K = c.dp_kernel;
  const size_t B = (size_t)NB;
  if (!c.dp_present || v->dp.empty()) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "voice has no duration predictor (dp_present = 0): supply durations");
  if (!dds_layer_eligible(H, K)) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "duration predictor: hidden %d / kernel %d not covered", H, K);
  float* a0 = ar.f32(B * H * T);
  float* a1 = ar.f32(B * H * T);
  float* cond = ar.f32(B * H * T);                  // the predictor's conditioning x for the flows
  float* hsp = ar.f32(B * (size_t)(3 * nbins - 1) * T);
  float* z = ar.f32(B * 2 * T);
  float* logw = ar.f32(B * T);
  s.dp_noise = ar.f32(B * 2 * T);
  s.dp_scalars = ar.raw(dp_scalars_bytes(NB));
  s.dp_dur = (int32_t*)ar.raw(B * T * sizeof(int32_t));
  if (ar.rc) return ar.rc;
  const int* lensT = b.lensT;
  auto conv_k1 = [&](const std::string& name, const ConvW& w, const float* in, int64_t in_bs, float* out, const float* res, bool spk = false) {
    ConvArgs a;
    a.x = in; a.y = out; a.N = NB; a.Lin = T; a.Lout = T; a.x_batch_stride = in_bs; a.y_batch_stride = (int64_t)w.Cout * T; a.y_len = T;
    a.len_ptr = lensT; a.res = res;
    if (spk) b.speaker_bias(a, 0);  // x = dp.pre(x) + dp.cond(g): the first rows of the speaker row
    b.conv(name, w, a, T);
  };
  auto dds_stack = [&](const std::string& name, const std::vector<piper_hip_voice::DdsLayer>& layers, float* cur, float* other) {
    // layer i: cur → other, then swap; returns where the result lives
    int dil = 1;
    for (size_t i = 0; i < layers.size(); i++) {
      const auto& L = layers[i];
      const float *src = cur, *dw_w = L.dw_w, *dw_b = L.dw_b, *g1 = L.g1, *b1 = L.b1, *pw = L.pw.w16, *pwb = L.pw.bias, *g2 = L.g2, *b2 = L.b2;
      float* dst = other;
      const int steps = (int)(packed_conv_floats(H, H, 1, 16) / ((size_t)ceil_div(H, 16) * 64));
      const int d2 = dil;
      b.step(name + ".dds" + std::to_string(i), "dds_layer", NB * (conv_flops(H, H, 1, T) + conv_flops(H, 1, K, T)), NB * 4.0 * (2.0 * H * T + (double)H * H),
             [=](hipStream_t q) { return launch_dds_layer(ctx, q, src, dw_w, dw_b, g1, b1, pw, pwb, g2, b2, dst, NB, H, T, K, d2, steps, lensT, 1e-5f); });
      std::swap(cur, other);
      dil *= K;
    }
    return cur;
  };
  // x → pre → DDSConv → proj = the conditioning of every flow
  conv_k1("dp.pre", v->dp[0].pre, x, (int64_t)H * T, a0, nullptr, true);
  float* r = dds_stack("dp", v->dp[0].dds, a0, a1);
  conv_k1("dp.proj", v->dp[0].proj, r, (int64_t)H * T, cond, nullptr);
  const float* nz = s.dp_noise;
  const void* sc = s.dp_scalars;
  b.step("dp.init_latent", "", 0, 0, [=](hipStream_t q) { return launch_dp_init(q, nz, sc, z, NB, T, lensT); });
  for (size_t bi = 1; bi < v->dp.size(); bi++) {
    const auto& Bk = v->dp[bi];
    const std::string p = "dp.flow" + std::to_string(Bk.flow);
    conv_k1(p + ".pre_add_cond", Bk.pre, z, (int64_t)2 * T, a0, cond);  // h = pre(z0) + g: the DDSConv's `x + g`
    float* hr = dds_stack(p, Bk.dds, a0, a1);
    conv_k1(p + ".proj", Bk.proj, hr, (int64_t)H * T, hsp, nullptr);
    const float tb = c.dp_tail_bound, fc = (float)H;
    b.step(p + ".spline_flip", "", 0, 0, [=](hipStream_t q) { return launch_dp_spline(q, hsp, z, NB, T, nbins, tb, fc, lensT); });
  }
  {
    const float *m = v->dp_m, *lg = v->dp_logs;
    int32_t* dur = s.dp_dur;
    if (s.pro) {  // a plan of requests with prosody: length, ceiling and floor per id, and w0 kept for the "dp.w" tap (prosody.hip)
      s.pro_len = ar.f32(B * T);
      s.pro_min = (int32_t*)ar.raw(B * T * sizeof(int32_t));
      s.pro_max = (int32_t*)ar.raw(B * T * sizeof(int32_t));
      s.dp_w = ar.f32(B * T);
      if (ar.rc) return ar.rc;
      const float* pl = s.pro_len;
      const int32_t *pmin = s.pro_min, *pmax = s.pro_max;
      float* w0 = s.dp_w;
      b.step("dp.affine_exp_ceil_prosody", "", 0, 0,
             [=](hipStream_t q) { return launch_dp_final_prosody(q, z, m, lg, sc, pl, pmin, pmax, logw, w0, dur, NB, T, lensT); });
      b.tap("dp.w", s.dp_w, 1, T, 0);
      // the same two buffers as whole bucket rows [T] per item (fixed length, not compacted): what lies past an item's length, which is 0
      b.tap("dp.w.row", s.dp_w, 1, T, -1);
      b.tap("dp.dur.row", (const float*)s.dp_dur, 1, T, -1);
    } else
      b.step("dp.affine_exp_ceil", "", 0, 0, [=](hipStream_t q) { return launch_dp_final(q, z, m, lg, sc, logw, dur, NB, T, lensT); });
  }
  b.tap("logw", logw, 1, T, 0);
  // the predictor's work buffers ("@<step>" selector); dp.dur holds the int32 frames per id as raw bits
  b.tap("dp.a0", a0, H, T, 0);
  b.tap("dp.a1", a1, H, T, 0);
  b.tap("dp.cond", cond, H, T, 0);
  b.tap("dp.hsp", hsp, 3 * nbins - 1, T, 0);
  b.tap("dp.z", z, 2, T, 0);
  b.tap("dp.logw", logw, 1, T, 0);
  b.tap("dp.dur", (const float*)s.dp_dur, 1, T, 0);
  return PIPER_HIP_OK;
}

// Buffer planning, then the builders of what the plan's kind asks for at the voice's precision.
int build_schedule(piper_hip_voice* v, Slot& s, int T, int F, int NB, PlanKind kind = PLAN_WHOLE, bool pro = false) {
  const piper_hip_voice_config& c = v->cfg;
  const int H = c.hidden, I = c.inter;
  const GenF32Switches& sw = gen_f32_switches();
  Builder b(v, s, T, F, NB);
  Arena& ar = b.ar;
  if (c.n_rb != 3) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "voice: n_rb=%d (only the 3-kernel MRF of Piper voices is scheduled)", c.n_rb);
  s.T = T; s.F = F; s.NB = NB;
  s.kind = kind;
  s.pro = pro && kind != PLAN_GENERATOR;  // (a window plan reads latents: nothing of the prosody reaches it)
  s.prec = v->precision;
  s.arena_bytes = 0;
  s.parallel = sw.parallel_rb;
  const size_t B = (size_t)NB;
  s.lensT = (int*)ar.raw(B * sizeof(int));
  s.lensF = (int*)ar.raw(B * sizeof(int));
  if (ar.rc) return ar.rc;
  b.lensT = s.lensT;
  b.lensF = s.lensF;
  if (v->spk.S) {  // a voice with a speaker table (one without allocates and schedules exactly what it did before there were any)
    const SpeakerTables tab = v->spk;
    if (kind == PLAN_GENERATOR) {
      s.spk_bias = ar.f32(B * (size_t)c.up_initial);  // the rows' conv_pre biases, copied in with their latent windows
      if (ar.rc) return ar.rc;
    } else {
      s.spk_in = (piper_hip_speaker*)ar.raw(B * sizeof(piper_hip_speaker));
      s.spk_g = ar.f32(B * (size_t)tab.gin);
      s.spk_bias = ar.f32(B * (size_t)tab.Ctot);
      if (ar.rc) return ar.rc;
      // the predictor plan computes the dp.pre rows, the others the flow and generator rows: nothing is computed twice
      const int row0 = kind == PLAN_PREDICT ? 0 : v->spk_dp_rows, rows = kind == PLAN_PREDICT ? v->spk_dp_rows : tab.Ctot - v->spk_dp_rows;
      const piper_hip_speaker* in = s.spk_in;
      float *g = s.spk_g, *e = s.spk_bias;
      b.step("spk.rows", "speaker", NB * 2.0 * rows * tab.gin, 4.0 * ((double)rows * tab.gin + 2.0 * rows + NB * ((double)rows + 5.0 * tab.gin)),
             [=](hipStream_t q) { return launch_speaker_rows(q, tab, in, NB, row0, rows, g, e); });
      b.tap("spk.g", s.spk_g, 1, tab.gin, -1);
      b.tap("spk.bias", s.spk_bias, 1, tab.Ctot, -1);
    }
  }
  const float* z = nullptr;
  float* dec0 = nullptr;
  if (kind == PLAN_GENERATOR) {  // streaming: only the generator, over a window of the latent that the caller copies into zin
    s.zin = ar.f32(B * (size_t)I * F);
    dec0 = ar.f32(B * (size_t)c.up_initial * F);
    if (ar.rc) return ar.rc;
    z = s.zin;
  } else {
    s.ids = (int64_t*)ar.raw(B * T * sizeof(int64_t));
    s.frame2id = (int32_t*)ar.raw(B * F * sizeof(int32_t));
    s.noise = ar.f32(B * I * F);
    s.noise_scale = ar.f32(B);
    s.rng = (unsigned*)ar.raw(B * 2 * sizeof(unsigned));
    FrontBuffers fb{};
    fb.x = ar.f32(B * (size_t)H * T);
    fb.x1 = ar.f32(B * (size_t)H * T);
    fb.qkv = ar.f32(B * (size_t)3 * H * T);
    fb.att = ar.f32(B * (size_t)H * T);
    // long rows: the attention core runs key-split in two parts plus a merge (attention.hip); scratch for the parts, shared by the layers
    fb.att_parts = rel_attention_split_parts(v->ctx, NB, c.n_heads, H / std::max(1, c.n_heads), T, c.window);
    fb.att_po = fb.att_parts > 1 ? ar.f32(B * (size_t)fb.att_parts * H * T) : nullptr;
    fb.att_pml = fb.att_parts > 1 ? ar.f32(B * (size_t)c.n_heads * fb.att_parts * 2 * T) : nullptr;
    fb.y = ar.f32(B * (size_t)H * T);
    fb.ff = ar.f32(B * (size_t)c.ffn * T);
    fb.stats = ar.f32(B * (size_t)2 * I * T);
    fb.zp = ar.f32(B * (size_t)I * F);
    fb.zflip = ar.f32(B * (size_t)I * F);
    fb.zp_tap = ar.f32(B * (size_t)I * F);
    fb.h = ar.f32(B * (size_t)H * F);
    fb.acts = ar.f32(B * (size_t)H * F);
    fb.skip = ar.f32(B * (size_t)H * F);
    dec0 = ar.f32(B * (size_t)c.up_initial * F);
    if (s.pro && kind != PLAN_PREDICT) {  // (behind everything a plan without prosody allocates)
      s.pro_noise = ar.f32(B * T);
      s.pro_fit = (int32_t*)ar.raw(B * sizeof(int32_t));
    }
    if (ar.rc) return ar.rc;
    s.stats = fb.stats;
    // The front half's work buffers as taps: reused layer after layer, so only meaningful with the "@<step>" selector of piper_hip_voice_tap.
    b.tap("front.x", fb.x, H, T, 0);
    b.tap("front.x1", fb.x1, H, T, 0);
    b.tap("front.qkv", fb.qkv, 3 * H, T, 0);
    b.tap("front.att", fb.att, H, T, 0);
    b.tap("front.y", fb.y, H, T, 0);
    b.tap("front.ff", fb.ff, c.ffn, T, 0);
    b.tap("front.stats", fb.stats, 2 * I, T, 0);
    b.tap("front.zp", fb.zp, I, F, 1);
    b.tap("front.zflip", fb.zflip, I, F, 1);
    b.tap("front.h", fb.h, H, F, 1);
    b.tap("front.acts", fb.acts, H, F, 1);
    b.tap("front.skip", fb.skip, H, F, 1);
    if (kind != PLAN_FROM_STATS) {
      const int rc = build_encoder(b, fb, kind == PLAN_PREDICT);
      if (rc) return rc;
    }
    if (kind == PLAN_PREDICT) return build_duration_predictor(b, fb.x);
    b.tap("m_p", fb.stats, I, T, 0, (size_t)2 * I * T);  // halves of the [2I, T] projection
    b.tap("logs_p", fb.stats + (size_t)I * T, I, T, 0, (size_t)2 * I * T);
    z = s.z_out = build_flow(b, fb);
  }
  b.tap("z", z, I, F, 1);
  if (v->precision == PIPER_HIP_PRECISION_BF16) return build_generator_bf16(b, z, dec0);
  // ---------------- HiFi-GAN generator, fp32
  {
    ConvArgs a = b.plain(z, dec0, I, c.up_initial, F, b.lensF);
    a.padL = 3;
    b.speaker_bias(a, kind == PLAN_GENERATOR ? -1 : v->spk_pre_off);  // x = dec.conv_pre(z) + dec.cond(g)
    b.conv("dec.conv_pre", v->conv_pre, a, F);
  }
  b.tap("dec_pre", dec0, c.up_initial, F, 1);
  const bool no_merge = no_merged_rb();
  // Advancing the three ResBlocks in one launch pays while a single conv cannot fill the chip (short utterances, small
  // batches); with many tiles per conv (NB·F large) the per-conv schedule with the mean fused into its producer is faster
  // (measured at 8 × factor 8: 2 650 vs 2 840 utterances/s).
  // r2t: with two chained convs per launch (rb_pair.hip) the merged schedule is also the faster one for long rows;
  // PIPER_HIP_MERGED_MAX_F restores a frames × batch limit for A/B runs.
  static const int64_t merged_max = [] { const char* e = getenv("PIPER_HIP_MERGED_MAX_F"); return e ? (int64_t)atoll(e) : (int64_t)1 << 40; }();
  if (sw.use_win && !no_merge && !sw.parallel_rb && (int64_t)NB * F <= merged_max) {
    const size_t mark = s.steps.size();
    const int rcm = build_generator_merged(b, dec0);
    if (rcm != PIPER_HIP_ERR_UNSUPPORTED) return rcm;
    s.steps.resize(mark);  // geometry outside the window kernel: schedule conv by conv below
  }
  return build_generator_f32_per_conv(b, dec0);
}

int run_schedule(Slot& s, hipStream_t q, bool parallel) {
  if (parallel) {
    const int rc0 = ensure_side_streams(s);
    if (rc0) return rc0;
  }
  for (auto& st : s.steps) {
    if (st.kind == Step::FORK) {
      if (parallel) {
        PH_HIP(hipEventRecord(s.set.ev_fork, q), PIPER_HIP_ERR_LAUNCH);
        for (int i = 0; i < 2; i++) PH_HIP(hipStreamWaitEvent(s.set.side[i], s.set.ev_fork, 0), PIPER_HIP_ERR_LAUNCH);
      }
      continue;
    }
    if (st.kind == Step::JOIN) {
      if (parallel)
        for (int i = 0; i < 2; i++) {
          PH_HIP(hipEventRecord(s.set.ev_join[i], s.set.side[i]), PIPER_HIP_ERR_LAUNCH);
          PH_HIP(hipStreamWaitEvent(q, s.set.ev_join[i], 0), PIPER_HIP_ERR_LAUNCH);
        }
      continue;
    }
    hipStream_t target = (parallel && st.lane > 0) ? s.set.side[st.lane - 1] : q;
    int rc = st.enqueue(target);
    if (rc) return rc;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "schedule launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

// What `enqueue(q)` issues on q, captured into *g and instantiated into *ge. On failure neither is left behind (both stay null) and the
// error message starts with `what`. `ms` (optional): wall time of the capture [0] and of the instantiate [1].
template <typename Enqueue>
int capture_graph(hipStream_t q, Enqueue&& enqueue, hipGraph_t* g, hipGraphExec_t* ge, const char* what, double* ms = nullptr) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  *g = nullptr;
  *ge = nullptr;
  hipError_t e = hipStreamBeginCapture(q, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "%s: begin capture failed: %s", what, hipGetErrorString(e));
  const int rc = enqueue(q);
  e = hipStreamEndCapture(q, g);
  const auto t1 = clk::now();
  const char* failed = "graph capture";
  if (!rc && e == hipSuccess) {
    e = hipGraphInstantiate(ge, *g, nullptr, nullptr, 0);
    failed = "graph instantiate";
  }
  if (rc || e != hipSuccess) {
    if (*g) (void)hipGraphDestroy(*g);
    *g = nullptr;
    *ge = nullptr;
    if (rc) return rc;
    PH_FAIL(PIPER_HIP_ERR_LAUNCH, "%s: %s failed: %s", what, failed, hipGetErrorString(e));
  }
  if (ms) {
    ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] = std::chrono::duration<double, std::milli>(clk::now() - t1).count();
  }
  return PIPER_HIP_OK;
}

// What every prepare / predict checks on item b of a batch: ids given, 1 ≤ t ≤ 4096 (the --max-phonemes cap, PiperCLI.swift:394), a known
// noise_mode
int check_item(const piper_hip_utterance& u, int b) {
  if (!u.phoneme_ids) PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: null ids", b);
  if (u.t < 1 || u.t > 4096) PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: %d ids outside [1,4096] (PiperCLI.swift:394)", b, u.t);
  if (u.noise_mode != PIPER_HIP_NOISE_INJECTED && u.noise_mode != PIPER_HIP_NOISE_DEVICE)
    PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: unknown noise_mode %d", b, u.noise_mode);
  return PIPER_HIP_OK;
}

// Frames of item b (its ids already checked): the sum of its durations, or −1 when they are to be predicted
int utt_frames(const piper_hip_voice* v, const piper_hip_utterance& u, int b, int64_t* F_out) {
  if (!u.durations) {  // to be predicted: the frame count is not known yet
    if (!v->cfg.dp_present) PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: durations are NULL and the voice has no duration predictor", b);
    // `noise` is [inter, F] and F is what the predictor is about to decide: the caller cannot have sized it, and the ABI carries no
    // size to check it against (in the reference an override tensor brings its shape, TensorValue.swift:4-43)
    if (u.noise)
      PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: noise given but durations are NULL — its [inter, F] shape depends on the predicted durations: call "
                                 "piper_hip_voice_predict_durations first and pass durations + noise, or use noise_mode = DEVICE", b);
    *F_out = -1;
    return PIPER_HIP_OK;
  }
  int64_t F = 0;
  for (int i = 0; i < u.t; i++) {
    if (u.durations[i] < 0) PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: negative duration", b);
    F += u.durations[i];
  }
  if (F < 1) PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: zero frames", b);
  if (F * v->hop > 0x3fffffff / 64) PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: %lld frames too long", b, (long long)F);
  *F_out = F;
  return PIPER_HIP_OK;
}

// The speaker of item i of a prepare on slot id `slot`: entry i of the slot's assignment, its last entry past the end, speaker 0 alone
// without one (piper_hip_voice_slot_speakers)
piper_hip_speaker speaker_of(const piper_hip_voice* v, int slot, int i) {
  const auto& a = v->slot_spk[slot];
  if (a.empty()) {
    piper_hip_speaker d{};
    d.n = 1;
    d.weights[0] = 1.0f;
    return d;
  }
  return a[std::min((size_t)i, a.size() - 1)];
}

// What the host checks of entry i, so that the device never indexes past the table
int check_speaker(const piper_hip_voice* v, const piper_hip_speaker& sp, int i) {
  if (sp.n < 1 || sp.n > 4) PH_FAIL(PIPER_HIP_ERR_ARG, "speaker %d: a mix of %d entries (1 … 4)", i, sp.n);
  for (int k = 0; k < sp.n; k++) {
    if (sp.ids[k] < 0 || sp.ids[k] >= v->spk.S) PH_FAIL(PIPER_HIP_ERR_ARG, "speaker %d: id %d outside the table's %d rows", i, sp.ids[k], v->spk.S);
    if (!std::isfinite(sp.weights[k])) PH_FAIL(PIPER_HIP_ERR_ARG, "speaker %d: weight %d is not finite", i, k);
  }
  return PIPER_HIP_OK;
}

// The speakers of a prepare of n items on slot id `slot` → the plan's input (nothing for a voice without a table), from the slot id's
// page-locked staging on q. The caller has waited for whatever used that staging before.
int stage_speakers(piper_hip_voice* v, int slot, Slot& plan, int n, hipStream_t q) {
  if (!v->spk.S || !plan.spk_in) return PIPER_HIP_OK;
  auto& sg = v->staging[slot];
  if (int rc = sg.h_spk.ensure((size_t)n, 256)) return rc;  // kMaxGroup records, once per slot id
  for (int b = 0; b < n; b++) sg.h_spk[b] = speaker_of(v, slot, b);
  PH_HIP(hipMemcpyAsync(plan.spk_in, sg.h_spk, (size_t)n * sizeof(piper_hip_speaker), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// ids of n utterances → rows of T, zero past each one's end (any legal id)
void pack_ids(const piper_hip_utterance* utts, int n, int T, int64_t* ids) {
  for (int b = 0; b < n; b++) {
    int64_t* row = ids + (size_t)b * T;
    memcpy(row, utts[b].phoneme_ids, (size_t)utts[b].t * sizeof(int64_t));
    std::fill(row + utts[b].t, row + T, (int64_t)0);
  }
}

// The duration predictor's inputs of n utterances: each one's `dp` noise [2, t] in two rows of T (zero past t; all zero without one), and
// its DpScalars. (Device mode draws element (row, t) of the item's OWN [1, 2, T_b] tensor: the kernel indexes the bucket row, so the draw
// index must be remapped when T_b < T — done by generating on the host side of the index: see dp_init_kernel (uses T).)
void pack_dp_inputs(const piper_hip_utterance* utts, int n, int T, float* noise, void* scalars) {
  for (int b = 0; b < n; b++) {
    const piper_hip_utterance& u = utts[b];
    for (int r = 0; r < 2; r++) {
      float* row = noise + ((size_t)b * 2 + r) * T;
      const int given = u.dp_noise ? u.t : 0;
      if (given) memcpy(row, u.dp_noise + (size_t)r * u.t, (size_t)given * sizeof(float));
      std::fill(row + given, row + T, 0.0f);
    }
    dp_scalars_fill(scalars, b, u.noise_w, u.length_scale == 0.0f ? 1.0f : u.length_scale,
                    (!u.dp_noise && u.noise_mode == PIPER_HIP_NOISE_DEVICE) ? 1u : 0u, u.seed);
  }
}

}  // namespace

PH_EXPORT int piper_hip_voice_create(piper_hip_ctx* ctx, const piper_hip_voice_config* cfg, const float* blob, int on_device,
                                     piper_hip_voice** out) {
  PH_CHECK_CTX(ctx);
  if (!out || !blob) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_create: null argument");
  *out = nullptr;
  int rc = validate_config(cfg);
  if (rc) return rc;
  // hidden % 32: the gated convs pair tanh / sigmoid rows in 64-row units of 2·hidden; inter % 32: the couplings work on 16-row tiles of
  // inter / 2 channels (x_low: 48 = 3 tiles)
  if (cfg->hidden % 32 || cfg->inter % 32) PH_FAIL(PIPER_HIP_ERR_SHAPE, "voice: hidden and inter must be multiples of 32");
  PH_HIP(hipSetDevice(ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  std::unique_ptr<piper_hip_voice> v(new piper_hip_voice());
  v->ctx = ctx;
  v->cfg = *cfg;
  v->hop = 1;
  for (int u = 0; u < cfg->n_ups; u++) v->hop *= cfg->up_rates[u];
  IndexOut io{&v->index};
  v->blob_floats = piper_hip_layout_walk(cfg, index_visit, &io);
  void* p = nullptr;
  if ((rc = ctx->pool.alloc(v->blob_floats * sizeof(float), &p))) return rc;
  v->blob = (float*)p;
  v->owned.push_back(p);
  hipStream_t s = ctx->default_stream;
  PH_HIP(hipMemcpyAsync(v->blob, blob, v->blob_floats * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s),
         PIPER_HIP_ERR_LAUNCH);
  // measure, allocate, pack
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);  // pack kernels / the blob copy may still be running on these blocks
    for (void* q : v->owned) (void)ctx->pool.release(q);
    return code;
  };
  Packer dry{v.get(), 0, s};
  compile_weights(v.get(), dry, true, nullptr);
  v->packed_floats = dry.off;
  if ((rc = ctx->pool.alloc(v->packed_floats * sizeof(float), &p))) return fail(rc);
  v->packed = (float*)p;
  v->owned.push_back(p);
  std::vector<float*> qkvb;
  for (int l = 0; l < cfg->n_layers; l++) {
    if ((rc = ctx->pool.alloc((size_t)3 * cfg->hidden * sizeof(float), &p))) return fail(rc);
    v->owned.push_back(p);
    qkvb.push_back((float*)p);
  }
  Packer pk{v.get(), 0, s};
  if ((rc = compile_weights(v.get(), pk, false, &qkvb))) return fail(rc);
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    fail(0);
    PH_FAIL(PIPER_HIP_ERR_LAUNCH, "voice_create: packing failed: %s", hipGetErrorString(e));
  }
  ph::warm_all_modules();  // every translation unit's code object, now instead of under the first request that needs it (common.h)
  // plan memory up front (Pool::reserve): a no-op when the host reserved its own amount before creating the voice
  {
    static const size_t reserve_mb = [] { const char* e = getenv("PIPER_HIP_RESERVE_MB"); return e ? (size_t)atoll(e) : (size_t)8192; }();
    (void)ctx->pool.reserve(reserve_mb << 20);
  }
  // Four stream sets up front: creating a HIP stream costs ≈ 3 ms (8 ms for the first of a process, tools/probe/cold_prepare.py) — paid here,
  // while the voice loads, it is off the first request (first_request_ms 21 → 13 in bench.py). Plans take sets from this list (slot_init)
  // and give them back when they go idle (detach); a voice serving more than four slot ids at once creates the rest on demand.
  // … and the process's first graph capture + instantiate (≈ 8 ms against ≈ 1 ms for later ones: the runtime sets its graph machinery up
  // on first use) on a one-kernel graph, for the same reason. Failure is not fatal.
  if (const hipStream_t q = precreate_sets(v.get(), 4)) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    auto one_kernel = [](hipStream_t q) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, q); return PIPER_HIP_OK; };
    if (capture_graph(q, one_kernel, &g, &ge, "voice_create") == PIPER_HIP_OK) {
      (void)hipGraphLaunch(ge, q);
      (void)hipStreamSynchronize(q);
      (void)hipGraphExecDestroy(ge);
      (void)hipGraphDestroy(g);
    }
    (void)hipGetLastError();
  }
  *out = v.release();
  return PIPER_HIP_OK;
}

// ---- speakers (piper_hip.h "Multi-speaker voices") --------------------------------------------------------------------------------
PH_EXPORT int piper_hip_voice_attach_speakers(piper_hip_voice* v, const piper_hip_speaker_config* scfg, const float* blob, int on_device) {
  if (!v || !blob) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_attach_speakers: null argument");
  int rc = validate_speaker_config(&v->cfg, scfg);
  if (rc) return rc;
  if (v->spk.S) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_attach_speakers: the voice has a speaker table already");
  if (v->planned) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_attach_speakers: the voice has prepared already (attach the table before the first prepare)");
  piper_hip_ctx* ctx = v->ctx;
  const piper_hip_voice_config& c = v->cfg;
  PH_HIP(hipSetDevice(ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  std::map<std::string, piper_tensor_desc> idx;
  IndexOut io{&idx};
  piper_hip_speaker_layout_walk(&c, scfg, index_visit, &io);
  const int gin = scfg->gin, S = scfg->n_speakers, H = c.hidden;
  const int Ctot = (int)piper_hip_speaker_row_floats(&c), dp_rows = (int)piper_hip_speaker_dp_rows(&c);
  void* p = nullptr;
  if ((rc = ctx->pool.alloc(((size_t)S * gin + (size_t)Ctot * gin + 2 * (size_t)Ctot) * sizeof(float), &p))) return rc;
  float* emb = (float*)p;
  float* w = emb + (size_t)S * gin;
  float* bc = w + (size_t)Ctot * gin;
  float* b_own = bc + Ctot;
  const hipStream_t q = ctx->default_stream;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(emb, blob + idx["emb_g.weight"].offset, (size_t)S * gin * sizeof(float), kind, q);
  int row = 0;
  bool missing = false;
  // `rows` rows of the speaker row from here on: the cond conv `cond` (or a slice of it, from cond row `from`) over the conv `own`
  auto put = [&](const std::string& cond, int from, int rows, const std::string& own) {
    const float* ob = tensor(v, own + ".bias");
    if (!ob) { missing = true; return; }
    if (e == hipSuccess) e = hipMemcpyAsync(w + (size_t)row * gin, blob + idx[cond + ".weight"].offset + (size_t)from * gin, (size_t)rows * gin * sizeof(float), kind, q);
    if (e == hipSuccess) e = hipMemcpyAsync(bc + row, blob + idx[cond + ".bias"].offset + from, (size_t)rows * sizeof(float), kind, q);
    if (e == hipSuccess) e = hipMemcpyAsync(b_own + row, ob, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, q);
    row += rows;
  };
  if (dp_rows) put("dp.cond", 0, H, "dp.pre");
  for (int f = 0; f < c.n_flows; f++)
    for (int l = 0; l < c.wn_layers; l++)
      put("flow.flows." + std::to_string(2 * f) + ".enc.cond_layer", 2 * H * l, 2 * H, "flow.flows." + std::to_string(2 * f) + ".enc.in_layers." + std::to_string(l));
  const int pre_off = row;
  put("dec.cond", 0, c.up_initial, "dec.conv_pre");
  if (e == hipSuccess) e = hipStreamSynchronize(q);  // (a host blob may go away when this returns)
  if (e != hipSuccess || missing || row != Ctot) {
    (void)hipStreamSynchronize(q);
    (void)ctx->pool.release(p);
    if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "voice_attach_speakers: %s", hipGetErrorString(e));
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "voice_attach_speakers: the voice lacks a bias the speakers condition");
  }
  v->owned.push_back(p);
  v->spk.emb = emb; v->spk.w = w; v->spk.bc = bc; v->spk.b_own = b_own;
  v->spk.S = S; v->spk.gin = gin; v->spk.Ctot = Ctot;
  v->spk_dp_rows = dp_rows;
  v->spk_pre_off = pre_off;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_num_speakers(const piper_hip_voice* v) { return v ? v->spk.S : 0; }

PH_EXPORT int piper_hip_voice_slot_speakers(piper_hip_voice* v, int slot, const piper_hip_speaker* spk, int n) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (!v->spk.S) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "voice_slot_speakers: the voice has no speaker table (piper_hip_voice_attach_speakers)");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (n < 0 || n > 256 || (n > 0 && !spk)) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_slot_speakers: %d entries (0 … 256)", n);
  for (int i = 0; i < n; i++)
    if (int rc = check_speaker(v, spk[i], i)) return rc;  // (the assignment in place stays on a refusal)
  v->slot_spk[slot].assign(spk, spk + n);
  return PIPER_HIP_OK;
}

// ---- prosody (piper_hip.h "Per-phoneme prosody") ----------------------------------------------------------------------------------
PH_EXPORT int piper_hip_voice_slot_prosody(piper_hip_voice* v, int slot, const piper_hip_prosody* items, int n) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (n < 0 || n > 256 || (n > 0 && !items)) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_slot_prosody: %d entries (0 … 256)", n);
  for (int i = 0; i < n; i++)
    if (int rc = prosody_check_item(&items[i], i)) return rc;  // (the assignment in place stays on a refusal)
  std::vector<piper_hip_voice::Prosody> own((size_t)n);
  for (int i = 0; i < n; i++) {  // the arrays are copied: the caller's memory may go away at once
    const piper_hip_prosody& p = items[i];
    piper_hip_voice::Prosody& o = own[i];
    o.t = p.t;
    o.fit = p.fit != 0;
    if (p.length) o.length.assign(p.length, p.length + p.t);
    if (p.min_frames) o.min_frames.assign(p.min_frames, p.min_frames + p.t);
    if (p.max_frames) o.max_frames.assign(p.max_frames, p.max_frames + p.t);
    if (p.noise) o.noise.assign(p.noise, p.noise + p.t);
  }
  v->slot_pro[slot].swap(own);
  return PIPER_HIP_OK;
}

// ---- per-phoneme volume (piper_hip.h "Per-phoneme volume") ------------------------------------------------------------------------
PH_EXPORT int piper_hip_voice_slot_volume(piper_hip_voice* v, int slot, const piper_hip_volume* items, int n) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (n < 0 || n > 256 || (n > 0 && !items)) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_slot_volume: %d entries (0 … 256)", n);
  for (int i = 0; i < n; i++)
    if (int rc = volume_check_item(&items[i], i)) return rc;  // (the assignment in place stays on a refusal)
  std::vector<piper_hip_voice::Volume> own((size_t)n);
  for (int i = 0; i < n; i++) {  // the arrays are copied: the caller's memory may go away at once
    own[i].t = items[i].t;
    if (items[i].gain) own[i].gain.assign(items[i].gain, items[i].gain + items[i].t);
  }
  v->slot_vol[slot].swap(own);
  return PIPER_HIP_OK;
}

// ---- pitch (piper_hip.h "Pitch") ---------------------------------------------------------------------------------------------------
PH_EXPORT int piper_hip_voice_slot_pitch(piper_hip_voice* v, int slot, const piper_hip_pitch* items, int n) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (n < 0 || n > 256 || (n > 0 && !items)) PH_FAIL(PIPER_HIP_ERR_ARG, "voice_slot_pitch: %d entries (0 … 256)", n);
  for (int i = 0; i < n; i++) {  // (the assignment in place stays on a refusal)
    char who[48];
    snprintf(who, sizeof who, "voice_slot_pitch: entry %d", i);
    uint64_t Q;
    if (int rc = pt_step(who, items[i].semitones, &Q)) return rc;
    if (items[i].keep_tempo != 0 && items[i].keep_tempo != 1)
      PH_FAIL(PIPER_HIP_ERR_ARG, "voice_slot_pitch: entry %d: keep_tempo %d (0 or 1)", i, items[i].keep_tempo);
  }
  v->slot_pt[slot].assign(items, items + n);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_set_precision(piper_hip_voice* v, int precision) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (precision != PIPER_HIP_PRECISION_F32 && precision != PIPER_HIP_PRECISION_BF16)
    PH_FAIL(PIPER_HIP_ERR_ARG, "voice_set_precision: unknown precision %d", precision);
  if (precision == v->precision) return PIPER_HIP_OK;
  piper_hip_ctx* ctx = v->ctx;
  const piper_hip_voice_config& c = v->cfg;
  PH_HIP(hipSetDevice(ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  PH_HIP(hipDeviceSynchronize(), PIPER_HIP_ERR_LAUNCH);
  if (precision == PIPER_HIP_PRECISION_BF16 && v->up_b.empty()) {
    // every generator conv must fall inside the bf16 kernels' geometry; otherwise the voice stays fp32
    if (!conv_bf16_eligible(c.up_initial, c.inter, 7, 1, 3, 3))
      PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "bf16 generator: conv_pre %d→%d not covered", c.inter, c.up_initial);
    size_t elems = packed_conv_bf16_elems(c.up_initial, c.inter, 7);
    for (const auto& S : v->stages) {
      if (!convt_bf16_eligible(S.Cin, S.Cout, S.K, S.stride, S.pad, S.pad, 1, 0))
        PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "bf16 generator: ConvTranspose %d→%d k%d s%d not covered", S.Cin, S.Cout, S.K, S.stride);
      elems += packed_convt_bf16_elems(S.Cin, S.Cout, S.K, S.stride);
      for (int j = 0; j < c.n_rb; j++)
        for (int di = 0; di < c.rb_n_dil; di++) {
          const int K = c.rb_kernels[j], dl = c.rb_dilations[j][di], pad = (K * dl - dl) / 2;
          if (!conv_bf16_eligible(S.Cout, S.Cout, K, dl, pad, pad))
            PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "bf16 generator: ResBlock conv C=%d k%d d%d not covered", S.Cout, K, dl);
          elems += (c.resblock_type == 1 ? 2 : 1) * packed_conv_bf16_elems(S.Cout, S.Cout, K);
        }
    }
    void* p = nullptr;
    int rc = ctx->pool.alloc(elems * 2 + 256 * (size_t)(2 + c.n_ups * (1 + c.n_rb * c.rb_n_dil * 2)), &p);
    if (rc) return rc;
    v->owned.push_back(p);
    uint16_t* cur = (uint16_t*)p;
    hipStream_t q = ctx->default_stream;
    auto take = [&](size_t n) { uint16_t* r = cur; cur += (n + 127) & ~(size_t)127; return r; };
    auto conv = [&](const std::string& prefix, int Cout, int Cin, int K) {
      piper_hip_voice::ConvWB w;
      w.Cout = Cout; w.Cin = Cin; w.K = K;
      uint16_t* img = take(packed_conv_bf16_elems(Cout, Cin, K));
      pack_conv_weights_bf16(q, tensor(v, prefix + ".weight"), Cout, Cin, K, img);
      w.w = img;
      w.bias = tensor(v, prefix + ".bias");
      return w;
    };
    v->conv_pre_b = conv("dec.conv_pre", c.up_initial, c.inter, 7);
    char nm[128];
    for (int u = 0; u < c.n_ups; u++) {
      const auto& S = v->stages[u];
      piper_hip_voice::ConvWB w;
      w.Cout = S.Cout; w.Cin = S.Cin; w.K = S.K;
      uint16_t* img = take(packed_convt_bf16_elems(S.Cin, S.Cout, S.K, S.stride));
      snprintf(nm, sizeof nm, "dec.ups.%d", u);
      pack_convt_weights_bf16(q, tensor(v, std::string(nm) + ".weight"), S.Cin, S.Cout, S.K, S.stride, S.pad, img);
      w.w = img;
      w.bias = tensor(v, std::string(nm) + ".bias");
      v->up_b.push_back(w);
      std::vector<std::vector<piper_hip_voice::ConvWB>> rbs;
      for (int j = 0; j < c.n_rb; j++) {
        std::vector<piper_hip_voice::ConvWB> convs;
        const int rb = u * c.n_rb + j;
        for (int di = 0; di < c.rb_n_dil; di++) {
          if (c.resblock_type == 1) {
            snprintf(nm, sizeof nm, "dec.resblocks.%d.convs1.%d", rb, di);
            convs.push_back(conv(nm, S.Cout, S.Cout, c.rb_kernels[j]));
            snprintf(nm, sizeof nm, "dec.resblocks.%d.convs2.%d", rb, di);
            convs.push_back(conv(nm, S.Cout, S.Cout, c.rb_kernels[j]));
          } else {
            snprintf(nm, sizeof nm, "dec.resblocks.%d.convs.%d", rb, di);
            convs.push_back(conv(nm, S.Cout, S.Cout, c.rb_kernels[j]));
          }
        }
        rbs.push_back(convs);
      }
      v->rb_b.push_back(rbs);
    }
    hipError_t e = hipStreamSynchronize(q);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "voice_set_precision: packing failed: %s", hipGetErrorString(e));
  }
  for (auto& pl : v->plans) slot_release(v, *pl);  // every plan was built for the old precision: the next prepare rebuilds
  v->plans.clear();
  for (auto& at : v->attached) at = nullptr;
  v->precision = precision;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_precision(const piper_hip_voice* v) { return v ? v->precision : -1; }

PH_EXPORT void piper_hip_voice_destroy(piper_hip_voice* v) {
  if (!v) return;
  (void)hipSetDevice(v->ctx->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < kMaxSlots; i++) pool_close(v, i);
  for (auto& pl : v->plans) slot_release(v, *pl);
  for (auto& sg : v->staging) {
    for (hipEvent_t* ev : {&sg.eq_ev, &sg.join_ev})  // the copies queued from h_eq / h_join have run before their buffers go
      if (*ev) { (void)hipEventSynchronize(*ev); (void)hipEventDestroy(*ev); }
    sg.each([](auto& b) { b.release(); });
    for (hipEvent_t e : sg.chunk_ev) (void)hipEventDestroy(e);
  }
  for (auto& st : v->free_sets) destroy_set(st);
  for (void* p : v->owned) (void)v->ctx->pool.release(p);
  for (auto& rt : v->rate_tables) (void)v->ctx->pool.release(rt.second.taps);
  delete v;
}

PH_EXPORT int64_t piper_hip_voice_num_samples(const piper_hip_voice* v, const piper_hip_utterance* u) {
  int64_t F = 0;
  if (!v || !u || !u->phoneme_ids || u->t < 1 || u->t > 4096 || utt_frames(v, *u, 0, &F)) return -1;  // (noise_mode is not looked at)
  if (F < 0) return -2;
  return F * v->hop;
}

namespace {

// Buckets: phoneme rows in steps of 16 (the tile width of the short-row kernels), frame rows in steps of 16 up to 1024 frames
// and 64 beyond (long utterances: ≤ 6 % padding, far fewer distinct graphs).
int bucket_t(int T) { return (int)ceil_div(T, 16) * 16; }
int bucket_f(int F) { return F <= 1024 ? (int)ceil_div(F, 16) * 16 : (int)ceil_div(F, 64) * 64; }

constexpr size_t kPlanCacheMax = 128;                   // default plans kept per voice (r3: 48 → 128; an idle plan holds an arena, no stream) …
constexpr size_t kPlanCacheBytes = (size_t)24 << 30;    // … and arena bytes (of 288 GB): least recently used idle plans go first
// (piper_hip_voice_set_plan_cache changes both per voice)

Slot* slot_plan(const piper_hip_voice* v, int slot) {
  if (!v || slot < 0 || slot >= kMaxSlots) return nullptr;
  Slot* p = v->attached[slot];
  return (p && p->built) ? p : nullptr;
}

// The encoder + predictor plan the "predict:" selectors address for the prepared plan `owner` of slot id `slot`: the plan the slot's last
// prepare ran — the one a bounded prepare left attached to the slot id, else the one prepare_batch remembered if the cache still holds
// it — and only then the first cached plan of the slot's form (with or without prosody), bucket T and batch size. Null: none is cached.
Slot* predict_plan_of(piper_hip_voice* v, int slot, const Slot& owner) {
  auto fits = [&](const Slot* p) {
    return p && p->built && p->kind == PLAN_PREDICT && p->pro == owner.pro && p->T == owner.T && p->NB == owner.NB && p->prec == v->precision;
  };
  if (slot >= 0 && slot < kMaxSlots && fits(v->attached_dp[slot])) return v->attached_dp[slot];
  Slot* first = nullptr;
  for (auto& p : v->plans) {
    if (!fits(p.get())) continue;
    if (p.get() == owner.ran_predict) return p.get();
    if (!first) first = p.get();
  }
  return first;
}

void evict_idle_plans(piper_hip_voice* v) {
  auto total = [&]() { size_t b = 0; for (auto& p : v->plans) b += p->arena_bytes; return b; };
  while (v->plans.size() > v->plan_cache_max || total() > v->plan_cache_bytes) {
    int victim = -1;
    for (int i = 0; i < (int)v->plans.size(); i++)
      if (!v->plans[i]->in_use && (victim < 0 || v->plans[i]->last_use < v->plans[victim]->last_use)) victim = i;
    if (victim < 0) return;  // everything is attached: nothing to evict
    Slot& d = *v->plans[victim];
    if (d.set.stream) (void)hipStreamSynchronize(d.set.stream);
    slot_release(v, d);
    v->plans.erase(v->plans.begin() + victim);
  }
}

// Run a plan once on its stream. A plan that has a graph replays it; a freshly built one runs its schedule eagerly (the answer of
// the request that missed the cache) and captures + instantiates the graph behind that run, so that the next request of the bucket
// replays. The capture enqueues nothing; it and the instantiate are host work that overlaps the eager pass on the GPU.
// `on`: the stream the plan runs on (default: its own). A plan without parallel lanes may run on any stream — the bounded prepare puts
// the predictor plan on the stream of the plan that continues from it, so the two need no event between them.
int launch_plan(piper_hip_voice* v, Slot& s, hipStream_t on = nullptr) {
  const hipStream_t q = on ? on : s.set.stream;
  if (s.exec) {
    PH_HIP(hipGraphLaunch(s.exec, q), PIPER_HIP_ERR_LAUNCH);
    return PIPER_HIP_OK;
  }
  const int rc = run_schedule(s, q, false);
  if (rc) return rc;
  // fp32 generator: parallel ResBlock branches measured SLOWER on hipGraph (fork/join edges cost more than the three
  // short kernels gain), so that graph stays a single chain unless asked otherwise. The bf16 generator's builder decides
  // for itself (s.parallel).
  const bool parallel = s.parallel && !on;
  return capture_graph(q, [&](hipStream_t q) { return run_schedule(s, q, parallel); }, &s.graph, &s.exec, "plan", v->last_build_ms + 4);
}

// An idle plan for (kind, Tb, Fb, NB) at the voice's precision, built (schedule + arena; its graph follows its first run) if
// the cache has none. *built reports whether this call paid for a build ("cold" prepare).
// pro: the plan of requests that carry prosody — a kind of its own in the cache, never handed to a request without (and the other way round).
int acquire_plan(piper_hip_voice* v, PlanKind kind, int Tb, int Fb, int NB, Slot** out, bool* built, bool pro = false) {
  *built = false;
  v->planned = true;
  for (auto& p : v->plans)
    if (!p->in_use && p->built && p->kind == kind && p->pro == pro && p->T == Tb && p->F == Fb && p->NB == NB && p->prec == v->precision) {
      const int rc0 = slot_init(v, *p);  // a plan that went idle gave its stream set back (detach)
      if (rc0) return rc0;
      *out = p.get();
      return PIPER_HIP_OK;
    }
  std::unique_ptr<Slot> np(new Slot());
  using clk = std::chrono::steady_clock;
  auto t_prev = clk::now();
  int phase = 0;
  auto lap = [&]() {  // wall time of the build's phases → piper_hip_voice_last_build_breakdown
    const auto now = clk::now();
    if (phase < 6) v->last_build_ms[phase++] = std::chrono::duration<double, std::milli>(now - t_prev).count();
    t_prev = now;
  };
  int rc = slot_init(v, *np);
  if (rc) { slot_release(v, *np); return rc; }
  lap();
  if ((rc = build_schedule(v, *np, Tb, Fb, NB, kind, pro))) { slot_release(v, *np); return rc; }
  lap();
  Slot& s = *np;
  // a plan may be captured / profiled before every input has been uploaded: give the length arrays and index inputs legal values
  {
    hipLaunchKernelGGL(fill_lens_kernel, dim3((unsigned)ceil_div(NB, 64)), dim3(64), 0, s.set.stream, s.lensT, s.lensF, Tb, Fb, NB);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && s.ids) e = hipMemsetAsync(s.ids, 0, (size_t)NB * Tb * sizeof(int64_t), s.set.stream);
    if (e == hipSuccess && s.frame2id) e = hipMemsetAsync(s.frame2id, 0, (size_t)NB * Fb * sizeof(int32_t), s.set.stream);
    if (e == hipSuccess && s.rng) e = hipMemsetAsync(s.rng, 0, (size_t)NB * 2 * sizeof(unsigned), s.set.stream);
    if (e == hipSuccess && s.dp_scalars) e = hipMemsetAsync(s.dp_scalars, 0, dp_scalars_bytes(NB), s.set.stream);
    if (e == hipSuccess && s.dp_noise) e = hipMemsetAsync(s.dp_noise, 0, (size_t)NB * 2 * Tb * sizeof(float), s.set.stream);
    // speakers: a zeroed record is an empty mix (g = 0); the rows this plan does not compute, and a window plan's rows, read as 0.0
    if (e == hipSuccess && s.spk_in) e = hipMemsetAsync(s.spk_in, 0, (size_t)NB * sizeof(piper_hip_speaker), s.set.stream);
    if (e == hipSuccess && s.spk_g) e = hipMemsetAsync(s.spk_g, 0, (size_t)NB * v->spk.gin * sizeof(float), s.set.stream);
    if (e == hipSuccess && s.spk_bias)
      e = hipMemsetAsync(s.spk_bias, 0, (size_t)NB * (kind == PLAN_GENERATOR ? v->cfg.up_initial : v->spk.Ctot) * sizeof(float), s.set.stream);
    // prosody inputs: neutral (length and noise 1.0f, no floor, no ceiling, no fit)
    const int one_bits = 0x3f800000;
    if (e == hipSuccess && s.pro_len) e = hipMemsetD32Async((hipDeviceptr_t)s.pro_len, one_bits, (size_t)NB * Tb, s.set.stream);
    if (e == hipSuccess && s.pro_noise) e = hipMemsetD32Async((hipDeviceptr_t)s.pro_noise, one_bits, (size_t)NB * Tb, s.set.stream);
    if (e == hipSuccess && s.pro_min) e = hipMemsetAsync(s.pro_min, 0, (size_t)NB * Tb * sizeof(int32_t), s.set.stream);
    if (e == hipSuccess && s.pro_max) e = hipMemsetAsync(s.pro_max, 0, (size_t)NB * Tb * sizeof(int32_t), s.set.stream);
    if (e == hipSuccess && s.pro_fit) e = hipMemsetAsync(s.pro_fit, 0, (size_t)NB * sizeof(int32_t), s.set.stream);
    if (e == hipSuccess) e = stream_wait(s.set.stream);
    if (e != hipSuccess) { slot_release(v, s); PH_FAIL(PIPER_HIP_ERR_LAUNCH, "voice_prepare: arena initialisation failed: %s", hipGetErrorString(e)); }
  }
  lap();
  // No validation pass and no capture here (until round 3 a build ran the schedule once eagerly, waited for it, captured it and
  // instantiated the graph before the caller's inputs were even uploaded: 1–6 ms of GPU time + 0.3 ms on the critical path of the
  // first request of a bucket). The plan's FIRST launch goes out eagerly — that run IS the request's answer — and the graph is
  // captured and instantiated right behind it, host work that overlaps the GPU's (launch_plan).
  s.built = true;
  v->last_build_ms[3] = v->last_build_ms[4] = v->last_build_ms[5] = 0;  // [3] kept for the ABI; [4] / [5]: the plan's first launch
  *out = np.get();
  v->plans.push_back(std::move(np));
  *built = true;
  return PIPER_HIP_OK;
}

// The bounded prepare's encoder + predictor plan of slot id `slot` goes idle (it keeps its stream set, see detach).
void release_dp(piper_hip_voice* v, int slot) {
  if (v->attached_dp[slot]) v->attached_dp[slot]->in_use = false;
  v->attached_dp[slot] = nullptr;
}

void detach(piper_hip_voice* v, int slot) {
  v->windows[slot] = WindowRecord();  // what the slot id streamed is gone with what it held
  Slot* p = v->attached[slot];
  if (!p) return;
  if (p->set.stream) (void)hipStreamSynchronize(p->set.stream);  // its last launch may still be running / reading the inputs
  p->in_use = false;
  reset_stream_state(*p);
  p->bounded_pending = false;
  v->attached[slot] = nullptr;
  release_dp(v, slot);  // ran on p's stream: idle now
  give_back_set(v, *p);
}

// The plan of bucket (kind, T, F, NB) on slot id `slot`: the one attached already if it matches, otherwise the attached one is detached and
// the bucket's plan is taken from the cache (or built) and attached. Then, if `evict`, idle plans beyond the cache's bounds go.
int attach_plan(piper_hip_voice* v, int slot, PlanKind kind, int T, int F, int NB, Slot** out, bool evict = true, bool pro = false) {
  pool_close(v, slot);  // a prepare replaces what the slot id holds, a streaming pool included
  v->windows[slot] = WindowRecord();  // (and the record of its latest stream step)
  Slot* cur = v->attached[slot];
  if (!(cur && cur->built && cur->kind == kind && cur->pro == pro && cur->T == T && cur->F == F && cur->NB == NB && cur->prec == v->precision)) {
    if (cur) detach(v, slot);
    bool built = false;
    const int rc = acquire_plan(v, kind, T, F, NB, &cur, &built, pro);
    if (rc) return rc;
    cur->in_use = true;
    v->attached[slot] = cur;
    if (evict) evict_idle_plans(v);
  }
  *out = cur;
  return PIPER_HIP_OK;
}

}  // namespace

namespace {
// ---- the controls of a staging call: what piper_hip_voice_slot_prosody / _volume / _pitch left pending on its slot id
using ProsodyItems = std::vector<piper_hip_voice::Prosody>;
using VolumeItems = std::vector<piper_hip_voice::Volume>;
using PitchItems = std::vector<piper_hip_pitch>;
struct Controls {
  ProsodyItems pro;
  VolumeItems vol;
  PitchItems pit;
};
// A staging call takes the slot id's assignments, whether or not it goes on to succeed.
Controls take_controls(piper_hip_voice* v, int slot) {
  Controls c;
  if (v && slot >= 0 && slot < kMaxSlots) {
    c.pro.swap(v->slot_pro[slot]);
    c.vol.swap(v->slot_vol[slot]);
    c.pit.swap(v->slot_pt[slot]);
  }
  return c;
}
// The entry points that reach prepare* only behind refusals of their own clear the assignments on every way out.
struct ControlsClear {
  piper_hip_voice* v;
  int slot;
  ~ControlsClear() { (void)take_controls(v, slot); }
};

// ---- prosody (piper_hip.h "Per-phoneme prosody") ----
// What a staging call checks before it stages anything. bounded: the route has a frame bound (fit is allowed).
int check_prosody(const ProsodyItems& pro, const piper_hip_utterance* utts, int n, bool bounded) {
  for (int b = 0; b < n && b < (int)pro.size(); b++) {
    const auto& p = pro[b];
    if (p.t != utts[b].t) PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: its prosody has %d entries, the utterance %d ids", b, p.t, utts[b].t);
    if (utts[b].durations && (!p.length.empty() || !p.min_frames.empty() || !p.max_frames.empty() || p.fit))
      PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: durations are supplied, so length, min_frames, max_frames and fit of its prosody do not apply (the "
                                 "caller owns those durations; noise alone applies)", b);
    if (p.fit && !bounded)
      PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: prosody fit needs a frame bound (prepare_batch_bounded / stream_pool_join_bounded)", b);
  }
  return PIPER_HIP_OK;
}
// The per-id arrays of n items in bucket rows [n][T] (null: not wanted), neutral where an item or a field has none, and fit [n].
void pack_prosody(const ProsodyItems& pro, int n, int T, float* len, int32_t* mn, int32_t* mx, float* noise, int32_t* fit) {
  for (int b = 0; b < n; b++) {
    const piper_hip_voice::Prosody* p = b < (int)pro.size() ? &pro[b] : nullptr;
    for (int t = 0; t < T; t++) {
      const size_t i = (size_t)b * T + t;
      const bool in = p && t < p->t;
      if (len) len[i] = in && !p->length.empty() ? p->length[t] : 1.0f;
      if (mn) mn[i] = in && !p->min_frames.empty() ? p->min_frames[t] : 0;
      if (mx) mx[i] = in && !p->max_frames.empty() ? p->max_frames[t] : 0;
      if (noise) noise[i] = in && !p->noise.empty() ? p->noise[t] : 1.0f;
    }
    if (fit) fit[b] = p ? p->fit : 0;
  }
}
// ---- per-phoneme volume (piper_hip.h "Per-phoneme volume") ----
// What a staging call checks before it stages anything.
int check_volume(const VolumeItems& vol, const piper_hip_utterance* utts, int n) {
  for (int b = 0; b < n && b < (int)vol.size(); b++)
    if (vol[b].t != utts[b].t)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "utterance %d: its volume has %d entries, the utterance %d ids", b, vol[b].t, utts[b].t);
  return PIPER_HIP_OK;
}
// The gains of a request with a volume → the plan's vol_gain [n][T], from the slot id's page-locked staging on the plan's stream (which
// the caller has synchronised: the previous request's copy is done). A request without: the plan has none.
int stage_volume(piper_hip_voice* v, int slot, Slot& s, const VolumeItems& vol, int n, int T, hipStream_t q);

// ---- pitch (piper_hip.h "Pitch") ----
// Streams have no pitch: a stream's staging call with one pending on its slot id refuses, stages nothing and clears it.
int refuse_pitch(piper_hip_voice* v, int slot, const char* who) {
  if (!v || slot < 0 || slot >= kMaxSlots || v->slot_pt[slot].empty()) return PIPER_HIP_OK;
  v->slot_pt[slot].clear();
  PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "%s: slot %d has a pitch pending (piper_hip_voice_slot_pitch), and streams have no pitch: it has been cleared", who, slot);
}
// What a staging call checks before it stages anything, and the tempo: `tempo` receives the utterances with length_scale' = fl(ls·rf)
// on the items that keep theirs (it stays empty where no item does).
int check_pitch(const PitchItems& pit, const piper_hip_utterance* utts, int n, std::vector<piper_hip_utterance>* tempo) {
  for (int b = 0; b < n && b < (int)pit.size(); b++) {
    if (!pit[b].keep_tempo) continue;
    if (utts[b].durations)
      PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: durations are supplied, so keep_tempo of its pitch does not apply (the caller owns those durations)", b);
    uint64_t Q;
    if (int rc = pt_step("pitch", pit[b].semitones, &Q)) return rc;
    if (tempo->empty()) tempo->assign(utts, utts + n);
    const float rf = (float)((double)Q / 4294967296.0);
    const float ls = utts[b].length_scale == 0.0f ? 1.0f : utts[b].length_scale;
    (*tempo)[b].length_scale = ls * rf;
  }
  return PIPER_HIP_OK;
}
// The steps and tables of a request with a pitch → the plan's pt_dev, from the slot id's page-locked staging on the plan's stream (which
// the caller has synchronised: the previous request's copy is done). A request without, or whose entries are all neutral: the plan has none.
int stage_pitch(piper_hip_voice* v, int slot, Slot& s, const PitchItems& pit, int n, hipStream_t q);

// Everything a staging call checks of its controls before it stages anything: prosody, volume, pitch, in that order.
int check_controls(const Controls& ctl, const piper_hip_utterance* utts, int n, bool bounded, std::vector<piper_hip_utterance>* tempo) {
  int rc;
  if ((rc = check_prosody(ctl.pro, utts, n, bounded)) || (rc = check_volume(ctl.vol, utts, n))) return rc;
  return check_pitch(ctl.pit, utts, n, tempo);
}

// ---- the geometry of what a whole-item plan delivers
// Frames of a row of s.audio.
int row_frames(const piper_hip_voice* v, const Slot& s) { return (int)std::min<int64_t>(s.F, s.n_samples / v->hop); }
// Frames item b of the plan delivers when it has `frames` of its own: F' = ceil(N' / hop) under the item's pitch, `frames` without one.
int pitch_frames(const piper_hip_voice* v, const Slot& s, int b, int frames) {
  if (!s.chain.pt_on || s.chain.pt_q[b] == kPtOne) return frames;
  return (int)ceil_div(pt_count((int64_t)frames * v->hop, s.chain.pt_q[b]), v->hop);
}
// Samples item b delivers, under a pitch or not, when it has `frames` of its own, and at its true length (a bounded slot before its
// collect: at its capacity).
int64_t item_samples(const piper_hip_voice* v, const Slot& s, int b, int frames) { return (int64_t)pitch_frames(v, s, b, frames) * v->hop; }
int64_t item_samples(const piper_hip_voice* v, const Slot& s, int b) { return item_samples(v, s, b, s.h_F[b]); }
// Samples the latest collect of slot id `slot` delivered, at the voice's rate or through the resampler `rd`: the programme's count where
// a join reported one, otherwise the items back to back, each at its own true length.
int64_t delivered_samples(const piper_hip_voice* v, int slot, const Slot& s, const RsDesign* rd = nullptr) {
  const auto out_len = [&](int64_t samples) { return rd ? rs_count(*rd, samples) : samples; };
  if (v->slot_jn[slot].on && !s.chain.h_jrep.empty()) return out_len(s.chain.h_jrep[0]);
  int64_t total = 0;
  for (int b = 0; b < s.NB; b++) total += out_len(item_samples(v, s, b));
  return total;
}

// ---- the inputs of a predictor plan (PLAN_PREDICT) of n items in rows of T, in host memory the caller supplies: the bounded prepare its
// slot id's page-locked staging, predict_impl pageable vectors (it has no slot id). spk: null where the caller stages the speakers itself
// (stage_speakers) or the voice has no table; pro: null on a plan without prosody.
struct PredictorInputs {
  int64_t* ids;        // [n][T]
  int* lensT;          // [n]
  float* dp_noise;     // [n][2][T]
  void* dp_scalars;    // dp_scalars_bytes(n)
  const piper_hip_speaker* spk;  // [n]
  int32_t* pro;        // [3][n][T]: length (floats), min_frames, max_frames
};
void pack_predictor_inputs(const piper_hip_utterance* utts, int n, int T, const ProsodyItems* pro, const PredictorInputs& h) {
  pack_ids(utts, n, T, h.ids);
  pack_dp_inputs(utts, n, T, h.dp_noise, h.dp_scalars);
  for (int b = 0; b < n; b++) h.lensT[b] = utts[b].t;
  if (h.pro) pack_prosody(*pro, n, T, (float*)h.pro, h.pro + (size_t)n * T, h.pro + 2 * (size_t)n * T, nullptr, nullptr);
}
// One copy per array to plan dp on q; the first failure is returned and ends it.
hipError_t upload_predictor_inputs(Slot& dp, int n, const PredictorInputs& h, hipStream_t q) {
  const size_t nT = (size_t)n * dp.T;
  hipError_t e = hipMemcpyAsync(dp.ids, h.ids, nT * sizeof(int64_t), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) e = hipMemcpyAsync(dp.lensT, h.lensT, (size_t)n * sizeof(int), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) e = hipMemcpyAsync(dp.dp_noise, h.dp_noise, 2 * nT * sizeof(float), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) e = hipMemcpyAsync(dp.dp_scalars, h.dp_scalars, dp_scalars_bytes(n), hipMemcpyHostToDevice, q);
  if (e == hipSuccess && dp.spk_in && h.spk) e = hipMemcpyAsync(dp.spk_in, h.spk, (size_t)n * sizeof(piper_hip_speaker), hipMemcpyHostToDevice, q);
  if (e == hipSuccess && h.pro) e = hipMemcpyAsync(dp.pro_len, h.pro, nT * sizeof(float), hipMemcpyHostToDevice, q);
  if (e == hipSuccess && h.pro) e = hipMemcpyAsync(dp.pro_min, h.pro + nT, nT * sizeof(int32_t), hipMemcpyHostToDevice, q);
  if (e == hipSuccess && h.pro) e = hipMemcpyAsync(dp.pro_max, h.pro + 2 * nT, nT * sizeof(int32_t), hipMemcpyHostToDevice, q);
  return e;
}

// ---- the whole-plan scalars of a request of n items, at the front of the slot id's h_misc (request_scalars_bytes; what a route keeps
// behind them is its own): rng {drawn on the device?, seed} [n][2], noise_scale [n], lensT [n]. One upload to plan s on q, with zero noise
// for the items that bring none: INJECTED without a tensor.
struct RequestScalars {
  unsigned* rng;
  float* ns;
  int* lensT;
  char* end;  // h + request_scalars_bytes(n)
};
size_t request_scalars_bytes(int n) { return (size_t)n * (2 * sizeof(unsigned) + sizeof(float) + sizeof(int)); }
RequestScalars request_scalars(char* h, int n) {
  unsigned* rng = (unsigned*)h;
  float* ns = (float*)(rng + 2 * (size_t)n);
  int* lensT = (int*)(ns + n);
  return RequestScalars{rng, ns, lensT, (char*)(lensT + n)};
}
int stage_request_scalars(const piper_hip_voice* v, Slot& s, char* h, const piper_hip_utterance* utts, int n, hipStream_t q) {
  const auto [rng, ns, lensT, end] = request_scalars(h, n);
  const size_t row = (size_t)v->cfg.inter * s.F;
  for (int b = 0; b < n; b++) {
    const piper_hip_utterance& u = utts[b];
    rng[2 * b] = (!u.noise && u.noise_mode == PIPER_HIP_NOISE_DEVICE) ? 1u : 0u;
    rng[2 * b + 1] = u.seed;
    ns[b] = u.noise_scale;
    lensT[b] = u.t;
    if (!u.noise && !rng[2 * b]) PH_HIP(hipMemsetAsync(s.noise + b * row, 0, row * sizeof(float), q), PIPER_HIP_ERR_LAUNCH);
  }
  PH_HIP(hipMemcpyAsync(s.rng, rng, 2 * (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipMemcpyAsync(s.noise_scale, ns, (size_t)n * sizeof(float), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipMemcpyAsync(s.lensT, lensT, (size_t)n * sizeof(int), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// The inputs a plan of requests with prosody has of its own, from the front of the slot id's h_pro: the noise multiplier per id [n][T],
// then fit [n] (all zero on a route without a frame bound: check_prosody has refused a fit there).
int stage_prosody_noise(Slot& s, int32_t* h, const ProsodyItems& pro, int n, int T, hipStream_t q) {
  const size_t nT = (size_t)n * T;
  pack_prosody(pro, n, T, nullptr, nullptr, nullptr, (float*)h, h + nT);
  PH_HIP(hipMemcpyAsync(s.pro_noise, h, nT * sizeof(float), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipMemcpyAsync(s.pro_fit, h + nT, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// The host's record of the request just staged on plan s. frames: the items' true frame counts (their durations are utts[b].durations),
// or null — a bounded prepare: the plan's capacity F stands in until collect has the device's answer, at most bounded_cap per item.
// wanted: Σ d of the frame rule per item, or null where the device reports it with the lengths. ran_predict: the predictor plan that ran.
void plan_staged(Slot& s, const piper_hip_utterance* utts, int n, const std::vector<int>* frames, const std::vector<int64_t>* wanted, Slot* ran_predict,
                 int bounded_cap) {
  reset_stream_state(s);
  s.h_T.assign(n, 0);
  s.h_dur.clear();
  for (int b = 0; b < n; b++) {
    s.h_T[b] = utts[b].t;
    if (frames) s.h_dur.insert(s.h_dur.end(), utts[b].durations, utts[b].durations + utts[b].t);
  }
  if (frames) s.h_F = *frames;
  else s.h_F.assign(n, s.F);
  s.h_wanted = wanted ? *wanted : std::vector<int64_t>();
  s.h_fitted.assign(wanted ? n : 0, 0);
  s.ran_predict = ran_predict;
  s.bounded_pending = !frames;
  if (!frames) s.bounded_cap = bounded_cap;
  s.timed = false;
  chain_invalidate(s.chain);
}

// piper_hip_voice_predict_durations, and the predictor pass of a prepare_batch whose items have no durations.
// plan_out (optional): the encoder + predictor plan that ran, left marked in_use so that its m_p / logs_p stay put until the caller
// has enqueued the copy into the plan that continues from them (the caller clears in_use); set on success only
// speakers (optional): [n], one per utterance, checked by the caller; null on a voice with a table = speaker 0 alone
// pro (optional): the request has a prosody: the predictor plan of such requests runs, its per-id inputs staged with the ids
int predict_impl(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int32_t* durations_out, float* logw_out, int max_entries, Slot** plan_out,
                 const piper_hip_speaker* speakers = nullptr, const ProsodyItems* pro = nullptr) {
  if (!v || !utts || !durations_out) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (n < 1 || n > 256) PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch size %d outside [1,256]", n);
  if (!v->cfg.dp_present) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "voice has no duration predictor (dp_present = 0)");
  std::vector<piper_hip_speaker> spk;
  if (v->spk.S) {
    piper_hip_speaker d{};
    d.n = 1;
    d.weights[0] = 1.0f;
    spk.assign((size_t)n, d);
    if (speakers) spk.assign(speakers, speakers + n);
  }
  int Tmax = 0, rc;
  int64_t total = 0;
  for (int b = 0; b < n; b++) {
    if ((rc = check_item(utts[b], b))) return rc;
    Tmax = std::max(Tmax, utts[b].t);
    total += utts[b].t;
  }
  if (max_entries < total) PH_FAIL(PIPER_HIP_ERR_SHAPE, "predict_durations: output holds %d < %lld entries", max_entries, (long long)total);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  const int T = bucket_t(Tmax);
  Slot* pl = nullptr;
  bool built = false;
  if ((rc = acquire_plan(v, PLAN_PREDICT, T, 16, n, &pl, &built, pro != nullptr))) return rc;
  Slot& s = *pl;
  s.in_use = true;
  s.last_use = ++v->use_clock;
  struct Release {  // on every way out but the one that hands the plan on: the plan is idle again, and the cache is brought back to its bounds
    piper_hip_voice* v;
    Slot* pl;
    ~Release() {
      if (pl) pl->in_use = false;
      evict_idle_plans(v);
    }
  } release{v, pl};
  const hipStream_t q = s.set.stream;
  const auto failed = [](hipError_t e) { PH_FAIL(PIPER_HIP_ERR_LAUNCH, "predict_durations: %s", hipGetErrorString(e)); };
  const size_t nT = (size_t)n * T;
  std::vector<int64_t> ids(nT);
  std::vector<int> lens(n);
  std::vector<float> nz(2 * nT);
  std::vector<int32_t> pr(pro ? 3 * nT : 0);
  std::vector<char> sc(dp_scalars_bytes(n));
  const PredictorInputs in{ids.data(), lens.data(), nz.data(), sc.data(), spk.empty() ? nullptr : spk.data(), pro ? pr.data() : nullptr};
  pack_predictor_inputs(utts, n, T, pro, in);
  if (hipError_t e = upload_predictor_inputs(s, n, in, q)) return failed(e);
  if (launch_plan(v, s)) return failed(hipErrorUnknown);
  std::vector<int32_t> dur(nT);
  std::vector<float> lw(logw_out ? nT : 0);
  if (hipError_t e = hipMemcpyAsync(dur.data(), s.dp_dur, dur.size() * sizeof(int32_t), hipMemcpyDeviceToHost, q)) return failed(e);
  if (logw_out)
    if (hipError_t e = hipMemcpyAsync(lw.data(), s.taps["logw"].p, lw.size() * sizeof(float), hipMemcpyDeviceToHost, q)) return failed(e);
  if (hipError_t e = stream_wait(q)) return failed(e);
  if (plan_out) {  // stays in_use: see above
    *plan_out = pl;
    release.pl = nullptr;
  }
  int64_t off = 0;
  for (int b = 0; b < n; b++) {
    memcpy(durations_out + off, dur.data() + (size_t)b * T, (size_t)utts[b].t * sizeof(int32_t));
    if (logw_out) memcpy(logw_out + off, lw.data() + (size_t)b * T, (size_t)utts[b].t * sizeof(float));
    off += utts[b].t;
  }
  return PIPER_HIP_OK;
}
}

PH_EXPORT int piper_hip_voice_prepare_batch(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot) {
  const Controls ctl = take_controls(v, slot);  // this call's, whatever becomes of it (piper_hip_voice_slot_prosody / _volume / _pitch)
  if (!v || !utts) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (n < 1 || n > 256) PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch size %d outside [1,256]", n);
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  // the batch items may differ in length: the plan is the bucket of the longest, each item carries its own true lengths
  int Tmax = 0, rc;
  int64_t Fmax = 0;
  std::vector<int> hF(n);
  const bool has_pro = !ctl.pro.empty();  // the request runs the plans of requests with prosody
  std::vector<piper_hip_utterance> tempo;  // the utterances at length_scale' where a pitch keeps the tempo
  if ((rc = check_controls(ctl, utts, n, false, &tempo))) return rc;
  if (!tempo.empty()) utts = tempo.data();
  std::vector<int64_t> wanted(n, -1);  // Σ d of the frame rule per item (there is no fitting on this route)
  // utterances without durations: run the text encoder + duration predictor first (its own cached plan), then continue with
  // the predicted frames per id exactly as if the caller had supplied them
  std::vector<piper_hip_utterance> resolved;
  std::vector<int32_t> predicted;
  Slot* dp_plan = nullptr;  // the encoder + predictor plan whose m_p / logs_p the main plan continues from (PLAN_FROM_STATS: no second encoder pass)
  struct DpRelease {
    Slot*& p;
    ~DpRelease() { if (p) p->in_use = false; }
  } dp_release{dp_plan};
  {
    bool any_null = false;
    for (int b = 0; b < n; b++) any_null = any_null || (utts[b].phoneme_ids && !utts[b].durations);
    if (any_null) {
      int64_t total = 0;
      for (int b = 0; b < n; b++) {
        if ((rc = check_item(utts[b], b))) return rc;
        if (!utts[b].durations && utts[b].noise)  // the refusal utt_frames makes: here the durations are still NULL, below they are the predicted ones
          PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: noise given but durations are NULL — its [inter, F] shape depends on the predicted durations: call "
                                     "piper_hip_voice_predict_durations first and pass durations + noise, or use noise_mode = DEVICE", b);
        total += utts[b].t;
      }
      predicted.resize((size_t)total);
      std::vector<piper_hip_speaker> spk;  // the predictor is conditioned too: x = dp.pre(x) + dp.cond(g)
      for (int b = 0; b < n && v->spk.S; b++) spk.push_back(speaker_of(v, slot, b));
      if ((rc = predict_impl(v, utts, n, predicted.data(), nullptr, (int)total, &dp_plan, spk.empty() ? nullptr : spk.data(), has_pro ? &ctl.pro : nullptr)))
        return rc;
      resolved.assign(utts, utts + n);
      int64_t off = 0;
      for (int b = 0; b < n; b++) {
        if (!resolved[b].durations) {
          int64_t F = 0;
          for (int t = 0; t < utts[b].t; t++) F += predicted[off + t];
          wanted[b] = F;
          if (F < 1) predicted[off] = 1;  // Piper: y_lengths = clamp_min(Σ w_ceil, 1)
          resolved[b].durations = predicted.data() + off;
        }
        off += utts[b].t;
      }
      utts = resolved.data();
    }
  }
  for (int b = 0; b < n; b++) {
    int64_t Fb = 0;
    if ((rc = check_item(utts[b], b)) || (rc = utt_frames(v, utts[b], b, &Fb))) return rc;
    hF[b] = (int)Fb;
    if (wanted[b] < 0) wanted[b] = Fb;
    Tmax = std::max(Tmax, utts[b].t);
    Fmax = std::max(Fmax, Fb);
  }
  const int T = bucket_t(Tmax), F = bucket_f((int)Fmax), I = v->cfg.inter;
  if ((int64_t)F * v->hop * n > 0x3fffffff) PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch too large");
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  const PlanKind kind = (dp_plan && dp_plan->stats && dp_plan->T == T && dp_plan->NB == n) ? PLAN_FROM_STATS : PLAN_WHOLE;
  Slot* cur = nullptr;
  if ((rc = attach_plan(v, slot, kind, T, F, n, &cur, true, has_pro))) return rc;
  Slot& s = *cur;
  const hipStream_t q = s.set.stream;
  s.last_use = ++v->use_clock;
  // the previous launch on this plan may still be reading the inputs
  PH_HIP(stream_wait(q), PIPER_HIP_ERR_LAUNCH);
  s.bounded_pending = false;
  release_dp(v, slot);
  if (kind == PLAN_FROM_STATS)  // the predictor's plan has finished (predict synchronises): its projection becomes this plan's input
  {
    PH_HIP(hipMemcpyAsync(s.stats, dp_plan->stats, (size_t)n * 2 * I * T * sizeof(float), hipMemcpyDeviceToDevice, q), PIPER_HIP_ERR_LAUNCH);
    // the predictor plan goes back to the cache when this function returns: whatever runs on it next must not overwrite the
    // projection before this copy has read it
    if (!s.ev_in) PH_HIP(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
    PH_HIP(hipEventRecord(s.ev_in, q), PIPER_HIP_ERR_LAUNCH);
    PH_HIP(hipStreamWaitEvent(dp_plan->set.stream, s.ev_in, 0), PIPER_HIP_ERR_LAUNCH);
  }
  plan_staged(s, utts, n, &hF, &wanted, dp_plan, 0);  // (in front of the uploads: a prepare that fails below leaves this request's record)
  // Everything that goes to the device leaves from page-locked memory of the slot id (the plan's stream was synchronised above): an
  // asynchronous copy from PAGEABLE memory makes the runtime pin (or stage) the caller's pages on the spot. The noise tensor is copied into
  // bucket rows here, on the host.
  auto& sg = v->staging[slot];
  bool any_noise = false;
  for (int b = 0; b < n; b++) any_noise = any_noise || utts[b].noise;
  if ((rc = sg.h_ids.ensure((size_t)T * n)) || (rc = sg.h_f2i.ensure((size_t)F * n)) || (rc = sg.h_lens.ensure((size_t)n)) ||
      (any_noise && (rc = sg.h_noise.ensure((size_t)n * I * F))) || (rc = sg.h_misc.ensure(request_scalars_bytes(n))))
    return rc;
  if ((rc = stage_speakers(v, slot, s, n, q)) || (rc = stage_volume(v, slot, s, ctl.vol, n, T, q)) || (rc = stage_pitch(v, slot, s, ctl.pit, n, q)))
    return rc;
  if (s.pro)  // the noise multiplier per id, a plan input like the ids (no fitting on this route)
    if ((rc = sg.h_pro.ensure((size_t)n * T + n)) || (rc = stage_prosody_noise(s, sg.h_pro, ctl.pro, n, T, q))) return rc;
  if ((rc = stage_request_scalars(v, s, sg.h_misc, utts, n, q))) return rc;
  pack_ids(utts, n, T, sg.h_ids);
  for (int b = 0; b < n; b++) {
    const piper_hip_utterance* u = &utts[b];
    const int Tb = u->t, Fb = hF[b];
    sg.h_lens[b] = Fb;
    int f = 0;  // generate_path: frame f belongs to the phoneme whose cumulative duration covers it
    for (int t = 0; t < Tb; t++)
      for (int j = 0; j < u->durations[t]; j++) sg.h_f2i[(size_t)b * F + f++] = t;
    for (; f < F; f++) sg.h_f2i[(size_t)b * F + f] = 0;
    if (!u->noise) continue;
    // noise [I, Fb] → rows of the bucket [I, F]
    float* hb = sg.h_noise + (size_t)b * I * F;
    for (int c = 0; c < I; c++) {
      memcpy(hb + (size_t)c * F, u->noise + (size_t)c * Fb, (size_t)Fb * sizeof(float));
      if (Fb < F) memset(hb + (size_t)c * F + Fb, 0, (size_t)(F - Fb) * sizeof(float));
    }
    PH_HIP(hipMemcpyAsync(s.noise + (size_t)b * I * F, hb, (size_t)I * F * sizeof(float), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  }
  PH_HIP(hipMemcpyAsync(s.ids, sg.h_ids, (size_t)T * n * sizeof(int64_t), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipMemcpyAsync(s.frame2id, sg.h_f2i, (size_t)F * n * sizeof(int32_t), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipMemcpyAsync(s.lensF, sg.h_lens, (size_t)n * sizeof(int), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(stream_wait(q), PIPER_HIP_ERR_LAUNCH);  // noise / scalars come from caller memory
  return slot;
}

namespace {
// generate_path on the device (GraphExecutor runs the exported graph's CumSum / Less / Cast chain): per item, frames per id → the frame
// count (Piper: clamp_min(Σ w_ceil, 1)), clamped to the plan's capacity, and the id every frame belongs to. One block per item; the
// cumulative sums live in LDS (T ≤ 4096), every frame finds its id by bisection. `rep` (host-mapped, may be null) receives
// [n] predicted frame counts BEFORE clamping, then the items' durations at rep + n + b·T.
__global__ __launch_bounds__(256) void dp_paths_kernel(const int32_t* __restrict__ dur, const int* __restrict__ lensT, int T, int F, int cap,
                                                        int32_t* __restrict__ frame2id, int* __restrict__ lensF, int32_t* __restrict__ rep, int n) {
  __shared__ int cum[4096];
  __shared__ int part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = min(lensT[b], T);
  const int per = (T + 255) / 256;  // ids per thread, consecutive
  const int t0 = tid * per;
  int sum = 0;
  for (int i = 0; i < per; i++) {
    const int t = t0 + i;
    const int d = t < Tb ? max(dur[(size_t)b * T + t], 0) : 0;
    if (rep && t < T) rep[n + (size_t)b * T + t] = d;
    sum += d;
    if (t < T) cum[t] = sum;  // within the thread's run
  }
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive scan of the per-thread sums
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int base = tid ? part[tid - 1] : 0;
  for (int i = 0; i < per; i++)
    if (t0 + i < T) cum[t0 + i] += base;
  __syncthreads();
  const int total = part[255];
  const int want = max(total, 1);          // an all-zero prediction still yields one frame (of id 0)
  const int Fv = min(min(want, cap), F);
  if (tid == 0) {
    lensF[b] = Fv;
    if (rep) { rep[b] = want; if (total < 1) rep[n + (size_t)b * T] = 1; }
  }
  for (int f = tid; f < F; f += 256) {
    int id = 0;
    if (f < Fv && f < total) {  // smallest t with cum[t] > f
      int lo = 0, hi = Tb - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > f) hi = mid; else lo = mid + 1;
      }
      id = lo;
    }
    frame2id[(size_t)b * F + f] = id;
  }
}

// The argument refusals of a bounded prepare, in the words of the entry point that makes them: piper_hip_voice_prepare_batch_bounded
// (join = false; it alone checks `slot`, between the batch size and the bound) or stream_pool_join_bounded (join = true), which makes them
// before it looks at or regrows anything of its pool.
int bounded_refusals(const piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot, int max_frames, bool join) {
  const char* who = join ? "stream_pool_join_bounded" : "prepare_batch_bounded";
  if (n < 1 || n > 256) {
    if (join) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_pool_join_bounded: %d items outside [1,256]", n);
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch size %d outside [1,256]", n);
  }
  if (!join && (slot < 0 || slot >= kMaxSlots)) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (max_frames < 1 || (int64_t)max_frames * std::max(v->hop, 1) > 0x3fffffff / 64) PH_FAIL(PIPER_HIP_ERR_SHAPE, "%s: max_frames %d out of range", who, max_frames);
  if (!v->cfg.dp_present)
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "voice has no duration predictor (dp_present = 0): supply durations%s", join ? " (stream_pool_join)" : "");
  for (int b = 0; b < n; b++) {
    if (int rc = check_item(utts[b], b)) return rc;
    if (utts[b].durations || utts[b].noise)
      PH_FAIL(PIPER_HIP_ERR_ARG, "utterance %d: %s predicts the durations and cannot take a host noise tensor (its shape depends on them): pass "
                                 "durations = noise = NULL (noise_mode DEVICE draws it on the device)", b, who);
  }
  return PIPER_HIP_OK;
}

}  // namespace

// Whole utterances with PREDICTED durations and no host round trip between the predictor and the rest: the caller states an upper bound on
// the frames per item; the plan is the bucket of that bound and every kernel masks by the frame count the device decides. One stream carries
// uploads → encoder + predictor → generate_path (dp_paths_kernel) → flow + generator; the host learns the lengths with the waveform (collect).
PH_EXPORT int piper_hip_voice_prepare_batch_bounded(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot, int max_frames) {
  const Controls ctl = take_controls(v, slot);  // this call's, whatever becomes of it (piper_hip_voice_slot_prosody / _volume / _pitch)
  const bool has_pro = !ctl.pro.empty();
  if (!v || !utts) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  int Tmax = 0, rc;
  if ((rc = bounded_refusals(v, utts, n, slot, max_frames, false))) return rc;
  for (int b = 0; b < n; b++) Tmax = std::max(Tmax, utts[b].t);
  std::vector<piper_hip_utterance> tempo;  // the utterances at length_scale' where a pitch keeps the tempo
  if ((rc = check_controls(ctl, utts, n, true, &tempo))) return rc;
  if (!tempo.empty()) utts = tempo.data();
  const int T = bucket_t(Tmax), F = bucket_f(max_frames), I = v->cfg.inter;
  if ((int64_t)F * v->hop * n > 0x3fffffff) PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch too large");
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  Slot* cur = nullptr;
  if ((rc = attach_plan(v, slot, PLAN_FROM_STATS, T, F, n, &cur, false, has_pro))) return rc;
  Slot& s = *cur;
  s.last_use = ++v->use_clock;
  PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);  // the previous request of this slot id: its staging and its predictor plan are idle now
  Slot* dp = v->attached_dp[slot];
  if (dp && !(dp->built && dp->pro == has_pro && dp->T == T && dp->NB == n && dp->prec == v->precision)) {
    release_dp(v, slot);
    dp = nullptr;
  }
  if (!dp) {
    bool built = false;
    if ((rc = acquire_plan(v, PLAN_PREDICT, T, 16, n, &dp, &built, has_pro))) return rc;
    dp->in_use = true;
    v->attached_dp[slot] = dp;
  }
  dp->last_use = s.last_use;
  evict_idle_plans(v);  // only now: neither plan can be evicted between the two acquires
  auto& sg = v->staging[slot];
  const size_t nT = (size_t)n * T;
  if ((rc = sg.h_ids.ensure(nT)) || (rc = sg.h_misc.ensure(request_scalars_bytes(n) + dp_scalars_bytes(n))) || (rc = sg.h_dpn.ensure(2 * nT)) ||
      (rc = sg.h_res.ensure(has_pro ? prosody_report_entries(n, T) : (size_t)n + nT)) || (has_pro && (rc = sg.h_pro.ensure(4 * nT + n))))
    return rc;
  for (int b = 0; b < n; b++) sg.h_res[b] = -1;
  const hipStream_t q = s.set.stream;
  if ((rc = stage_speakers(v, slot, *dp, n, q)) || (rc = stage_speakers(v, slot, s, n, q)) || (rc = stage_volume(v, slot, s, ctl.vol, n, T, q)) ||
      (rc = stage_pitch(v, slot, s, ctl.pit, n, q)))
    return rc;
  // this plan's own inputs: the request scalars, and of a request with prosody the noise multipliers and fit (the front of h_pro)
  if ((rc = stage_request_scalars(v, s, sg.h_misc, utts, n, q)) || (has_pro && (rc = stage_prosody_noise(s, sg.h_pro, ctl.pro, n, T, q)))) return rc;
  // the predictor plan's: lensT is the one of the request scalars, the predictor's own scalars lie behind them, and length, floor and
  // ceiling behind this plan's part of h_pro
  const RequestScalars rq = request_scalars(sg.h_misc, n);
  const PredictorInputs in{sg.h_ids, rq.lensT, sg.h_dpn, rq.end, nullptr, has_pro ? sg.h_pro + nT + n : nullptr};
  pack_predictor_inputs(utts, n, T, &ctl.pro, in);
  PH_HIP(upload_predictor_inputs(*dp, n, in, q), PIPER_HIP_ERR_LAUNCH);
  if ((rc = launch_plan(v, *dp, q))) return rc;
  PH_HIP(hipMemcpyAsync(s.stats, dp->stats, (size_t)n * 2 * I * T * sizeof(float), hipMemcpyDeviceToDevice, q), PIPER_HIP_ERR_LAUNCH);
  int32_t* const rep = sg.h_res.mapped();
  if (!rep) PH_FAIL(PIPER_HIP_ERR_UNAVAILABLE, "prepare_batch_bounded: page-locked memory has no device mapping on this system");
  if (has_pro) {  // generate_path with the fit step (prosody.hip), in the place of dp_paths_kernel
    if ((rc = launch_dp_paths_prosody(q, dp->dp_dur, dp->lensT, s.pro_fit, T, F, std::min(max_frames, F), s.frame2id, s.lensF, rep, n))) return rc;
  } else
    hipLaunchKernelGGL(dp_paths_kernel, dim3(n), dim3(256), 0, q, dp->dp_dur, dp->lensT, T, F, std::min(max_frames, F), s.frame2id, s.lensF, rep, n);
  PH_HIP(hipGetLastError(), PIPER_HIP_ERR_LAUNCH);
  plan_staged(s, utts, n, nullptr, nullptr, nullptr, std::min(max_frames, F));  // (the predictor plan stays attached to the slot id: attached_dp)
  return slot;
}

namespace {
// The copy-out thresholds of piper_hip_voice_collect (the measurements behind them are told there), in bytes on the wire; the 16-bit PCM
// paths (pcm_route / pcm_land) use the same ones: kernel stores or one DMA into page-locked staging up to kPinnedMax, kChunk pieces with
// the host copying behind them up to kChunkedMax, the runtime's own pipelined copy beyond.
constexpr size_t kPinnedMax = (size_t)1 << 20, kChunkedMax = (size_t)16 << 20, kChunk = (size_t)1 << 20;
// The least size, in floats, of a slot id's page-locked landing buffer of the waveform (sg.h_audio): 16 Ki floats = 64 KiB.
constexpr size_t kAudioMinCap = (size_t)16 << 10;

// Did the caller page-lock this destination itself (piper_hip_host_alloc)? Then it takes a DMA or kernel stores directly.
bool is_caller_pinned(const void* host) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, host) == hipSuccess) return at.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  return false;
}

// after the slot's stream has been synchronised: the device's frame counts and durations → h_F / h_dur; an item over the bound is an error
int bounded_finish(piper_hip_voice* v, int slot, Slot& s) {
  const auto& sg = v->staging[slot];
  s.bounded_pending = false;
  s.h_dur.clear();
  s.h_wanted.assign(s.NB, 0);
  s.h_fitted.assign(s.NB, 0);
  // a plan of requests with prosody: behind the durations, the fitted flags and the totals before fitting (dp_paths_prosody_kernel)
  const int32_t* tail = s.pro ? sg.h_res + s.NB + (size_t)s.NB * s.T : nullptr;
  int over = -1;
  for (int b = 0; b < s.NB; b++) {
    const int want = sg.h_res[b];
    if (want < 1) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "bounded utterance %d: the device reported no frame count (was the slot launched?)", b);
    s.h_wanted[b] = tail ? (int64_t)(((uint64_t)(uint32_t)tail[s.NB + 2 * b + 1] << 32) | (uint32_t)tail[s.NB + 2 * b]) : want;
    s.h_fitted[b] = tail ? tail[b] : 0;
    if (want > s.bounded_cap && over < 0) over = b;
    s.h_F[b] = std::min(want, s.bounded_cap);
    const int32_t* d = sg.h_res + s.NB + (size_t)b * s.T;
    s.h_dur.insert(s.h_dur.end(), d, d + s.h_T[b]);
  }
  if (over >= 0)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "bounded utterance %d: the predictor wants %d frames, the caller allowed %d — prepare it again with a larger bound "
                                 "(or without one)", over, sg.h_res[over], s.bounded_cap);
  return PIPER_HIP_OK;
}

// item b of a bounded slot → page-locked host memory at its bucket offset; the length comes from device memory
__global__ __launch_bounds__(256) void copy_out_len_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ lensF, int b, int hop) {
  const int64_t n = (int64_t)lensF[b] * hop;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t n4 = n >> 2;  // hop·F·4 bytes: rows are 16-byte aligned when hop % 4 == 0 (checked by the caller)
  for (int64_t i = tid; i < n4; i += nth) ((float4*)dst)[i] = ((const float4*)src)[i];
  for (int64_t i = (n4 << 2) + tid; i < n; i += nth) dst[i] = src[i];
}
}  // namespace

PH_EXPORT int piper_hip_voice_predict_durations(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int32_t* durations_out, float* logw_out,
                                                int max_entries) {
  return predict_impl(v, utts, n, durations_out, logw_out, max_entries, nullptr);
}
PH_EXPORT int piper_hip_voice_predict_durations_speakers(piper_hip_voice* v, const piper_hip_utterance* utts, int n, const piper_hip_speaker* speakers,
                                                         int32_t* durations_out, float* logw_out, int max_entries) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (speakers) {
    if (!v->spk.S) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "predict_durations_speakers: the voice has no speaker table (piper_hip_voice_attach_speakers)");
    if (n < 1 || n > 256) PH_FAIL(PIPER_HIP_ERR_SHAPE, "batch size %d outside [1,256]", n);
    for (int i = 0; i < n; i++)
      if (int rc = check_speaker(v, speakers[i], i)) return rc;
  }
  return predict_impl(v, utts, n, durations_out, logw_out, max_entries, nullptr, speakers);
}
PH_EXPORT int piper_hip_voice_prepared_samples(const piper_hip_voice* v, int slot, int64_t* per_item, int max_items, int64_t* total) {
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  int64_t sum = 0;
  for (int b = 0; b < p->NB; b++) {
    const int64_t nb = (int64_t)p->h_F[b] * v->hop;
    if (per_item && b < max_items) per_item[b] = nb;
    sum += nb;
  }
  if (total) *total = sum;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_pitch_samples(piper_hip_voice* v, int slot, int64_t* per_item, int max_items, int64_t* total) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  int64_t sum = 0;
  for (int b = 0; b < p->NB; b++) {  // (a bounded slot before collect: h_F is the capacity)
    const int64_t nb = item_samples(v, *p, b);
    if (per_item && b < max_items) per_item[b] = nb;
    sum += nb;
  }
  if (total) *total = sum;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_durations(const piper_hip_voice* v, int slot, int32_t* out, int max_entries, int* n_entries) {
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (n_entries) *n_entries = (int)p->h_dur.size();
  if (out) {
    if (max_entries < (int)p->h_dur.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "durations: buffer too small");
    memcpy(out, p->h_dur.data(), p->h_dur.size() * sizeof(int32_t));
  }
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_prosody_report(const piper_hip_voice* v, int slot, int64_t* wanted_frames, int32_t* fitted, int max_items) {
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (p->bounded_pending || (int)p->h_wanted.size() != p->NB)
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "prosody_report: the slot's frame counts are still on the device (collect first)");
  for (int b = 0; b < p->NB && b < max_items; b++) {
    if (wanted_frames) wanted_frames[b] = p->h_wanted[b];
    if (fitted) fitted[b] = p->h_fitted[b];
  }
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_prepare(piper_hip_voice* v, const piper_hip_utterance* u, int slot) {
  return piper_hip_voice_prepare_batch(v, u, 1, slot);
}

PH_EXPORT int piper_hip_voice_batch_size(const piper_hip_voice* v, int slot) {
  const Slot* p = slot_plan(v, slot);
  return p ? p->NB : 0;
}

PH_EXPORT int piper_hip_voice_set_plan_cache(piper_hip_voice* v, int max_plans, size_t max_bytes) {
  if (!v || max_plans < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "set_plan_cache: need a voice and max_plans >= 1");
  v->plan_cache_max = (size_t)max_plans;
  v->plan_cache_bytes = max_bytes ? max_bytes : kPlanCacheBytes;
  evict_idle_plans(v);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_last_build_breakdown(const piper_hip_voice* v, double out_ms[6]) {
  if (!v || !out_ms) PH_FAIL(PIPER_HIP_ERR_ARG, "last_build_breakdown: null argument");
  for (int i = 0; i < 6; i++) out_ms[i] = v->last_build_ms[i];
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_plan_info(const piper_hip_voice* v, int slot, int32_t* bucket_t_out, int32_t* bucket_f_out, int32_t* cached_plans,
                                        size_t* cached_bytes) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  const Slot* p = slot_plan(v, slot);
  if (bucket_t_out) *bucket_t_out = p ? p->T : 0;
  if (bucket_f_out) *bucket_f_out = p ? p->F : 0;
  if (cached_plans) *cached_plans = (int32_t)v->plans.size();
  if (cached_bytes) {
    size_t b = 0;
    for (auto& pl : v->plans) b += pl->arena_bytes;
    *cached_bytes = b;
  }
  return PIPER_HIP_OK;
}

namespace {
// waveform → page-locked host memory through its device mapping (collect): 16-byte stores where both sides allow, grid-stride
__global__ __launch_bounds__(256) void copy_out_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) ((float4*)dst)[i] = ((const float4*)src)[i];
    for (int64_t i = (n4 << 2) + tid; i < n; i += nth) dst[i] = src[i];
  } else {
    for (int64_t i = tid; i < n; i += nth) dst[i] = src[i];
  }
}

int plan_alloc(piper_hip_voice* v, Slot& s, size_t bytes, void** out);
void plan_free(piper_hip_voice* v, Slot& s, void* p, size_t bytes);

void plan_release(piper_hip_voice* v, Slot& s, PlanBuf& b) {
  if (b.p) plan_free(v, s, b.p, b.bytes);
  b = PlanBuf();
}

// `bytes` at least in buffer `b` of the plan's chain: allocated on first use, replaced where it is too small (nothing on the GPU still
// reads the old one: every collect ends with a wait, and a staging call has waited for the plan's stream). What a stage had computed
// into it is gone then: `*holds`, where given, is cleared.
int plan_ensure(piper_hip_voice* v, Slot& s, PlanBuf& b, size_t bytes, bool* holds = nullptr) {
  if (b.p && b.bytes >= bytes) return PIPER_HIP_OK;
  void* q = nullptr;
  if (int rc = plan_alloc(v, s, bytes, &q)) return rc;
  plan_release(v, s, b);
  b = PlanBuf{q, bytes};
  if (holds) *holds = false;
  return PIPER_HIP_OK;
}

int stage_volume(piper_hip_voice* v, int slot, Slot& s, const VolumeItems& vol, int n, int T, hipStream_t q) {
  s.vol_on = !vol.empty();
  s.chain.shaped_ok = false;
  if (!s.vol_on) return PIPER_HIP_OK;
  auto& sg = v->staging[slot];
  int rc;
  if ((rc = sg.h_vol.ensure((size_t)n * T))) return rc;
  if (!s.vol_gain) {
    void* p = nullptr;
    if ((rc = plan_alloc(v, s, (size_t)s.NB * s.T * sizeof(float), &p))) return rc;
    s.vol_gain = (float*)p;
  }
  for (int b = 0; b < n; b++) {
    const piper_hip_voice::Volume* it = b < (int)vol.size() ? &vol[b] : nullptr;
    for (int t = 0; t < T; t++) sg.h_vol[(size_t)b * T + t] = it && !it->gain.empty() && t < it->t ? it->gain[t] : 1.0f;
  }
  PH_HIP(hipMemcpyAsync(s.vol_gain, sg.h_vol, (size_t)n * T * sizeof(float), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// ---- the output chain of a whole-item plan: one forward walk over its stages (chain_walk)

// The rows a stage reads and the rows it hands on: [NB][row] floats, item b over lensF[b] frames (device memory) of at most F. Every
// stage below takes the view of its predecessor in `c` and leaves its own there; a stage that is off leaves `c` as it is. All launches
// go behind the plan's graph on its stream and read lengths the device holds (plain, ragged and bounded slots alike).
struct Chain {
  const float* audio = nullptr;
  int64_t row = 0;
  const int* lensF = nullptr;
  int F = 0;
};

// The plan's own rows: what the walk starts from, and what a plan without a stage hands to the sinks.
Chain chain_source(const piper_hip_voice* v, const Slot& s) { return Chain{s.audio, s.n_samples, s.lensF, row_frames(v, s)}; }

// Volume — the plan's latest staging carried one: shaped [NB][n_samples], v = x·e per item (include/piper_hip.h "Per-phoneme volume"),
// once per launch, from the frame-to-id map the device holds.
int chain_volume(piper_hip_voice* v, Slot& s, Chain& c) {
  OutputChain& ch = s.chain;
  if (!s.vol_on) return PIPER_HIP_OK;
  if (c.F < 1 || !s.vol_gain || !s.frame2id || !s.lensF) PH_FAIL(PIPER_HIP_ERR_SHAPE, "volume: the slot holds no samples to shape");
  if (int rc = plan_ensure(v, s, ch.shaped, (size_t)s.NB * s.n_samples * sizeof(float), &ch.shaped_ok)) return rc;
  if (!ch.shaped_ok) {
    PH_HIP(launch_volume_items(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, s.frame2id, s.F, s.vol_gain, s.T,
                               ch.shaped.as<float>(), s.n_samples),
           PIPER_HIP_ERR_LAUNCH);
    ch.shaped_ok = true;
  }
  c.audio = ch.shaped.as<float>();
  return PIPER_HIP_OK;
}

int stage_pitch(piper_hip_voice* v, int slot, Slot& s, const PitchItems& pit, int n, hipStream_t q) {
  OutputChain& ch = s.chain;
  ch.pt_on = false;
  ch.pitched_ok = false;
  ch.pt_q.assign((size_t)s.NB, kPtOne);
  ch.pt_qmin = ch.pt_qmax = kPtOne;
  ch.pt_pmax = 0;
  std::vector<const PtDesign*> tabs;  // one per distinct step of the batch
  int rc;
  for (int b = 0; b < n && b < (int)pit.size(); b++) {
    uint64_t Q;
    if ((rc = pt_step("pitch", pit[b].semitones, &Q))) return rc;
    if (Q == kPtOne) continue;  // not a filter: the item has no pitch
    ch.pt_q[b] = Q;
    ch.pt_qmin = std::min(ch.pt_qmin, Q);
    ch.pt_qmax = std::max(ch.pt_qmax, Q);
    const PtDesign* d = nullptr;
    if ((rc = pt_design(Q, &d))) return rc;
    ch.pt_pmax = std::max(ch.pt_pmax, d->P);
    if (std::find(tabs.begin(), tabs.end(), d) == tabs.end()) tabs.push_back(d);
  }
  if (tabs.empty()) return PIPER_HIP_OK;
  const size_t head = ((size_t)s.NB * sizeof(PtItem) + 15) & ~(size_t)15;
  size_t bytes = head;
  for (const PtDesign* d : tabs) bytes += (d->taps.size() * sizeof(float) + 15) & ~(size_t)15;
  auto& sg = v->staging[slot];
  if ((rc = sg.h_pt.ensure(bytes))) return rc;
  if ((rc = plan_ensure(v, s, ch.pt_dev, bytes))) return rc;
  char* const dev = ch.pt_dev.as<char>();
  PtItem* items = (PtItem*)sg.h_pt.p;
  for (int b = 0; b < s.NB; b++) items[b] = PtItem{nullptr, kPtOne, 0, 0};
  size_t off = head;
  for (const PtDesign* d : tabs) {
    memcpy(sg.h_pt + off, d->taps.data(), d->taps.size() * sizeof(float));
    for (int b = 0; b < s.NB; b++)
      if (ch.pt_q[b] == d->Q) items[b] = PtItem{(const float*)(dev + off), d->Q, d->P, 0};
    off += (d->taps.size() * sizeof(float) + 15) & ~(size_t)15;
  }
  PH_HIP(hipMemcpyAsync(dev, sg.h_pt, bytes, hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  ch.pt_on = true;
  return PIPER_HIP_OK;
}

// The geometry of the rows behind the pitch without a launch, over the plan's own audio and lengths: what the host-side bounds of the
// sinks are taken from. A plan without a pitch: exactly the plan's own rows.
Chain chain_geometry(const piper_hip_voice* v, const Slot& s) {
  Chain c = chain_source(v, s);
  if (!s.chain.pt_on || c.F < 1) return c;
  c.F = (int)ceil_div(pt_count((int64_t)c.F * v->hop, s.chain.pt_qmin), v->hop);  // the plan's frame bucket under the least step of the batch
  c.row = (int64_t)c.F * v->hop;
  return c;
}

// Pitch, and the single owner of the geometry of every later stage — the plan's latest staging carried one: pitched [NB][F'cap·hop] with
// the frame counts the kernel wrote, once per launch. Where the rows have grown, the row-sized buffers of the later stages go back.
int chain_pitch(piper_hip_voice* v, Slot& s, Chain& c) {
  OutputChain& ch = s.chain;
  const Chain g = chain_geometry(v, s);
  if (g.row > ch.row) {
    for (PlanBuf* b : ch.row_sized()) plan_release(v, s, *b);
    ch.eq_ok = false;
    ch.loud_ok = false;
    ch.row = g.row;
    ch.F = g.F;
  }
  if (!ch.pt_on) return PIPER_HIP_OK;
  if (c.F < 1 || !ch.pt_dev.p || !s.lensF) PH_FAIL(PIPER_HIP_ERR_SHAPE, "pitch: the slot holds no samples to shift");
  int rc;
  if ((rc = plan_ensure(v, s, ch.pitched, (size_t)s.NB * g.row * sizeof(float), &ch.pitched_ok))) return rc;
  if ((rc = plan_ensure(v, s, ch.pt_lensF, (size_t)s.NB * sizeof(int), &ch.pitched_ok))) return rc;
  if (!ch.pitched_ok) {
    PH_HIP(launch_pitch_items(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, 0, ch.pt_dev.as<const PtItem>(), PtItem{}, ch.pt_qmin,
                              ch.pt_qmax, ch.pt_pmax, ch.pitched.as<float>(), g.row, ch.pt_lensF.as<int>()),
           PIPER_HIP_ERR_LAUNCH);
    ch.pitched_ok = true;
  }
  c = Chain{ch.pitched.as<float>(), g.row, ch.pt_lensF.as<int>(), g.F};
  return PIPER_HIP_OK;
}

// Settings of a slot id on their way to a plan: one T in the slot id's page-locked `host`, written by `fill`, then copied to `dev` on q.
// The staging buffer is rewritten only once the copy queued from it last time has run (`ev`), even where that call failed before its wait.
template <class T, class Fill>
int upload_settings(PinnedBuf<T>& host, hipEvent_t& ev, void* dev, hipStream_t q, Fill fill) {
  if (ev) PH_HIP(hipEventSynchronize(ev), PIPER_HIP_ERR_LAUNCH);
  else PH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
  int rc;
  if ((rc = host.ensure(1, 1)) || (rc = fill(host.p))) return rc;
  PH_HIP(hipMemcpyAsync(dev, host, sizeof(T), hipMemcpyHostToDevice, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipEventRecord(ev, q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// EQ — the slot id has one (piper_hip_voice_slot_eq): eqd [NB][row], once per launch and EQ. Whenever the EQ the chain reads through
// changes, the loudness measured behind it is dropped.
int chain_eq(piper_hip_voice* v, int slot, Slot& s, Chain& c) {
  OutputChain& ch = s.chain;
  const auto& se = v->slot_eq[slot];
  if (ch.eq_on != se.on || (se.on && memcmp(&ch.eq_held, &se.eq, sizeof(piper_hip_eq)) != 0)) {
    ch.eq_on = se.on;
    ch.eq_held = se.eq;
    ch.eq_ok = false;
    ch.loud_ok = false;
  }
  if (!se.on) return PIPER_HIP_OK;
  if (c.F < 1) PH_FAIL(PIPER_HIP_ERR_SHAPE, "eq: the slot holds no samples to filter");
  int rc;
  if ((rc = plan_ensure(v, s, ch.eqd, (size_t)s.NB * ch.row * sizeof(float), &ch.eq_ok))) return rc;
  if ((rc = plan_ensure(v, s, ch.eq_work, (size_t)s.NB * eq_work_row((int64_t)ch.F * v->hop, kEqMaxD) * sizeof(double)))) return rc;
  if ((rc = plan_ensure(v, s, ch.eq_dev, sizeof(EqDesign), &ch.eq_dev_ok))) return rc;
  if (!ch.eq_ok) {
    if (!ch.eq_dev_ok || memcmp(&ch.eq_dev_eq, &se.eq, sizeof(piper_hip_eq)) != 0) {
      auto& sg = v->staging[slot];
      if ((rc = upload_settings(sg.h_eq, sg.eq_ev, ch.eq_dev.p, s.set.stream,
                                [&](EqDesign* d) { return eq_build(&se.eq, v->cfg.sample_rate, d); })))
        return rc;
      ch.eq_dev_ok = true;
      ch.eq_dev_eq = se.eq;
    }
    PH_HIP(launch_eq_items(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, 0, ch.eq_dev.as<EqDesign>(), se.eq.n,
                           ch.eq_work.as<double>(), ch.eqd.as<float>(), c.row),
           PIPER_HIP_ERR_LAUNCH);
    ch.eq_ok = true;
  }
  c.audio = ch.eqd.as<float>();
  return PIPER_HIP_OK;
}

// {L, g} of the rows `c` (what the walk hands out behind the EQ) into loud_rep: the K-weighted segment powers once per launch, the
// gates and the gain of target `t` every time (include/piper_hip.h "Loudness").
int chain_measure(piper_hip_voice* v, Slot& s, const Chain& c, const LdFilter& f, const LdTarget& t) {
  OutputChain& ch = s.chain;
  if (c.F < 1) PH_FAIL(PIPER_HIP_ERR_SHAPE, "loudness: the slot holds no samples");
  int rc;
  if ((rc = plan_ensure(v, s, ch.loud_seg, (size_t)s.NB * ld_work_row((int64_t)ch.F * v->hop) * sizeof(double), &ch.loud_ok))) return rc;
  if ((rc = plan_ensure(v, s, ch.loud_rep, (size_t)s.NB * 2 * sizeof(float)))) return rc;
  if (!ch.loud_ok) {
    PH_HIP(launch_loudness_measure(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, 0, f, ch.loud_seg.as<double>()), PIPER_HIP_ERR_LAUNCH);
    ch.loud_ok = true;
  }
  PH_HIP(launch_loudness_gate(s.set.stream, c.lensF, c.F, v->hop, s.NB, 0, f.h, ch.loud_seg.as<double>(), t, ch.loud_rep.as<float>()),
         PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// Loudness — the slot id has a target (piper_hip_voice_slot_loudness): measure, gate, then gained [NB][row], u = x·g per item.
int chain_loudness(piper_hip_voice* v, int slot, Slot& s, Chain& c) {
  OutputChain& ch = s.chain;
  const auto& sl = v->slot_ld[slot];
  if (!sl.on) return PIPER_HIP_OK;
  LdTarget t;
  int rc = ld_resolve(&sl.ld, &t);
  if (rc) return rc;
  if (c.F < 1) return PIPER_HIP_OK;
  LdFilter f;
  if ((rc = ld_filter(v->cfg.sample_rate, &f)) || (rc = chain_measure(v, s, c, f, t))) return rc;
  if ((rc = plan_ensure(v, s, ch.gained, (size_t)s.NB * ch.row * sizeof(float)))) return rc;
  PH_HIP(launch_loudness_gain(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, ch.loud_rep.as<float>(), ch.gained.as<float>(), c.row),
         PIPER_HIP_ERR_LAUNCH);
  c.audio = ch.gained.as<float>();
  return PIPER_HIP_OK;
}

// Level — the slot id has one (piper_hip_voice_slot_level): lim [NB][row], the limited items.
int chain_level(piper_hip_voice* v, int slot, Slot& s, Chain& c) {
  OutputChain& ch = s.chain;
  const auto& sl = v->slot_lv[slot];
  if (!sl.on) return PIPER_HIP_OK;
  LvParams p;
  int rc = lv_resolve(&sl.lv, v->cfg.sample_rate, &p);
  if (rc) return rc;
  if (c.F < 1) return PIPER_HIP_OK;
  if ((rc = plan_ensure(v, s, ch.lim, (size_t)s.NB * ch.row * sizeof(float)))) return rc;
  if ((rc = plan_ensure(v, s, ch.lim_scratch, lv_scratch_floats(s.NB, (int64_t)ch.F * v->hop) * sizeof(float)))) return rc;
  PH_HIP(launch_level_items(s.set.stream, c.audio, c.row, c.lensF, c.F, v->hop, s.NB, 0, p, ch.lim_scratch.as<float>(), ch.lim.as<float>(), c.row),
         PIPER_HIP_ERR_LAUNCH);
  c.audio = ch.lim.as<float>();
  return PIPER_HIP_OK;
}

// The walk: volume, pitch, EQ — `behind_eq` receives that view, what piper_hip_voice_loudness measures and normalize = 1 takes its
// peaks from — and, where `items` is given, on through loudness and level to what the sinks and the join read. A plan and a slot id with
// no stage: the plan's own rows, and nothing is launched or allocated.
int chain_walk(piper_hip_voice* v, int slot, Slot& s, Chain* behind_eq, Chain* items) {
  Chain c = chain_source(v, s);
  int rc;
  if ((rc = chain_volume(v, s, c)) || (rc = chain_pitch(v, s, c)) || (rc = chain_eq(v, slot, s, c))) return rc;
  if (behind_eq) *behind_eq = c;
  if (!items) return PIPER_HIP_OK;
  if ((rc = chain_loudness(v, slot, s, c)) || (rc = chain_level(v, slot, s, c))) return rc;
  *items = c;
  return PIPER_HIP_OK;
}

// ---- join (include/piper_hip.h "Join"): the items a collect reads → ONE programme in the plan's jn_buf

// The no-trim bound on the programme of slot id `slot`'s join over the prepared plan, at the voice's rate: a bounded slot whose lengths
// are still on the device counts every item at its frame capacity.
int join_capacity(const piper_hip_voice* v, int slot, const Slot& s, int64_t* cap) {
  const auto& sj = v->slot_jn[slot];
  if (s.NB > kJoinMaxItems) PH_FAIL(PIPER_HIP_ERR_SHAPE, "join: %d items (at most %d)", s.NB, kJoinMaxItems);
  const int F = row_frames(v, s);
  int64_t sum = 0;  // (under a pitch: of the pitched items)
  for (int b = 0; b < s.NB; b++) sum += item_samples(v, s, b, s.bounded_pending ? F : std::min(s.h_F[b], F));
  *cap = join_bound(sj.p, s.NB, sum);
  if (*cap > INT_MAX) PH_FAIL(PIPER_HIP_ERR_SHAPE, "join: a programme of up to %lld samples does not fit an int", (long long)*cap);
  return PIPER_HIP_OK;
}

// What the sinks read in place of the items: one row of `cap` floats whose true length is the device int `total`.
struct Joined {
  const float* prog = nullptr;
  const int* total = nullptr;
  int64_t cap = 0;
};

// The join of slot id `slot` over `items` (what the walk handed out) into a programme of at most `cap` samples (join_capacity), behind
// the plan's graph on its stream, from lengths the device holds. The report lands in the slot id's page-locked h_jrep — through its
// mapping where there is one, else by a copy behind the launches — and is the host's once the stream has been waited for (join_landed).
int join_items(piper_hip_voice* v, int slot, Slot& s, const Chain& items, int64_t cap, Joined* out) {
  OutputChain& ch = s.chain;
  const auto& sj = v->slot_jn[slot];
  auto& sg = v->staging[slot];
  const int F = items.F;
  int rc;
  if ((rc = plan_ensure(v, s, ch.jn_buf, (size_t)std::max<int64_t>(cap, 1) * sizeof(float)))) return rc;
  const size_t o_rep = sizeof(JoinParams), o_rows = o_rep + (size_t)kJoinReport * sizeof(int64_t);
  const size_t o_edges = o_rows + (size_t)kJoinMaxItems * sizeof(JoinRow);
  if ((rc = plan_ensure(v, s, ch.jn_dev, o_edges + (2 * (size_t)kJoinMaxItems + 1) * sizeof(int)))) return rc;  // (allocated once: jn_gen is 0 then)
  char* const dev = ch.jn_dev.as<char>();
  const hipStream_t st = s.set.stream;
  if (ch.jn_gen != sj.gen) {
    if ((rc = upload_settings(sg.h_join, sg.join_ev, dev, st, [&](JoinParams* p) { *p = sj.p; return PIPER_HIP_OK; }))) return rc;
    ch.jn_gen = sj.gen;
  }
  if ((rc = sg.h_jrep.ensure((size_t)kJoinReport, (size_t)kJoinReport))) return rc;
  int64_t* const rep_host = sg.h_jrep.mapped();
  int64_t z = sj.p.tail;
  for (int b = 0; b + 1 < s.NB; b++) z = std::max(z, sj.p.gap[b]);
  int* edges = (int*)(dev + o_edges);
  const JoinSrc src{items.audio, items.row, items.lensF, F, v->hop, nullptr, nullptr};
  PH_HIP(launch_join(st, src, s.NB, (int64_t)F * v->hop, sj.p.lead + z, (const JoinParams*)dev, sj.p.trim != 0, edges,
                     (JoinRow*)(dev + o_rows), edges + 2 * kJoinMaxItems, (int64_t*)(dev + o_rep), rep_host, ch.jn_buf.as<float>()),
         PIPER_HIP_ERR_LAUNCH);
  if (!rep_host)
    PH_HIP(hipMemcpyAsync(sg.h_jrep, dev + o_rep, (size_t)(1 + 2 * s.NB) * sizeof(int64_t), hipMemcpyDeviceToHost, st), PIPER_HIP_ERR_LAUNCH);
  out->prog = ch.jn_buf.as<float>();
  out->total = edges + 2 * kJoinMaxItems;
  out->cap = cap;
  return PIPER_HIP_OK;
}

// after the slot's stream has been synchronised behind join_items: the report → h_jrep (piper_hip_voice_join_report); returns the total
int64_t join_landed(piper_hip_voice* v, int slot, Slot& s) {
  const auto& sg = v->staging[slot];
  s.chain.h_jrep.assign(sg.h_jrep.p, sg.h_jrep + 1 + 2 * s.NB);
  return s.chain.h_jrep[0];
}

// A chunked landing in the slot id's page-locked buffer (collect, pcm_land): chunk_mark records event k behind the copy of chunk k on q,
// chunk_wait polls for it — the chunks arrive every ≈ 20 µs — and reports a failure under the caller's name.
int chunk_mark(piper_hip_voice::Staging& sg, size_t k, hipStream_t q) {
  if (sg.chunk_ev.size() <= k) {
    hipEvent_t e = nullptr;
    PH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
    sg.chunk_ev.push_back(e);
  }
  PH_HIP(hipEventRecord(sg.chunk_ev[k], q), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}
int chunk_wait(const piper_hip_voice::Staging& sg, size_t k, const char* who) {
  for (;;) {
    const hipError_t e = hipEventQuery(sg.chunk_ev[k]);
    if (e == hipSuccess) return PIPER_HIP_OK;
    if (e != hipErrorNotReady) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    (void)hipGetLastError();
    for (int i = 0; i < 16; i++) __builtin_ia32_pause();
  }
}

// collect on a slot id with a join: the programme's floats, of which the caller's buffer holds `cap` (join_capacity) at least. Up to
// kPinnedMax they leave through the slot id's page-locked buffer by a kernel that reads the length from device memory — one
// synchronisation for report, lengths and samples; a longer programme waits for its length first and is copied at it.
int collect_joined(piper_hip_voice* v, int slot, Slot& s, const Chain& items, int64_t cap, float* host_audio) {
  auto& sg = v->staging[slot];
  Joined j;
  int rc = join_items(v, slot, s, items, cap, &j);
  if (rc) return rc;
  const hipStream_t st = s.set.stream;
  float* dst_dev = nullptr;
  if ((size_t)cap * sizeof(float) <= kPinnedMax && !is_caller_pinned(host_audio)) {
    if (sg.h_audio.ensure((size_t)std::max<int64_t>(cap, 1), kAudioMinCap)) (void)hipGetLastError();
    dst_dev = sg.h_audio.mapped();
  }
  if (dst_dev) {
    const int blocks = (int)std::min<int64_t>(std::max<int64_t>((cap + 4 * 256 - 1) / (4 * 256), 1), 1024);
    hipLaunchKernelGGL(copy_out_len_kernel, dim3(blocks), dim3(256), 0, st, j.prog, dst_dev, j.total, 0, 1);
    PH_HIP(hipGetLastError(), PIPER_HIP_ERR_LAUNCH);
  }
  PH_HIP(stream_wait(st), PIPER_HIP_ERR_LAUNCH);
  const int64_t total = join_landed(v, slot, s);
  if (s.bounded_pending && (rc = bounded_finish(v, slot, s))) return rc;
  if (dst_dev) {
    memcpy(host_audio, sg.h_audio, (size_t)total * sizeof(float));
  } else if (total > 0) {
    PH_HIP(hipMemcpyAsync(host_audio, j.prog, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st), PIPER_HIP_ERR_LAUNCH);
    PH_HIP(hipStreamSynchronize(st), PIPER_HIP_ERR_LAUNCH);
  }
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_launch(piper_hip_voice* v, int slot) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  Slot& s = *p;
  PH_HIP(hipEventRecord(s.set.ev0, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  {
    const int lrc = launch_plan(v, s);
    if (lrc) return lrc;
  }
  PH_HIP(hipEventRecord(s.set.ev1, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  s.timed = true;
  chain_invalidate(s.chain);  // (the peaks, the measurement, the rows and the report of earlier collects belong to the previous run)
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_collect(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  Slot& s = *p;
  auto& sg = v->staging[slot];
  Chain chain = chain_geometry(v, s);  // the items the collect reads: the walk's where there is a buffer to fill, else only their geometry
  const bool joined = host_audio && v->slot_jn[slot].on;
  int64_t jcap = 0;
  if (joined) {  // (a buffer too short for the programme is refused before anything is enqueued)
    if (int jrc = join_capacity(v, slot, s, &jcap)) return jrc;
    if (max_samples < jcap)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect: the join needs room for %lld samples (piper_hip_voice_join_capacity), got %lld", (long long)jcap,
              (long long)max_samples);
  }
  if (host_audio && !joined && s.bounded_pending) {  // (a buffer too short for the capacity is refused before anything is enqueued)
    int64_t need = 0;
    for (int b = 0; b < s.NB; b++) need += item_samples(v, s, b, s.F);
    if (max_samples < need)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect: a bounded slot needs room for its capacity (%lld samples: piper_hip_voice_%s_samples before collect), got %lld",
              (long long)need, s.chain.pt_on ? "pitch" : "prepared", (long long)max_samples);
  }
  if (host_audio)
    if (int wrc = chain_walk(v, slot, s, nullptr, &chain)) return wrc;
  const float* audio = chain.audio;
  if (joined) return collect_joined(v, slot, s, chain, jcap, host_audio);  // (a slot id with a join: the programme)
  // The slot id's page-locked landing buffer of the waveform (kAudioMinCap at least). Failing to grow it is not fatal: the waveform
  // then goes to the caller's buffer directly, and the sticky error of the failed hipHostMalloc is cleared (the next launch would report it).
  if (s.bounded_pending) {
    // lengths still on the device. Short buckets: the waveform rows go to the slot id's page-locked buffer at bucket stride by a kernel that
    // reads each length from device memory — ONE synchronisation for lengths and samples; long ones: synchronise, then the usual copy.
    const int64_t row = s.chain.pt_on ? chain.row : (int64_t)s.F * v->hop;
    const size_t ub = (size_t)row * s.NB * sizeof(float);
    float* dst_dev = nullptr;
    if (host_audio && ub <= ((size_t)1 << 20) && (v->hop & 3) == 0) {
      if (sg.h_audio.ensure((size_t)row * s.NB, kAudioMinCap)) (void)hipGetLastError();
      dst_dev = sg.h_audio.mapped();
    }
    if (dst_dev) {
      for (int b = 0; b < s.NB; b++) {
        const int blocks = (int)std::min<int64_t>((row + 4 * 256 - 1) / (4 * 256), 1024);
        hipLaunchKernelGGL(copy_out_len_kernel, dim3(blocks), dim3(256), 0, s.set.stream, audio + (int64_t)b * chain.row, dst_dev + (int64_t)b * row, chain.lensF, b, v->hop);
        PH_HIP(hipGetLastError(), PIPER_HIP_ERR_LAUNCH);
      }
    }
    PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
    const int frc = bounded_finish(v, slot, s);
    if (frc) return frc;
    if (dst_dev) {
      int64_t off = 0;
      for (int b = 0; b < s.NB; b++) {
        const int64_t nb = item_samples(v, s, b);
        memcpy(host_audio + off, sg.h_audio + (int64_t)b * row, (size_t)nb * sizeof(float));
        off += nb;
      }
      return PIPER_HIP_OK;
    }
    // fall through: the lengths are known now
  }
  if (host_audio) {
    const int64_t total = delivered_samples(v, slot, s);  // (no join here: batch items back to back, each at its own true length)
    if (max_samples < total) PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect: buffer holds %lld < %lld samples", (long long)max_samples, (long long)total);
    // A copy into the caller's (pageable) buffer goes through the runtime's own staging in chunks and its time varies from
    // box to box (r2z: 45 … 130 µs for 344 KB). Up to 1 MB (a factor-8 … 16 utterance) the waveform lands in a pinned buffer of
    // the plan by one DMA and is copied out by the host; beyond that the runtime's pipelined chunks beat DMA + memcpy
    // (factor 64, 2.75 MB: +0.12 ms with the pinned hop).
    // 1 … 16 MB into PAGEABLE memory: handing the caller's buffer to the runtime makes it page-lock that buffer on the spot, and for a buffer
    // it has not seen before that took 7 ms (r3, tools/probe/first_run.py: the first 1.2 MB waveform of a process, 9.4 ms in collect for
    // 1.9 ms of GPU work). Such waveforms land in the slot id's page-locked buffer in 1 MB chunks, each followed by an event, and the host
    // copies chunk k out while chunk k + 1 is on the wire. Larger ones still go to the runtime (its pipelined staging wins there).
    const size_t bytes = (size_t)total * sizeof(float);
    // a destination the caller page-locked itself (piper_hip_host_alloc) takes the DMA directly
    const bool caller_pinned = is_caller_pinned(host_audio);
    if (!caller_pinned && bytes <= kChunkedMax && sg.h_audio.ensure((size_t)total, kAudioMinCap)) (void)hipGetLastError();
    float* h_audio = sg.h_audio.cap >= (size_t)total ? sg.h_audio.p : nullptr;
    if (!caller_pinned && bytes > kPinnedMax && bytes <= kChunkedMax && h_audio) {
      // the items back to back in the staging buffer, cut into chunks; `cuts` = end offset (floats) of each chunk
      std::vector<int64_t> cuts;
      int64_t off = 0;
      for (int b = 0; b < s.NB; b++) {
        const int64_t nb = item_samples(v, s, b);
        const float* src = audio + (int64_t)b * chain.row;
        for (int64_t c0 = 0; c0 < nb; c0 += (int64_t)(kChunk / sizeof(float))) {
          const int64_t cn = std::min<int64_t>((int64_t)(kChunk / sizeof(float)), nb - c0);
          PH_HIP(hipMemcpyAsync(h_audio + off + c0, src + c0, (size_t)cn * sizeof(float), hipMemcpyDeviceToHost, s.set.stream), PIPER_HIP_ERR_LAUNCH);
          if (int mrc = chunk_mark(sg, cuts.size(), s.set.stream)) return mrc;
          cuts.push_back(off + c0 + cn);
        }
        off += nb;
      }
      int64_t done = 0;
      for (size_t k = 0; k < cuts.size(); k++) {
        if (int wrc = chunk_wait(sg, k, "collect")) return wrc;
        memcpy(host_audio + done, h_audio + done, (size_t)(cuts[k] - done) * sizeof(float));
        done = cuts[k];
      }
      return PIPER_HIP_OK;
    }
    float* dst = (!caller_pinned && bytes <= kPinnedMax && h_audio) ? h_audio : host_audio;
    // Short waveforms into page-locked memory are written by a KERNEL through the host mapping instead of the copy engine: the
    // hand-over from the last kernel of the graph to another kernel costs ≈ 2 µs, to the DMA engine ≈ 10 µs (PIPER_HIP_COLLECT_DMA=1:
    // always the copy engine).
    static const bool dma_only = getenv("PIPER_HIP_COLLECT_DMA") != nullptr;
    float* dst_dev = nullptr;
    // (a destination the caller page-locked takes the copy kernel up to 16 MB: the engine's hand-over and completion varied 0.07 … 0.3 ms
    // from process to process on a 2.75 MB waveform, r3)
    if (!dma_only && (caller_pinned ? bytes <= kChunkedMax : bytes <= kPinnedMax) && (caller_pinned || dst == h_audio)) {
      if (hipHostGetDevicePointer((void**)&dst_dev, dst, 0) != hipSuccess) { dst_dev = nullptr; (void)hipGetLastError(); }
    }
    int64_t off = 0;
    for (int b = 0; b < s.NB; b++) {
      const int64_t nb = item_samples(v, s, b);
      const float* src = audio + (int64_t)b * chain.row;
      if (dst_dev && nb > 0) {
        const int blocks = (int)std::min<int64_t>((nb + 4 * 256 - 1) / (4 * 256), 1024);
        hipLaunchKernelGGL(copy_out_kernel, dim3(blocks), dim3(256), 0, s.set.stream, src, dst_dev + off, nb);
        PH_HIP(hipGetLastError(), PIPER_HIP_ERR_LAUNCH);
      } else {
        PH_HIP(hipMemcpyAsync(dst + off, src, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, s.set.stream), PIPER_HIP_ERR_LAUNCH);
      }
      off += nb;
    }
    // a copy-ENGINE transfer completes through the runtime's own signal handling: polling the stream next to it delayed the completion of a
    // 2.75 MB waveform by ≈ 0.2 ms (factor 64, r3) — park for those, poll only behind the copy kernel
    if (dst_dev) PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
    else PH_HIP(hipStreamSynchronize(s.set.stream), PIPER_HIP_ERR_LAUNCH);
    if (dst != host_audio) memcpy(host_audio, dst, bytes);
    return PIPER_HIP_OK;
  }
  PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// ---- streaming: encoder + flow once, then the generator window by window --------------------------------------------
namespace {

// Frames of latent the generator needs on each side of an output frame (its receptive field, walked from the waveform back
// to z): conv_post ±3 samples; per stage the widest ResBlock reach, then the ConvTranspose; conv_pre ±3 frames.
int generator_halo_frames(const piper_hip_voice_config& c) {
  int64_t r = 3;
  for (int u = c.n_ups - 1; u >= 0; u--) {
    int64_t rb = 0;
    for (int j = 0; j < c.n_rb; j++) {
      int64_t reach = 0;
      for (int di = 0; di < c.rb_n_dil; di++) {
        const int64_t k = c.rb_kernels[j], d = c.rb_dilations[j][di];
        reach += (k * d - d) / 2 + (c.resblock_type == 1 ? (k - 1) / 2 : 0);
      }
      rb = std::max(rb, reach);
    }
    r += rb;
    r = (r + c.up_kernels[u]) / c.up_rates[u] + 1;
  }
  return (int)(r + 3);
}

int run_steps(Slot& s, const std::vector<int>& pick, hipStream_t q) {
  for (int i : pick) {
    const int rc = s.steps[i].enqueue(q);
    if (rc) return rc;
  }
  return PIPER_HIP_OK;
}

// graph of the steps selected by `pick` (eager pass first: validates launches and sets kernel attributes)
int capture_steps(Slot& s, const std::vector<int>& pick, hipGraph_t* g, hipGraphExec_t* ge) {
  const int rc = run_steps(s, pick, s.set.stream);
  if (rc) return rc;
  PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
  return capture_graph(s.set.stream, [&](hipStream_t q) { return run_steps(s, pick, q); }, g, ge, "stream");
}

}  // namespace

PH_EXPORT int piper_hip_voice_receptive_field(const piper_hip_voice* v) { return v ? generator_halo_frames(v->cfg) : -1; }

namespace {
// The prepared slot's encoder + flow as their own graph (everything before the generator's first launch), captured on first use, then
// launched; z is ready when the plan's ev1 fires. Shared by the single and the batched stream. front_steps: the launches it consists of.
int stream_volume_begin(piper_hip_voice* v, Slot& s, const float** gf);
std::vector<int> front_steps(const Slot& s) {
  std::vector<int> front;
  for (int i = 0; i < (int)s.steps.size(); i++) {
    if (s.steps[i].name.compare(0, 4, "dec.") == 0) break;
    if (s.steps[i].kind == Step::LAUNCH) front.push_back(i);
  }
  return front;
}

int launch_front(Slot& s) {
  if (!s.front_exec) {
    const int rc = capture_steps(s, front_steps(s), &s.front_graph, &s.front_exec);
    if (rc) return rc;
  }
  PH_HIP(hipGraphLaunch(s.front_exec, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipEventRecord(s.set.ev1, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_begin(piper_hip_voice* v, const piper_hip_utterance* u, int slot, int chunk_frames) {
  const ControlsClear cc{v, slot};  // a staging call: the slot id's prosody, volume and pitch are this call's, on every way out
  if (int prc = refuse_pitch(v, slot, "stream_begin")) return prc;
  if (chunk_frames < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_begin: chunk_frames must be >= 1");
  int rc = piper_hip_voice_prepare(v, u, slot);
  if (rc < 0) return rc;
  Slot& s = *v->attached[slot];
  const float* gf = nullptr;  // the item's gains per frame where the request carried a volume
  if ((rc = stream_volume_begin(v, s, &gf))) return rc;
  if ((rc = launch_front(s))) return rc;
  Stream& st = s.stream;
  st.plan = &s;
  st.chunk = chunk_frames;
  st.halo = generator_halo_frames(v->cfg);
  st.NBg = 1;
  st.single = true;
  st.rows.assign(1, StreamRow{s.h_F[0], 0, s.h_F[0] > 0});
  st.rows[0].gf = gf;
  return (int)ceil_div(s.h_F[0], chunk_frames);
}

namespace {
// ---- 16-bit PCM out of a plan: where the convert kernel stores and how the samples reach the caller. The policy and the thresholds are
// collect's (see there for the measurements behind them): a destination the caller page-locked takes kernel stores through its host
// mapping up to 16 MB; a pageable one is served through the slot id's page-locked staging — kernel stores up to 1 MB, 1 MB chunks by the
// copy engine with the host copying behind them up to 16 MB — and handed to the runtime beyond that. PIPER_HIP_COLLECT_DMA: always the
// copy engine. The staging is sg.h_audio, the waveform's own landing buffer, holding two int16 samples per float or four G.711 bytes.
// elem = bytes of a sample (2, or 1 for G.711); the thresholds apply to the byte count.

struct PcmRoute {
  void* kdst = nullptr;        // where the convert kernel stores
  void* stage = nullptr;       // the slot id's page-locked staging when it holds the samples, else null
  bool mapped = false;         // kdst is host memory seen from the device: the stores are the transfer
  bool caller_pinned = false;  // (then kdst is the caller's buffer itself)
};

// `samples` will travel to `host`; a device buffer, if one is needed, belongs to `plan` and holds `dev_samples`
int pcm_route(piper_hip_voice* v, Slot& plan, piper_hip_voice::Staging& sg, void* host, size_t elem, size_t samples, size_t dev_samples,
              PcmRoute* r) {
  const size_t bytes = samples * elem;
  r->caller_pinned = is_caller_pinned(host);
  if (!r->caller_pinned && bytes <= kChunkedMax && sg.h_audio.ensure((bytes + 3) / 4, kAudioMinCap)) (void)hipGetLastError();
  r->stage = (!r->caller_pinned && sg.h_audio && sg.h_audio.cap * sizeof(float) >= bytes) ? (void*)sg.h_audio.p : nullptr;
  static const bool dma_only = getenv("PIPER_HIP_COLLECT_DMA") != nullptr;
  void* target = r->caller_pinned ? (bytes <= kChunkedMax ? (void*)host : nullptr) : (bytes <= kPinnedMax ? (void*)r->stage : nullptr);
  if (!dma_only && target) {
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, target, 0) == hipSuccess && dev) { r->kdst = dev; r->mapped = true; }
    else (void)hipGetLastError();
  }
  if (!r->mapped) {
    if (plan.pcm_cap < dev_samples * elem) {
      void* p = nullptr;
      const int rc = plan_alloc(v, plan, dev_samples * elem, &p);  // (a smaller one stays with the plan until it is released)
      if (rc) return rc;
      plan.pcm = p;
      plan.pcm_cap = dev_samples * elem;
    }
    r->kdst = plan.pcm;
  }
  return PIPER_HIP_OK;
}

// Behind the convert kernel on q: wait for it, and bring `samples` samples to `host` unless the kernel stored them through a mapping
// (then they are in the caller's buffer already, or in r.stage, from where the caller copies what it needs).
int pcm_land(piper_hip_voice::Staging& sg, const PcmRoute& r, hipStream_t q, void* host, size_t elem, size_t samples) {
  if (r.mapped) {
    PH_HIP(stream_wait(q), PIPER_HIP_ERR_LAUNCH);
    return PIPER_HIP_OK;
  }
  const size_t bytes = samples * elem;
  if (!r.caller_pinned && r.stage && bytes > kPinnedMax && bytes <= kChunkedMax) {
    const size_t nchunks = (bytes + kChunk - 1) / kChunk;
    for (size_t k = 0; k < nchunks; k++) {
      const size_t at = k * kChunk, cb = std::min(kChunk, bytes - at);
      PH_HIP(hipMemcpyAsync((char*)r.stage + at, (const char*)r.kdst + at, cb, hipMemcpyDeviceToHost, q), PIPER_HIP_ERR_LAUNCH);
      if (int rc = chunk_mark(sg, k, q)) return rc;
    }
    for (size_t k = 0; k < nchunks; k++) {
      if (int rc = chunk_wait(sg, k, "pcm16")) return rc;
      const size_t at = k * kChunk;
      memcpy((char*)host + at, (const char*)r.stage + at, std::min(kChunk, bytes - at));
    }
    return PIPER_HIP_OK;
  }
  void* dst = (!r.caller_pinned && r.stage && bytes <= kPinnedMax) ? r.stage : host;
  PH_HIP(hipMemcpyAsync(dst, r.kdst, bytes, hipMemcpyDeviceToHost, q), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(hipStreamSynchronize(q), PIPER_HIP_ERR_LAUNCH);
  if (dst != host) memcpy(host, dst, bytes);
  return PIPER_HIP_OK;
}

// params of a PCM entry point → gain (0 = 1.0) and the normalize flag; a negative or non-finite gain is an argument error
int pcm_params(const piper_hip_pcm_params* p, float* gain, bool* normalize) {
  *gain = 1.0f;
  *normalize = false;
  if (!p) return PIPER_HIP_OK;
  if (!(p->gain >= 0.0f) || !std::isfinite(p->gain)) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16: gain %g is negative or not finite", (double)p->gain);
  if (p->gain != 0.0f) *gain = p->gain;
  *normalize = p->normalize != 0;
  return PIPER_HIP_OK;
}

// The filter from the voice's rate to out_rate, its table in device memory (uploaded on first use, kept by the voice).
int voice_filter(piper_hip_voice* v, int out_rate, const RsDesign** d, RsFilter* f) {
  const RsDesign* des = nullptr;
  int rc = rs_design(v->cfg.sample_rate, out_rate, &des);
  if (rc) return rc;
  auto it = v->rate_tables.find(out_rate);
  if (it == v->rate_tables.end()) {
    void* p = nullptr;
    if ((rc = v->ctx->pool.alloc(des->taps.size() * sizeof(float), &p))) return rc;
    if (hipMemcpy(p, des->taps.data(), des->taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)v->ctx->pool.release(p);
      PH_FAIL(PIPER_HIP_ERR_LAUNCH, "resample: the filter table could not be uploaded");
    }
    piper_hip_voice::RateTable t;
    t.d = des; t.taps = (float*)p;
    it = v->rate_tables.emplace(out_rate, t).first;
  }
  if (d) *d = des;
  *f = RsFilter{it->second.taps, des->L, des->M, des->P};
  return PIPER_HIP_OK;
}

// The outputs [j0, j1) a resampling step emits for a row whose chunk is the input samples [s, e) of N: everything whose taps end before e
// (the halo behind e is an approximation, the next chunk does not exist yet), the rest of the item on its last step.
void rate_range(const RsDesign& d, int64_t s, int64_t e, int64_t N, int64_t* j0, int64_t* j1) {
  *j0 = s == 0 ? 0 : rs_ready(d, s);
  *j1 = e >= N ? rs_count(d, N) : std::max(*j0, rs_ready(d, e));
}

// ints of a slot id's page-locked descriptor staging: the kDesc* table of a step, then the RsStepRow table of a resampling one
constexpr size_t kDescStageInts = (size_t)256 * kDescInts;
constexpr size_t kRateStageInts = kDescStageInts + (size_t)256 * sizeof(RsStepRow) / sizeof(int);
constexpr size_t kMixStageInts = kDescStageInts + (size_t)256 * sizeof(MixStepRow) / sizeof(int);  // (a mixed step: the MixStepRow table instead)
// a step of a slot with a level: the LvStepRow table behind whichever of the tables above the step uses
constexpr size_t kLvStageOff = kMixStageInts > kRateStageInts ? kMixStageInts : kRateStageInts;
constexpr size_t kLvStageInts = kLvStageOff + (size_t)256 * sizeof(LvStepRow) / sizeof(int);
static_assert(kLvStageOff * sizeof(int) % alignof(LvStepRow) == 0 && sizeof(LvStepRow) % sizeof(int) == 0, "the LvStepRow table starts aligned");
static_assert(kDescStageInts * sizeof(int) % alignof(RsStepRow) == 0, "the RsStepRow table starts aligned");
static_assert(kDescStageInts * sizeof(int) % alignof(MixStepRow) == 0 && sizeof(MixStepRow) % sizeof(int) == 0, "the MixStepRow table starts aligned");

// Samples at the voice's rate one row hands its output stage in a step: the chunk, or on a slot with a level the limiter's bound
// (include/piper_hip.h "Level control"). What every capacity and every packed buffer of a stream is sized by.
int64_t step_samples(const piper_hip_voice* v, const Stream& st) {
  const int64_t chunk = (int64_t)st.chunk * v->hop;
  return st.lv.on ? lv_step_bound(chunk) : chunk;
}

// ---- mixed formats (include/piper_hip.h "Mixed formats"): what a row's format means on the host
int fmt_elem(int enc) { return enc == PIPER_HIP_ENC_F32 ? 4 : enc == PIPER_HIP_ENC_S16 ? 2 : 1; }  // bytes of a sample
int64_t round_up4(int64_t bytes) { return (bytes + 3) & ~(int64_t)3; }

// A caller's format → the row's record, every check of the header's table on the host; nothing is uploaded here.
int check_format(const piper_hip_voice* v, const char* who, const piper_hip_stream_format& in, RowFormat* out) {
  if (in.encoding < PIPER_HIP_ENC_S16 || in.encoding > PIPER_HIP_ENC_F32) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: encoding %d outside [0,3]", who, in.encoding);
  if (!(in.gain >= 0.0f) || !std::isfinite(in.gain)) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: gain %g is negative or not finite", who, (double)in.gain);
  if (in.encoding == PIPER_HIP_ENC_F32 && in.gain != 0.0f && in.gain != 1.0f)
    PH_FAIL(PIPER_HIP_ERR_ARG, "%s: an F32 row has no gain (got %g)", who, (double)in.gain);
  RowFormat f;
  f.enc = in.encoding;
  f.gain = in.gain == 0.0f ? 1.0f : in.gain;
  f.rate = (in.out_rate == 0 || in.out_rate == v->cfg.sample_rate) ? 0 : in.out_rate;
  if (f.rate) {
    const RsDesign* d = nullptr;
    if (int rc = rs_design(v->cfg.sample_rate, f.rate, &d)) return rc;
  }
  *out = f;
  return PIPER_HIP_OK;
}

// bytes a row of that format can deliver in one step over chunk_samples input samples, rounded up to the next row's start
int64_t fmt_step_bytes(const piper_hip_voice* v, const RowFormat& f, int64_t chunk_samples) {
  int64_t n = chunk_samples;
  if (f.rate) {
    const RsDesign* d = nullptr;
    if (rs_design(v->cfg.sample_rate, f.rate, &d)) return 0;  // (checked when the format was supplied)
    n = rs_step_bound(*d, chunk_samples);
  }
  return round_up4(n * fmt_elem(f.enc));
}

// What one stream step decodes of an utterance of F frames whose next frame is `next`: latent frames [a, a + Fc), of whose audio the first
// `skip` samples are dropped and the following `n` are the chunk; `end` is the stream's next frame afterwards.
struct Window {
  int a = 0, Fc = 0, skip = 0, n = 0, end = 0;
};

// window = chunk + receptive field, clamped to the utterance: at the utterance's own ends the convs' zero padding is
// then the same zero padding the whole-utterance run sees, inside it the halo frames are recomputed and dropped
Window window_of(int F, int next, int chunk, int halo, int hop) {
  const int f0 = next, f1 = std::min(F, f0 + chunk);
  const int a = std::max(0, f0 - halo), b = std::min(F, f1 + halo);
  return Window{a, b - a, (f0 - a) * hop, (f1 - f0) * hop, f1};
}

// Where the output of a step or a collect goes: the caller's buffer (null: deliver nothing), the samples it holds, the encoding
// (PIPER_HIP_ENC_*: F32 = the float entry points, S16 / MULAW / ALAW = the PCM and G.711 ones, converted by a kernel with `gain`).
// byte_off != nullptr: a mixed step — every row in its own format (StreamRow::fmt) at the 4-byte-aligned byte offsets reported there,
// `cap` counts BYTES, enc and gain are not read. Each exported entry point builds its sink once, after its own argument checks.
struct Sink {
  void* host = nullptr;
  int64_t cap = 0;
  int enc = PIPER_HIP_ENC_F32;
  float gain = 1.0f;
  int64_t* byte_off = nullptr;
};
// the `law` argument of the PCM kernels: the G.711 encodings are their own laws (PIPER_HIP_ENC_MULAW == PIPER_HIP_G711_MULAW …), 0 = int16
int sink_law(const Sink& o) { return o.enc == PIPER_HIP_ENC_MULAW || o.enc == PIPER_HIP_ENC_ALAW ? o.enc : 0; }

// The limited samples [lo, hi) a step hands its output stage for a row whose window is w (include/piper_hip.h "Level control", the emit
// rule), and the row of the limiter's own descriptor: the chunk behind the halo skip, and how many samples of the carry stand before it.
LvStepRow level_range(const StreamRow& row, const Window& w, int hop, int64_t* lo, int64_t* hi) {
  const int64_t s = (int64_t)row.next * hop, e = (int64_t)w.end * hop, N = (int64_t)row.F * hop;
  *lo = row.next == 0 ? 0 : row.lim_lo;  // a row's new occupant starts from nothing
  *hi = e >= N ? N : lv_ready(e);
  return LvStepRow{w.skip, w.n, (int)(s - *lo), (int)(*hi - *lo)};
}

int stream_alloc(piper_hip_voice* v, Stream& st, size_t bytes, void** out);
void stream_free(piper_hip_voice* v, Stream& st, void* p, size_t bytes);

// ---- per-phoneme volume on streams (include/piper_hip.h "Per-phoneme volume")
// A begin on a plan whose staging carried a volume: the gains per frame of its items, gf [NB][F], written on the plan's stream in front of
// its encoder + flow (so whatever waits for those finds them). Returns the row of item 0, null for a request without a volume.
int stream_volume_begin(piper_hip_voice* v, Slot& s, const float** gf) {
  *gf = nullptr;
  if (!s.vol_on) return PIPER_HIP_OK;
  if (!s.vol_gf) {
    void* q = nullptr;
    if (int rc = plan_alloc(v, s, (size_t)s.NB * s.F * sizeof(float), &q)) return rc;
    s.vol_gf = (float*)q;
  }
  PH_HIP(launch_volume_frame_gains(s.set.stream, s.lensF, s.F, s.NB, s.frame2id, s.F, s.vol_gain, s.T, s.vol_gf), PIPER_HIP_ERR_LAUNCH);
  *gf = s.vol_gf;
  return PIPER_HIP_OK;
}

// The row of a step's VolStepRow table for a row whose window is w: the window's own chunk, at its absolute place in the item.
VolStepRow volume_range(const StreamRow& row, const Window& w, int hop) {
  return VolStepRow{row.gf, (int64_t)row.next * hop, row.F, w.skip, w.n, 0};
}

// What a step with a shaped row needs: st.vol of `bytes` (the window plan's audio), the device table and its page-locked staging.
int volume_step_buffers(piper_hip_voice* v, int slot, Stream& st, size_t bytes) {
  int rc;
  void* p = nullptr;
  if (st.vol_bytes < bytes) {  // (no step is in flight: every step ends with a wait)
    if ((rc = stream_alloc(v, st, bytes, &p))) return rc;
    stream_free(v, st, st.vol, st.vol_bytes);
    st.vol = (float*)p;
    st.vol_bytes = bytes;
  }
  if (!st.vol_desc) {
    if ((rc = stream_alloc(v, st, (size_t)256 * sizeof(VolStepRow), &p))) return rc;
    st.vol_desc = (VolStepRow*)p;
  }
  auto& sg = v->staging[slot];
  return sg.h_vstep.ensure((size_t)256);
}

// One launch behind the window plan's graph: the chunks of `rows` generator rows of audio [rows][row] under their envelopes → st.vol.
hipError_t volume_step(piper_hip_voice* v, int slot, Stream& st, const VolStepRow* tab, int rows, const float* audio, int64_t row, hipStream_t q) {
  auto& sg = v->staging[slot];
  int64_t max_n = 0;
  for (int r = 0; r < rows; r++) {
    sg.h_vstep[r] = tab[r];
    max_n = std::max<int64_t>(max_n, tab[r].n);
  }
  if (max_n < 1) return hipSuccess;
  hipError_t e = hipMemcpyAsync(st.vol_desc, sg.h_vstep, (size_t)rows * sizeof(VolStepRow), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) e = launch_volume_step(q, rows, max_n, audio, row, st.vol_desc, v->hop, st.vol);
  return e;
}

// One launch behind the volume step: the chunks of `rows` generator rows of audio [rows][row] through the stream's EQ → st.eq.out, at the
// same places (include/piper_hip.h "Equaliser"). A row's chunk is the one the volume step reads: the window's, from sample next · hop.
hipError_t eq_step(piper_hip_voice* v, int slot, Stream& st, const std::vector<EqStepRow>& tab, const float* audio, int64_t row, size_t bytes,
                   hipStream_t q) {
  StreamEq& sq = st.eq;
  auto& sg = v->staging[slot];
  if (sq.out_bytes < bytes) {  // (no step is in flight: every step ends with a wait)
    void* p = nullptr;
    if (stream_alloc(v, st, bytes, &p)) return hipErrorOutOfMemory;
    stream_free(v, st, sq.out, sq.out_bytes);
    sq.out = (float*)p;
    sq.out_bytes = bytes;
  }
  if (sg.h_estep.ensure((size_t)sq.rows, (size_t)256)) return hipErrorOutOfMemory;
  const int rows = (int)tab.size();
  if (rows > sq.rows) return hipErrorInvalidValue;
  int max_n = 0;
  for (int r = 0; r < rows; r++) {
    sg.h_estep[r] = tab[r];
    max_n = std::max(max_n, tab[r].n);
  }
  if (max_n < 1) return hipSuccess;
  if (max_n > sq.blocks * kEqBlock) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(sq.desc, sg.h_estep, (size_t)rows * sizeof(EqStepRow), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) e = launch_eq_step(q, rows, sq.blocks * kEqBlock, audio, row, sq.desc, sq.dev, sq.eq.n, sq.carry, sq.scratch, sq.out);
  return e;
}

// stream_next. A PCM sink: the chunk leaves as int16 or one G.711 byte per sample — converted by a kernel behind the window's graph —
// instead of fp32; the step is the same in every other respect
int stream_step(piper_hip_voice* v, int slot, const Sink& out, int64_t* n_samples) {
  if (!v || !n_samples) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  const bool pcm = out.enc != PIPER_HIP_ENC_F32, want_out = out.host != nullptr;
  const size_t elem = fmt_elem(out.enc);
  const int law = sink_law(out);
  Slot* sp = slot_plan(v, slot);
  if (sp && sp->stream.items() > 1)
    PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds a group of %d streams: use stream_next_batch", slot, sp->stream.items());
  if (!sp || !sp->stream.single) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d has no stream in progress", slot);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  Slot& s = *sp;
  StreamRow& row = s.stream.rows[0];
  const int Ftrue = row.F;
  *n_samples = 0;
  if (row.next >= Ftrue) return PIPER_HIP_OK;  // end of stream
  const Window w = window_of(Ftrue, row.next, s.stream.chunk, s.stream.halo, v->hop);
  const int a = w.a, Fc = w.Fc;
  int64_t want = w.n;
  // a slot with a level: the limiter stands between the window's audio and the output stage, which then sees the limited range [lo, hi)
  // as its chunk (include/piper_hip.h "Level control")
  StreamLevel& lvl = s.stream.lv;
  LvStepRow lrow{};
  int64_t dn_s = (int64_t)row.next * v->hop, lim_hi = 0;  // where the output stage's chunk starts in the item
  int dn_skip = w.skip;
  if (lvl.on) {
    if (int rc0 = v->staging[slot].h_desc.ensure(kLvStageInts)) return rc0;
    lrow = level_range(row, w, v->hop, &dn_s, &lim_hi);
    want = lim_hi - dn_s;
    dn_skip = 0;
  }
  const int64_t dn_n = want;
  // a slot with an output rate of its own delivers int16 only: the chunk goes through the resampling step kernel instead of the flat one
  StreamRate& rs = s.stream.rs;
  const RsDesign* rd = nullptr;
  RsFilter rf{};
  RsStepRow rrow{};
  if (rs.rate) {
    if (!pcm) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next: slot %d delivers at %d Hz: use stream_next_pcm16", slot, rs.rate);
    if (!want_out) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next_pcm16: a stream with an output rate needs a buffer");
    int rc0 = voice_filter(v, rs.rate, &rd, &rf);
    if (!rc0) rc0 = v->staging[slot].h_desc.ensure(kRateStageInts);
    if (rc0) return rc0;
    int64_t j0, j1;
    rate_range(*rd, dn_s, dn_s + dn_n, (int64_t)Ftrue * v->hop, &j0, &j1);
    rrow = RsStepRow{dn_s, j0, dn_skip, (int)dn_n, (int)(j1 - j0), 0};
    want = j1 - j0;
  }
  if (want_out && out.cap < want) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_next: buffer holds %lld < %lld samples", (long long)out.cap, (long long)want);
  // generator-only plan of the window's bucket (first / interior / last windows of a stream usually share one)
  Slot* gs = nullptr;
  bool built = false;
  int rc = acquire_plan(v, PLAN_GENERATOR, 0, bucket_f(Fc), 1, &gs, &built);
  if (rc) return rc;
  if (row.gf && (rc = volume_step_buffers(v, slot, s.stream, (size_t)gs->n_samples * sizeof(float)))) return rc;
  gs->in_use = true;
  gs->last_use = ++v->use_clock;
  v->windows[slot] = WindowRecord{gs, gs->last_use, {Fc}};
  const int I = v->cfg.inter;
  hipError_t e = hipStreamWaitEvent(gs->set.stream, s.set.ev1, 0);
  int lens[2] = {0, Fc};
  if (e == hipSuccess) e = hipMemcpyAsync(gs->lensF, &lens[1], sizeof(int), hipMemcpyHostToDevice, gs->set.stream);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(gs->zin, (size_t)gs->F * sizeof(float), s.z_out + a, (size_t)s.F * sizeof(float), (size_t)Fc * sizeof(float), (size_t)I,
                         hipMemcpyDeviceToDevice, gs->set.stream);
  if (e == hipSuccess && gs->spk_bias)  // the item's conv_pre row travels with its latent window
    e = hipMemcpyAsync(gs->spk_bias, s.spk_bias + v->spk_pre_off, (size_t)v->cfg.up_initial * sizeof(float), hipMemcpyDeviceToDevice, gs->set.stream);
  if (e == hipSuccess && launch_plan(v, *gs)) e = hipErrorUnknown;
  const float* win_audio = gs->audio;  // the window's audio, or — the item has a volume — its chunk under the envelope, at the same place
  if (row.gf) {
    const VolStepRow vr = volume_range(row, w, v->hop);
    if (e == hipSuccess) e = volume_step(v, slot, s.stream, &vr, 1, gs->audio, 0, gs->set.stream);
    win_audio = s.stream.vol;
  }
  if (s.stream.eq.on) {  // (the EQ'd chunk at the same place: the later stages read it as they read the window's)
    const std::vector<EqStepRow> er{EqStepRow{(int64_t)row.next * v->hop, w.skip, (int)w.n}};
    if (e == hipSuccess) e = eq_step(v, slot, s.stream, er, win_audio, 0, (size_t)gs->n_samples * sizeof(float), gs->set.stream);
    win_audio = s.stream.eq.out;
  }
  const float* chunk_audio = win_audio;  // what the output stage reads, its chunk behind dn_skip
  if (lvl.on) {  // (with or without a buffer: the row's carry moves on with the stream)
    LvStepRow* h = (LvStepRow*)(v->staging[slot].h_desc + kLvStageOff);
    if (e == hipSuccess) { *h = lrow; e = hipMemcpyAsync(lvl.desc, h, sizeof(LvStepRow), hipMemcpyHostToDevice, gs->set.stream); }
    if (e == hipSuccess)
      e = launch_level_step(gs->set.stream, 1, s.stream.chunk * v->hop, win_audio, 0, lvl.desc, lvl.carry, lvl.p, lvl.lim, lvl.row);
    chunk_audio = lvl.lim;
  }
  if (pcm && want_out) {
    PcmRoute r;
    const size_t dev_samples = (size_t)std::max<int64_t>(std::max<int64_t>((int64_t)gs->F * v->hop, want), rd ? rs_step_bound(*rd, (int64_t)gs->F * v->hop) : 0);
    if (e == hipSuccess) rc = pcm_route(v, *gs, v->staging[slot], out.host, elem, (size_t)want, dev_samples, &r);
    if (rd) {  // (every step ends with a wait: the staged descriptor of the previous one has been read)
      RsStepRow* h = (RsStepRow*)(v->staging[slot].h_desc + kDescStageInts);
      if (e == hipSuccess && !rc) { *h = rrow; e = hipMemcpyAsync(rs.desc, h, sizeof(RsStepRow), hipMemcpyHostToDevice, gs->set.stream); }
      if (e == hipSuccess && !rc)
        e = launch_resample_step(gs->set.stream, 1, rrow.count, chunk_audio, 0, rs.desc, rs.hist + (size_t)rs.parity * rs.rows * kRsHist,
                                 rs.hist + (size_t)(rs.parity ^ 1) * rs.rows * kRsHist, rf, out.gain, r.kdst, law);
    } else if (e == hipSuccess && !rc) {
      e = launch_pcm16_flat(gs->set.stream, chunk_audio + dn_skip, want, out.gain, r.kdst, law, v->ctx->num_cus);
    }
    if (e == hipSuccess && !rc) rc = pcm_land(v->staging[slot], r, gs->set.stream, out.host, elem, (size_t)want);
    if (e == hipSuccess && !rc && r.mapped && !r.caller_pinned) memcpy(out.host, r.stage, (size_t)want * elem);
    if (e != hipSuccess || rc) (void)hipStreamSynchronize(gs->set.stream);  // nothing of the window may still run when its plan goes idle
  } else {
    if (e == hipSuccess && want_out)
      e = hipMemcpyAsync(out.host, chunk_audio + dn_skip, (size_t)want * elem, hipMemcpyDeviceToHost, gs->set.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(gs->set.stream);
  }
  gs->in_use = false;
  evict_idle_plans(v);
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream_next: %s", hipGetErrorString(e));
  if (rc) return rc;
  *n_samples = want;
  row.next = w.end;
  row.lim_lo = lim_hi;
  rs.started = true;
  if (rd) rs.parity ^= 1;
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_next(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples, int64_t* n_samples) {
  return stream_step(v, slot, Sink{host_audio, max_samples}, n_samples);
}

// ---- batched streaming: a group of n utterances on one slot, the next chunk of every active item in one generator launch ------------
namespace {

constexpr int kMaxGroup = 256;

// The generator's batch of a batched stream of n rows: n rounded up to a power of two, fixed for the life of the group or pool.
int group_batch(int n) {
  int NBg = 1;
  while (NBg < n) NBg <<= 1;
  return NBg;
}

// The limits of a step of n rows of chunk_frames each, reported in the name of the entry point `who`.
int check_step_size(const piper_hip_voice* v, const char* who, int n, int chunk_frames) {
  if (chunk_frames < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: chunk_frames must be >= 1", who);
  if ((int64_t)chunk_frames * v->hop * n > 0x3fffffff) PH_FAIL(PIPER_HIP_ERR_SHAPE, "%s: %d × %d frames per step too many", who, n, chunk_frames);
  return PIPER_HIP_OK;
}
// The per-step descriptor (kDescSrc … kDescInts: pcm16.h, shared with the int16 pack kernel): one row of kDescInts per generator row — source
// item, window start a, window length Fc (0: finished, dropped or pad row), halo skip (f0 − a)·hop, samples of the chunk, offset of the
// chunk in the packed output.

// z windows of one step → the generator plan's input: row r of zin [NBg][I][Fg] = z[src][:, a .. a + Fc), zero past Fc; lensF[r] = Fc.
// One thread per 4 frames of one channel, so the loads run along frames (coalesced); float4 loads where the window start is 16-byte
// aligned (z rows are bucket rows, F % 16 == 0). A row of length 0 writes only its length.
// The latent of source item src is z + src·I·Fz, rows of Fz floats (a group: the front plan's z), or, where `rows` is given, the row store
// rows[src] (a pool: base pointer and row stride from the table). The choice is the same for every thread of the launch.
__global__ __launch_bounds__(256) void stream_window_gather_kernel(const float* __restrict__ z, int Fz, const PoolRowRef* __restrict__ rows,
                                                                  const int* __restrict__ desc, float* __restrict__ zin,
                                                                  int* __restrict__ lensF, int I, int Fg, const float* __restrict__ spk_src,
                                                                  int64_t spk_stride, float* __restrict__ spk_dst, int U) {
  const int r = blockIdx.y;
  const int* d = desc + r * kDescInts;
  const int src = d[kDescSrc], a = d[kDescA], Fc = d[kDescFc];
  if (blockIdx.x == 0 && threadIdx.x == 0) lensF[r] = Fc;
  // a voice with speakers (spk_dst): the source item's conv_pre row [U] moves with its latent — spk_src + src·spk_stride → row r
  if (spk_dst && blockIdx.x == 0)
    for (int i = threadIdx.x; i < U; i += 256) spk_dst[(int64_t)r * U + i] = spk_src[(int64_t)src * spk_stride + i];
  if (Fc == 0) return;
  const int q4 = Fg >> 2;  // Fg % 16 == 0
  const int total = I * q4;
  int64_t F;
  const float* zr;
  if (rows) {
    F = rows[src].stride;
    zr = rows[src].z + a;
  } else {
    F = Fz;
    zr = z + (int64_t)src * I * Fz + a;
  }
  float* out = zin + (int64_t)r * I * Fg;
  const bool vec = (a & 3) == 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i / q4, j = (i - c * q4) * 4;
    const float* zp = zr + (int64_t)c * F + j;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j < Fc) {
      if (vec) {  // a + j is a multiple of 4 below F (a multiple of 16): all four lie in the row
        const float4 t = *(const float4*)zp;
        v.x = t.x; v.y = j + 1 < Fc ? t.y : 0.0f; v.z = j + 2 < Fc ? t.z : 0.0f; v.w = j + 3 < Fc ? t.w : 0.0f;
      } else {
        v.x = zp[0];
        if (j + 1 < Fc) v.y = zp[1];
        if (j + 2 < Fc) v.z = zp[2];
        if (j + 3 < Fc) v.w = zp[3];
      }
    }
    *(float4*)(out + (int64_t)c * Fg + j) = v;
  }
}

// Each active row's chunk out of the generator plan's audio [NBg][row] (the halo samples dropped), packed back to back.
__global__ __launch_bounds__(256) void stream_chunk_pack_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ desc,
                                                                float* __restrict__ out) {
  const int* d = desc + blockIdx.y * kDescInts;
  const int n = d[kDescN];
  if (n == 0) return;
  const float* src = audio + (int64_t)blockIdx.y * row + d[kDescSkip];
  float* dst = out + d[kDescOff];
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) && (n & 3) == 0) {
    for (int i = tid; i < (n >> 2); i += nth) ((float4*)dst)[i] = ((const float4*)src)[i];
  } else {
    for (int i = tid; i < n; i += nth) dst[i] = src[i];
  }
}

// A device buffer of the plan (released with it, see slot_release)
int plan_alloc(piper_hip_voice* v, Slot& s, size_t bytes, void** out) {
  const int rc = v->ctx->pool.alloc(bytes, out);
  if (rc) return rc;
  s.owned.push_back(*out);
  s.arena_bytes += bytes;
  return PIPER_HIP_OK;
}

void plan_free(piper_hip_voice* v, Slot& s, void* p, size_t bytes) {
  auto it = std::find(s.owned.begin(), s.owned.end(), p);
  if (it == s.owned.end()) return;
  s.owned.erase(it);
  s.arena_bytes -= bytes;
  (void)v->ctx->pool.release(p);
}

// A device buffer of a stream, from its owner: the plan (counted in its arena_bytes, kept across streams, released with it) or, for a
// streaming pool, the context pool (given back in pool_close). The one place that knows the difference.
int stream_alloc(piper_hip_voice* v, Stream& st, size_t bytes, void** out) {
  return st.plan ? plan_alloc(v, *st.plan, bytes, out) : v->ctx->pool.alloc(bytes, out);
}

// Gives back a buffer that a larger one replaces. Every step ends with a host wait, so nothing on the GPU still reads it.
void stream_free(piper_hip_voice* v, Stream& st, void* p, size_t bytes) {
  if (!p) return;
  if (st.plan) plan_free(v, *st.plan, p, bytes);
  else (void)v->ctx->pool.release(p);
}

// A packed-output buffer of at least `bytes` for the batched stream (no step is in flight: every step ends with a wait).
int pack_buffer(piper_hip_voice* v, Stream& st, size_t bytes) {
  if (st.single || st.pack_bytes >= bytes) return PIPER_HIP_OK;  // (a single stream packs nothing: its chunk is the window's own audio)
  bytes = round_up4((int64_t)bytes);
  void* p = nullptr;
  if (int rc = stream_alloc(v, st, bytes, &p)) return rc;
  stream_free(v, st, st.pack, st.pack_bytes);
  st.pack = p;
  st.pack_bytes = bytes;
  return PIPER_HIP_OK;
}

}  // namespace

// ---- streaming pool: the rows of a batched stream are taken and freed while it runs ------------------------------------------------------
namespace {

StreamPool* slot_pool(const piper_hip_voice* v, int slot) { return (v && slot >= 0 && slot < kMaxSlots) ? v->pools[slot].get() : nullptr; }

// A join's latents → the pool's row stores: entry j of `tab` copies the first F columns of item src of the work plan's z [n][I][Fw] into
// the store of pool row `row`, rows[row] = [I][stride], and zeroes the columns from F to stride, so a row never shows what an earlier, longer item left there.
// One thread per 4 frames of one channel, along frames (coalesced); both sides are bucket rows on 16-byte-aligned bases (Fw % 16 ==
// stride % 16 == 0, stride = bucket_f(F) ≤ Fw), so every access is an aligned float4 inside its row. blockIdx.y = the join's entry.
__global__ __launch_bounds__(256) void stream_adopt_kernel(const float* __restrict__ z, int Fw, const PoolJoinEnt* __restrict__ tab,
                                                          const PoolRowRef* __restrict__ rows, int I, const float* __restrict__ spk_src,
                                                          int64_t spk_stride, float* __restrict__ spk_rows, int U) {
  const PoolJoinEnt e = tab[blockIdx.y];
  const PoolRowRef rr = rows[e.row];
  // a voice with speakers (spk_rows): the item's conv_pre row [U] enters the pool with its latent and stays until the row is taken again
  if (spk_rows && blockIdx.x == 0)
    for (int i = threadIdx.x; i < U; i += 256) spk_rows[(int64_t)e.row * U + i] = spk_src[(int64_t)e.src * spk_stride + i];
  const int stride = (int)rr.stride, q4 = stride >> 2;
  const int total = I * q4;
  const float* zi = z + (int64_t)e.src * I * Fw;
  float* out = (float*)rr.z;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i / q4, j = (i - c * q4) * 4;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j < e.F) {
      t = *(const float4*)(zi + (int64_t)c * Fw + j);
      if (j + 1 >= e.F) t.y = 0.0f;
      if (j + 2 >= e.F) t.z = 0.0f;
      if (j + 3 >= e.F) t.w = 0.0f;
    }
    *(float4*)(out + (int64_t)c * stride + j) = t;
  }
}

// stream_adopt_kernel for a bounded join (stream_pool_join_bounded): the item's frame count is not a table entry but the work plan's
// device lensF[src], which dp_paths_kernel decided on the same stream just before the flow. Entry j's F is the join's bound (cap); the
// kernel copies min(lensF, cap, stride, Fw) columns — every index below comes from that clamped length — and zeroes the rest of the row up
// to its stride. The same layout rules hold (Fw % 16 == stride % 16 == 0, 16-byte-aligned bases), so every access is an aligned float4
// inside its row. One thread per entry reports {wanted frames, cap} of the row to rep [capacity][2] (page-locked host memory, its device
// mapping): want[src] is dp_paths_kernel's count BEFORE clamping, the number the host decides "fits / over the bound" by.
__global__ __launch_bounds__(256) void stream_adopt_bounded_kernel(const float* __restrict__ z, int Fw, const int* __restrict__ lensF,
                                                                  const int32_t* __restrict__ want, const PoolJoinEnt* __restrict__ tab,
                                                                  const PoolRowRef* __restrict__ rows, int I, const float* __restrict__ spk_src,
                                                                  int64_t spk_stride, float* __restrict__ spk_rows, int U, int32_t* __restrict__ rep) {
  const PoolJoinEnt e = tab[blockIdx.y];
  const PoolRowRef rr = rows[e.row];
  if (spk_rows && blockIdx.x == 0)
    for (int i = threadIdx.x; i < U; i += 256) spk_rows[(int64_t)e.row * U + i] = spk_src[(int64_t)e.src * spk_stride + i];
  const int stride = (int)rr.stride, q4 = stride >> 2;
  const int cap = max(min(min(e.F, stride), Fw), 0);
  const int F = min(max(lensF[e.src], 0), cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) *(int2*)(rep + 2 * (int64_t)e.row) = make_int2(want[e.src], e.F);
  const int total = I * q4;
  const float* zi = z + (int64_t)e.src * I * Fw;
  float* out = (float*)rr.z;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i / q4, j = (i - c * q4) * 4;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j < F) {  // (j + 3 < Fw: j is a multiple of 4 below F ≤ Fw, and Fw % 4 == 0)
      t = *(const float4*)(zi + (int64_t)c * Fw + j);
      if (j + 1 >= F) t.y = 0.0f;
      if (j + 2 >= F) t.z = 0.0f;
      if (j + 3 >= F) t.w = 0.0f;
    }
    *(float4*)(out + (int64_t)c * stride + j) = t;
  }
}

int pool_free_rows(const StreamPool& P) {
  int k = 0;
  for (const auto& r : P.st.rows) k += r.active ? 0 : 1;
  return k;
}

// An event for a join's adopt: one that an earlier step has consumed, or a new one.
int pool_event(StreamPool& P, hipEvent_t* out) {
  if (!P.ev_free.empty()) {
    *out = P.ev_free.back();
    P.ev_free.pop_back();
    return PIPER_HIP_OK;
  }
  PH_HIP(hipEventCreateWithFlags(out, hipEventDisableTiming), PIPER_HIP_ERR_LAUNCH);
  return PIPER_HIP_OK;
}

// What a batched step needs to be told that the stream's record does not hold: a group's (batch_step) or a pool's (pool_step).
struct StepSource {
  const float* z;            // the latents as stream_window_gather_kernel takes them: z [n][I][Fz] …
  int Fz;
  const PoolRowRef* d_rows;  // … or the device row table
  const hipEvent_t* wait;    // "the latents are there": what the step's stream waits for (the GPU waits, the host does not)
  size_t n_wait;
  const float* spk;          // a voice with speakers: the items' conv_pre rows, item src at spk + src·spk_stride (null otherwise)
  int64_t spk_stride;
};

// stream_next_batch: the next chunk of every active row in one generator launch at the stream's fixed batch; *ran = a step ran and has
// been waited for (false: no active row, nothing was launched).
// A PCM sink: the chunks leave as int16 instead of fp32 — the int16 sibling of the pack kernel writes them into the same device and
// staging buffers, half filled, and half the bytes cross the bus — or as one G.711 byte per sample: a quarter filled, a quarter of the bytes.
// A mixed sink (out.byte_off): the step of a mixed slot (stream_next_batch_mixed). The generator part is the same.
// A resampling step packs int16 through resample_step_kernel and its own descriptor (st.rs).
int batched_step(piper_hip_voice* v, int slot, Stream& st, const StepSource& src, const Sink& out, int64_t* n_samples, bool* ran) {
  *ran = false;
  StreamRate& rs = st.rs;
  int64_t* const mix = out.byte_off;
  if (rs.mixed && !mix) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds a mixed-format stream: use stream_next_batch_mixed", slot);
  if (!rs.mixed && mix) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next_batch_mixed: slot %d is not mixed (stream_set_mixed)", slot);
  const bool pcm = mix || out.enc != PIPER_HIP_ENC_F32, want_out = out.host != nullptr;
  const size_t sample_bytes = mix ? 1 : fmt_elem(out.enc);  // (a mixed step's totals count bytes)
  const int law = sink_law(out);
  const float gain = out.gain;
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  std::vector<StreamRow>& rows = st.rows;
  const int n = st.items(), NBg = st.NBg, hop = v->hop;
  auto& sg = v->staging[slot];
  const RsDesign* rd = nullptr;
  RsFilter rf{};
  int rc;
  if (rs.rate) {
    if (!pcm) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next_batch: slot %d delivers at %d Hz: use stream_next_batch_pcm16", slot, rs.rate);
    if (!want_out) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next_batch_pcm16: a stream with an output rate needs a buffer");
    if ((rc = voice_filter(v, rs.rate, &rd, &rf))) return rc;
  }
  StreamLevel& lvl = st.lv;
  if ((rc = sg.h_desc.ensure(lvl.on ? kLvStageInts : mix ? kMixStageInts : rd ? kRateStageInts : kDescStageInts))) return rc;
  LvStepRow* lrow = (LvStepRow*)(sg.h_desc + kLvStageOff);  // (only touched on a slot with a level)
  std::vector<int64_t> lim_hi(n, 0);
  RsStepRow* rrow = (RsStepRow*)(sg.h_desc + kDescStageInts);  // (only touched when rd)
  MixStepRow* mrow = (MixStepRow*)(sg.h_desc + kDescStageInts);  // (only touched when mix: the same place)
  std::vector<int64_t> cnt(n, 0);  // samples each item delivers in this step
  int max_cnt = 0;
  // the descriptor of this step (the previous step's upload has completed: every step ends with a wait)
  int* d = sg.h_desc;
  std::vector<Window> win(n);
  int64_t total = 0;
  int Fmax = 0;
  bool live = false;  // a row delivers in this step
  std::vector<int> ghost_end(n, -1);
  // a stream with a volume on some row: the step's VolStepRow table. A stream without one never builds it.
  bool any_vol = false;
  for (int r = 0; r < n; r++) any_vol = any_vol || (rows[r].active && rows[r].gf != nullptr);
  std::vector<VolStepRow> vrow;
  if (any_vol) vrow.assign((size_t)NBg, VolStepRow{nullptr, 0, 0, 0, 0, 0});
  for (int r = 0; r < NBg; r++) {
    int* e = d + (size_t)r * kDescInts;
    for (int k = 0; k < kDescInts; k++) e[k] = 0;
    e[kDescSrc] = r < n ? r : 0;
    if (rd) rrow[r] = RsStepRow{0, 0, 0, 0, 0, 0};
    if (mix) mrow[r] = MixStepRow{};
    if (lvl.on) lrow[r] = LvStepRow{0, 0, 0, 0};
    if (mix && r < n) mix[r] = round_up4(total);  // (a row that delivers nothing: where the next delivering row starts)
    if (r < n && !rows[r].active && rows[r].ghost) {  // a dropped item: length 0 in the step, its window only sizes the plan
      const Window g = window_of(rows[r].F, rows[r].next, st.chunk, st.halo, hop);
      Fmax = std::max(Fmax, g.Fc);
      ghost_end[r] = g.end;
    }
    if (r >= n || !rows[r].active) continue;
    live = true;
    const Window w = win[r] = window_of(rows[r].F, rows[r].next, st.chunk, st.halo, hop);
    if (any_vol) vrow[r] = volume_range(rows[r], w, hop);
    e[kDescA] = w.a;
    e[kDescFc] = w.Fc;
    // what the output stage takes for its chunk: the window's, or — a slot with a level — the limited range [lo, hi) in the row of lvl.lim
    int64_t dn_s = (int64_t)rows[r].next * hop, dn_n = w.n;
    int dn_skip = w.skip;
    if (lvl.on) {
      lrow[r] = level_range(rows[r], w, hop, &dn_s, &lim_hi[r]);
      dn_n = lim_hi[r] - dn_s;
      dn_skip = 0;
    }
    e[kDescSkip] = dn_skip;
    e[kDescN] = (int)dn_n;
    e[kDescOff] = (int)total;
    cnt[r] = dn_n;
    if (rd) {
      int64_t j0, j1;
      rate_range(*rd, dn_s, dn_s + dn_n, (int64_t)rows[r].F * hop, &j0, &j1);
      rrow[r] = RsStepRow{dn_s, j0, dn_skip, (int)dn_n, (int)(j1 - j0), (int)total};
      cnt[r] = j1 - j0;
      max_cnt = std::max(max_cnt, (int)(j1 - j0));
    }
    if (mix) {  // the row's own design, count, byte offset and descriptor (the filter table was uploaded when the format was supplied)
      const RowFormat& fm = rows[r].fmt;
      MixStepRow m{};
      m.s = dn_s;
      m.skip = dn_skip; m.n_in = (int)dn_n; m.count = (int)dn_n;
      m.elem = fmt_elem(fm.enc);
      m.law = m.elem == 1 ? fm.enc : 0;
      m.gain = fm.gain;
      if (fm.rate) {
        const RsDesign* fd = nullptr;
        RsFilter ff{};
        if ((rc = voice_filter(v, fm.rate, &fd, &ff))) return rc;
        int64_t j0, j1;
        rate_range(*fd, m.s, m.s + dn_n, (int64_t)rows[r].F * hop, &j0, &j1);
        m.j0 = j0; m.count = (int)(j1 - j0);
        m.taps = ff.taps; m.L = ff.L; m.M = ff.M; m.P = ff.P;
      }
      cnt[r] = m.count;
      if (m.count > 0) total = round_up4(total);  // (a row that delivers nothing owns no byte, pad included)
      m.off = mix[r];
      mrow[r] = m;
    }
    total += mix ? cnt[r] * mrow[r].elem : cnt[r];  // (a mixed step's total counts bytes)
    Fmax = std::max(Fmax, w.Fc);
  }
  for (int i = 0; i < n; i++) n_samples[i] = 0;
  if (!live) return PIPER_HIP_OK;  // end of the group / an idle pool (dropped items alone run no step)
  if (want_out && out.cap < total)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_next_batch: buffer holds %lld < %lld %s", (long long)out.cap, (long long)total, mix ? "bytes" : "samples");
  const size_t total_bytes = (size_t)total * sample_bytes;  // what the pack kernel writes and the host receives
  if (total_bytes > st.pack_bytes)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_next_batch: %lld samples exceed the group's %zu", (long long)total, st.pack_bytes / sizeof(float));
  if (want_out && (rc = sg.h_audio.ensure(mix ? ((size_t)total + 3) / 4 : rd ? ((size_t)total + 1) / 2 : (size_t)total, kAudioMinCap))) return rc;
  // generator-only plan of the step's longest window at the stream's batch size (rows past their end have length 0): a pool and a group
  // of the same size use the same plans
  Slot* gs = nullptr;
  bool built = false;
  if ((rc = acquire_plan(v, PLAN_GENERATOR, 0, bucket_f(Fmax), NBg, &gs, &built))) return rc;
  if (any_vol && (rc = volume_step_buffers(v, slot, st, (size_t)NBg * gs->n_samples * sizeof(float)))) return rc;
  gs->in_use = true;
  gs->last_use = ++v->use_clock;
  {
    WindowRecord& wr = v->windows[slot];
    wr.plan = gs;
    wr.stamp = gs->last_use;
    wr.Fc.assign((size_t)NBg, 0);
    for (int r = 0; r < n; r++) wr.Fc[r] = win[r].Fc;  // (a row that is not active kept the default window: Fc = 0)
  }
  const hipStream_t q = gs->set.stream;
  const int I = v->cfg.inter, Fg = gs->F;
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < src.n_wait; k++)
    if (e == hipSuccess) e = hipStreamWaitEvent(q, src.wait[k], 0);
  if (e == hipSuccess) e = hipMemcpyAsync(st.d_desc, d, (size_t)NBg * kDescInts * sizeof(int), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) {
    const int gx = (int)std::min<int64_t>(ceil_div((int64_t)I * (Fg / 4), 256), 64);
    hipLaunchKernelGGL(stream_window_gather_kernel, dim3(gx, NBg), dim3(256), 0, q, src.z, src.Fz, src.d_rows, st.d_desc, gs->zin, gs->lensF, I, Fg, src.spk,
                       src.spk_stride, src.spk ? gs->spk_bias : nullptr, v->cfg.up_initial);
    e = hipGetLastError();
  }
  if (e == hipSuccess && launch_plan(v, *gs)) e = hipErrorUnknown;
  const float* win_audio = gs->audio;  // the windows' audio, or — a delivering row has a volume — every row's chunk as it leaves the volume stage
  if (any_vol) {
    if (e == hipSuccess) e = volume_step(v, slot, st, vrow.data(), NBg, gs->audio, gs->n_samples, q);
    win_audio = st.vol;
  }
  if (st.eq.on) {  // every delivering row's chunk through the EQ, at the same place; a row that delivers nothing has n = 0
    std::vector<EqStepRow> er((size_t)NBg, EqStepRow{0, 0, 0});
    for (int r = 0; r < n; r++)
      if (rows[r].active) er[r] = EqStepRow{(int64_t)rows[r].next * hop, win[r].skip, (int)win[r].n};
    if (e == hipSuccess) e = eq_step(v, slot, st, er, win_audio, gs->n_samples, (size_t)NBg * gs->n_samples * sizeof(float), q);
    win_audio = st.eq.out;
  }
  const float* chunk_audio = win_audio;  // what the output stage reads: rows of chunk_row floats, each row's chunk behind its skip
  int64_t chunk_row = gs->n_samples;
  if (lvl.on) {
    if (e == hipSuccess) e = hipMemcpyAsync(lvl.desc, lrow, (size_t)NBg * sizeof(LvStepRow), hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = launch_level_step(q, NBg, st.chunk * hop, win_audio, gs->n_samples, lvl.desc, lvl.carry, lvl.p, lvl.lim, lvl.row);
    chunk_audio = lvl.lim;
    chunk_row = lvl.row;
  }
  if (e == hipSuccess) {
    const int px = (int)std::min<int64_t>(ceil_div((int64_t)st.chunk * hop, 1024), 64);
    if (mix) {
      int gx;
      size_t lds;
      mix_step_plan(mrow, NBg, px, &gx, &lds);
      e = hipMemcpyAsync(rs.mdesc, mrow, (size_t)NBg * sizeof(MixStepRow), hipMemcpyHostToDevice, q);
      if (e == hipSuccess)
        e = launch_mixed_step(q, NBg, gx, lds, chunk_audio, chunk_row, rs.mdesc, rs.hist + (size_t)rs.parity * rs.rows * kRsHist,
                              rs.hist + (size_t)(rs.parity ^ 1) * rs.rows * kRsHist, st.pack);
    } else if (rd) {
      e = hipMemcpyAsync(rs.desc, rrow, (size_t)NBg * sizeof(RsStepRow), hipMemcpyHostToDevice, q);
      if (e == hipSuccess)
        e = launch_resample_step(q, NBg, max_cnt, chunk_audio, chunk_row, rs.desc, rs.hist + (size_t)rs.parity * rs.rows * kRsHist,
                                 rs.hist + (size_t)(rs.parity ^ 1) * rs.rows * kRsHist, rf, gain, st.pack, law);
    } else if (pcm) {
      e = launch_stream_chunk_pack_pcm16(q, px, NBg, chunk_audio, chunk_row, st.d_desc, gain, st.pack, law);
    } else {
      hipLaunchKernelGGL(stream_chunk_pack_kernel, dim3(px, NBg), dim3(256), 0, q, chunk_audio, chunk_row, st.d_desc, (float*)st.pack);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && want_out) e = hipMemcpyAsync(sg.h_audio, st.pack, total_bytes, hipMemcpyDeviceToHost, q);
  if (e == hipSuccess) e = stream_wait(q);
  gs->in_use = false;
  evict_idle_plans(v);
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream_next_batch: %s", hipGetErrorString(e));
  *ran = true;
  if (want_out) memcpy(out.host, sg.h_audio, total_bytes);
  rs.started = true;
  if (rd || mix) rs.parity ^= 1;  // (a mixed step: whichever rows had a filter)
  for (int i = 0; i < n; i++) {
    n_samples[i] = cnt[i];
    if (ghost_end[i] >= 0) {
      rows[i].next = ghost_end[i];
      if (ghost_end[i] >= rows[i].F) rows[i].ghost = false;
    }
    if (!win[i].n) continue;
    rows[i].next = win[i].end;
    rows[i].lim_lo = lim_hi[i];
    if (win[i].end >= rows[i].F) rows[i].active = false;  // last chunk delivered (a pool: the row is free for the next join)
  }
  return PIPER_HIP_OK;
}

// The bounded joins since the last resolve (stream_pool_join_bounded) become ordinary rows: the host waits for each join's event — its
// adopt has run, and dp_paths_kernel before it — and reads what the adopt reported per row. F ≤ cap: the row is active with that F from
// here on. F > cap: the row is free again and remembers both numbers for stream_pool_item_samples; the join's other rows are not
// touched. A work slot that still holds the join's prepare learns its lengths and durations here (piper_hip_voice_durations).
int pool_resolve(piper_hip_voice* v, StreamPool& P) {
  if (P.bounded.empty()) return PIPER_HIP_OK;
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  for (const auto& j : P.bounded) PH_HIP(hipEventSynchronize(j.ev), PIPER_HIP_ERR_LAUNCH);
  for (const auto& j : P.bounded) {
    Slot* w = v->attached[j.work_slot];
    if (w && w == j.plan && w->last_use == j.prepared && w->bounded_pending) (void)bounded_finish(v, j.work_slot, *w);  // (an item over its bound is the row's error)
  }
  P.bounded.clear();
  int bad = -1;
  for (int r = 0; r < P.st.items(); r++) {
    StreamRow& row = P.st.rows[r];
    StreamPool::Row& x = P.ext[r];
    if (!x.pending) continue;
    x.pending = false;
    const int want = P.h_rep[2 * r], cap = P.h_rep[2 * r + 1];
    if (want >= 1 && want <= cap && cap <= x.stride) {
      row.F = want;
      row.next = 0;
      x.held = true;
    } else {
      row.active = false;
      x.over_want = want > cap ? want : 0;
      x.over_cap = cap;
      if (want <= cap) bad = r;
    }
  }
  if (bad >= 0) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream pool: the device reported no frame count for row %d (the row is free)", bad);
  return PIPER_HIP_OK;
}

// stream_next_batch on a pool slot: the latents are the row stores, ready when the adopts of the joins since the last step have run
int pool_step(piper_hip_voice* v, int slot, StreamPool& P, const Sink& out, int64_t* n_samples) {
  if (int rc0 = pool_resolve(v, P)) return rc0;
  const StepSource src{nullptr, 0, P.d_rows, P.ev_pending.data(), P.ev_pending.size(), P.spk_rows, v->cfg.up_initial};
  bool ran = false;
  const int rc = batched_step(v, slot, P.st, src, out, n_samples, &ran);
  if (rc || !ran) return rc;  // (an idle pool: joins since the last step stay pending)
  // the step's wait covers the adopts its stream waited for: their events can be recorded again
  P.ev_free.insert(P.ev_free.end(), P.ev_pending.begin(), P.ev_pending.end());
  P.ev_pending.clear();
  return PIPER_HIP_OK;
}

}  // namespace

PH_EXPORT int piper_hip_voice_stream_begin_batch(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot, int chunk_frames) {
  const ControlsClear cc{v, slot};  // a staging call: the slot id's prosody, volume and pitch are this call's, on every way out
  if (int prc = refuse_pitch(v, slot, "stream_begin_batch")) return prc;
  if (!v || !utts) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (n < 1 || n > kMaxGroup) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_begin_batch: group of %d outside [1,%d]", n, kMaxGroup);
  if (int rc = check_step_size(v, "stream_begin_batch", n, chunk_frames)) return rc;
  int rc = piper_hip_voice_prepare_batch(v, utts, n, slot);  // encoder (+ predictor) inputs of the whole group on one plan
  if (rc < 0) return rc;
  Slot& s = *v->attached[slot];
  Stream& st = s.stream;  // (no stream is in progress: the prepare reset it; the buffers of an earlier one are still the plan's)
  st.plan = &s;
  if (!st.d_desc) {
    void* p = nullptr;
    if ((rc = stream_alloc(v, st, (size_t)kMaxGroup * kDescInts * sizeof(int), &p))) return rc;
    st.d_desc = (int*)p;
  }
  if ((rc = pack_buffer(v, st, (size_t)n * chunk_frames * v->hop * sizeof(float)))) return rc;
  const float* gf = nullptr;  // the items' gains per frame [n][F] where the request carried a volume
  if ((rc = stream_volume_begin(v, s, &gf))) return rc;
  if ((rc = launch_front(s))) return rc;
  st.chunk = chunk_frames;
  st.halo = generator_halo_frames(v->cfg);
  st.NBg = group_batch(n);
  st.rows.resize(n);
  for (int b = 0; b < n; b++) {
    st.rows[b] = StreamRow{s.h_F[b], 0, s.h_F[b] > 0};
    st.rows[b].gf = gf ? gf + (size_t)b * s.F : nullptr;
  }
  int steps = 0;
  for (int b = 0; b < n; b++) steps = std::max(steps, (int)ceil_div(s.h_F[b], chunk_frames));
  return steps;
}

namespace {
// stream_next_batch. A group's latents are the front plan's z, ready when its ev1 fires.
int batch_step(piper_hip_voice* v, int slot, const Sink& out, int64_t* n_samples) {
  if (!v || !n_samples) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (StreamPool* P = slot_pool(v, slot)) return pool_step(v, slot, *P, out, n_samples);
  Slot* sp = slot_plan(v, slot);
  if (!sp || sp->stream.single || sp->stream.rows.empty()) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d has no batched stream in progress", slot);
  Slot& s = *sp;
  const StepSource src{s.z_out, s.F, nullptr, &s.set.ev1, 1, s.spk_bias ? s.spk_bias + v->spk_pre_off : nullptr, v->spk.Ctot};
  bool ran = false;
  return batched_step(v, slot, s.stream, src, out, n_samples, &ran);
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_next_batch(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples, int64_t* n_samples) {
  return batch_step(v, slot, Sink{host_audio, max_samples}, n_samples);
}

PH_EXPORT int piper_hip_voice_stream_drop(piper_hip_voice* v, int slot, int item) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (StreamPool* P = slot_pool(v, slot)) {  // the session in that row leaves: the row is free for the next join
    if (item < 0 || item >= P->st.items()) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_drop: item %d outside [0,%d)", item, P->st.items());
    P->st.rows[item].active = false;
    P->ext[item].pending = false;  // (a bounded join still in flight: ev_pending keeps its adopt away from the row's next occupant)
    return PIPER_HIP_OK;
  }
  Slot* sp = slot_plan(v, slot);
  if (!sp || sp->stream.single || sp->stream.rows.empty()) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d has no batched stream in progress", slot);
  const int n = sp->stream.items();
  if (item < 0 || item >= n) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_drop: item %d outside [0,%d)", item, n);
  StreamRow& row = sp->stream.rows[item];
  if (row.active) row.ghost = row.next < row.F;
  row.active = false;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_pool_open(piper_hip_voice* v, int slot, int capacity, int chunk_frames) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (capacity < 1 || capacity > kMaxGroup) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_open: capacity %d outside [1,%d]", capacity, kMaxGroup);
  if (int rc = check_step_size(v, "stream_pool_open", capacity, chunk_frames)) return rc;
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  pool_close(v, slot);
  detach(v, slot);  // what the slot id held is replaced, as by a prepare
  v->planned = true;
  std::unique_ptr<StreamPool> P(new StreamPool());
  Stream& st = P->st;
  st.NBg = group_batch(capacity);
  st.chunk = chunk_frames;
  st.halo = generator_halo_frames(v->cfg);
  st.rows.resize(capacity);
  P->ext.resize(capacity);
  void* p = nullptr;
  int rc = v->ctx->pool.alloc((size_t)st.NBg * sizeof(PoolRowRef) + (size_t)capacity * sizeof(PoolJoinEnt), &p);
  if (!rc) P->d_rows = (PoolRowRef*)p;
  if (!rc) { rc = stream_alloc(v, st, (size_t)st.NBg * kDescInts * sizeof(int), &p); if (!rc) st.d_desc = (int*)p; }
  if (!rc) rc = pack_buffer(v, st, (size_t)capacity * chunk_frames * v->hop * sizeof(float));
  if (!rc && v->spk.S) {  // the rows' conv_pre biases; a row never taken reads as 0.0
    const size_t bytes = (size_t)capacity * v->cfg.up_initial * sizeof(float);
    rc = v->ctx->pool.alloc(bytes, &p);
    if (!rc) {
      P->spk_rows = (float*)p;
      if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipGetLastError(); rc = PIPER_HIP_ERR_LAUNCH; ph::set_error("stream_pool_open: clearing the speaker rows failed"); }
    }
  }
  v->pools[slot] = std::move(P);
  if (rc) { pool_close(v, slot); return rc; }
  return PIPER_HIP_OK;
}

namespace {
// launch_front for a join that must not wait: a plan whose front has no graph yet runs the front steps eagerly — that run is the join's
// answer — and captures the graph behind it, as launch_plan does for a plan's first run (the capture enqueues nothing).
int launch_front_async(Slot& s) {
  if (s.front_exec) return launch_front(s);
  const std::vector<int> front = front_steps(s);
  int rc = run_steps(s, front, s.set.stream);
  if (rc) return rc;
  PH_HIP(hipEventRecord(s.set.ev1, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  return capture_graph(s.set.stream, [&](hipStream_t q) { return run_steps(s, front, q); }, &s.front_graph, &s.front_exec, "stream");
}

// stream_pool_join; fmts != nullptr: stream_pool_join_formats — one format per joining item of a mixed pool (nullptr there: the default).
// bound > 0: stream_pool_join_bounded — the work slot is prepared by prepare_batch_bounded, the frame counts stay on the device and the
// rows are pending until pool_resolve; nothing below waits for the GPU then, but for the two waits the header names.
int pool_join(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot, const piper_hip_stream_format* fmts,
              bool with_formats, int* items_out, int64_t* samples_out, int bound = 0) {
  const ControlsClear cc{v, work_slot};  // a staging call: the work slot's prosody, volume and pitch are this join's, on every way out
  if (int prc = refuse_pitch(v, work_slot, "stream_pool_join")) return prc;
  if (!v || !utts) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  StreamPool* P = slot_pool(v, slot);
  if (!P) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds no streaming pool", slot);
  Stream& st = P->st;
  const int capacity = st.items();
  if (with_formats && !st.rs.mixed) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_join_formats: the pool on slot %d is not mixed (stream_set_mixed)", slot);
  if (with_formats && !fmts) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_join_formats: null formats");
  if (work_slot < 0 || work_slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "work slot %d out of range [0,%d)", work_slot, kMaxSlots);
  if (work_slot == slot) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_join: the work slot is the pool's slot %d", slot);
  if (slot_pool(v, work_slot)) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_join: work slot %d holds a streaming pool", work_slot);
  if (n < 1) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_pool_join: %d items", n);
  const int free_rows = pool_free_rows(*P);
  if (n > free_rows) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_pool_join: %d items, %d free rows of %d", n, free_rows, capacity);
  const RsDesign* rate_d = nullptr;  // samples_out counts what the pool delivers
  if (st.rs.rate)
    if (int rc0 = rs_design(v->cfg.sample_rate, st.rs.rate, &rate_d)) return rc0;
  // a mixed pool: the joining items' formats, checked on the host, their filter tables uploaded here (never inside a step), and a packed
  // buffer that holds a step of the rows as they will stand (no step is in flight: every step ends with a wait)
  std::vector<RowFormat> jf(st.rs.mixed ? n : 0);
  if (with_formats)
    for (int i = 0; i < n; i++)
      if (int rc0 = check_format(v, "stream_pool_join_formats", fmts[i], &jf[i])) return rc0;
  if (st.rs.mixed) {
    PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
    int64_t bytes = 0;
    for (const auto& r : st.rows) bytes += r.active ? fmt_step_bytes(v, r.fmt, step_samples(v, st)) : 0;
    for (int i = 0; i < n; i++) {
      RsFilter ff{};
      if (jf[i].rate)
        if (int rc0 = voice_filter(v, jf[i].rate, nullptr, &ff)) return rc0;
      bytes += fmt_step_bytes(v, jf[i], step_samples(v, st));
    }
    if (int rc0 = pack_buffer(v, st, (size_t)bytes)) return rc0;
  }
  // encoder (+ predictor) inputs of the join on the work slot's plan, then encoder + flow on that plan's stream
  int rc = bound ? piper_hip_voice_prepare_batch_bounded(v, utts, n, work_slot, bound) : piper_hip_voice_prepare_batch(v, utts, n, work_slot);
  if (rc < 0) return rc;
  Slot& w = *v->attached[work_slot];
  const int I = v->cfg.inter;
  // a bounded join: every row has the work plan's frame bucket for its stride (w.h_F holds that bucket until the lengths are known)
  auto item_stride = [&](int i) { return bound ? w.F : bucket_f(w.h_F[i]); };
  int32_t* want_rep = nullptr;  // bounded: the device mapping of the work slot's report (dp_paths_kernel's counts before clamping)
  if (bound) {
    // the pool's own report, allocated by its first bounded join (capacity >= 1: pool_open refuses less), and the work slot's
    if (!P->d_rep) {
      if ((rc = P->h_rep.ensure((size_t)capacity * 2, (size_t)capacity * 2))) return rc;
      P->d_rep = P->h_rep.mapped();
    }
    want_rep = v->staging[work_slot].h_res.mapped();
    if (!P->d_rep || !want_rep)
      PH_FAIL(PIPER_HIP_ERR_UNAVAILABLE, "stream_pool_join_bounded: page-locked memory has no device mapping on this system");
  }
  // rows, lowest free index first, and their stores. Nothing of the pool changes before everything that can fail has succeeded.
  std::vector<int> take;
  for (int r = 0; r < capacity && (int)take.size() < n; r++)
    if (!st.rows[r].active) take.push_back(r);
  auto& sg = v->staging[work_slot];  // free: prepare_batch waited for whatever used this slot id's staging before
  const size_t tab_ints = (size_t)st.NBg * sizeof(PoolRowRef) / sizeof(int), join_ints = (size_t)n * sizeof(PoolJoinEnt) / sizeof(int);
  if ((rc = sg.h_desc.ensure((size_t)kMaxGroup * (sizeof(PoolRowRef) + sizeof(PoolJoinEnt)) / sizeof(int)))) return rc;
  int stride_max = 0;
  for (int i = 0; i < n; i++) {
    auto& r = P->ext[take[i]];
    const int stride = item_stride(i);
    stride_max = std::max(stride_max, stride);
    const size_t need = (size_t)I * stride;
    if (w.vol_on && r.gf_cap < (size_t)stride) {  // the occupant's gains per frame, next to its latent (the wait: as for the latent below)
      for (hipEvent_t ev : P->ev_pending) PH_HIP(hipEventSynchronize(ev), PIPER_HIP_ERR_LAUNCH);
      void* p = nullptr;
      if ((rc = v->ctx->pool.alloc((size_t)stride * sizeof(float), &p))) return rc;
      if (r.gf) (void)v->ctx->pool.release(r.gf);
      r.gf = (float*)p;
      r.gf_cap = (size_t)stride;
    }
    if (r.cap >= need) continue;
    // a longer utterance takes the row: a larger store. No step is in flight (every step ends with a host wait); an adopt of a join
    // since the last step may still be writing the old store (joined, dropped, row taken again) — wait for those.
    for (hipEvent_t ev : P->ev_pending) PH_HIP(hipEventSynchronize(ev), PIPER_HIP_ERR_LAUNCH);
    void* p = nullptr;
    if ((rc = v->ctx->pool.alloc(need * sizeof(float), &p))) return rc;
    if (r.z) (void)v->ctx->pool.release(r.z);
    r.z = (float*)p;
    r.cap = need;
  }
  hipEvent_t ev = nullptr;
  if ((rc = pool_event(*P, &ev))) return rc;
  if ((rc = bound ? launch_front_async(w) : launch_front(w))) { P->ev_free.push_back(ev); return rc; }
  // The adopt runs on the work plan's own stream: behind its front graph, and ahead of everything that waits for that stream before the
  // plan's arena is reused (prepare on the same plan, detach, evict_idle_plans). It first waits for the adopts of earlier joins since the
  // last step: they read the tables this join uploads anew, and one of them may write a row this join takes again.
  const hipStream_t q = w.set.stream;
  PoolRowRef* tab = (PoolRowRef*)sg.h_desc.p;  // the whole row table as it stands after this join, then the join's own table
  PoolJoinEnt* jt = (PoolJoinEnt*)(sg.h_desc + tab_ints);
  for (int r = 0; r < st.NBg; r++) {
    tab[r].z = r < capacity ? P->ext[r].z : nullptr;
    tab[r].stride = r < capacity ? P->ext[r].stride : 0;
  }
  for (int i = 0; i < n; i++) {
    tab[take[i]].stride = item_stride(i);
    jt[i] = PoolJoinEnt{i, take[i], bound ? w.bounded_cap : w.h_F[i], 0};
  }
  hipError_t e = hipSuccess;
  for (hipEvent_t pe : P->ev_pending)
    if (e == hipSuccess) e = hipStreamWaitEvent(q, pe, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_rows, sg.h_desc, (tab_ints + join_ints) * sizeof(int), hipMemcpyHostToDevice, q);
  if (e == hipSuccess) {
    const int gx = (int)std::min<int64_t>(ceil_div((int64_t)I * (stride_max / 4), 256), 64);
    const float* spk_src = w.spk_bias ? w.spk_bias + v->spk_pre_off : nullptr;
    if (bound)
      hipLaunchKernelGGL(stream_adopt_bounded_kernel, dim3(gx, n), dim3(256), 0, q, w.z_out, w.F, w.lensF, want_rep,
                         (const PoolJoinEnt*)(P->d_rows + st.NBg), P->d_rows, I, spk_src, (int64_t)v->spk.Ctot, w.spk_bias ? P->spk_rows : nullptr,
                         v->cfg.up_initial, P->d_rep);
    else
      hipLaunchKernelGGL(stream_adopt_kernel, dim3(gx, n), dim3(256), 0, q, w.z_out, w.F, (const PoolJoinEnt*)(P->d_rows + st.NBg), P->d_rows, I,
                         spk_src, (int64_t)v->spk.Ctot, w.spk_bias ? P->spk_rows : nullptr, v->cfg.up_initial);
    e = hipGetLastError();
  }
  // a join with a volume: every item's gains per frame into its row's own store, behind the adopt on the same stream — from the work plan's
  // frame-to-id map and the lengths the device holds (a bounded join: what generate_path decided), so nothing here waits
  for (int i = 0; i < n && w.vol_on && e == hipSuccess; i++)
    e = launch_volume_frame_gains(q, w.lensF + i, std::min(w.F, item_stride(i)), 1, w.frame2id + (size_t)i * w.F, w.F, w.vol_gain + (size_t)i * w.T, w.T,
                                  P->ext[take[i]].gf);
  if (e == hipSuccess) e = hipEventRecord(ev, q);
  if (e != hipSuccess) { P->ev_free.push_back(ev); PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream_pool_join: %s", hipGetErrorString(e)); }
  P->ev_pending.push_back(ev);
  if (bound) P->bounded.push_back(StreamPool::BoundedJoin{ev, work_slot, &w, w.last_use});
  for (int i = 0; i < n; i++) {  // active from the next step on
    StreamRow& r = st.rows[take[i]];
    StreamPool::Row& x = P->ext[take[i]];
    x.stride = item_stride(i);
    r.F = bound ? 0 : w.h_F[i];  // (bounded: pool_resolve brings it before any step reads it)
    r.next = 0;
    r.active = true;
    r.gf = w.vol_on ? x.gf : nullptr;  // a new occupant brings its own gains, or none: never its predecessor's
    x.pending = bound != 0;
    x.held = !bound;
    x.over_want = x.over_cap = 0;
    r.fmt = st.rs.mixed ? jf[i] : RowFormat();
    if (items_out) items_out[i] = take[i];
    const RsDesign* item_d = rate_d;
    if (r.fmt.rate) (void)rs_design(v->cfg.sample_rate, r.fmt.rate, &item_d);  // (checked above)
    if (samples_out) samples_out[i] = item_d ? rs_count(*item_d, (int64_t)w.h_F[i] * v->hop) : (int64_t)w.h_F[i] * v->hop;
  }
  st.rs.started = true;  // the pool's output rate is fixed from its first join on
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_pool_join(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                               int* items_out, int64_t* samples_out) {
  return pool_join(v, slot, utts, n, work_slot, nullptr, false, items_out, samples_out);
}

PH_EXPORT int piper_hip_voice_stream_pool_join_formats(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                                       const piper_hip_stream_format* fmts, int* items_out, int64_t* samples_out) {
  return pool_join(v, slot, utts, n, work_slot, fmts, true, items_out, samples_out);
}

PH_EXPORT int piper_hip_voice_stream_pool_join_bounded(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                                       int max_frames, const piper_hip_stream_format* fmts, int* items_out) {
  const ControlsClear cc{v, work_slot};  // a staging call: the work slot's prosody, volume and pitch are this join's, on every way out
  if (int prc = refuse_pitch(v, work_slot, "stream_pool_join_bounded")) return prc;
  if (!v || !utts) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  // prepare_batch_bounded's own refusals, before anything of the pool is looked at or regrown (it repeats them)
  if (int rc = bounded_refusals(v, utts, n, work_slot, max_frames, true)) return rc;
  return pool_join(v, slot, utts, n, work_slot, fmts, fmts != nullptr, items_out, nullptr, max_frames);
}

PH_EXPORT int piper_hip_voice_stream_pool_item_samples(piper_hip_voice* v, int slot, int item, int64_t* samples) {
  if (!v || !samples) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  StreamPool* P = slot_pool(v, slot);
  if (!P) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds no streaming pool", slot);
  if (item < 0 || item >= P->st.items()) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_item_samples: item %d outside [0,%d)", item, P->st.items());
  if (P->ext[item].pending)
    if (int rc = pool_resolve(v, *P)) return rc;
  const StreamPool::Row& r = P->ext[item];
  const StreamRow& row = P->st.rows[item];
  if (r.over_want > 0)
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream pool row %d: the predictor wants %d frames, the join allowed %d — the item delivers nothing and its row is "
                                 "free: join it again with a larger bound", item, r.over_want, r.over_cap);
  if (!r.held) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_pool_item_samples: row %d of the pool on slot %d holds no item whose length is known", item, slot);
  const int64_t N = (int64_t)row.F * v->hop;
  const int rate = P->st.rs.mixed ? row.fmt.rate : P->st.rs.rate;
  const RsDesign* d = nullptr;
  if (rate)
    if (int rc = rs_design(v->cfg.sample_rate, rate, &d)) return rc;
  *samples = d ? rs_count(*d, N) : N;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_pool_joins_pending(piper_hip_voice* v, int slot) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  const StreamPool* P = slot_pool(v, slot);
  if (!P) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds no streaming pool", slot);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  int k = 0;
  for (hipEvent_t ev : P->ev_pending) {  // one per join since the last step that ran
    const hipError_t e = hipEventQuery(ev);
    if (e == hipErrorNotReady) { k++; (void)hipGetLastError(); continue; }  // (not an error: nothing for the next launch check to find)
    if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "stream_pool_joins_pending: %s", hipGetErrorString(e));
  }
  return k;
}

PH_EXPORT int piper_hip_voice_stream_pool_free_rows(const piper_hip_voice* v, int slot) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  const StreamPool* P = slot_pool(v, slot);
  if (!P) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds no streaming pool", slot);
  return pool_free_rows(*P);
}

PH_EXPORT int piper_hip_voice_stream_pool_close(piper_hip_voice* v, int slot) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (!slot_pool(v, slot)) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds no streaming pool", slot);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  pool_close(v, slot);
  return PIPER_HIP_OK;
}

// ---- 16-bit PCM straight from the device (pcm16.hip): the launches go on the slot's stream behind the plan's graph, outside it -----------
namespace {
// collect_pcm16, and collect_pcm16_rate where out_rate differs from the voice's own: then item b is J(its true samples) long and the pack
// kernel's place is taken by the resampling one (rd / rf: its filter); everything else — the peaks, the route, the landing — is shared.
// A G.711 sink: collect_g711 — the same kernels with their one-byte sink, the host buffer a byte buffer. The sink's gain is the params',
// read here behind the slot's own refusal.
int collect_pcm(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int out_rate, Sink out) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  const size_t elem = fmt_elem(out.enc);
  const int law = sink_law(out);
  void* const host_pcm = out.host;
  Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  bool normalize;
  int rc = pcm_params(params, &out.gain, &normalize);
  if (rc) return rc;
  if (normalize && v->slot_lv[slot].on)
    PH_FAIL(PIPER_HIP_ERR_ARG, "collect_pcm16: normalize = 1 on slot %d, which has a level (piper_hip_voice_slot_level)", slot);
  if (normalize && v->slot_ld[slot].on)
    PH_FAIL(PIPER_HIP_ERR_ARG, "collect_pcm16: normalize = 1 on slot %d, which has a loudness (piper_hip_voice_slot_loudness)", slot);
  const float gain = out.gain;
  const RsDesign* rd = nullptr;
  RsFilter rf{};
  if (out_rate != v->cfg.sample_rate) {
    if ((rc = rs_design(v->cfg.sample_rate, out_rate, &rd))) return rc;  // (a rate outside the contract is refused before anything waits)
    if (host_pcm) {
      PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
      if ((rc = voice_filter(v, out_rate, &rd, &rf))) return rc;
    }
  }
  const auto out_len = [&](int64_t samples) { return rd ? rs_count(*rd, samples) : samples; };
  if (!host_pcm) return piper_hip_voice_collect(v, slot, nullptr, 0);  // just wait (a bounded slot: and learn the lengths)
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  Slot& s = *p;
  auto& sg = v->staging[slot];
  const int NB = s.NB, hop = v->hop;
  if (NB > kMaxGroup) PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect_pcm16: %d items (at most %d)", NB, kMaxGroup);
  Chain chain = chain_geometry(v, s);  // the items the sinks read: their geometry for the bounds, then the walk's
  const int F = chain.F;  // frames of a row of the items
  const int F_own = row_frames(v, s);
  const bool bounded = s.bounded_pending;
  // a slot id with a join: the sinks read the programme, ONE item whose length the device knows, the caller makes room for its bound
  const bool joined = v->slot_jn[slot].on;
  int64_t jcap = 0;
  if (joined && (rc = join_capacity(v, slot, s, &jcap))) return rc;
  // a bounded slot's lengths are still on the device: the caller makes room for the capacity, as for collect
  int64_t need = 0;
  if (joined) need = out_len(jcap);
  else for (int b = 0; b < NB; b++) need += out_len(item_samples(v, s, b, bounded ? F_own : s.h_F[b]));
  if (out.cap < need) {
    if (joined)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect_pcm16: the join needs room for %lld samples (piper_hip_voice_join_capacity), got %lld", (long long)need,
              (long long)out.cap);
    if (bounded)
      PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect_pcm16: a bounded slot needs room for its capacity (%lld samples: piper_hip_voice_%s_samples before collect), got %lld",
              (long long)need, s.chain.pt_on ? "pitch" : "prepared", (long long)out.cap);
    PH_FAIL(PIPER_HIP_ERR_SHAPE, "collect_pcm16: buffer holds %lld < %lld samples", (long long)out.cap, (long long)need);
  }
  float* peaks_host = nullptr;
  if (normalize) {
    if ((rc = plan_ensure(v, s, s.chain.peaks, (size_t)NB * sizeof(float)))) return rc;
    if ((rc = sg.h_peaks.ensure((size_t)kMaxGroup, (size_t)kMaxGroup))) return rc;
    peaks_host = sg.h_peaks.mapped();
  }
  PcmRoute r;
  const int64_t dev_samples = joined ? std::max(out_len(jcap), jcap) : std::max<int64_t>(out_len((int64_t)F * hop), (int64_t)F * hop) * NB;
  if ((rc = pcm_route(v, s, sg, host_pcm, elem, (size_t)need, (size_t)dev_samples, &r))) return rc;
  const hipStream_t q = s.set.stream;
  Chain peak_src;  // (the peak of normalize = 1 is that of the shaped, pitched, EQ'd items where there are a volume, a pitch, an EQ)
  if ((rc = chain_walk(v, slot, s, &peak_src, &chain))) return rc;
  const float* audio = chain.audio;
  float* const peaks = s.chain.peaks.as<float>();
  if (joined) {
    // The programme is one row of device-known length: the sinks take it as NB = 1, hop = 1, F = its bound, with the device's total as
    // the length. normalize = 1 takes ONE peak, over the programme (no level and no loudness then: the joined EQ'd items).
    Joined j;
    if ((rc = join_items(v, slot, s, chain, jcap, &j))) return rc;
    const int JF = (int)std::max<int64_t>(j.cap, 1);
    if (normalize) PH_HIP(launch_pcm16_peak(q, j.prog, JF, j.total, JF, 1, 1, peaks), PIPER_HIP_ERR_LAUNCH);
    if (rd)
      PH_HIP(launch_resample_items(q, j.prog, JF, j.total, JF, 1, 1, 0, rf, gain, normalize ? peaks : nullptr, peaks_host, r.kdst, (int)elem, law),
             PIPER_HIP_ERR_LAUNCH);
    else
      PH_HIP(launch_pcm16_pack(q, j.prog, JF, j.total, JF, 1, 1, gain, normalize ? peaks : nullptr, peaks_host, r.kdst, law), PIPER_HIP_ERR_LAUNCH);
    if (normalize && !peaks_host) PH_HIP(hipMemcpyAsync(sg.h_peaks, peaks, sizeof(float), hipMemcpyDeviceToHost, q), PIPER_HIP_ERR_LAUNCH);
    if ((rc = pcm_land(sg, r, q, host_pcm, elem, (size_t)need))) return rc;
    const int64_t total = out_len(join_landed(v, slot, s));
    if (bounded && (rc = bounded_finish(v, slot, s))) return rc;
    if (r.mapped && !r.caller_pinned) memcpy(host_pcm, r.stage, (size_t)total * elem);
    if (normalize) s.chain.h_peaks.assign(sg.h_peaks.p, sg.h_peaks + 1);
    return PIPER_HIP_OK;
  }
  if (normalize) PH_HIP(launch_pcm16_peak(q, peak_src.audio, chain.row, chain.lensF, F, hop, NB, peaks), PIPER_HIP_ERR_LAUNCH);
  if (rd)
    PH_HIP(launch_resample_items(q, audio, chain.row, chain.lensF, F, hop, NB, 0, rf, gain, normalize ? peaks : nullptr, peaks_host, r.kdst, (int)elem, law),
           PIPER_HIP_ERR_LAUNCH);
  else
    PH_HIP(launch_pcm16_pack(q, audio, chain.row, chain.lensF, F, hop, NB, gain, normalize ? peaks : nullptr, peaks_host, r.kdst, law), PIPER_HIP_ERR_LAUNCH);
  if (normalize && !peaks_host) PH_HIP(hipMemcpyAsync(sg.h_peaks, peaks, (size_t)NB * sizeof(float), hipMemcpyDeviceToHost, q), PIPER_HIP_ERR_LAUNCH);
  if ((rc = pcm_land(sg, r, q, host_pcm, elem, (size_t)need))) return rc;
  if (bounded && (rc = bounded_finish(v, slot, s))) return rc;
  if (r.mapped && !r.caller_pinned) {  // the kernel stored into the staging: the true total is known by now
    memcpy(host_pcm, r.stage, (size_t)delivered_samples(v, slot, s, rd) * elem);
  }
  if (normalize) s.chain.h_peaks.assign(sg.h_peaks.p, sg.h_peaks + NB);
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_collect_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm, int64_t max_samples) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  return collect_pcm(v, slot, params, v->cfg.sample_rate, Sink{host_pcm, max_samples, PIPER_HIP_ENC_S16});
}

PH_EXPORT int piper_hip_voice_collect_pcm16_rate(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int32_t out_rate, int16_t* host_pcm,
                                                 int64_t max_samples) {
  return collect_pcm(v, slot, params, out_rate, Sink{host_pcm, max_samples, PIPER_HIP_ENC_S16});
}

PH_EXPORT int piper_hip_voice_peaks(const piper_hip_voice* v, int slot, float* peaks, int max_items) {
  if (!v || !peaks) PH_FAIL(PIPER_HIP_ERR_ARG, "peaks: null argument");
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (p->chain.h_peaks.empty()) PH_FAIL(PIPER_HIP_ERR_ARG, "peaks: slot %d has not been collected with normalize = 1 since its last launch", slot);
  if (max_items < (int)p->chain.h_peaks.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "peaks: buffer holds %d < %d items", max_items, (int)p->chain.h_peaks.size());
  memcpy(peaks, p->chain.h_peaks.data(), p->chain.h_peaks.size() * sizeof(float));
  return PIPER_HIP_OK;
}

namespace {
int g711_law(const char* who, int law);

// synthesize_pcm16 / _pcm16_rate / _g711: prepare, launch and collect_pcm on slot 0. The refusals come in
// the order law (who != nullptr: a G.711 entry point, enc is the caller's law), params, rate design, prepare.
int synthesize_pcm(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params, int out_rate, const char* who, int enc,
                   void* host, int64_t max_samples, int64_t* n_samples) {
  const ControlsClear cc{v, 0};  // a staging call on slot 0
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  float gain;
  bool normalize;
  int rc = who ? g711_law(who, enc) : PIPER_HIP_OK;
  if (!rc) rc = pcm_params(params, &gain, &normalize);
  if (rc) return rc;
  if (normalize && v->slot_lv[0].on) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16: normalize = 1 on slot 0, which has a level (piper_hip_voice_slot_level)");
  if (normalize && v->slot_ld[0].on) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16: normalize = 1 on slot 0, which has a loudness (piper_hip_voice_slot_loudness)");
  const RsDesign* rd = nullptr;
  if (out_rate != v->cfg.sample_rate && (rc = rs_design(v->cfg.sample_rate, out_rate, &rd))) return rc;
  if ((rc = piper_hip_voice_prepare(v, u, 0)) < 0) return rc;
  if ((rc = piper_hip_voice_launch(v, 0))) return rc;
  if ((rc = collect_pcm(v, 0, params, out_rate, Sink{host, max_samples, enc}))) return rc;
  const Slot& s0 = *v->attached[0];
  if (n_samples) *n_samples = delivered_samples(v, 0, s0, rd);  // (a join: the programme's count)
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_synthesize_pcm16(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                               int64_t max_samples, int64_t* n_samples) {
  return synthesize_pcm(v, u, params, v ? v->cfg.sample_rate : 0, nullptr, PIPER_HIP_ENC_S16, host_pcm, max_samples, n_samples);
}

PH_EXPORT int piper_hip_voice_synthesize_pcm16_rate(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params,
                                                    int32_t out_rate, int16_t* host_pcm, int64_t max_samples, int64_t* n_samples) {
  return synthesize_pcm(v, u, params, out_rate, nullptr, PIPER_HIP_ENC_S16, host_pcm, max_samples, n_samples);
}

namespace {
// The stream slot id `slot` holds — a pool's, a group's or a single one — for the entry point `who`.
Stream* slot_stream(piper_hip_voice* v, int slot, const char* who) {
  if (!v) { ph::set_error("null voice"); return nullptr; }
  if (StreamPool* P = slot_pool(v, slot)) return &P->st;
  Slot* sp = slot_plan(v, slot);
  if (sp && !sp->stream.rows.empty()) return &sp->stream;
  ph::set_error("%s: slot %d has no stream in progress", who, slot);
  return nullptr;
}
// the same for the mixed entry points: a batched stream (group or pool) that stream_set_mixed has marked
Stream* slot_stream_mixed(piper_hip_voice* v, int slot, const char* who) {
  Stream* st = slot_stream(v, slot, who);
  if (st && !st->rs.mixed) { ph::set_error("%s: slot %d is not mixed (stream_set_mixed)", who, slot); return nullptr; }
  return st;
}
bool is_pool(const Stream& st) { return !st.plan; }
int64_t chunk_samples(const piper_hip_voice* v, const Stream& st) { return (int64_t)st.chunk * v->hop; }
int rate_buffers(piper_hip_voice* v, Stream& st);
}  // namespace

PH_EXPORT int piper_hip_voice_stream_set_rate(piper_hip_voice* v, int slot, int32_t out_rate) {
  Stream* sp = slot_stream(v, slot, "stream_set_rate");
  if (!sp) return PIPER_HIP_ERR_ARG;
  Stream& st = *sp;
  StreamRate& rs = st.rs;
  if (rs.mixed) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_rate: slot %d is mixed: every row has its own rate", slot);
  if (rs.started)
    PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_rate: slot %d has %s: the rate is set before", slot, is_pool(st) ? "stepped or been joined" : "stepped");
  if (out_rate == v->cfg.sample_rate) {  // not a filter: the steps are the un-resampled ones
    rs.rate = 0;
    return PIPER_HIP_OK;
  }
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  const RsDesign* rd = nullptr;
  RsFilter rf{};
  int rc;
  if ((rc = voice_filter(v, out_rate, &rd, &rf))) return rc;
  // the history and the descriptor of the stream's rows, and a packed-output buffer that holds a step at this rate
  if ((rc = rate_buffers(v, st))) return rc;
  if ((rc = pack_buffer(v, st, (size_t)st.items() * (size_t)rs_step_bound(*rd, step_samples(v, st)) * sizeof(int16_t)))) return rc;
  rs.parity = 0;
  rs.rate = out_rate;
  return PIPER_HIP_OK;
}

namespace {
// The per-row history [2][rows][kRsHist] and the RsStepRow table of the stream's generator rows (kept when they are large enough already).
int rate_buffers(piper_hip_voice* v, Stream& st) {
  StreamRate& rs = st.rs;
  if (rs.rows >= st.NBg) return PIPER_HIP_OK;
  const size_t hist_row = (size_t)2 * kRsHist * sizeof(float);
  stream_free(v, st, rs.hist, rs.rows * hist_row);
  stream_free(v, st, rs.desc, rs.rows * sizeof(RsStepRow));
  rs.hist = nullptr; rs.desc = nullptr; rs.rows = 0;
  void *h = nullptr, *d = nullptr;
  int rc;
  if ((rc = stream_alloc(v, st, st.NBg * hist_row, &h))) return rc;
  if ((rc = stream_alloc(v, st, st.NBg * sizeof(RsStepRow), &d))) { stream_free(v, st, h, st.NBg * hist_row); return rc; }
  rs.hist = (float*)h;
  rs.desc = (RsStepRow*)d;
  rs.rows = st.NBg;
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_rate(piper_hip_voice* v, int slot) {
  const Stream* st = slot_stream(v, slot, "stream_rate");
  if (!st) return PIPER_HIP_ERR_ARG;
  if (st->rs.mixed) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_rate: slot %d is mixed: every row has its own rate (stream_item_format)", slot);
  return st->rs.rate ? st->rs.rate : v->cfg.sample_rate;
}

// ---- level control (include/piper_hip.h "Level control")

PH_EXPORT int piper_hip_voice_slot_level(piper_hip_voice* v, int slot, const piper_hip_level* level) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (level)
    if (int rc = piper_hip_level_check(level)) return rc;
  v->slot_lv[slot].on = level != nullptr;
  v->slot_lv[slot].lv = level ? *level : piper_hip_level{0.0f, 0.0f, 0.0f};
  return PIPER_HIP_OK;
}

// ---- equaliser (include/piper_hip.h "Equaliser")

PH_EXPORT int piper_hip_voice_slot_eq(piper_hip_voice* v, int slot, const piper_hip_eq* eq) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (eq)
    if (int rc = piper_hip_eq_check(eq, v->cfg.sample_rate)) return rc;
  v->slot_eq[slot].on = eq != nullptr;
  v->slot_eq[slot].eq = piper_hip_eq{};
  if (eq) {  // (only the sections in use: two EQs that differ past n are the same EQ)
    v->slot_eq[slot].eq.n = eq->n;
    for (int i = 0; i < eq->n; i++) v->slot_eq[slot].eq.section[i] = eq->section[i];
  }
  return PIPER_HIP_OK;
}

// ---- join (include/piper_hip.h "Join")

PH_EXPORT int piper_hip_voice_slot_join(piper_hip_voice* v, int slot, const piper_hip_join* join, const float* gaps, int n_gaps) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  JoinParams p{};
  if (join)
    if (int rc = join_build(join, gaps, n_gaps, v->cfg.sample_rate, &p)) return rc;
  auto& sj = v->slot_jn[slot];
  sj.on = join != nullptr;
  sj.p = p;
  sj.gen = ++v->join_clock;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_join_capacity(piper_hip_voice* v, int slot, int32_t out_rate, int64_t* samples) {
  if (!v || !samples) PH_FAIL(PIPER_HIP_ERR_ARG, "join_capacity: null argument");
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (!v->slot_jn[slot].on) PH_FAIL(PIPER_HIP_ERR_ARG, "join_capacity: slot %d has no join (piper_hip_voice_slot_join)", slot);
  int64_t cap = 0;
  int rc = join_capacity(v, slot, *p, &cap);
  if (rc) return rc;
  if (out_rate != 0 && out_rate != v->cfg.sample_rate) {
    const RsDesign* rd = nullptr;
    if ((rc = rs_design(v->cfg.sample_rate, out_rate, &rd))) return rc;
    cap = rs_count(*rd, cap);
  }
  *samples = cap;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_join_report(const piper_hip_voice* v, int slot, int64_t* start, int64_t* len, int max_items, int64_t* total) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "join_report: null voice");
  const Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (p->chain.h_jrep.empty()) PH_FAIL(PIPER_HIP_ERR_ARG, "join_report: slot %d has not been collected with a join since its last launch", slot);
  const int NB = (int)(p->chain.h_jrep.size() - 1) / 2;
  if ((start || len) && max_items < NB) PH_FAIL(PIPER_HIP_ERR_SHAPE, "join_report: buffer holds %d < %d items", max_items, NB);
  if (start) memcpy(start, p->chain.h_jrep.data() + 1, (size_t)NB * sizeof(int64_t));
  if (len) memcpy(len, p->chain.h_jrep.data() + 1 + NB, (size_t)NB * sizeof(int64_t));
  if (total) *total = p->chain.h_jrep[0];
  return PIPER_HIP_OK;
}

// ---- loudness (include/piper_hip.h "Loudness")

PH_EXPORT int piper_hip_voice_slot_loudness(piper_hip_voice* v, int slot, const piper_hip_loudness* loudness) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (slot < 0 || slot >= kMaxSlots) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d out of range [0,%d)", slot, kMaxSlots);
  if (loudness) {
    if (int rc = piper_hip_loudness_check(loudness)) return rc;
    LdFilter f;
    if (int rc = ld_filter(v->cfg.sample_rate, &f)) return rc;  // (the voice's rate is outside the contract)
  }
  v->slot_ld[slot].on = loudness != nullptr;
  v->slot_ld[slot].ld = loudness ? *loudness : piper_hip_loudness{0.0f, 0.0f};
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_loudness(piper_hip_voice* v, int slot, float* lufs, float* gain, int max_items) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  Slot* p = slot_plan(v, slot);
  if (!p) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  Slot& s = *p;
  if (s.bounded_pending) PH_FAIL(PIPER_HIP_ERR_ARG, "loudness: the slot's frame counts are still on the device (collect first)");
  if ((lufs || gain) && max_items < s.NB) PH_FAIL(PIPER_HIP_ERR_SHAPE, "loudness: buffer holds %d < %d items", max_items, s.NB);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  LdTarget t;
  int rc = ld_resolve(v->slot_ld[slot].on ? &v->slot_ld[slot].ld : nullptr, &t);
  if (rc) return rc;
  LdFilter f;
  if ((rc = ld_filter(v->cfg.sample_rate, &f))) return rc;
  Chain c;  // the items the loudness stage reads: shaped, pitched and EQ'd where there are a volume, a pitch, an EQ
  if ((rc = chain_walk(v, slot, s, &c, nullptr)) || (rc = chain_measure(v, s, c, f, t))) return rc;
  auto& sg = v->staging[slot];
  if ((rc = sg.h_loud.ensure((size_t)2 * s.NB, (size_t)2 * kMaxGroup))) return rc;
  PH_HIP(hipMemcpyAsync(sg.h_loud, s.chain.loud_rep.p, (size_t)2 * s.NB * sizeof(float), hipMemcpyDeviceToHost, s.set.stream), PIPER_HIP_ERR_LAUNCH);
  PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
  for (int b = 0; b < s.NB; b++) {
    if (lufs) lufs[b] = sg.h_loud[2 * b];
    if (gain) gain[b] = sg.h_loud[2 * b + 1];
  }
  return PIPER_HIP_OK;
}

namespace {
// The packed-output buffer of a batched stream for the rows as they stand: what begin_batch / pool_open, set_rate, item_formats and the
// joins size, at the slot's current per-row bound (step_samples).
int pack_resize(piper_hip_voice* v, Stream& st) {
  const int64_t n_in = step_samples(v, st);
  int64_t bytes = 0;
  if (st.rs.mixed) {
    for (const StreamRow& row : st.rows)
      if (!is_pool(st) || row.active) bytes += fmt_step_bytes(v, row.fmt, n_in);
  } else if (st.rs.rate) {
    const RsDesign* rd = nullptr;
    if (int rc = rs_design(v->cfg.sample_rate, st.rs.rate, &rd)) return rc;
    bytes = (int64_t)st.items() * rs_step_bound(*rd, n_in) * (int64_t)sizeof(int16_t);
  } else {
    bytes = (int64_t)st.items() * n_in * (int64_t)sizeof(float);
  }
  return pack_buffer(v, st, (size_t)bytes);
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_set_level(piper_hip_voice* v, int slot, const piper_hip_level* level) {
  Stream* sp = slot_stream(v, slot, "stream_set_level");
  if (!sp) return PIPER_HIP_ERR_ARG;
  Stream& st = *sp;
  StreamLevel& lv = st.lv;
  if (!level) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_level: null level");
  if (st.rs.started)
    PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_level: slot %d has %s: the level is set before", slot, is_pool(st) ? "stepped or been joined" : "stepped");
  LvParams p;
  int rc = lv_resolve(level, v->cfg.sample_rate, &p);
  if (rc) return rc;
  const int64_t chunk = chunk_samples(v, st);
  if (chunk < 512)
    PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_level: chunk_frames · hop = %lld < 512 (a step before the last must deliver samples)", (long long)chunk);
  if (chunk > 0x3fffffff || !lv_step_lds(chunk)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_set_level: %lld samples per step too many", (long long)chunk);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  // the carry, the descriptor and the limited samples of one step for the stream's generator rows (kept when they are large enough)
  const int64_t row = (lv_step_bound(chunk) + 1 + 3) & ~(int64_t)3;
  if (lv.rows < st.NBg || lv.row < row) {
    stream_free(v, st, lv.carry, (size_t)lv.rows * kLvCarry * sizeof(float));
    stream_free(v, st, lv.lim, (size_t)lv.rows * lv.row * sizeof(float));
    stream_free(v, st, lv.desc, (size_t)lv.rows * sizeof(LvStepRow));
    lv.carry = lv.lim = nullptr; lv.desc = nullptr; lv.rows = 0; lv.row = 0;
    void *c = nullptr, *l = nullptr, *d = nullptr;
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * kLvCarry * sizeof(float), &c))) return rc;
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * row * sizeof(float), &l))) { stream_free(v, st, c, (size_t)st.NBg * kLvCarry * sizeof(float)); return rc; }
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * sizeof(LvStepRow), &d))) {
      stream_free(v, st, c, (size_t)st.NBg * kLvCarry * sizeof(float));
      stream_free(v, st, l, (size_t)st.NBg * row * sizeof(float));
      return rc;
    }
    lv.carry = (float*)c; lv.lim = (float*)l; lv.desc = (LvStepRow*)d;
    lv.rows = st.NBg; lv.row = row;
  }
  const bool was = lv.on;
  lv.on = true;
  if ((rc = pack_resize(v, st))) { lv.on = was; return rc; }
  lv.p = p;
  lv.lv = piper_hip_level{p.drive, p.ceiling, level->release_ms == 0.0f ? 50.0f : level->release_ms};
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_level(piper_hip_voice* v, int slot, piper_hip_level* out) {
  const Stream* st = slot_stream(v, slot, "stream_level");
  if (!st) return PIPER_HIP_ERR_ARG;
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_level: null output");
  if (!st->lv.on) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_level: slot %d has no level", slot);
  *out = st->lv.lv;
  return PIPER_HIP_OK;
}

// ---- equaliser on streams (include/piper_hip.h "Equaliser")

PH_EXPORT int piper_hip_voice_stream_set_eq(piper_hip_voice* v, int slot, const piper_hip_eq* eq) {
  Stream* sp = slot_stream(v, slot, "stream_set_eq");
  if (!sp) return PIPER_HIP_ERR_ARG;
  Stream& st = *sp;
  StreamEq& sq = st.eq;
  if (!eq) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_eq: null eq");
  if (st.rs.started)
    PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_eq: slot %d has %s: the EQ is set before", slot, is_pool(st) ? "stepped or been joined" : "stepped");
  int rc = piper_hip_eq_check(eq, v->cfg.sample_rate);
  if (rc) return rc;
  if (v->hop % kEqBlock != 0)
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "stream_set_eq: hop %d is not a multiple of %d: a step's chunk would not start on a block", v->hop, kEqBlock);
  const int64_t chunk = chunk_samples(v, st);
  if (chunk < 1 || chunk > 0x3fffffff) PH_FAIL(PIPER_HIP_ERR_SHAPE, "stream_set_eq: %lld samples per step", (long long)chunk);
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  const int blocks = (int)ceil_div(chunk, kEqBlock);
  if (!sq.dev) {
    void* p = nullptr;
    if ((rc = stream_alloc(v, st, sizeof(EqDesign), &p))) return rc;
    sq.dev = (EqDesign*)p;
  }
  if (sq.rows < st.NBg || sq.blocks < blocks) {  // the carry, the scratch and the descriptor of the stream's generator rows
    stream_free(v, st, sq.carry, (size_t)sq.rows * kEqCarry * sizeof(double));
    stream_free(v, st, sq.scratch, (size_t)sq.rows * sq.blocks * 2 * kEqMaxD * sizeof(double));
    stream_free(v, st, sq.desc, (size_t)sq.rows * sizeof(EqStepRow));
    sq.carry = sq.scratch = nullptr; sq.desc = nullptr; sq.rows = 0; sq.blocks = 0;
    void *c = nullptr, *w = nullptr, *d = nullptr;
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * kEqCarry * sizeof(double), &c))) return rc;
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * blocks * 2 * kEqMaxD * sizeof(double), &w))) {
      stream_free(v, st, c, (size_t)st.NBg * kEqCarry * sizeof(double));
      return rc;
    }
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * sizeof(EqStepRow), &d))) {
      stream_free(v, st, c, (size_t)st.NBg * kEqCarry * sizeof(double));
      stream_free(v, st, w, (size_t)st.NBg * blocks * 2 * kEqMaxD * sizeof(double));
      return rc;
    }
    sq.carry = (double*)c; sq.scratch = (double*)w; sq.desc = (EqStepRow*)d;
    sq.rows = st.NBg; sq.blocks = blocks;
  }
  // the design, built and uploaded here, never inside a step (a blocking copy: no step of this stream has run)
  std::vector<EqDesign> hold(1);
  if ((rc = eq_build(eq, v->cfg.sample_rate, hold.data()))) return rc;
  PH_HIP(hipMemcpy(sq.dev, hold.data(), sizeof(EqDesign), hipMemcpyHostToDevice), PIPER_HIP_ERR_LAUNCH);
  sq.eq = piper_hip_eq{};
  sq.eq.n = eq->n;
  for (int i = 0; i < eq->n; i++) sq.eq.section[i] = eq->section[i];
  sq.on = true;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_eq(piper_hip_voice* v, int slot, piper_hip_eq* out) {
  const Stream* st = slot_stream(v, slot, "stream_eq");
  if (!st) return PIPER_HIP_ERR_ARG;
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_eq: null output");
  if (!st->eq.on) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_eq: slot %d has no EQ", slot);
  *out = st->eq.eq;
  return PIPER_HIP_OK;
}

// ---- mixed formats (include/piper_hip.h "Mixed formats")

PH_EXPORT int piper_hip_voice_stream_set_mixed(piper_hip_voice* v, int slot) {
  Stream* sp = slot_stream(v, slot, "stream_set_mixed");
  if (!sp) return PIPER_HIP_ERR_ARG;
  Stream& st = *sp;
  StreamRate& rs = st.rs;
  if (st.single) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_mixed: slot %d holds a single stream (stream_set_rate and a law per step serve it)", slot);
  if (rs.mixed) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_mixed: slot %d is mixed already", slot);
  if (rs.rate) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_mixed: slot %d has the output rate %d set", slot, rs.rate);
  if (rs.started)
    PH_FAIL(PIPER_HIP_ERR_ARG, "stream_set_mixed: slot %d has %s", slot, is_pool(st) ? "stepped or been joined" : "stepped");
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  int rc;
  if ((rc = rate_buffers(v, st))) return rc;
  if (rs.mix_rows < st.NBg) {
    stream_free(v, st, rs.mdesc, (size_t)rs.mix_rows * sizeof(MixStepRow));
    rs.mdesc = nullptr; rs.mix_rows = 0;
    void* p = nullptr;
    if ((rc = stream_alloc(v, st, (size_t)st.NBg * sizeof(MixStepRow), &p))) return rc;
    rs.mdesc = (MixStepRow*)p;
    rs.mix_rows = st.NBg;
  }
  for (StreamRow& row : st.rows) row.fmt = RowFormat();  // (s16 at the voice's rate: the buffer of the begin / open holds it)
  rs.parity = 0;
  rs.mixed = true;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_item_formats(piper_hip_voice* v, int slot, const piper_hip_stream_format* fmts, int n) {
  Stream* sp = slot_stream_mixed(v, slot, "stream_item_formats");
  if (!sp) return PIPER_HIP_ERR_ARG;
  Stream& st = *sp;
  if (is_pool(st)) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_formats: slot %d holds a pool: the join brings the formats (stream_pool_join_formats)", slot);
  if (!fmts || n < 1) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_formats: %d formats", fmts ? n : 0);
  if (st.rs.started) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_formats: slot %d has stepped: a row keeps its format", slot);
  const int items = st.items();
  std::vector<RowFormat> f(items);
  int rc;
  for (int i = 0; i < items; i++)
    if ((rc = check_format(v, "stream_item_formats", fmts[std::min(i, n - 1)], &f[i]))) return rc;
  PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
  int64_t bytes = 0;
  for (int i = 0; i < items; i++) {
    RsFilter ff{};
    if (f[i].rate && (rc = voice_filter(v, f[i].rate, nullptr, &ff))) return rc;
    bytes += fmt_step_bytes(v, f[i], step_samples(v, st));
  }
  if ((rc = pack_buffer(v, st, (size_t)bytes))) return rc;
  for (int i = 0; i < items; i++) st.rows[i].fmt = f[i];
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_stream_next_batch_mixed(piper_hip_voice* v, int slot, void* host, int64_t max_bytes, int64_t* n_samples,
                                                      int64_t* byte_off) {
  if (!v || !n_samples || !byte_off) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  if (!slot_stream_mixed(v, slot, "stream_next_batch_mixed")) return PIPER_HIP_ERR_ARG;
  if (!host) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_next_batch_mixed: a mixed step needs a buffer");
  return batch_step(v, slot, Sink{host, max_bytes, PIPER_HIP_ENC_S16, 1.0f, byte_off}, n_samples);
}

PH_EXPORT int64_t piper_hip_voice_stream_step_capacity_bytes(piper_hip_voice* v, int slot) {
  const Stream* st = slot_stream_mixed(v, slot, "stream_step_capacity_bytes");
  if (!st) return PIPER_HIP_ERR_ARG;
  int64_t bytes = 0;
  for (const StreamRow& row : st->rows)
    if (row.active) bytes += fmt_step_bytes(v, row.fmt, step_samples(v, *st));
  return bytes;
}

PH_EXPORT int piper_hip_voice_stream_item_format(piper_hip_voice* v, int slot, int item, piper_hip_stream_format* out) {
  const Stream* st = slot_stream_mixed(v, slot, "stream_item_format");
  if (!st) return PIPER_HIP_ERR_ARG;
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_format: null output");
  if (item < 0 || item >= st->items()) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_format: item %d outside [0,%d)", item, st->items());
  const StreamRow& row = st->rows[item];
  if (is_pool(*st) && !row.active) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_item_format: row %d of the pool on slot %d is free", item, slot);
  out->out_rate = row.fmt.rate;
  out->encoding = row.fmt.enc;
  out->gain = row.fmt.gain;
  return PIPER_HIP_OK;
}

PH_EXPORT int64_t piper_hip_voice_stream_step_capacity(piper_hip_voice* v, int slot) {
  const Stream* st = slot_stream(v, slot, "stream_step_capacity");
  if (!st) return PIPER_HIP_ERR_ARG;
  if (st->rs.mixed) PH_FAIL(PIPER_HIP_ERR_ARG, "stream_step_capacity: slot %d is mixed: stream_step_capacity_bytes", slot);
  if (!st->rs.rate) return (int64_t)st->items() * step_samples(v, *st);
  const RsDesign* rd = nullptr;
  if (int rc = rs_design(v->cfg.sample_rate, st->rs.rate, &rd)) return rc;
  return (int64_t)st->items() * rs_step_bound(*rd, step_samples(v, *st));
}

namespace {
// a stream step's params: normalisation needs the utterance's peak, which no step before the last knows
int pcm_step_params(const piper_hip_voice* v, const piper_hip_pcm_params* params, float* gain) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  bool normalize;
  const int rc = pcm_params(params, gain, &normalize);
  if (rc) return rc;
  if (normalize) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "pcm16: normalize = 1 on a stream step (the utterance's peak is not known before its last window)");
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_stream_next_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                                int64_t max_samples, int64_t* n_samples) {
  float gain;
  const int rc = pcm_step_params(v, params, &gain);
  if (rc) return rc;
  if (slot_pool(v, slot)) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds a streaming pool: use stream_next_batch_pcm16", slot);
  return stream_step(v, slot, Sink{host_pcm, max_samples, PIPER_HIP_ENC_S16, gain}, n_samples);
}

PH_EXPORT int piper_hip_voice_stream_next_batch_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                                      int64_t max_samples, int64_t* n_samples) {
  float gain;
  const int rc = pcm_step_params(v, params, &gain);
  if (rc) return rc;
  return batch_step(v, slot, Sink{host_pcm, max_samples, PIPER_HIP_ENC_S16, gain}, n_samples);
}

// ---- G.711 (include/piper_hip.h "G.711 output"): the PCM entry points with a one-byte sink; the law is an argument of each call ---------
namespace {
int g711_law(const char* who, int law) {
  if (law != PIPER_HIP_G711_MULAW && law != PIPER_HIP_G711_ALAW) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: law %d (1 = mu-law, 2 = A-law)", who, law);
  return PIPER_HIP_OK;
}
}  // namespace

PH_EXPORT int piper_hip_voice_collect_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, int32_t out_rate,
                                           uint8_t* host, int64_t max_samples) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  if (int rc = g711_law("collect_g711", law)) return rc;
  return collect_pcm(v, slot, params, out_rate, Sink{host, max_samples, law});
}

PH_EXPORT int piper_hip_voice_synthesize_g711(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params, int law,
                                              int32_t out_rate, uint8_t* host, int64_t max_samples, int64_t* n_samples) {
  return synthesize_pcm(v, u, params, out_rate, "synthesize_g711", law, host, max_samples, n_samples);
}

PH_EXPORT int piper_hip_voice_stream_next_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, uint8_t* host,
                                               int64_t max_samples, int64_t* n_samples) {
  float gain;
  int rc = pcm_step_params(v, params, &gain);
  if (!rc) rc = g711_law("stream_next_g711", law);
  if (rc) return rc;
  if (slot_pool(v, slot)) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d holds a streaming pool: use stream_next_batch_g711", slot);
  return stream_step(v, slot, Sink{host, max_samples, law, gain}, n_samples);
}

PH_EXPORT int piper_hip_voice_stream_next_batch_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, uint8_t* host,
                                                     int64_t max_samples, int64_t* n_samples) {
  float gain;
  int rc = pcm_step_params(v, params, &gain);
  if (!rc) rc = g711_law("stream_next_batch_g711", law);
  if (rc) return rc;
  return batch_step(v, slot, Sink{host, max_samples, law, gain}, n_samples);
}

PH_EXPORT int piper_hip_voice_synthesize(piper_hip_voice* v, const piper_hip_utterance* u, float* host_audio,
                                         int64_t max_samples, int64_t* n_samples) {
  int rc = piper_hip_voice_prepare(v, u, 0);
  if (rc < 0) return rc;
  if ((rc = piper_hip_voice_launch(v, 0))) return rc;
  if ((rc = piper_hip_voice_collect(v, 0, host_audio, max_samples))) return rc;
  const Slot& s0 = *v->attached[0];
  if (n_samples) *n_samples = delivered_samples(v, 0, s0);  // (a join: the programme's count; no buffer: none was made, the item's own)
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_tap(piper_hip_voice* v, int slot, const char* name, float* host, size_t max_floats,
                                  size_t* n_floats) {
  if (!v || !name) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  // grammar: ["predict:"] <tensor> ["@" <step name>]   |   ["predict:"] "@steps"   |   ["window:"] <tensor>   |   "window:@steps"
  //          ["predict:" | "window:"] "@routes"
  std::string full(name);
  Slot* sp = slot_plan(v, slot);
  const WindowRecord* win = nullptr;  // "window:": the generator plan of the slot's latest stream step, rows at that step's window lengths
  if (full.compare(0, 7, "window:") == 0) {
    full.erase(0, 7);
    if (slot < 0 || slot >= kMaxSlots || (!sp && !slot_pool(v, slot))) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': slot %d holds no stream", name, slot);
    win = &v->windows[slot];
    if (!win->plan) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': no stream step has run on slot %d", name, slot);
    Slot* gp = nullptr;
    for (auto& p : v->plans)
      if (p.get() == win->plan && p->built && p->kind == PLAN_GENERATOR) gp = p.get();
    if (!gp) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': the window plan of slot %d's latest step has been evicted", name, slot);
    if (gp->last_use != win->stamp || gp->NB != (int)win->Fc.size())
      PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': the window plan of slot %d's latest step has run another step since", name, slot);
    sp = gp;
  }
  if (!sp) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  const Slot& owner = *sp;  // the true lengths of the items are the slot's
  Slot* tp = sp;
  if (!win && full.compare(0, 8, "predict:") == 0) {  // the cached encoder + predictor plan of the slot's bucket T and batch size
    full.erase(0, 8);
    tp = predict_plan_of(v, slot, owner);
    if (!tp) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': no predictor plan of %d ids x %d items is cached", name, owner.T, owner.NB);
  }
  Slot& s = *tp;
  const size_t at = full.find('@');
  const std::string tensor_name = full.substr(0, at), step_name = at == std::string::npos ? std::string() : full.substr(at + 1);
  if (at != std::string::npos && tensor_name.empty() && step_name == "routes") {
    // one line per launch: step name, tab, the route records of its most recent enqueue ("; " between the records of one launch; nothing
    // behind the tab when the context was not armed then). Runs nothing and changes no tensor.
    std::string all;
    for (const Step& st : s.steps) {
      if (st.kind != Step::LAUNCH) continue;
      all += st.name + "\t";
      for (const char c : st.routes) {
        if (c == '\n') all += "; ";
        else all += c;
      }
      all += "\n";
    }
    if (n_floats) *n_floats = all.size();
    if (host) {
      if (max_floats < all.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "tap buffer too small");
      for (size_t i = 0; i < all.size(); i++) host[i] = (float)(unsigned char)all[i];
    }
    return PIPER_HIP_OK;
  }
  if (at != std::string::npos && tensor_name.empty() && step_name == "steps") {
    // the names of the schedule's launches in order, one per line, one character per float: what piper_hip_voice_profile reports, for a plan
    // that no slot id reaches
    std::string all;
    for (const Step& st : s.steps)
      if (st.kind == Step::LAUNCH) all += st.name + "\n";
    if (n_floats) *n_floats = all.size();
    if (host) {
      if (max_floats < all.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "tap buffer too small");
      for (size_t i = 0; i < all.size(); i++) host[i] = (float)(unsigned char)all[i];
    }
    return PIPER_HIP_OK;
  }
  if (!win && tp == sp && at == std::string::npos && tensor_name == "vol.gain") {
    // gf of the items, each compacted to its true F: written by a kernel of its own from the plan's frame-to-id map and the staged gains
    if (!s.vol_on) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': the last staging of slot %d carried no volume (piper_hip_voice_slot_volume)", name, slot);
    if (s.bounded_pending) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "tap '%s': the slot's frame counts are still on the device (collect first)", name);
    size_t total = 0;
    for (int b = 0; b < s.NB; b++) total += (size_t)s.h_F[b];
    if (n_floats) *n_floats = total;
    if (!host) return PIPER_HIP_OK;
    if (max_floats < total) PH_FAIL(PIPER_HIP_ERR_SHAPE, "tap buffer too small");
    PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
    if (!s.vol_gf) {
      void* q = nullptr;
      if (int rc = plan_alloc(v, s, (size_t)s.NB * s.F * sizeof(float), &q)) return rc;
      s.vol_gf = (float*)q;
    }
    PH_HIP(launch_volume_frame_gains(s.set.stream, s.lensF, s.F, s.NB, s.frame2id, s.F, s.vol_gain, s.T, s.vol_gf), PIPER_HIP_ERR_LAUNCH);
    size_t off = 0;
    for (int b = 0; b < s.NB; b++) {
      PH_HIP(hipMemcpyAsync(host + off, s.vol_gf + (size_t)b * s.F, (size_t)s.h_F[b] * sizeof(float), hipMemcpyDeviceToHost, s.set.stream),
             PIPER_HIP_ERR_LAUNCH);
      off += (size_t)s.h_F[b];
    }
    PH_HIP(hipStreamSynchronize(s.set.stream), PIPER_HIP_ERR_LAUNCH);
    return PIPER_HIP_OK;
  }
  auto it = s.taps.find(tensor_name);
  if (it == s.taps.end()) PH_FAIL(PIPER_HIP_ERR_ARG, "unknown tap '%s'", name);
  const Slot::Tap& t = it->second;
  int upto = -1;  // index of the named step
  if (at != std::string::npos) {
    // the schedule replays from the inputs that prepare staged: they must still be in place
    if (s.kind == PLAN_GENERATOR) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "tap '%s': a generator-only window plan keeps no inputs to replay from", name);
    if (owner.bounded_pending) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "tap '%s': the slot's frame counts are still on the device (collect first)", name);
    for (int i = 0; i < (int)s.steps.size() && upto < 0; i++)
      if (s.steps[i].kind == Step::LAUNCH && s.steps[i].name == step_name) upto = i;
    if (upto < 0) PH_FAIL(PIPER_HIP_ERR_ARG, "tap '%s': the schedule has no step '%s'", name, step_name.c_str());
  }
  // items back to back, each compacted to its true length: [C][len_b]
  // (unit < 0: a tensor of fixed length, the whole row for every item — the speaker taps)
  // (a window plan: the window lengths of the recorded step, in place of a slot's frame counts)
  auto item_len = [&](int b) {
    return (size_t)(t.unit < 0 ? t.row : t.unit == 0 ? (win ? 0 : owner.h_T[b]) : (win ? win->Fc[b] : owner.h_F[b]) * t.unit);
  };
  size_t total = 0;
  for (int b = 0; b < s.NB; b++) total += (size_t)t.C * item_len(b);
  if (n_floats) *n_floats = total;
  if (host) {
    if (max_floats < total) PH_FAIL(PIPER_HIP_ERR_SHAPE, "tap buffer too small");
    PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
    if (tp != sp) {  // an idle plan has given its stream set back
      PH_HIP(stream_wait(owner.set.stream), PIPER_HIP_ERR_LAUNCH);
      const int rc = slot_init(v, s);
      if (rc) return rc;
    }
    const hipStream_t q = s.set.stream;
    if (q) PH_HIP(stream_wait(q), PIPER_HIP_ERR_LAUNCH);  // (a window plan's step ended with a wait; the plan may have given its set back)
    auto run_range = [&](int from, int to) -> int {  // eagerly, in schedule order on the plan's stream (as piper_hip_voice_profile does)
      for (int i = from; i < to; i++)
        if (s.steps[i].kind == Step::LAUNCH) {
          const int rc = s.steps[i].enqueue(q);
          if (rc) return rc;
        }
      PH_HIP(hipGetLastError(), PIPER_HIP_ERR_LAUNCH);
      PH_HIP(stream_wait(q), PIPER_HIP_ERR_LAUNCH);
      return PIPER_HIP_OK;
    };
    if (upto >= 0) {
      const int rc = run_range(0, upto + 1);
      if (rc) return rc;
    }
    size_t off = 0;
    for (int b = 0; b < s.NB; b++) {
      const size_t len = item_len(b);
      if (len)
        PH_HIP(hipMemcpy2D(host + off, len * sizeof(float), t.p + (size_t)b * t.batch_stride, (size_t)t.row * sizeof(float), len * sizeof(float),
                           (size_t)t.C, hipMemcpyDeviceToHost), PIPER_HIP_ERR_LAUNCH);
      off += (size_t)t.C * len;
    }
    if (upto >= 0) {  // the rest of the schedule: every buffer ends as a full run leaves it
      const int rc = run_range(upto + 1, (int)s.steps.size());
      if (rc) return rc;
    }
  }
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_last_gpu_ms(piper_hip_voice* v, int slot, double* ms) {
  if (!v || !ms) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  Slot* sp = slot_plan(v, slot);
  if (!sp || !sp->timed) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d has no timed launch", slot);
  Slot& s = *sp;
  PH_HIP(hipEventSynchronize(s.set.ev1), PIPER_HIP_ERR_LAUNCH);
  float f = 0;
  PH_HIP(hipEventElapsedTime(&f, s.set.ev0, s.set.ev1), PIPER_HIP_ERR_LAUNCH);
  *ms = f;
  return PIPER_HIP_OK;
}

PH_EXPORT piper_hip_stream piper_hip_voice_slot_stream(piper_hip_voice* v, int slot) {
  Slot* sp = slot_plan(v, slot);
  return sp ? (piper_hip_stream)sp->set.stream : nullptr;
}

PH_EXPORT int piper_hip_voice_profile(piper_hip_voice* v, int slot, int iters, piper_hip_kernel_stat* out, int max_entries,
                                      int* n_entries) {
  if (!v) PH_FAIL(PIPER_HIP_ERR_ARG, "null voice");
  Slot* sp = slot_plan(v, slot);
  if (!sp) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (iters < 1) iters = 1;
  Slot& s = *sp;
  const int n = (int)s.steps.size();
  if (n_entries) *n_entries = n;
  if (!out) return PIPER_HIP_OK;
  std::vector<hipEvent_t> ev((size_t)n + 1);
  for (auto& e : ev) PH_HIP(hipEventCreate(&e), PIPER_HIP_ERR_LAUNCH);
  std::vector<std::vector<float>> samples((size_t)n);  // per launch: one delta per pass — the MEDIAN is reported (a stall of one
                                                        // pass on a fresh box must not poison a row: BENCH_r01 showed a 324 µs enc2.qkv)
  int rc = PIPER_HIP_OK;
  for (int it = 0; it < iters + 1 && !rc; it++) {  // first pass is warm-up
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s.set.stream, (unsigned long long)(100 * (1500 + 12 * n)));  // µs → ticks
    PH_HIP(hipEventRecord(ev[0], s.set.stream), PIPER_HIP_ERR_LAUNCH);
    for (int i = 0; i < n && !rc; i++) {
      if (s.steps[i].kind == Step::LAUNCH) rc = s.steps[i].enqueue(s.set.stream);
      if (!rc && hipEventRecord(ev[i + 1], s.set.stream) != hipSuccess) rc = PIPER_HIP_ERR_LAUNCH;
    }
    if (rc) break;
    PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
    if (it == 0) continue;
    for (int i = 0; i < n; i++) {
      float ms = 0;
      PH_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]), PIPER_HIP_ERR_LAUNCH);
      samples[i].push_back(ms * 1000.0f);
    }
  }
  // event floor: the same bracket around an empty kernel (dispatch boundary + event markers, no work) — what has to be
  // subtracted from a step's event delta to compare it with rocprofv3's begin→end kernel duration
  double floor_us = 0.0;
  if (!rc) {
    const int nf = std::min(32, n);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s.set.stream, (unsigned long long)(100 * 800));
    if (hipEventRecord(ev[0], s.set.stream) != hipSuccess) rc = PIPER_HIP_ERR_LAUNCH;
    for (int i = 1; i <= nf && !rc; i++) {
      hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, s.set.stream);
      if (hipEventRecord(ev[i], s.set.stream) != hipSuccess) rc = PIPER_HIP_ERR_LAUNCH;
    }
    if (!rc && nf > 0 && stream_wait(s.set.stream) == hipSuccess) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[0], ev[nf]) == hipSuccess) floor_us = ms * 1000.0 / nf;
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (rc) return rc;
  for (int i = 0; i < n && i < max_entries; i++) {
    memset(&out[i], 0, sizeof out[i]);
    snprintf(out[i].name, sizeof out[i].name, "%s", s.steps[i].name.c_str());
    std::vector<float>& sm = samples[i];
    std::sort(sm.begin(), sm.end());
    out[i].avg_us = sm.empty() ? 0.0 : (sm.size() & 1 ? sm[sm.size() / 2] : 0.5 * (sm[sm.size() / 2 - 1] + sm[sm.size() / 2]));
    out[i].flops = s.steps[i].flops;
    out[i].bytes = s.steps[i].bytes;
  }
  if (n < max_entries) {  // extra pseudo-entry carrying the calibration
    memset(&out[n], 0, sizeof out[n]);
    snprintf(out[n].name, sizeof out[n].name, "(event floor: empty kernel)");
    out[n].avg_us = floor_us;
    if (n_entries) *n_entries = n + 1;
  }
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_voice_time_subset(piper_hip_voice* v, int slot, const char* name_filter, int iters, double* avg_launch_us,
                                          int* n_launches, double* flops, double* bytes) {
  if (!v || !name_filter) PH_FAIL(PIPER_HIP_ERR_ARG, "null argument");
  Slot* sp = slot_plan(v, slot);
  if (!sp) PH_FAIL(PIPER_HIP_ERR_ARG, "slot %d is not prepared", slot);
  if (iters < 1) iters = 1;
  if (strncmp(name_filter, "predict:", 8) == 0) {  // the predictor plan the slot's last prepare ran, as for piper_hip_voice_tap
    name_filter += 8;
    Slot* tp = predict_plan_of(v, slot, *sp);
    if (!tp) PH_FAIL(PIPER_HIP_ERR_ARG, "time_subset: no predictor plan of %d ids x %d items is cached", sp->T, sp->NB);
    PH_HIP(hipSetDevice(v->ctx->device), PIPER_HIP_ERR_UNAVAILABLE);
    PH_HIP(stream_wait(sp->set.stream), PIPER_HIP_ERR_LAUNCH);  // (a bounded prepare ran it on the slot's stream)
    if (int rc0 = slot_init(v, *tp)) return rc0;                 // an idle plan has given its stream set back
    sp = tp;
  }
  Slot& s = *sp;
  std::vector<int> pick;
  double fl = 0, by = 0;
  // "a|b|c": the launches with exactly these names (one replayed graph for a whole kernel family); otherwise substring / tag match
  std::vector<std::string> exact;
  if (strchr(name_filter, '|')) {
    std::string f(name_filter);
    size_t b = 0;
    while (b <= f.size()) {
      const size_t e = f.find('|', b);
      const std::string part = f.substr(b, e == std::string::npos ? std::string::npos : e - b);
      if (!part.empty()) exact.push_back(part);
      if (e == std::string::npos) break;
      b = e + 1;
    }
  }
  auto wanted = [&](const Step& st) {
    if (!exact.empty()) return std::find(exact.begin(), exact.end(), st.name) != exact.end();
    return st.name.find(name_filter) != std::string::npos || (!st.tag.empty() && st.tag == name_filter);
  };
  for (int i = 0; i < (int)s.steps.size(); i++)
    if (s.steps[i].kind == Step::LAUNCH && wanted(s.steps[i])) {
      pick.push_back(i);
      fl += s.steps[i].flops;
      by += s.steps[i].bytes;
    }
  if (n_launches) *n_launches = (int)pick.size();
  if (flops) *flops = fl;
  if (bytes) *bytes = by;
  if (pick.empty()) {
    if (avg_launch_us) *avg_launch_us = 0;
    return PIPER_HIP_OK;
  }
  PH_HIP(stream_wait(s.set.stream), PIPER_HIP_ERR_LAUNCH);
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  const int rc = capture_graph(s.set.stream, [&](hipStream_t q) { return run_steps(s, pick, q); }, &g, &ge, "time_subset");
  if (rc) return rc;
  hipError_t e = hipGraphLaunch(ge, s.set.stream);  // warm-up
  if (e == hipSuccess) e = hipEventRecord(s.set.ev0, s.set.stream);
  for (int it = 0; it < iters && e == hipSuccess; it++) e = hipGraphLaunch(ge, s.set.stream);
  if (e == hipSuccess) e = hipEventRecord(s.set.ev1, s.set.stream);
  if (e == hipSuccess) e = hipEventSynchronize(s.set.ev1);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, s.set.ev0, s.set.ev1);
  (void)hipGraphExecDestroy(ge);
  (void)hipGraphDestroy(g);
  s.timed = false;
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "time_subset: %s", hipGetErrorString(e));
  if (avg_launch_us) *avg_launch_us = (double)ms * 1000.0 / ((double)iters * (double)pick.size());
  return PIPER_HIP_OK;
}
