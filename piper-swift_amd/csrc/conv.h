// conv.h — internal interface of the Conv1d / ConvTranspose1d kernel family (conv.hip).
#pragma once
#include "common.h"

namespace ph {

// input transform applied while the B operand (activations) is loaded
enum Prologue : int {
  PRO_NONE = 0,
  PRO_LRELU = 1,       // x = lrelu(x, alpha)
  PRO_AVG3_LRELU = 2,  // x = lrelu(((x + x2) + x3) / 3, alpha)   (HiFi-GAN MRF mean folded into the consumer)
  PRO_LN = 3,          // x = ((x − mean_t) / sd_t)·ln_gamma[c] + ln_beta[c]: channel LayerNorm folded into the consumer (K ∈ {1,3})
};

// output transform / routing applied to the accumulator tile
enum Epilogue : int {
  EPI_STORE = 0,        // y = v (+ res)                         v = bias + conv
  EPI_RELU = 1,         // y = relu(v)
  EPI_TANH = 2,         // y = tanh(v)
  EPI_RSUB = 3,         // y = res − v                           (flow coupling reverse: x1 − m)
  EPI_WN_RES_SKIP = 4,  // co <  wn_c: y[co] = res[co] + v ; co ≥ wn_c: y2[co−wn_c] = (skip? skip[..]:0) + v
  EPI_WN_SKIP_LAST = 5, // y2[co] = (skip? skip[co]:0) + v
  EPI_CONVT = 6,        // rows are (co, phase): y[co][q·s + phase − padL] = v
  EPI_MRF_MEAN = 7,     // r2 = v + res;  y = lrelu(((mrf_a + mrf_b) + r2) / 3, alpha2)   (last ResBlock conv of a stage)
};

// the names route records use (common.h: PH_ROUTE)
inline const char* prologue_name(int p) {
  static const char* const n[] = {"none", "lrelu", "avg3_lrelu", "ln"};
  return p >= 0 && p < 4 ? n[p] : "?";
}
inline const char* epilogue_name(int e) {
  static const char* const n[] = {"store", "relu", "tanh", "rsub", "wn_res_skip", "wn_skip_last", "convt", "mrf_mean"};
  return e >= 0 && e < 8 ? n[e] : "?";
}

// one record of a launcher that works on ConvArgs `a`: "<family and its parameters> gate=… pro=… epi=… res=… conv|convT"
#define PH_ROUTE_CONV(ctx, a, fmt, ...)                                                                                         \
  PH_ROUTE(ctx, (a).Cout, (a).Cin, (a).Lout, (a).N, fmt " gate=%d pro=%s epi=%s res=%d %s", ##__VA_ARGS__, (a).gate,           \
           ::ph::prologue_name((a).prologue), ::ph::epilogue_name((a).epilogue), (a).res ? 1 : 0, (a).epilogue == ::ph::EPI_CONVT ? "convT" : "conv")

struct ConvArgs {
  // tensors
  const float* x = nullptr;   // [N, x_channels, Lin]
  const float* x2 = nullptr;  // PRO_AVG3_LRELU
  const float* x3 = nullptr;
  const float* w = nullptr;   // MFMA path: packed 32-wide fragments (pack_conv_weights); direct path: raw ONNX layout
  const float* w16 = nullptr; // optional packed 16-wide fragments (short-utterance geometry)
  const float* w8 = nullptr;   // optional 8-row fragment image (pack_conv_weights_rows8): many input channels, few output rows (conv_lean.hip)
  const float* w16g = nullptr; // gated convs: 16-wide fragments with 8 tanh rows + their 8 sigmoid rows per tile (pack_conv_weights_gate16; conv_short.hip)
  const float* bias = nullptr;
  const float* res = nullptr;   // residual / minuend, same addressing as y
  const float* skip = nullptr;  // EPI_WN_*: running skip sum, same addressing as y2 (may be null)
  float* y = nullptr;
  float* y2 = nullptr;
  // geometry
  int N = 1, Cin = 0, Cout = 0, K = 1, dil = 1, padL = 0, Lin = 0, Lout = 0;
  int stride = 1, groups = 1;  // direct path only
  int64_t x_batch_stride = 0;  // floats between batch items of x (x2/x3 share it)
  int64_t y_batch_stride = 0;  // floats between batch items of y / res
  int64_t y2_batch_stride = 0;
  int64_t bias_batch_stride = 0;  // floats between the bias rows of batch items; 0 = one row shared by all (speaker-conditioned convs: an item's effective bias)
  int in_ch_base = 0, in_ch_sign = 1;    // physical input channel = in_ch_base + in_ch_sign·ci  (folds Flip/Split)
  int out_ch_base = 0, out_ch_sign = 1;  // physical output channel of y/res = out_ch_base + out_ch_sign·co
  int y_len = 0;                         // row length of y/res/y2/skip (floats)
  int prologue = PRO_NONE;
  float alpha = 0.0f;
  int epilogue = EPI_STORE;
  int gate = 0;  // MFMA path: Cout = 2·H rows; emits H rows tanh(a)·sigmoid(b)
  unsigned long long* trace = nullptr;  // tools/probe/streamprobe (-DPH_STREAM_TRACE): s_memtime stamps per wave; unused otherwise
  int wn_c = 0;  // EPI_WN_RES_SKIP split point
  // ConvTranspose (EPI_CONVT): GEMM rows = Cout_ct·ct_stride, GEMM cols = q
  int ct_stride = 0, ct_padL = 0, ct_Lout = 0;
  int ct_shift = -1;  // log2(ct_stride) when it is a power of two (set by launch_conv_mfma)
  // EPI_MRF_MEAN: the two other ResBlock outputs of the stage (addressed like y) and the slope applied after the mean
  const float* mrf_a = nullptr;
  const float* mrf_b = nullptr;
  float alpha2 = 0.0f;
  // bucketed schedules: batch item n really holds len_ptr[n]·len_mul input positions per row (≤ Lin, the row stride); taps
  // beyond read as zero padding, exactly as if the tensor ended there. null ⇒ Lin. Outputs past the true length are
  // don't-care values (never read unmasked by anything downstream).
  const int* len_ptr = nullptr;
  int len_mul = 1;
  // LayerNorm across a kernel boundary without a kernel of its own (GraphExecutor.swift:2071-2125: ReduceMean / Sub / Pow /
  // ReduceMean / Add / Sqrt / Div / Mul / Add). PRODUCER (EPI_STORE with stats_out): besides y = res + conv it writes, per
  // 16-row slot and column, Σ y and the CENTRED Σ (y − mean_slot)² of its rows → stats_out [N][ceil(Cout/16)][y_len][2] (a 32-row
  // tile writes its two slots, so the consumer never needs to know the producer's tile size; fixed slots ⇒ deterministic).
  // CONSUMER (PRO_LN): combines the slots of a column with Chan's parallel-variance formula — mean = ΣΣ / C, M2 = Σ [M2_i +
  // n_i·(mean_i − mean)²], var = M2 / C: the two-pass accuracy of the graph's chain in one memory round trip (r3; the one-pass
  // Σ y² / C − mean² of round 2 lost (mean / sigma)²·6e-8) — and normalises its B operand on load; the waves of row tile 0 also
  // write the normalised tensor to ln_out (the residual operand of the next Add, and the "enc_out" tap).
  float* stats_out = nullptr;
  const float* ln_stats = nullptr;
  const float* ln_gamma = nullptr;
  const float* ln_beta = nullptr;
  float* ln_out = nullptr;
  float ln_eps = 1e-5f;
  int ln_self = 0;  // PRO_LN without ln_stats: the consumer computes the statistics of its own operand (conv_lean.hip; conv_lean_ln_self_ok says when)
};

// number of floats of the packed fragment image for a [Cout, Cin, K] conv
size_t packed_conv_floats(int Cout, int Cin, int K, int tm = 32);
// ConvTranspose [Cin, Cout, K] stride s → rows Cout·s, taps ceil(K/s)
size_t packed_convt_floats(int Cin, int Cout, int K, int s, int tm = 32);
int pack_conv_weights(hipStream_t s, const float* w, int Cout, int Cin, int K, float* packed, int tm = 32);
int pack_convt_weights(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, float* packed, int tm = 32);
// gated conv (Cout = 2·H rows, tanh half then sigmoid half): 16-row tiles of rows {8m … 8m+7} ∪ {H + 8m … H + 8m+7}; same size as the tm = 16 image
int pack_conv_weights_gate16(hipStream_t s, const float* w, int Cout, int Cin, int K, float* packed);
// 8-row tiles: [ceil(Cout/8)][Cin/4 · K steps][32 floats = 4 channels × 8 rows]; Cin % 4 == 0
size_t packed_conv_rows8_floats(int Cout, int Cin, int K);
int pack_conv_weights_rows8(hipStream_t s, const float* w, int Cout, int Cin, int K, float* packed);
// tile geometry launch_conv_mfma will pick for this problem when 16-wide fragments are available (32 or 16)
int conv_pick_tile(piper_hip_ctx* ctx, int Cout, int Lout, int N, int gate);

// true when the MFMA implicit-GEMM path can run this geometry
bool conv_mfma_eligible(int Cout, int Cin, int K, int stride, int groups);
// Enqueue one conv on `s`. args.w must already be packed for the MFMA path.
int launch_conv_mfma(piper_hip_ctx* ctx, hipStream_t s, const ConvArgs& a);
// The k = 1 convs of one utterance with a minimal instruction count: conv_lean.hip. Same return convention as try_launch_conv_short.
int try_launch_conv_lean(piper_hip_ctx* ctx, hipStream_t s, const ConvArgs& a);
bool conv_lean_ln_self_ok(piper_hip_ctx* ctx, int Cin, int Cout, int K, int padL, int L, int N);
// The linear tail of a reverse flow coupling as ONE k = 1 conv (conv_lean.hip: conv_k1_tail_kernel). The last WaveNet
// layer's res_skip conv (H → H, skip only), post (H → half), x1 − m, the Flip and the next coupling's pre (half → H) have no
// nonlinearity between them: fold_flow_tail multiplies them out once per voice (float64, rounded once) into the 16-row fragment image
// the launch reads. seam = 0: the last coupling, whose tail ends at x1new.
struct FlowTailArgs {
  const float *acts = nullptr, *skip = nullptr;  // [N][H][F]: the last gated conv's output, the skip sum of the layers before it
  const float* zin = nullptr;                    // [N][2·half][F]: the buffer that holds x1
  float* zout = nullptr;                         // x1new goes here (seam: a different buffer, other row tiles read x1 as an operand)
  float* h = nullptr;                            // [N][H][F]: the next coupling's pre (seam)
  const float *w = nullptr, *bias = nullptr;     // fold_flow_tail's image and bias
  const int* len_ptr = nullptr;
  int N = 1, H = 0, half = 0, F = 0, seam = 0;
  int out_ch_base = 0, out_ch_sign = 1;          // x1 row r ↔ physical channel out_ch_base + out_ch_sign·r of z
};
bool flow_tail_shape_ok(int H, int half);
bool flow_tail_plan_ok(piper_hip_ctx* ctx, int H, int half, int F, int N);
inline int flow_tail_steps(int H, int half, int seam) { return (2 * H + (seam ? half : 0)) / 4; }
inline size_t flow_tail_image_floats(int H, int half, int seam) { return (size_t)((half + (seam ? H : 0)) / 16) * flow_tail_steps(H, half, seam) * 64; }
inline size_t flow_tail_scratch_doubles(int H, int half) { return (size_t)half * (H + 1) + (size_t)H * H; }
// w_rs / b_rs [H × H], w_post / b_post [half × H], w_pre / b_pre [H × half] (null: seam = 0): raw conv weights on the device.
// x1_sign: the coupling's channel map (+1 / −1). scratch: flow_tail_scratch_doubles doubles, free for reuse behind this call on `s`.
int fold_flow_tail(hipStream_t s, const float* w_rs, const float* b_rs, const float* w_post, const float* b_post, const float* w_pre, const float* b_pre,
                   int H, int half, int x1_sign, double* scratch, float* image, float* bias);
int launch_flow_tail(piper_hip_ctx* ctx, hipStream_t s, const FlowTailArgs& t);
// Short rows (one utterance's encoder / flow convs): conv_short.hip. 1 = enqueued, 0 = not this kernel's case (use launch_conv_mfma's
// streaming kernel), < 0 = error. Called by launch_conv_mfma.
int try_launch_conv_short(piper_hip_ctx* ctx, hipStream_t s, const ConvArgs& a);
// Thread-per-output kernel for everything else (groups, stride, tiny Cout). args.w is raw [Cout, Cin/g, K].
int launch_conv_direct(piper_hip_ctx* ctx, hipStream_t s, const ConvArgs& a);
// Thread-per-output ConvTranspose for geometries the phase decomposition does not cover. w raw [Cin, Cout/g, K].
int launch_convt_direct(piper_hip_ctx* ctx, hipStream_t s, const float* x, const float* w, const float* bias, float* y, int N,
                        int Cin, int Lin, int Cout, int K, int stride, int dil, int padL, int Lout, int groups);

// algorithmic work of one conv (SURVEY.md Appendix A recipe)
inline double conv_flops(int Cout, int Cin_per_g, int K, int64_t Lout) { return 2.0 * Cout * (double)Lout * Cin_per_g * K; }

}  // namespace ph
