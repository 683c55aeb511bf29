/*
 * piper_hip.h — C-ABI of the MI355X (gfx950) operator backend for Piper VITS inference.
 *
 * This is the drop-in boundary for the slot `Sources/PiperMetal` fills in ocrickard/piper-swift:
 * one entry point per `MetalBackend` per-op method that `GraphExecutor.executeNode` calls on the
 * hot path, plus fused / whole-utterance entry points whose results equal the
 * unfused composition.  Every declaration cites the reference interface it replaces (file:line,
 * relative to the reference repo root).
 *
 * Conventions (mirroring MetalBackend):
 *   - Tensors are dense row-major float32 on the device; shapes are int64_t arrays.
 *   - The callee ALLOCATES and returns the output buffer (MetalBackend returns a fresh MTLBuffer,
 *     MetalBackend.swift:1184, 1261, 1334).  If `*out` is non-NULL on entry it is used instead
 *     (caller-owned, must hold the output) — the zero-allocation path for static schedules.
 *   - Inputs are borrowed and never written.
 *   - `stream == NULL`  ⇔ `commandBuffer == nil`: run and BLOCK until complete
 *     (MetalBackend.swift:1223-1226).  Non-NULL ⇔ encode only; `piper_hip_stream_sync` ⇔ `flush`.
 *   - Swift `throws` → int status (0 ok, negative below) + thread-local `piper_hip_last_error()`.
 *   - One context per GPU, used from one host thread at a time (the reference has one queue, one
 *     executor, no locks: GraphExecutor.swift:27, MetalContext.swift:6,14).
 *   - No CPU fallback exists anywhere behind this header: without a gfx950 device every compute
 *     entry point returns PIPER_HIP_ERR_UNAVAILABLE.
 */
#ifndef PIPER_HIP_H
#define PIPER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIPER_HIP_ABI_VERSION 3

/* ---- status codes: ExecutionError (CPUBackend.swift:3-17) + NSError domain "MetalBackend" ---- */
enum {
  PIPER_HIP_OK = 0,
  PIPER_HIP_ERR_SHAPE = -1,       /* ExecutionError.shapeMismatch */
  PIPER_HIP_ERR_TYPE = -2,        /* ExecutionError.typeMismatch */
  PIPER_HIP_ERR_UNSUPPORTED = -3, /* ExecutionError.unsupportedOp */
  PIPER_HIP_ERR_UNAVAILABLE = -4, /* ExecutionError.metalUnavailable: no gfx950 device / HIP init failed */
  PIPER_HIP_ERR_ALLOC = -5,       /* NSError 600/610/620/760/904: output allocation failed */
  PIPER_HIP_ERR_LAUNCH = -6,      /* NSError 601/611/621/761/900: encode / execution failed */
  PIPER_HIP_ERR_ARG = -7          /* NULL / invalid handle (Swift's type system excludes these) */
};

typedef struct piper_hip_ctx piper_hip_ctx;     /* MetalBackend + MetalContext (device, queue, pipelines) */
typedef struct piper_hip_voice piper_hip_voice; /* a loaded voice: weights resident + static schedule */
typedef struct piper_hip_comm piper_hip_comm;   /* an RCCL communicator: one rank (= one GPU, one process) of a node */
typedef void* piper_hip_stream;                 /* hipStream_t; stands in for MTLCommandBuffer? */

/* Thread-local description of the last failure on this thread ("" if none). */
const char* piper_hip_last_error(void);
int piper_hip_abi_version(void);
/* The tuning / A-B switches (PIPER_HIP_* environment variables) this process has honoured so far, as "NAME=value …"; empty
 * when none. Switches are honoured only when PIPER_HIP_TUNING=1 is set too: an inherited environment does not change which kernels run. */
int piper_hip_config_string(char* buf, size_t n);
/* Number of visible HIP devices (0 when none); never initialises a device. */
int piper_hip_device_count(void);

/* ---- context, buffers, transfers ---- */
/* MetalContext.init (Metal/MetalContext.swift:9-33) + MetalBackend.init (MetalBackend.swift:12-15). */
int piper_hip_create(int device, piper_hip_ctx** out);
void piper_hip_destroy(piper_hip_ctx* ctx);
/* Route records, a debugging aid (DESIGN.md "Route records"): while armed (on != 0; off by default) every conv, ResBlock-pair, flow-seam and
 * attention launcher of this context appends one line "<variant> | Cout=… Cin=… Lout=… N=… CUs=…" when it has chosen its kernel: the variant is
 * the kernel family with its template and launch parameters, gate, prologue, epilogue and conv / convT; the shape stands apart. An op entry
 * point keeps the records of the last call: piper_hip_last_routes copies them out, '\n' between records ('\0'-terminated; *needed = bytes
 * with the terminator, buf may be NULL to ask). A voice plan keeps them per step: the "@routes" selectors of piper_hip_voice_tap. Arming or
 * disarming forgets the context's records; plans enqueued while disarmed report empty routes. One thread drives an armed context. */
int piper_hip_routes_arm(piper_hip_ctx* ctx, int on);
int piper_hip_last_routes(piper_hip_ctx* ctx, char* buf, size_t n, size_t* needed);
/* Device memory held by the context's pool (buffers + cached free blocks) and the part currently handed out. The pool
 * recycles power-of-two blocks, so a host that sees many utterance shapes plateaus instead of growing; `memory_trim`
 * returns the cached free blocks to the driver (the role ARC plays for MTLBuffer in the reference). */
int piper_hip_memory_stats(piper_hip_ctx* ctx, size_t* reserved_bytes, size_t* live_bytes);
int piper_hip_memory_trim(piper_hip_ctx* ctx);
/* Take `bytes` of device memory from the driver NOW, in one piece, and serve later allocations of this context (plan arenas, op outputs) from
 * it before asking the driver again. A fresh driver allocation is cheap to make but its first use can stall the GPU for tens of milliseconds
 * (page mapping / clearing): a serving process pays that while it loads. One slab per context (later calls are no-ops); piper_hip_voice_create
 * reserves 8 GiB (of the 288 GB of an MI355X; halved until it fits on a smaller part) if nothing was reserved before it (the reference's heaps: MetalBackend.swift:34-39 allocates per buffer). */
int piper_hip_memory_reserve(piper_hip_ctx* ctx, size_t bytes);
/* MetalBackend.allocateBuffer(length:) (MetalBackend.swift:34-39): at least 1 byte is allocated. */
int piper_hip_alloc(piper_hip_ctx* ctx, size_t bytes, void** out);
/* Buffer release (ARC drop in the reference; GraphExecutor.swift:216-225). Returns memory to the
 * context pool; stream-ordered with respect to work already enqueued on the context's streams. */
int piper_hip_free(piper_hip_ctx* ctx, void* buf);
/* MetalBackend.uploadFloat32 (MetalBackend.swift:983-993). */
int piper_hip_upload_f32(piper_hip_ctx* ctx, const float* host, size_t count, float** out);
int piper_hip_upload_i64(piper_hip_ctx* ctx, const int64_t* host, size_t count, int64_t** out);
/* MetalBackend.downloadFloat32 (MetalBackend.swift:963-981): blocks until `buf` is complete. */
int piper_hip_download_f32(piper_hip_ctx* ctx, const float* buf, float* host, size_t count);
/* Page-locked host memory — the analogue of reading `MTLBuffer.contents()` of a shared-storage buffer (MetalBackend.swift:963-981 copies out
 * of one): piper_hip_voice_collect / piper_hip_download_f32 into such a buffer is a single DMA, without the staging copy a pageable
 * destination needs. Plain malloc'ed buffers keep working everywhere. */
int piper_hip_host_alloc(piper_hip_ctx* ctx, size_t bytes, void** out);
int piper_hip_host_free(piper_hip_ctx* ctx, void* host);
/* MetalBackend.makeCommandBuffer / flush / flushWithTimings (MetalBackend.swift:841-874). */
int piper_hip_stream_create(piper_hip_ctx* ctx, piper_hip_stream* out);
int piper_hip_stream_destroy(piper_hip_ctx* ctx, piper_hip_stream s);
int piper_hip_stream_sync(piper_hip_ctx* ctx, piper_hip_stream s);
/* GPU time bracket on a stream (gpuStartTime/gpuEndTime, MetalBackend.swift:868-873). */
int piper_hip_timer_begin(piper_hip_ctx* ctx, piper_hip_stream s);
int piper_hip_timer_end(piper_hip_ctx* ctx, piper_hip_stream s, double* gpu_ms); /* syncs the stream */

/* ---- param PODs (MetalBackend.swift:876-961; MSL twins conv1d.metal:12-26,80-95) ---- */
typedef struct {
  int32_t stride, dilation, pad_l, pad_r, groups;
} piper_hip_conv1d_params;
typedef struct {
  int32_t stride, dilation, pad_l, pad_r, output_padding, groups;
} piper_hip_convtranspose1d_params;

typedef enum { /* unaryF32 / unaryAlphaF32 kernels (MetalBackend.swift:1501-1586; elementwise.metal:165-312) */
  PIPER_HIP_RELU = 0,
  PIPER_HIP_LEAKYRELU = 1, /* alpha */
  PIPER_HIP_TANH = 2,
  PIPER_HIP_SIGMOID = 3,
  PIPER_HIP_EXP = 4,
  PIPER_HIP_NEG = 5,
  PIPER_HIP_SQRT = 6,
  PIPER_HIP_SOFTPLUS = 7,
  PIPER_HIP_CEIL = 8,
  PIPER_HIP_ERF = 9
} piper_hip_unary_op;
typedef enum { /* add/sub/mul/div/pow broadcast kernels (MetalBackend.swift:2592-2610; elementwise.metal:52-130) */
  PIPER_HIP_ADD = 0,
  PIPER_HIP_SUB = 1,
  PIPER_HIP_MUL = 2,
  PIPER_HIP_DIV = 3,
  PIPER_HIP_POW = 4
} piper_hip_binary_op;

/* ---- per-op entry points (§8a rows a3-a9) ---- */

/* MetalBackend.conv1dF32 (MetalBackend.swift:1149-1228) → conv1d_f32 (conv1d.metal:28-71);
 * arithmetic spec CPUBackend.conv1d (CPUBackend.swift:20-73).
 * x [N,Cin,L], w [Cout,Cin/g,K], bias [Cout] or NULL → y [N,Cout,L_out],
 * L_out = (L + pad_l + pad_r − dilation·(K−1) − 1)/stride + 1 (integer division). */
int piper_hip_conv1d_f32(piper_hip_ctx* ctx, const float* x, const int64_t x_shape[3], const float* w,
                         const int64_t w_shape[3], const float* bias, const piper_hip_conv1d_params* p,
                         float** out, int64_t out_shape[3], piper_hip_stream stream);

/* MetalBackend.convTranspose1dF32 (MetalBackend.swift:2812-2895) → convtranspose1d_f32
 * (conv1d.metal:97-142). w is ONNX layout [Cin, Cout/g, K].
 * L_out = (L−1)·stride − pad_l − pad_r + dilation·(K−1) + output_padding + 1 (must be > 0). */
int piper_hip_convtranspose1d_f32(piper_hip_ctx* ctx, const float* x, const int64_t x_shape[3], const float* w,
                                  const int64_t w_shape[3], const float* bias,
                                  const piper_hip_convtranspose1d_params* p, float** out, int64_t out_shape[3],
                                  piper_hip_stream stream);

/* bf16-operand variants of the two contractions (SURVEY.md §8b "bf16 variants", §8d config 5). The reference has no
 * bf16 path, so these are a build extension with the SAME shapes, parameter structs and error behaviour as
 * conv1dF32 / convTranspose1dF32 (MetalBackend.swift:1149-1228, 2812-2895): fp32 tensors in and out, x and w rounded
 * to bf16 (nearest even) on the device, fp32 accumulation and bias on v_mfma_f32_32x32x16_bf16. Covered geometry:
 * stride 1 (conv) / K % stride == 0 with pads (K−stride)/2 (convT), groups 1, C_in % 32 == 0 (convT: C_out too),
 * padding and dilation reach ≤ 64; anything else returns PIPER_HIP_ERR_UNSUPPORTED so the caller can take the f32 op. */
int piper_hip_conv1d_bf16(piper_hip_ctx* ctx, const float* input, const int64_t input_shape[3], const float* weight,
                          const int64_t weight_shape[3], const float* bias, const piper_hip_conv1d_params* p, float** out,
                          int64_t out_shape[3], piper_hip_stream stream);
int piper_hip_convtranspose1d_bf16(piper_hip_ctx* ctx, const float* input, const int64_t input_shape[3],
                                   const float* weight, const int64_t weight_shape[3], const float* bias,
                                   const piper_hip_convtranspose1d_params* p, float** out, int64_t out_shape[3],
                                   piper_hip_stream stream);

/* MetalBackend.matmulF32 (MetalBackend.swift:1232-1323) → matmul_f32 (matmul.metal:22-49), with the
 * executor's rank-4 lead-dim broadcast (GraphExecutor.swift:1870-1899) done by stride-0 addressing
 * instead of a materialised expandF32.  Equal ranks ≥ 2 required (MetalBackend.swift:1236-1238);
 * lead dims must be equal or 1-broadcastable. */
int piper_hip_matmul_f32(piper_hip_ctx* ctx, const float* a, const int64_t* a_shape, const float* b,
                         const int64_t* b_shape, int rank, float** out, int64_t* out_shape,
                         piper_hip_stream stream);

/* MetalBackend.softmaxLastDimF32 (MetalBackend.swift:1326-1355) → softmax_lastdim_f32
 * (softmax.metal:13-41). Last dim must be > 0. */
int piper_hip_softmax_lastdim_f32(piper_hip_ctx* ctx, const float* x, const int64_t* shape, int rank, float** out,
                                  piper_hip_stream stream);

/* MetalBackend.{relu,leakyRelu,tanh,sigmoid,exp,neg,sqrt,softplus,ceil,erf}F32
 * (MetalBackend.swift:1501-1586). `alpha` is read only by PIPER_HIP_LEAKYRELU. */
int piper_hip_unary_f32(piper_hip_ctx* ctx, piper_hip_unary_op op, const float* x, size_t count, float alpha,
                        float** out, piper_hip_stream stream);

/* MetalBackend.{add,sub,mul,div,pow}F32 → binaryBroadcastF32 (MetalBackend.swift:2099-2134, 2592-2610);
 * NumPy broadcasting, output rank ≤ 4 (MetalBackend.swift:2065-2067). out_shape has max(ra,rb) entries. */
int piper_hip_binary_broadcast_f32(piper_hip_ctx* ctx, piper_hip_binary_op op, const float* a,
                                   const int64_t* a_shape, int a_rank, const float* b, const int64_t* b_shape,
                                   int b_rank, float** out, int64_t* out_shape, int* out_rank,
                                   piper_hip_stream stream);

/* Layout ops the rel-position skew and the flow coupling are made of (§8a rows a7, a9). */
/* MetalBackend.padConstantF32 (MetalBackend.swift:780-839) → pad_constant_f32_rank4 (pad.metal).
 * pads = [begin_0..begin_{r-1}, end_0..end_{r-1}], all ≥ 0, rank ≤ 4. */
int piper_hip_pad_constant_f32(piper_hip_ctx* ctx, const float* x, const int64_t* shape, int rank,
                               const int64_t* pads, float value, float** out, int64_t* out_shape,
                               piper_hip_stream stream);
/* Slice arms (GraphExecutor.swift:1322-1426) → slice.metal kernels. One axis, start/end already
 * clamped ONNX-style by the caller, step ≠ 0 (step −1 on axis 1 is VITS `Flip`). rank ≤ 4. */
int piper_hip_slice_f32(piper_hip_ctx* ctx, const float* x, const int64_t* shape, int rank, int axis, int64_t start,
                        int64_t end, int64_t step, float** out, int64_t* out_shape, piper_hip_stream stream);
/* MetalBackend.transposeF32 (MetalBackend.swift:995-1060) → transpose_f32_rank4 (transpose.metal:16-46). */
int piper_hip_transpose_f32(piper_hip_ctx* ctx, const float* x, const int64_t* shape, int rank, const int32_t* perm,
                            float** out, int64_t* out_shape, piper_hip_stream stream);
/* concat2_axis1_ncl_f32 / split2_axis1_ncl_f32 (tensorops.metal; GraphExecutor.swift:1107-1124, 2254-2262). */
int piper_hip_concat2_axis1_f32(piper_hip_ctx* ctx, const float* a, const int64_t a_shape[3], const float* b,
                                const int64_t b_shape[3], float** out, int64_t out_shape[3],
                                piper_hip_stream stream);
int piper_hip_split2_axis1_f32(piper_hip_ctx* ctx, const float* x, const int64_t x_shape[3], int64_t c0,
                               float** out0, float** out1, piper_hip_stream stream);
/* MetalBackend.expandF32 (MetalBackend.swift:2438-2458) → expand_f32_rank4 (expand.metal). */
int piper_hip_expand_f32(piper_hip_ctx* ctx, const float* x, const int64_t* in_shape, const int64_t* out_shape,
                         int rank, float** out, piper_hip_stream stream);
/* reduce_mean_lastdim_f32 (reduce.metal:12-25; MetalBackend.swift:1357-1390) — the LayerNorm building block. */
int piper_hip_reduce_mean_lastdim_f32(piper_hip_ctx* ctx, const float* x, const int64_t* shape, int rank,
                                      float** out, piper_hip_stream stream);

/* MetalBackend.randomNormalLike(shape:seed:) (MetalBackend.swift:3398-3426) → random_normal_like_f32 (elementwise.metal:139-163):
 * element i draws u0, u1 from xorshift32 seeded with (seed & 0xffffffff) ^ (i·747796405 + 2891336453), maps them to (0, 1] and
 * returns sqrt(−2·ln u0)·cos(2π·u1). The reference calls it with the fixed seed 1234 for both RandomNormalLike nodes of the
 * graph (GraphExecutor.swift:2656-2659). The integer stream is bit-exact; the floats agree to ≈ 1e-6 (Metal's log/cos are not
 * libm's). */
int piper_hip_random_normal_like_f32(piper_hip_ctx* ctx, size_t count, uint64_t seed, float** out, piper_hip_stream stream);
/* The raw draws behind it, for parity checks of the integer stream: out[2i] = u0, out[2i+1] = u1 of element i (device buffer). */
int piper_hip_random_draws_u32(piper_hip_ctx* ctx, size_t count, uint64_t seed, uint32_t** out, piper_hip_stream stream);

/* ---- fused entry points: results equal the unfused composition of the ops above ---- */

/* Text-encoder relative-position self-attention core (§8a rows a5+a6+a7), one call per layer:
 *   scores = (q/√d)·kᵀ + rel→abs( (q/√d)·E_kᵀ );  p = softmax(scores);  out = p·v + abs→rel(p)·E_v
 * q,k,v: [N, H·d, T] channel-major (the k=1 Conv outputs, head h = channels [h·d,(h+1)·d));
 * emb_rel_k/emb_rel_v: [2·window+1, d] shared over heads; out: [N, H·d, T].
 * Replaces the MatMul/Pad/Reshape/Slice/Softmax/Transpose chain of GraphExecutor.swift:1862-1929,
 * 1130-1210, 1371-1426, 901-947 without materialising [N,H,T,2T−1]. */
int piper_hip_rel_attention_f32(piper_hip_ctx* ctx, const float* q, const float* k, const float* v,
                                const float* emb_rel_k, const float* emb_rel_v, int64_t n, int64_t heads,
                                int64_t head_dim, int64_t t, int64_t window, float** out, piper_hip_stream stream);

/* The attention block of an encoder layer in ONE launch: out = LN_c(x + conv_o(rel_attention(q, k, v)))·gamma + beta, with
 * conv_o the k = 1 output projection (w_o [C, C, 1], b_o [C], C = heads·head_dim). Equals rel_attention_f32 → conv1d_f32 →
 * add_layernorm_f32 (GraphExecutor.swift:1862-1929 + Conv :1739-1810 + Add :741-779 + LayerNorm chain :2071-2125) without the
 * two intermediate tensors. Covered: head_dim 96, C ≤ 256, window ≤ 7, T ≤ 2048; otherwise PIPER_HIP_ERR_UNSUPPORTED and the
 * caller composes the three ops. */
int piper_hip_attention_block_f32(piper_hip_ctx* ctx, const float* q, const float* k, const float* v, const float* emb_rel_k,
                                  const float* emb_rel_v, const float* w_o, const float* b_o, const float* x, const float* gamma,
                                  const float* beta, int64_t n, int64_t heads, int64_t head_dim, int64_t t, int64_t window, float eps,
                                  float** out, piper_hip_stream stream);

/* Channel LayerNorm with fused residual: out = LN_c(x + y)·gamma + beta over C for each (n,t); y may be
 * NULL. Replaces Transpose + ReduceMean/Sub/Pow/Sqrt/Div/Mul/Add (GraphExecutor.swift:2071-2125). */
int piper_hip_add_layernorm_f32(piper_hip_ctx* ctx, const float* x, const float* y, const float* gamma,
                                const float* beta, int64_t n, int64_t c, int64_t t, float eps, float** out,
                                piper_hip_stream stream);

/* One WaveNet layer of the flow (§8a rows a3+a8): acts = tanh(a)·sigmoid(b), [a;b] = in_conv(x) (C→2C, k, dilation);
 * rs = res_skip_conv(acts) (k=1; C→2C, or C→C when `last`). If !last: x_out = x + rs[:C], skip_out = skip_in + rs[C:];
 * else skip_out = skip_in + rs. skip_in may be NULL (treated as 0). x_out/skip_out follow the `*out` convention
 * (x_out is not written when `last`). */
int piper_hip_wavenet_layer_f32(piper_hip_ctx* ctx, const float* x, const float* skip_in, const float* w_in,
                                const float* b_in, const float* w_rs, const float* b_rs, int64_t n, int64_t c,
                                int64_t t, int64_t k, int64_t dilation, int last, float** x_out, float** skip_out,
                                piper_hip_stream stream);

/* HiFi-GAN residual blocks (§8a rows a3+a8). type 1 (Piper "high"): for each dilation d_i:
 * x = x + conv2_i(lrelu(conv1_i(lrelu(x)), d=d_i), d=1); type 2 (Piper "medium"): x = x + conv_i(lrelu(x), d=d_i).
 * slope 0.1 (LeakyRelu alpha), `same` padding (k·d−d)/2. weights: n_dil (type 2) or 2·n_dil (type 1, ordered
 * c1_0,c2_0,c1_1,…) tensors [C,C,K] each followed by its bias [C], as arrays of device pointers on the host. */
int piper_hip_hifigan_resblock_f32(piper_hip_ctx* ctx, int type, const float* x, int64_t n, int64_t c, int64_t t,
                                   int64_t k, const int32_t* dilations, int n_dil, const float* const* weights,
                                   const float* const* biases, float lrelu_slope, float** out,
                                   piper_hip_stream stream);

/* ---- whole-utterance path: PiperMetalRuntime.synthesize (PiperMetalRuntime.swift:62-80) ---- */

#define PIPER_HIP_MAX_UPS 4
#define PIPER_HIP_MAX_RB 3
typedef struct {
  int32_t n_vocab;    /* embedding rows (Piper num_symbols, 256) */
  int32_t hidden;     /* 192 */
  int32_t n_heads;    /* 2 */
  int32_t n_layers;   /* 6 */
  int32_t ffn;        /* 768 */
  int32_t ffn_kernel; /* 3 */
  int32_t window;     /* 4 */
  int32_t inter;      /* 192 */
  int32_t n_flows;    /* 4 */
  int32_t wn_layers;  /* 4 */
  int32_t wn_kernel;  /* 5 */
  int32_t up_initial; /* 256 (medium) / 512 (high) */
  int32_t n_ups;      /* 3 / 4 */
  int32_t up_rates[PIPER_HIP_MAX_UPS];
  int32_t up_kernels[PIPER_HIP_MAX_UPS];
  int32_t resblock_type; /* 2 (medium) / 1 (high) */
  int32_t n_rb;          /* resblocks per stage (3) */
  int32_t rb_kernels[PIPER_HIP_MAX_RB];
  int32_t rb_n_dil; /* dilations per resblock: 2 (medium) / 3 (high) */
  int32_t rb_dilations[PIPER_HIP_MAX_RB][3];
  int32_t sample_rate; /* 22050 */
  /* ---- ABI 2: stochastic duration predictor (VITS `dp`; the Softplus / CumSum / GatherElements / … spline arms of
   * GraphExecutor.swift:2379-2645). dp_present = 0 ⇒ the blob carries no `dp.*` tensors and per-id durations must be
   * supplied with every utterance. */
  int32_t dp_present;    /* 1 */
  int32_t dp_kernel;     /* 3: depthwise kernel of the dilated depth-separable convs; dilation kernel^i */
  int32_t dp_dds_layers; /* 3 */
  int32_t dp_n_flows;    /* 4 ConvFlows in the module; inference runs the last dp_n_flows − 1 of them + the ElementwiseAffine */
  int32_t dp_bins;       /* 10 spline bins */
  float dp_tail_bound;   /* 5.0 */
} piper_hip_voice_config;

/* Piper's four published geometries (SURVEY.md §8a †). quality: 0 = medium, 1 = high, 2 = low (the medium geometry at
 * sample_rate 16000), 3 = x_low (hidden 96, inter 96, ffn 384, two heads of head_dim 48, the medium generator and
 * predictor fields, sample_rate 16000). Any other value: PIPER_HIP_ERR_ARG. */
int piper_hip_voice_config_preset(int quality, piper_hip_voice_config* out);
/* Number of floats in the packed weight blob for `cfg` (layout: include/piper_hip_voice_layout.h). */
int piper_hip_voice_blob_floats(const piper_hip_voice_config* cfg, size_t* n_floats);
/* One tensor of the blob (order = include/piper_hip_voice_layout.h). kind: 0 weight, 1 bias, 2 gamma, 3 beta, 4 embedding. */
typedef struct {
  char name[96];
  int32_t kind;
  int32_t rank;
  int64_t shape[3];
  int64_t fan_in;
  uint64_t offset; /* floats */
  uint64_t count;  /* floats */
} piper_hip_tensor_info;
int piper_hip_voice_blob_layout(const piper_hip_voice_config* cfg, piper_hip_tensor_info* out, int max_entries,
                                int* n_entries);
/* Fill a HOST blob with synthetic weights: the bench has no real voice offline. Counter-based
 * SplitMix64 → 24-bit uniform, zero-mean with the variance SURVEY.md §8d asks for (weights/embeddings
 * U(±√(3/fan_in)) ⇒ var 1/fan_in; biases U(±0.01·√3); gamma 1+U(±0.1); beta U(±0.1)) — uniform instead of
 * Box-Muller so that C and numpy (tests/katdata.py) produce bit-identical blobs. Host-only, no GPU needed. */
int piper_hip_voice_synthetic_blob(const piper_hip_voice_config* cfg, uint64_t seed, float* host_blob,
                                   size_t n_floats);
/* Load a voice from a packed fp32 blob; `on_device` ≠ 0 when `blob` is a device pointer (e.g. the RCCL-broadcast
 * copy). Packs MFMA weight fragments once; the blob itself is not retained. ⇔ GraphExecutor.init + persistent
 * initializer buffers (GraphExecutor.swift:42-71, 279-283). */
int piper_hip_voice_create(piper_hip_ctx* ctx, const piper_hip_voice_config* cfg, const float* blob, int on_device,
                           piper_hip_voice** out);
void piper_hip_voice_destroy(piper_hip_voice* v);

/* Arithmetic of the HiFi-GAN generator (94 % of the high voice's FLOPs). F32 (default): everything fp32, the parity
 * configuration. BF16: every generator Conv / ConvTranspose takes bf16 operands (weights, and
 * the LeakyReLU'd activations written by the producing conv) with fp32 accumulation; bias, residual stream, MRF mean,
 * conv_post, the text encoder and the flow stay fp32. Stated tolerance: waveform SNR ≥ 35 dB against the fp32 result.
 * Drops every prepared slot (prepare again). UNSUPPORTED when a generator conv is outside the bf16 kernels' geometry. */
#define PIPER_HIP_PRECISION_F32 0
#define PIPER_HIP_PRECISION_BF16 1
int piper_hip_voice_set_precision(piper_hip_voice* v, int precision);
int piper_hip_voice_precision(const piper_hip_voice* v);

/* ---- Piper `.onnx` / `.onnx.json` → voice blob (role of Sources/PiperONNX for this library) ----
 * Host-only (no GPU). Decodes the protobuf wire subset the reference's loader decodes (ONNXLoader.swift:34-37, 94-99,
 * 170-176, 214-223, 321-327): initializers (name, dims, data_type, float_data / raw_data little-endian, the flat order of
 * TensorValue.swift:45-116) and the Conv / ConvTranspose node attributes (strides, dilations). `infer_config` derives the
 * voice geometry from initializer shapes + those attributes; `build_blob` emits the initializers in the order of
 * include/piper_hip_voice_layout.h (names = the ONNX initializer names, e.g. `enc_p.encoder.attn_layers.0.conv_q.weight`,
 * ONNXParsingTests.swift:32), folding `weight_g`/`weight_v` pairs if the export kept weight norm. Tested against ONNX files
 * WRITTEN by the test-suite (no Piper voice exists offline): real-voice naming is unpinned. */
typedef struct piper_hip_onnx piper_hip_onnx;
typedef struct {
  char name[128];
  int32_t data_type; /* ONNX TensorProto.DataType: 1 FLOAT, 6 INT32, 7 INT64, 9 BOOL */
  int32_t rank;
  int64_t dims[8];
  int64_t count;
} piper_hip_onnx_tensor_info;
int piper_hip_onnx_open(const char* path, piper_hip_onnx** out); /* mmap: weights are copied once, by build_blob */
int piper_hip_onnx_open_memory(const void* data, size_t size, piper_hip_onnx** out);
void piper_hip_onnx_close(piper_hip_onnx* m);
/* ir_version, default-domain opset, node and initializer counts (ONNXParsingTests.swift:22-36 pins 15 / 2755 / 401). */
int piper_hip_onnx_counts(const piper_hip_onnx* m, int64_t* ir_version, int64_t* opset, int* n_nodes, int* n_initializers);
int piper_hip_onnx_initializer(const piper_hip_onnx* m, int index, piper_hip_onnx_tensor_info* out);
int piper_hip_onnx_find(const piper_hip_onnx* m, const char* name); /* initializer index or -1 */
int piper_hip_onnx_read_f32(const piper_hip_onnx* m, int index, float* dst, size_t n);
int piper_hip_onnx_infer_config(const piper_hip_onnx* m, piper_hip_voice_config* cfg);
/* Is the node graph the computation this library's fixed launch schedule performs for `cfg`? The reference executes whatever the graph
 * says (GraphExecutor.swift:227-265); this library does not look at the nodes when it runs, so it looks at them HERE: header (opset 15,
 * I/O names, Gather first — ONNXParsingTests.swift:22-36), op census (the 50 arms of GraphExecutor.swift:592-2659), every Conv /
 * ConvTranspose's attributes and effective padding, the attention / skew / softmax / LayerNorm(eps) / FFN structure per encoder layer,
 * Flips and tanh·sigmoid gates of the flow, LeakyRelu slopes, residual Adds and the MRF mean of the generator, the RandomNormalLike count.
 * PIPER_HIP_ERR_UNSUPPORTED + a message naming the first differing node otherwise (csrc/onnx_verify.cpp). */
int piper_hip_onnx_verify_graph(const piper_hip_onnx* m, const piper_hip_voice_config* cfg);
/* build_blob = verify_graph, then the initializers in layout order. _unchecked skips the verification: for weight containers that carry
 * no graph; the caller vouches that the weights belong to a standard Piper VITS. */
int piper_hip_onnx_build_blob(const piper_hip_onnx* m, const piper_hip_voice_config* cfg, float* host_blob, size_t n_floats);
int piper_hip_onnx_build_blob_unchecked(const piper_hip_onnx* m, const piper_hip_voice_config* cfg, float* host_blob, size_t n_floats);
/* The numbers this library needs from the voice's `.onnx.json` (PiperConfig.swift:3-47). */
typedef struct {
  int32_t sample_rate, num_symbols, num_speakers;
  float noise_scale, length_scale, noise_w;
} piper_hip_piper_json_info;
int piper_hip_piper_json(const char* json_text, piper_hip_piper_json_info* out);
/* Is the voice the `.onnx.json` describes one this library renders correctly with geometry `cfg` ALONE? ERR_UNSUPPORTED for
 * num_speakers > 1 (without its speaker table the audio would be wrong without any error; the opt-in route is
 * piper_hip_voice_check_json_speakers below), ERR_SHAPE when num_symbols differs from the embedding rows of the graph. */
int piper_hip_voice_check_json(const piper_hip_voice_config* cfg, const piper_hip_piper_json_info* info);

/* Waveform → 16-bit PCM / mono WAV (WavFileWriter.swift:20-30, 44-60): clamp to [−1,1], ×32767, truncate toward zero. */
int piper_hip_pcm16_from_f32(const float* samples, size_t n, int16_t* pcm);
int piper_hip_wav_write(const char* path, const float* samples, size_t n, int32_t sample_rate);

/* Inputs of one utterance ⇔ ExecutionInputs + overrides (GraphExecutor.swift:5-15, 101-104): phoneme ids, the three
 * `scales` of PiperMetalRuntime.synthesize (PiperMetalRuntime.swift:62-80), and the tensors the reference lets a caller
 * pre-seed by name — the duration predictor's output (per-id frame counts) and the two RandomNormalLike tensors
 * (PiperTestVector.swift:24-29: `dp` [1,2,T], `main` [1,inter,F]).
 * ABI 2 appended everything below `noise_scale`; zero-initialising the struct keeps the ABI-1 behaviour. */
#define PIPER_HIP_NOISE_INJECTED 0 /* NULL noise pointers mean zeros (deterministic parity runs) */
#define PIPER_HIP_NOISE_DEVICE 1   /* NULL noise pointers are generated on the device by the reference's RandomNormalLike
                                      stream (piper_hip_random_normal_like_f32) with `seed`; non-NULL pointers still win */
typedef struct {
  const int64_t* phoneme_ids; /* [T] host */
  int32_t t;
  const int32_t* durations; /* [T] host, frames per id (≥0), F = Σ durations — the `overrides` route; NULL: predicted on the device
                               by the voice's stochastic duration predictor from length_scale / noise_w / dp_noise (ABI 2) */
  const float* noise;       /* `main` RandomNormalLike [inter, F] host, may be NULL (see noise_mode). Must be NULL when durations is NULL
                               (F is not known to the caller then: PIPER_HIP_ERR_ARG; predict_durations first, or noise_mode DEVICE) */
  float noise_scale;        /* scales[0] */
  /* ---- ABI 2 ---- */
  int32_t noise_mode;       /* PIPER_HIP_NOISE_INJECTED / PIPER_HIP_NOISE_DEVICE */
  uint32_t seed;            /* PIPER_HIP_NOISE_DEVICE: RandomNormalLike seed; the reference hard-codes 1234 (GraphExecutor.swift:2658) */
  float length_scale;       /* scales[1]: w = exp(logw)·length_scale (only read when durations == NULL; 0 is taken as 1.0) */
  float noise_w;            /* scales[2]: scale of the predictor's latent noise (only read when durations == NULL) */
  const float* dp_noise;    /* `dp` RandomNormalLike [2, T] host, may be NULL (see noise_mode; both RandomNormalLike nodes of the
                               reference draw from the SAME seed, so device mode reproduces that) */
} piper_hip_utterance;

/* Samples `synthesize` will produce for this utterance (F · Π up_rates); −1 on a bad utterance, −2 when the durations are to
 * be predicted (unknown before `prepare`: ask piper_hip_voice_prepared_samples afterwards). */
int64_t piper_hip_voice_num_samples(const piper_hip_voice* v, const piper_hip_utterance* u);
/* After prepare: samples of each batch item of the slot (n_items entries) and/or their sum. */
int piper_hip_voice_prepared_samples(const piper_hip_voice* v, int slot, int64_t* per_item, int max_items, int64_t* total);
/* After prepare: the frames-per-id actually used (supplied or predicted), items back to back (Σ T_b entries). */
int piper_hip_voice_durations(const piper_hip_voice* v, int slot, int32_t* out, int max_entries, int* n_entries);
/* Attach a plan for this utterance's bucket to `slot` (building and caching it if the voice has none idle) and upload the
 * utterance's inputs; returns the slot id ≥ 0. Plans own a stream and an arena, so several prepared slots can be launched
 * back-to-back and overlap on the GPU. */
int piper_hip_voice_prepare(piper_hip_voice* v, const piper_hip_utterance* u, int slot);
/* The same for `n` utterances in ONE schedule whose kernels carry a batch dimension, so a launch costs what one utterance
 * costs in dispatches. The items may differ in length (ragged batch): the schedule is the bucket of the longest item, every
 * length-aware kernel reads each item's true lengths from device memory — taps past an item's end read as zero padding and
 * attention excludes the keys past it, i.e. the reference graph's x_mask / y_mask semantics — so each item's result is what
 * it would be alone, and tiles entirely past an item's end cost (almost) nothing. Group items of similar length to limit the
 * padding. `collect` returns the n waveforms back to back, each at its own length. */
int piper_hip_voice_prepare_batch(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot);
/* The same for utterances whose durations are to be PREDICTED (durations = noise = NULL), without the host round trip
 * prepare_batch makes between the duration predictor and the rest (it needs the frame count to pick the plan): the caller states an upper
 * bound on the frames per item, the plan is the bucket of `max_frames`, and the frame counts stay on the device — generate_path
 * (the exported graph's CumSum / Less chain, GraphExecutor.swift:1283-1330 CumSum) runs there too and every kernel masks by its result, so
 * the waveform is what prepare_batch would have produced. Nothing waits for the GPU here. Until `collect`,
 * piper_hip_voice_prepared_samples reports the CAPACITY (n · bucket(max_frames) · hop) — the room `collect` needs — and afterwards the
 * true lengths; piper_hip_voice_durations answers after `collect`. An item whose prediction exceeds `max_frames` makes `collect` fail
 * with PIPER_HIP_ERR_SHAPE (prepare it again with a larger bound or through prepare_batch) — unless the item carries a prosody with
 * `fit` (piper_hip_voice_slot_prosody): then its durations are compressed to the bound on the device and it succeeds. */
int piper_hip_voice_prepare_batch_bounded(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot, int max_frames);
/* Plans (schedule + arena + HIP graph) are cached per voice by bucket — phonemes rounded up to 16, frames to 16 (64 beyond
 * 1024) — and batch size, least recently used first out, so a (T, F) never seen before usually finds its graph ready and
 * `prepare` is only the input upload ("warm"); a new bucket pays schedule construction + arena inside `prepare` once ("cold"), and
 * the plan's first launch runs eagerly and captures + instantiates its graph behind itself. Reports the bucket of a prepared slot and
 * the cache's size. */
int piper_hip_voice_plan_info(const piper_hip_voice* v, int slot, int32_t* bucket_t, int32_t* bucket_f, int32_t* cached_plans,
                              size_t* cached_bytes);
/* Bounds of the voice's plan cache: at most `max_plans` plans and `max_bytes` of arenas (0 = the default 24 GiB) are kept; idle plans are
 * evicted least recently used first, plans attached to a slot never. Defaults: 128 plans. */
int piper_hip_voice_set_plan_cache(piper_hip_voice* v, int max_plans, size_t max_bytes);
/* Wall milliseconds of the phases of the LATEST plan build (a "cold" prepare): [0] stream / events, [1] schedule construction + arena
 * allocation, [2] arena initialisation, [3] always 0 (there is no validation pass any more; the entry is kept for the ABI), [4] graph
 * capture, [5] graph instantiate. [4] and [5] are 0 after the prepare and are filled by the plan's first launch. */
int piper_hip_voice_last_build_breakdown(const piper_hip_voice* v, double out_ms[6]);
/* Batch size of a prepared slot (0 if the slot is not prepared). */
int piper_hip_voice_batch_size(const piper_hip_voice* v, int slot);
/* Enqueue the prepared slot's forward pass (one hipGraphLaunch). No host sync. */
int piper_hip_voice_launch(piper_hip_voice* v, int slot);
/* Wait for the slot and copy the waveform(s) [batch · num_samples] to host (NULL = just wait). */
int piper_hip_voice_collect(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples);
/* The duration predictor alone (text encoder + `dp` of the graph): frames per id for `n` utterances (their `durations` fields are
 * ignored), items back to back in `durations_out` (Σ T_b entries); `logw_out` (optional, same length) receives the predictor's
 * log-durations before exp / length_scale / ceil. This is what `prepare` runs first when an utterance has durations == NULL. */
int piper_hip_voice_predict_durations(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int32_t* durations_out, float* logw_out,
                                      int max_entries);
/* Streaming ⇔ PiperMetalRuntime.synthesizeStream (PiperMetalRuntime.swift:82-115) — which "today chunks the final
 * waveform". Here the text encoder and the flow run once (stream_begin) and the HiFi-GAN generator decodes the latent
 * window by window: each stream_next decodes `chunk_frames` frames plus the generator's receptive field on both sides
 * (piper_hip_voice_receptive_field frames; clamped at the utterance's ends) and returns chunk_frames · hop samples, so the
 * first audio is available after encoder + flow + one window instead of the whole utterance. The samples equal
 * synthesize()'s up to fp32 summation order (tile splits depend on the window length). Batch 1.
 * stream_begin returns the number of chunks (≥ 1) or a negative status; stream_next sets *n_samples = 0 at the end. */
int piper_hip_voice_receptive_field(const piper_hip_voice* v);
int piper_hip_voice_stream_begin(piper_hip_voice* v, const piper_hip_utterance* u, int slot, int chunk_frames);
int piper_hip_voice_stream_next(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples, int64_t* n_samples);
/* Batched streaming: one slot holds a group of `n` utterances (1 ≤ n ≤ 256, ragged; durations may be NULL = predicted, as in
 * prepare_batch). The encoder and the flow run once for the whole group; each stream_next_batch then decodes the next `chunk_frames`
 * of every item still active in ONE generator launch (batch = n rounded up to a power of two; finished, dropped and pad rows have
 * length 0). Each item's chunks equal what stream_begin / stream_next give for that utterance alone.
 * stream_begin_batch returns the number of steps (max over items of ceil(F_i / chunk_frames)) or a negative status.
 * stream_next_batch writes the chunks of the active items back to back in item order into host_audio (at most n · chunk_frames · hop
 * samples); n_samples[i] (n entries) = samples of item i in this step, 0 once item i is finished or dropped. All zero = end of the
 * group. stream_next on a slot holding a group of n > 1 returns PIPER_HIP_ERR_ARG.
 * stream_drop: the client of item `item` went away; later steps skip it (its row has length 0). Until the frame where its stream would have
 * ended, the item's window still counts when a step picks its plan, so the other items receive, bit for bit, the samples they would have
 * received without the drop; once only dropped items are left the group has ended. */
int piper_hip_voice_stream_begin_batch(piper_hip_voice* v, const piper_hip_utterance* utts, int n, int slot, int chunk_frames);
int piper_hip_voice_stream_next_batch(piper_hip_voice* v, int slot, float* host_audio, int64_t max_samples, int64_t* n_samples);
int piper_hip_voice_stream_drop(piper_hip_voice* v, int slot, int item);
/* Streaming pool: a batched stream whose rows are taken and freed while it runs (continuous batching for the generator). The closest
 * reference role is still PiperMetalRuntime.synthesizeStream (PiperMetalRuntime.swift:82-115); the pool itself has no counterpart there.
 * A session joins at any time, is active from the next stream_next_batch on, and frees its row with its last chunk or a stream_drop; the
 * next join may take that row (free rows are handed out lowest index first). Each item's chunks are what stream_begin / stream_next give
 * for that utterance alone (same windows; fp32 summation order). The generator batch is `capacity` rounded up to a power of two for the
 * pool's whole life, as for a group, so groups and pools of one size share generator plans and no plan is built mid-stream.
 * On a pool slot: stream_next_batch takes n_samples[capacity] and packs the chunks back to back in row order; all zero = the pool is idle
 * (not closed). stream_drop(v, slot, item) drops the session in that row. stream_next returns PIPER_HIP_ERR_ARG. prepare*, stream_begin,
 * stream_begin_batch and stream_pool_open on the slot close the pool first, as a prepare replaces a prepare; voice_destroy closes open pools.
 * A refused join leaves nothing joined and the pool intact: more items than free rows = PIPER_HIP_ERR_SHAPE; work_slot == slot, or a
 * work_slot that itself holds a pool = PIPER_HIP_ERR_ARG. After a join, piper_hip_voice_durations / piper_hip_voice_prepared_samples on
 * work_slot report that join's items (it is a prepared slot). A join with supplied durations does not wait for its encoder + flow; with
 * durations == NULL it keeps prepare_batch's host round trip for the predicted frame counts (stream_pool_join_bounded, below, does not). */
/* An empty pool of `capacity` rows (1 ≤ capacity ≤ 256) on `slot`; every step decodes chunk_frames frames per active row. */
int piper_hip_voice_stream_pool_open(piper_hip_voice* v, int slot, int capacity, int chunk_frames);
/* Encoder + flow (and the predictor where durations == NULL) for n new utterances on `work_slot` (any other slot id; what it held is
 * replaced, and it may be reused for another join or prepare as soon as this returns). Their latents move into free rows of the pool.
 * items_out[n] = the rows taken (the item ids for n_samples / stream_drop). samples_out[n] = total samples each item will deliver. */
int piper_hip_voice_stream_pool_join(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                     int* items_out, int64_t* samples_out);
int piper_hip_voice_stream_pool_free_rows(const piper_hip_voice* v, int slot);   /* ≥ 0, or a negative status */
int piper_hip_voice_stream_pool_close(piper_hip_voice* v, int slot);
/* prepare + launch + collect: PiperMetalRuntime.synthesize (PiperMetalRuntime.swift:62-80). */
int piper_hip_voice_synthesize(piper_hip_voice* v, const piper_hip_utterance* u, float* host_audio,
                               int64_t max_samples, int64_t* n_samples);

/* ---- 16-bit PCM straight from the device (DESIGN.md §4 "PCM output") ----
 * Every host of this library ends in 16-bit PCM (WavFileWriter.swift:20-30 in the reference's CLI; Piper's own tools emit int16). These
 * entry points convert on the device, right behind the plan's graph on the slot's stream, and transfer int16: half the bytes of the fp32
 * waveform and no conversion pass on the host. The arithmetic is a contract, bit for bit:
 *   normalize == 0   y = x · gain (one fp32 multiply; gain 1 leaves x as it is), then exactly piper_hip_pcm16_from_f32(y): NaN → 0, clamp to
 *                    [−1, 1], × 32767.0 in DOUBLE precision, truncate toward zero.
 *   normalize == 1   Piper's audio_float_to_int16 carried out in float32, per utterance (batch item): peak = max |x| over the item's true
 *                    samples (NaN ignored; an empty item has peak 0), scale = the correctly rounded fp32 quotient 32767 / max(0.01, peak),
 *                    v = x · scale, then v · gain (both fp32), NaN → 0, clamp to [−32767, 32767], truncate toward zero.
 * gain: linear volume, 0 is taken as 1.0; negative or non-finite is PIPER_HIP_ERR_ARG. A NULL params pointer means {1.0, 0}. */
typedef struct {
  float gain;        /* linear volume; 0 is taken as 1.0 */
  int32_t normalize; /* 0: the reference conversion; 1: peak normalisation per utterance */
} piper_hip_pcm_params;
/* Per-op: `count` device floats → `count` device int16 (normalize == 0 arithmetic). `*out` convention of the other ops; a caller-supplied
 * `*out` needs 2-byte alignment only. count may be 0. */
int piper_hip_pcm16_f32(piper_hip_ctx* ctx, const float* x, size_t count, float gain, int16_t** out, piper_hip_stream stream);
/* piper_hip_voice_collect with int16 samples: waits like collect, leaves the slot as collect leaves it (the fp32 audio stays in the plan, so
 * collect and collect_pcm16 may each be called afterwards, in any order, with different params) and writes the items back to back at their
 * true lengths. On a bounded slot it is the collecting call: host_pcm needs room for the capacity (as collect), the first `total`
 * samples are the answer (piper_hip_voice_prepared_samples afterwards), an item over max_frames is PIPER_HIP_ERR_SHAPE. */
int piper_hip_voice_collect_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm, int64_t max_samples);
/* prepare + launch + collect_pcm16 on slot 0. */
int piper_hip_voice_synthesize_pcm16(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                     int64_t max_samples, int64_t* n_samples);
/* stream_next / stream_next_batch (groups and pools) with int16 samples. A PCM step consumes the step exactly as the float call does, and
 * float and PCM steps may alternate on one stream. normalize = 1 is PIPER_HIP_ERR_UNSUPPORTED and consumes nothing (an utterance's peak is
 * not known before its last window); gain is allowed. The stream-safe alternative is a level ("Level control" below). */
int piper_hip_voice_stream_next_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                      int64_t max_samples, int64_t* n_samples);
int piper_hip_voice_stream_next_batch_pcm16(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int16_t* host_pcm,
                                            int64_t max_samples, int64_t* n_samples);
/* After a collect_pcm16 with normalize = 1: max |x| of each item of the slot (PIPER_HIP_ERR_ARG before one). */
int piper_hip_voice_peaks(const piper_hip_voice* v, int slot, float* peaks, int max_items);

/* ---- Output rate: 8–48 kHz PCM from the device (DESIGN.md §4 "Output rate") ----
 * A voice synthesises at its own rate (22 050 Hz; low and x_low 16 000 Hz). These entry points convert to the consumer's rate on the device,
 * fused into the 16-bit PCM conversion, behind the plan's graph on the slot's stream. The conversion is a contract, bit for bit:
 *   ratio     g = gcd(in, out), L = out / g, M = in / g. Output sample j sits at input position j·M / L.
 *   filter    Kaiser-windowed sinc designed in double, once per (in, out): P = 2·ceil(24·max(L, M) / L) taps per phase (integer arithmetic),
 *             cutoff fc = 0.93·min(1, L / M); tap time tau(p, t) = t − (P/2 − 1) − p / L for phase p in [0, L), tap t in [0, P);
 *             h = fc·sinc(fc·tau), sinc(x) = sin(pi x) / (pi x); w = I0(9·sqrt(1 − (tau / (P/2))^2)) / I0(9) for |tau| < P/2, else 0;
 *             c[p][t] = h·w, every phase divided by its own sum in double (unit DC gain), rounded once to fp32. The table is [L][P] floats.
 *   sample    u = j·M in 64-bit integers, n = u div L, p = u mod L:  y[j] = sum over t = 0 … P−1 of c[p][t] · x[n − (P/2 − 1) + t],
 *             x reading as 0 outside [0, N); accumulated in fp32 in ascending t from 0.0f, each product rounded, then each sum (no FMA).
 *             An item of N samples yields J(N) = ceil(N·L / M) samples.
 *   to int16  y goes through exactly the contract of piper_hip_pcm_params above. With normalize = 1 the peak is that of the fp32 waveform
 *             at the voice's rate, so piper_hip_voice_peaks means the same at every rate; an overshoot of the resampled signal is clamped.
 *   rates     output 8000, 11025, 16000, 22050, 24000, 32000, 44100 or 48000, and L ≤ 640, P ≤ 256 (every pair from 16 000 and 22 050:
 *             P ≤ 134, table ≤ 121 KB); anything else is PIPER_HIP_ERR_UNSUPPORTED. out == in is not a filter: the call behaves bit for
 *             bit as the un-resampled one.
 * Streams are exact across chunk boundaries: a step whose chunk covers input samples [s, e) of N emits outputs [j0, j1), j0 where the
 * previous step ended (0 at the start), j1 = J(N) on the item's last step (e == N), else max(j0, ceil((e − P/2)·L / M)) — every output
 * whose taps end before e; the up to P − 1 samples before s come from a per-row history on the device. The concatenation of a row's
 * steps equals the whole-item conversion of the same fp32 samples bit for bit. A step delivers at most
 * ceil((e − s)·L / M) + ceil((P/2)·L / M) + 1 samples per row (piper_hip_resample_step_bound). */
/* Host-only (no device needed): L, M and taps per phase of a pair (each pointer may be NULL); the [L][P] table the kernels use;
 * J(n_in); the per-row step bound. The two counts return a negative status on a bad pair or a negative n_in. */
int piper_hip_resample_info(int32_t in_rate, int32_t out_rate, int32_t* L, int32_t* M, int32_t* taps);
int piper_hip_resample_taps(int32_t in_rate, int32_t out_rate, float* table, size_t max_floats);
int64_t piper_hip_resample_count(int32_t in_rate, int32_t out_rate, int64_t n_in);
int64_t piper_hip_resample_step_bound(int32_t in_rate, int32_t out_rate, int64_t n_in);
/* piper_hip_wav_write for samples that are 16-bit PCM already, at whatever rate they were delivered. */
int piper_hip_wav_write_pcm16(const char* path, const int16_t* pcm, size_t n, int32_t sample_rate);
/* Per-op: `count` device floats → J(count) device samples, the fp32 y (resample_f32) or int16 of y·gain (normalize == 0 arithmetic).
 * `*out` convention of the other ops; *out_count (may be NULL) receives J(count). */
int piper_hip_resample_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float** out,
                           size_t* out_count, piper_hip_stream stream);
int piper_hip_resample_pcm16_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float gain,
                                 int16_t** out, size_t* out_count, piper_hip_stream stream);
/* collect_pcm16 at out_rate: the same rules on plain, ragged and bounded slots, the items back to back at J(true length). The fp32 audio
 * stays in the plan, so it may follow or precede collect / collect_pcm16 in any order. On a bounded slot max_samples must cover J of the
 * capacity per item. */
int piper_hip_voice_collect_pcm16_rate(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int32_t out_rate, int16_t* host_pcm,
                                       int64_t max_samples);
/* prepare + launch + collect_pcm16_rate on slot 0; *n_samples = J(samples of the utterance). */
int piper_hip_voice_synthesize_pcm16_rate(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params,
                                          int32_t out_rate, int16_t* host_pcm, int64_t max_samples, int64_t* n_samples);
/* The output rate of the stream on `slot`: allowed after stream_begin, stream_begin_batch or stream_pool_open and before the slot's first
 * step (a pool: also before its first join); later it is PIPER_HIP_ERR_ARG. From then on stream_next_pcm16 / stream_next_batch_pcm16 on
 * that slot deliver at out_rate: n_samples[i] are output samples (all zero still means end / idle), stream_pool_join's samples_out reports
 * J(N_i), and the float steps stream_next / stream_next_batch return PIPER_HIP_ERR_ARG and consume nothing. A max_samples too small is
 * PIPER_HIP_ERR_SHAPE and consumes nothing; normalize = 1 stays PIPER_HIP_ERR_UNSUPPORTED on steps; a step at a rate needs a buffer
 * (host_pcm == NULL is PIPER_HIP_ERR_ARG on single streams, groups and pools alike, and consumes nothing). A new begin / open resets the
 * slot to the voice's own rate. stream_rate reports the current rate (or a negative status). Where normalize = 1 is refused, a level
 * ("Level control" below) is the stream-safe alternative. */
int piper_hip_voice_stream_set_rate(piper_hip_voice* v, int slot, int32_t out_rate);
int piper_hip_voice_stream_rate(piper_hip_voice* v, int slot);
/* The int16 samples one step of that slot can deliver at its current rate (rows × the per-row bound), or a negative status. */
int64_t piper_hip_voice_stream_step_capacity(piper_hip_voice* v, int slot);

/* ---- G.711 output: μ-law and A-law bytes from the device (DESIGN.md §4 "G.711 output") ----
 * A telephony consumer (RTP PCMU / PCMA, a SIP trunk) takes one G.711 byte per sample, not s16le. These entry points compand on the
 * device, in the kernels that write int16 otherwise, and transfer the bytes: half of what the PCM path carries and no companding pass on
 * the host. A byte is a pure function of the int16 sample the contracts above define: byte = law(s), s exactly what the 16-bit PCM
 * contract gives for that sample — normalize 0 or 1, with gain, at the voice's rate or resampled. Nothing about s changes. `>>` is an
 * arithmetic shift on a 32-bit int:
 *   μ-law   v = s >> 2;  neg = v < 0;  m = min(neg ? −v : v, 8159) + 33                      (33 … 8192)
 *           seg  = how many of {0x3F,0x7F,0xFF,0x1FF,0x3FF,0x7FF,0xFFF,0x1FFF} are < m        (0 … 8)
 *           code = seg == 8 ? 0x7F : (seg << 4) | ((m >> (seg + 1)) & 15)
 *           byte = code ^ (neg ? 0x7F : 0xFF)
 *   A-law   v = s >> 3;  neg = v < 0;  m = neg ? −v − 1 : v                                  (0 … 4095)
 *           seg  = how many of {0x1F,0x3F,0x7F,0xFF,0x1FF,0x3FF,0x7FF,0xFFF} are < m          (0 … 7)
 *           code = (seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15)
 *           byte = code ^ (neg ? 0x55 : 0xD5)
 * This is the definition of Sun's g711.c, which CPython's audioop.lin2ulaw / lin2alaw (width 2) implement; the tests compare against
 * tables made with audioop on all 65 536 inputs. It is NOT the one's-complement variant of ITU-T G.191, which differs on some negative
 * inputs: here μ(−1) = μ(−4) = 0x7E. Known answers (μ, A): 0 → 0xFF, 0xD5; −1 → 0x7E, 0x55; 32767 → 0x80, 0xAA; −32768 → 0x00, 0x2A.
 * μ-law produces 255 distinct codes (never 0x7F), A-law all 256.
 * Decoding is host only, for consumers and tests:
 *   μ-law   u = ~b & 0xFF;  t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);  s = (u & 0x80) ? 0x84 − t : t − 0x84
 *   A-law   a = b ^ 0x55;  t = (a & 15) << 4;  seg = (a & 0x70) >> 4;
 *           t = seg == 0 ? t + 8 : seg == 1 ? t + 0x108 : (t + 0x108) << (seg − 1);  s = (a & 0x80) ? t : −t
 * A law that is neither constant is PIPER_HIP_ERR_ARG everywhere. */
#define PIPER_HIP_G711_MULAW 1
#define PIPER_HIP_G711_ALAW  2
/* Host-only (no device needed): n int16 samples → n bytes, and back. n may be 0. */
int piper_hip_g711_from_pcm16(int law, const int16_t* pcm, size_t n, uint8_t* out);
int piper_hip_g711_to_pcm16(int law, const uint8_t* in, size_t n, int16_t* pcm);
/* A mono G.711 WAV file: an 18-byte fmt chunk (format tag 7 for μ-law, 6 for A-law, 1 channel, byte rate = sample rate, block align 1,
 * 8 bits, cbSize 0), a fact chunk holding n, the data chunk with a pad byte behind it when n is odd; the RIFF size counts all of it. */
int piper_hip_wav_write_g711(const char* path, int law, const uint8_t* bytes, size_t n, int32_t sample_rate);
/* Per-op: `count` device floats at in_rate → J(count) device bytes at out_rate, law(int16 of y·gain) with the normalize == 0 arithmetic.
 * `*out` convention of the other ops; a caller-supplied `*out` may sit at any byte address. *out_count (may be NULL) receives J(count).
 * in_rate == out_rate (> 0) is not a filter: the rates are not looked up in the list and the bytes are law(·) of what
 * piper_hip_pcm16_f32 gives. Otherwise the rate rules and status codes are those of piper_hip_resample_pcm16_f32. count may be 0. */
int piper_hip_g711_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float gain, int law, uint8_t** out,
                       size_t* out_count, piper_hip_stream stream);
/* collect_pcm16_rate / synthesize_pcm16_rate with G.711 bytes, every rule carried over: plain, ragged and bounded slots, the items back to
 * back at J(true length) (an item may start at any byte), the bounded slot's collecting call, any order with collect, collect_pcm16 and
 * collect_pcm16_rate (the fp32 audio stays in the plan), normalize = 1 with piper_hip_voice_peaks afterwards. out_rate equal to the
 * voice's rate is not a filter. max_samples and *n_samples count samples, which are bytes here. */
int piper_hip_voice_collect_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, int32_t out_rate, uint8_t* host,
                                 int64_t max_samples);
int piper_hip_voice_synthesize_g711(piper_hip_voice* v, const piper_hip_utterance* u, const piper_hip_pcm_params* params, int law,
                                    int32_t out_rate, uint8_t* host, int64_t max_samples, int64_t* n_samples);
/* stream_next_pcm16 / stream_next_batch_pcm16 (single streams, groups and pools) with G.711 bytes. The law is an argument of the step, not
 * state of the slot; the rate is what stream_set_rate set, or the voice's own. A G.711 step consumes the step exactly as a PCM step does —
 * the same output range [j0, j1), the same history update — so PCM and G.711 steps may alternate on one stream, and on a slot at the
 * voice's own rate float steps as well. n_samples[i] counts samples (= bytes); piper_hip_voice_stream_step_capacity answers for these
 * steps too. Refused calls follow the PCM steps and consume nothing: normalize = 1 is PIPER_HIP_ERR_UNSUPPORTED, a short buffer
 * PIPER_HIP_ERR_SHAPE, host == NULL on a slot with an output rate PIPER_HIP_ERR_ARG, a bad law PIPER_HIP_ERR_ARG. The stream-safe alternative to
 * normalize = 1 is a level ("Level control" below). */
int piper_hip_voice_stream_next_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, uint8_t* host,
                                     int64_t max_samples, int64_t* n_samples);
int piper_hip_voice_stream_next_batch_g711(piper_hip_voice* v, int slot, const piper_hip_pcm_params* params, int law, uint8_t* host,
                                           int64_t max_samples, int64_t* n_samples);

/* ---- Mixed formats: every row of a batched stream picks its rate, encoding and gain (DESIGN.md §4 "Mixed formats") ----
 * One process that serves a SIP trunk (8 kHz μ-law), browsers (48 kHz s16) and an ASR tap (16 kHz s16) from one voice wants ONE pool: one
 * generator launch per step for all of them, and one output launch behind it whatever the formats present. On a mixed slot the output
 * format is a property of the item (group) or of the row's occupant (pool), fixed from the call that supplies it until the row is freed.
 * Per row the arithmetic is the contracts above and nothing else: S16 rows follow "16-bit PCM" (normalize = 0) and "Output rate", μ-law and
 * A-law rows "G.711 output", each with the stream emit rule [j0, j1) of the row's own (L, M, P). F32 rows at a rate deliver the fp32 y of
 * piper_hip_resample_f32, F32 rows at the voice's own rate the float chunk itself. The concatenation of a row's chunks equals the
 * whole-item conversion of the item's fp32 samples at the row's format, bit for bit; a mixed slot whose rows all carry one format
 * delivers, row by row, the bytes and counts of a slot with stream_set_rate and the matching step call.
 * Normalisation is not offered: a format has no field for it, because steps never could normalise. Single streams (stream_begin) are out
 * of scope: one row has stream_set_rate plus a law per step already. A level ("Level control" below) is the stream-safe alternative.
 *
 * Layout of one step's output. Rows are written in row order. Row r's chunk starts at byte_off[r] and holds n_samples[r] · elem(r) bytes,
 * elem = 2 for S16, 1 for G.711, 4 for F32. byte_off of the first delivering row is 0; every later one is the previous delivering row's
 * end rounded up to a multiple of 4. A row that delivers nothing reports the offset the next delivering row takes (n_samples[r] = 0; it
 * owns no byte). The content of the pad bytes is unspecified. The step's total is the last delivering row's end.
 *
 * Sizing the buffer. A row's share of a step is B · elem rounded up to a multiple of 4, with B = chunk_frames · hop at the voice's own
 * rate and B = piper_hip_resample_step_bound(voice rate, out_rate, chunk_frames · hop) otherwise — host-only arithmetic, so a host can
 * size its buffer ahead of joins (capacity × the largest share it will ever admit). piper_hip_voice_stream_step_capacity_bytes sums the
 * shares of the rows as they stand.
 *
 * Format checks happen on the host, at the call that supplies the format: encoding outside 0 … 3, a negative or non-finite gain, or a
 * gain other than 0 or 1 on an F32 row is PIPER_HIP_ERR_ARG; a rate outside the "Output rate" list (or L > 640, or P > 256) is
 * PIPER_HIP_ERR_UNSUPPORTED. out_rate 0 or the voice's own rate is not a filter. */
#define PIPER_HIP_ENC_S16   0
#define PIPER_HIP_ENC_MULAW 1   /* == PIPER_HIP_G711_MULAW */
#define PIPER_HIP_ENC_ALAW  2   /* == PIPER_HIP_G711_ALAW  */
#define PIPER_HIP_ENC_F32   3
typedef struct {
  int32_t out_rate;  /* 0 = the voice's own rate (not a filter) */
  int32_t encoding;  /* PIPER_HIP_ENC_* */
  float   gain;      /* 0 is taken as 1.0; F32 rows: must be 0 or 1 */
} piper_hip_stream_format;   /* all zero = s16 at the voice's rate, gain 1 */
/* Marks the batched stream on `slot` mixed. Allowed exactly where stream_set_rate is: after stream_begin_batch or stream_pool_open, before
 * the slot's first step, and for a pool also before its first join. It allocates the per-row history as stream_set_rate does; every row
 * starts in the default format (all zero). PIPER_HIP_ERR_ARG, and nothing changes: on a single stream (stream_begin), on a slot that has
 * a rate set, on a second call, after the slot has started. A new begin / open resets the slot to not mixed. On a mixed slot
 * stream_set_rate, stream_rate and stream_step_capacity return PIPER_HIP_ERR_ARG. */
int piper_hip_voice_stream_set_mixed(piper_hip_voice* v, int slot);
/* A mixed GROUP, before its first step: the formats of items 0 … n−1 (n ≥ 1); items past n take the last entry. A refused call changes
 * nothing. On a pool it is PIPER_HIP_ERR_ARG: there the join brings the formats. */
int piper_hip_voice_stream_item_formats(piper_hip_voice* v, int slot, const piper_hip_stream_format* fmts, int n);
/* stream_pool_join on a mixed pool with one format per joining item. samples_out[i] = J(N_i) at item i's rate (N_i at the voice's own).
 * A row keeps its format until it is freed; the next occupant brings its own and never sees the previous occupant's history. A plain
 * stream_pool_join on a mixed pool joins its items in the default format. A refused join leaves nothing joined. On a pool that is not
 * mixed it is PIPER_HIP_ERR_ARG. */
int piper_hip_voice_stream_pool_join_formats(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                             const piper_hip_stream_format* fmts, int* items_out, int64_t* samples_out);
/* The step of a mixed slot, and the only one it accepts: every other stream_next call on a mixed slot, and this call on a slot that is not
 * mixed, is PIPER_HIP_ERR_ARG and consumes nothing. n_samples and byte_off have one entry per item (group) or row (pool); n_samples
 * counts samples, as the other steps do; the bytes follow the layout above. All n_samples zero means end / idle. max_bytes smaller than
 * the step's total is PIPER_HIP_ERR_SHAPE, host == NULL PIPER_HIP_ERR_ARG; both consume nothing. stream_drop works as before. */
int piper_hip_voice_stream_next_batch_mixed(piper_hip_voice* v, int slot, void* host, int64_t max_bytes, int64_t* n_samples, int64_t* byte_off);
/* The bytes one step of that mixed slot can deliver with the rows' current formats: the sum of the shares (above) of the rows that hold
 * an unfinished item. Free pool rows count 0, so ask again after a join. A negative status on a slot that is not mixed. */
int64_t piper_hip_voice_stream_step_capacity_bytes(piper_hip_voice* v, int slot);
/* The format of item / row `item` as the slot holds it: out_rate 0 when it is the voice's own rate, gain never 0. PIPER_HIP_ERR_ARG for
 * a free pool row, an item out of range, or a slot that is not mixed. */
int piper_hip_voice_stream_item_format(piper_hip_voice* v, int slot, int item, piper_hip_stream_format* out);

/* ---- Level control: a look-ahead limiter on every output route (DESIGN.md §4 "Level control") ----
 * normalize = 1 needs an utterance's peak, which no stream step before the last knows. What a streaming pipeline uses instead is a
 * look-ahead limiter: a drive, a ceiling and a short, known delay. It is one more stage of the output chain — generator → volume → EQ →
 * loudness gain → level → resampler → PCM / G.711 / mixed — on whole items and on every stream route, and it changes nothing for a request that does not ask
 * for it. The limiter is a contract, bit for bit. All arithmetic is fp32, each operation rounded on its own (no FMA); fl() marks a rounding:
 *   constants  B = 32 samples per block, W = 6 blocks of look-ahead      (PIPER_HIP_LEVEL_BLOCK, PIPER_HIP_LEVEL_LOOKAHEAD)
 *   params     drive (0 is taken as 1.0), ceiling (0 → 1.0), release_ms (0 → 50)
 *              drive finite in (0, 1000], ceiling in [0.001, 1], release_ms in [1, 10000]; otherwise PIPER_HIP_ERR_ARG
 *   rel        = fp32( min(1, 32·1000 / (rate · release_ms)) ), computed in double and rounded once.
 *              `rate` is the rate of the samples being limited: the voice's own rate on every voice route.
 *   u[n]       = fl(x[n] · drive)                                          n in [0, N), at the voice's own rate, before any resampling
 *   p[k]       = max |u[n]| over block k = [32k, 32k+32) ∩ [0, N).  NaN is ignored.  Blocks past the item have p = 0.
 *   r[k]       = p[k] > ceiling ? the correctly rounded fp32 quotient ceiling / p[k] : 1.0f
 *   m[k]       = min(r[k], r[k+1], …, r[k+W])
 *   G[k]       = min(m[k], fl(G[k−1] + rel)),  G[−1] = 1.0f                 (linear release, instant hold)
 *   node[0]    = G[0];  node[k] = min(G[k−1], G[k])                         k = 1 … K,  K = ceil(N / 32)
 *   g(n)       = fl(node[k] + fl(fl(node[k+1] − node[k]) · (i / 32)))       k = n div 32, i = n mod 32.  i / 32 is exact.
 *   y[n]       = fl(u[n] · g(n))
 * y then goes through the contracts above unchanged: "Output rate", "16-bit PCM" with normalize = 0, "G.711 output", "Mixed formats"; the
 * per-call or per-row gain is applied where it is applied without a level. Both nodes of block k are ≤ r[k], so |y| ≤ ceiling up to
 * rounding (≤ ceiling · (1 + 2^−22)). An item that never exceeds the ceiling with drive 1 passes bit for bit: G stays 1.0 and ·1.0f is exact.
 *
 * Emit rule for streams. When samples [0, e) of N are known and more follow, y is final on [0, ready(e)), ready(e) = max(0, 32·(e div 32 −
 * (W + 1))). A step whose chunk covers [s, e) hands the downstream stage the limited samples [lo, hi): lo where the previous step ended
 * (0 at the start), hi = N when e == N, else ready(e). Downstream applies its own rule to that range as if it were the chunk: the
 * "Output rate" emit rule with (s, e) = (lo, hi) on a rated or mixed row, hi − lo samples otherwise. The concatenation of a row's steps
 * equals the whole-item result bit for bit, on every format. A step delivers at most (e − s) + 255 limited samples per row
 * (piper_hip_level_step_bound); stream_step_capacity, stream_step_capacity_bytes and the share of a mixed row use that in place of
 * chunk_frames · hop on a slot with a level. Enabling a level requires chunk_frames · hop ≥ 512, so that a non-final step never delivers
 * nothing ("all zero" keeps meaning end / idle); smaller is PIPER_HIP_ERR_ARG. */
#define PIPER_HIP_LEVEL_BLOCK     32
#define PIPER_HIP_LEVEL_LOOKAHEAD 6
typedef struct {
  float drive;       /* 0 is taken as 1.0 */
  float ceiling;     /* 0 is taken as 1.0 */
  float release_ms;  /* 0 is taken as 50 */
} piper_hip_level;   /* all zero = {1, 1, 50} */
/* Host-only (no device needed). level_check: PIPER_HIP_ERR_ARG with a message that names the field. level_info: the fp32 rel of that level
 * at `rate`. level_ready: ready(e). level_step_bound: n_in + 255. The two counts return a negative status on a negative argument. */
int piper_hip_level_check(const piper_hip_level* level);
int piper_hip_level_info(const piper_hip_level* level, int32_t rate, float* rel);
int64_t piper_hip_level_ready(int64_t e);
int64_t piper_hip_level_step_bound(int64_t n_in);
/* Host-only twin of the kernels: n host floats → n host floats, the contract above. n may be 0. */
int piper_hip_level_from_f32(const piper_hip_level* level, int32_t rate, const float* x, size_t n, float* y);
/* Per-op: `count` device floats sampled at `rate` → `count` device floats. `*out` convention of the other ops; count may be 0. */
int piper_hip_level_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, const piper_hip_level* level, float** out,
                        piper_hip_stream stream);
/* Whole items: the level of slot id `slot`, state of the slot id like slot_speakers: it persists until replaced, or cleared with NULL.
 * Every later collect, collect_pcm16, collect_pcm16_rate, collect_g711 and the synthesize twins (slot 0) on that slot deliver y instead of
 * x, on plain, ragged and bounded slots. The fp32 audio in the plan stays raw: collects with and without a level may follow one launch in
 * any order, and the `audio` tap keeps returning x. normalize = 1 together with a level is PIPER_HIP_ERR_ARG, before anything is waited for. */
int piper_hip_voice_slot_level(piper_hip_voice* v, int slot, const piper_hip_level* level);
/* Streams: the level of the stream on `slot`, for every row of it. Allowed exactly where stream_set_rate is: after stream_begin,
 * stream_begin_batch or stream_pool_open, before the slot's first step, and for a pool also before its first join; later it is
 * PIPER_HIP_ERR_ARG. It combines with stream_set_rate or stream_set_mixed in either order, and a new begin / open clears it. All step
 * flavours work on such a slot — float, pcm16, g711, mixed — with their refusals unchanged. A pool row taken by a new occupant starts with
 * lo = 0 and G[−1] = 1 and never reads its predecessor's carry. stream_pool_join's samples_out and stream_pool_item_samples are unchanged:
 * the limiter neither adds nor drops samples over an item. stream_level reports what the slot holds, defaults resolved
 * (PIPER_HIP_ERR_ARG if none). */
int piper_hip_voice_stream_set_level(piper_hip_voice* v, int slot, const piper_hip_level* level);
int piper_hip_voice_stream_level(piper_hip_voice* v, int slot, piper_hip_level* out);

/* ---- Loudness: ITU-R BS.1770 / EBU R128 integrated loudness, measured and normalised on the device (DESIGN.md §4 "Loudness") ----
 * normalize = 1 is peak normalisation and says nothing about how loud an item sounds; a host that wants every prompt at one programme
 * loudness (−16 or −23 LUFS) measures by BS.1770. It is one more stage of the output chain on whole items — generator → volume → EQ →
 * loudness gain → level → resampler → PCM / G.711 — and it changes nothing for a request that does not ask for it. Each later stage is exactly as its
 * contract stands, reading u in place of x. The measurement is mono integrated loudness at the rate of the samples measured: the voice's
 * own rate on every voice route.
 *   rates      8000, 16000, 22050, 24000, 32000, 44100, 48000. Any other rate is PIPER_HIP_ERR_UNSUPPORTED (11025: 100 ms is not a whole
 *              number of samples).
 *   K-weight   all in double; two biquads re-derived per rate fs with K = tan(π·f0 / fs):
 *              shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                         Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K²,
 *                         b = [(Vh + Vb·K/Q + K²)/a0, 2(K² − Vh)/a0, (Vh − Vb·K/Q + K²)/a0],  a = [1, 2(K² − 1)/a0, (1 − K/Q + K²)/a0]
 *              high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, a0 = 1 + K/Q + K²,
 *                         b = [1, −2, 1],  a = [1, 2(K² − 1)/a0, (1 − K/Q + K²)/a0]
 *              (at 48 000 Hz these are the standard's table). y = HP(shelf(x)), each a direct recurrence from zero state; a non-finite
 *              x[n] reads as 0.
 *   blocks     h = fs/10;  J = (N − 4h) div h + 1 for N ≥ 4h, else 0;  z_j = (1/4h)·Σ y[n]² over [jh, jh + 4h);  l_j = −0.691 + 10·log10 z_j
 *   gates      A = {j : l_j > −70};  Γr = −0.691 + 10·log10(mean_A z) − 10;  R = {j ∈ A : l_j > Γr};  L = −0.691 + 10·log10(mean_R z).
 *              J = 0 or A empty: L = −∞, the item is unmeasurable. L is held in double and reported rounded once to fp32.
 *   target     target_lufs (0 is taken as −16; otherwise finite in [−70, −1]), max_gain_db (0 → 20; otherwise in (0, 60]); anything else is
 *              PIPER_HIP_ERR_ARG with a message that names the field.
 *   gain       d = min((double)target − (double)L, (double)max_gain_db) with L the reported fp32;  g = (float)pow(10, d/20).
 *              Attenuation is unbounded. An unmeasurable item has g = 1.0f.
 *   u[n]       = fl(x[n] · g), one fp32 multiply.
 * The device's L lies within 0.002 LU of the sequential float64 recurrence, and the same samples give the same bits of L on every run
 * (fixed-order sums, no floating-point atomics).
 * Streams are out of scope: an item's integrated loudness is not known before its end. Measure a voice or a speaker once with
 * piper_hip_voice_loudness and pass the resulting gain as a level's `drive` or a mixed row's `gain`; slot_loudness does not touch streams. */
typedef struct {
  float target_lufs;  /* 0 is taken as −16 */
  float max_gain_db;  /* 0 is taken as 20 */
} piper_hip_loudness; /* all zero = {−16, 20} */
/* Host-only (no device needed). loudness_check: PIPER_HIP_ERR_ARG with a message that names the field. loudness_coeffs: the two biquads at
 * `rate`, a[0] = 1. loudness_from_f32: the sequential double twin of the kernels, n host floats → L (n may be 0: −∞). loudness_gain: g for a
 * reported L (−∞ → 1.0; NaN or +∞ is PIPER_HIP_ERR_ARG). */
int piper_hip_loudness_check(const piper_hip_loudness* loudness);
int piper_hip_loudness_coeffs(int32_t rate, double shelf_b[3], double shelf_a[3], double hp_b[3], double hp_a[3]);
int piper_hip_loudness_from_f32(int32_t rate, const float* x, size_t n, float* lufs);
int piper_hip_loudness_gain(const piper_hip_loudness* loudness, float lufs, float* gain);
/* Per-op: `count` device floats sampled at `rate` → one fp32 L in host memory. With a non-NULL stream the value is there after
 * piper_hip_stream_sync. count may be 0, which gives −∞. */
int piper_hip_loudness_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, float* lufs_host, piper_hip_stream stream);
/* Whole items: the loudness target of slot id `slot`, state of the slot id exactly like slot_level: it persists until replaced, NULL
 * clears it. Every later collect, collect_pcm16, collect_pcm16_rate, collect_g711 and the synthesize twins (slot 0) on that slot deliver u
 * — or the limited u when the slot also has a level — on plain, ragged and bounded slots; on bounded slots the lengths are read from device
 * memory, and nothing new waits for the GPU. The fp32 audio in the plan and the `audio` tap stay raw. normalize = 1 together with a
 * loudness is PIPER_HIP_ERR_ARG, before anything is waited for. A voice whose rate is not in the list is PIPER_HIP_ERR_UNSUPPORTED here. */
int piper_hip_voice_slot_loudness(piper_hip_voice* v, int slot, const piper_hip_loudness* loudness);
/* Waits for the slot, measures the raw items of its latest launch if that has not happened yet (the measurement is kept until the next
 * launch or prepare), and returns per item L and the g the slot's target implies, 1.0 when the slot has no target. Either array may be
 * NULL; a non-NULL one holds max_items entries (fewer than the slot's items is PIPER_HIP_ERR_SHAPE). A bounded slot that has not been
 * collected is PIPER_HIP_ERR_ARG. */
int piper_hip_voice_loudness(piper_hip_voice* v, int slot, float* lufs, float* gain, int max_items);

/* ---- Per-phoneme volume: a gain envelope on the device (DESIGN.md §4 "Volume") ----
 * Prosody controls how long an id lasts and how lively it is, level and loudness how loud a whole item is. What is left is the volume of a
 * word or a phoneme: SSML <prosody volume>, <emphasis>, a ducked parenthesis, a muted id. A host cannot shape it afterwards: on the
 * bounded route the frames per id are decided on the device, and on the PCM, rate and G.711 routes it receives integers at another rate,
 * behind the limiter and the loudness gain. So the volume is one more stage of the output chain, on whole items and on every stream route
 * — generator → volume → EQ → loudness gain → level → resampler → PCM / G.711 / mixed — and it changes nothing for a request that does not ask
 * for it. The envelope is a
 * contract, bit for bit. All arithmetic is fp32, each operation rounded on its own (no FMA); fl() marks a rounding:
 *   gain[t]    one linear gain per phoneme id, finite, in [0, 16]; otherwise PIPER_HIP_ERR_ARG. A NULL array, or an item without a volume,
 *              is all 1.0.
 *   F, hop     the item's true frame count (the rule of every route: max(Σ d, 1)) and Π up_rates.
 *   gf[f]      = gain[t(f)], f in [0, F). t(f) is the id frame f belongs to: the smallest t with cum[t] > f, cum the running sum of the
 *              frames per id. The single frame of an all-zero duration row belongs to id 0. This is what the plan's frame-to-id map holds.
 *   c          = hop div 2. Frame f is centred on sample f·hop + c.
 *   for sample n in [0, F·hop):
 *     m = n − c;  k = floor(m / hop) (k = −1 for n < c);  i = m − k·hop, in [0, hop)
 *     a = gf[max(k, 0)];  b = gf[min(k + 1, F − 1)]
 *     w = the correctly rounded fp32 quotient (float)i / (float)hop          (exact for hop = 256, the hop of every preset)
 *     e(n) = fl(a + fl(fl(b − a) · w))
 *     v[n] = fl(x[n] · e(n))
 * Where neighbouring frames share a gain, b − a = 0 and e is that gain exactly; between two ids the gain moves linearly over one hop
 * (11.6 ms at 22 050 Hz), so there is no step in the waveform. An all-1.0 volume gives v = x bit for bit on every finite sample; a gain of
 * 0 mutes. Known answer: hop 4, gf = [1, 0.5], x all 1.0 → v = [1, 1, 1, 0.875, 0.75, 0.625, 0.5, 0.5].
 * Every later stage reads v in place of x, its own contract unchanged: the loudness measurement and piper_hip_voice_loudness measure v;
 * the limiter's u = fl(v · drive); the peak of normalize = 1, and piper_hip_voice_peaks, is max |v|; the resampler, PCM and G.711 follow.
 * The fp32 audio in the plan and the `audio` tap stay raw.
 * Streams (single, group, pool, mixed pool). A step whose chunk covers frames [fs, fe) shapes samples [fs·hop, fe·hop) with the absolute
 * sample index n; it reads gf of frames fs − 1 … fe, all known from the begin or the join on (a bounded join: from its resolution on, and
 * nothing in the join waits). There is no delay, no carry and no change to any count: n_samples, samples_out, stream_step_capacity* and
 * every emit rule downstream are what they are without a volume, and "window:audio" stays raw. The concatenation of a row's steps equals
 * the whole-item result bit for bit, on every format. A pool row's new occupant brings its own gains, or none, and never reads its
 * predecessor's. A stream whose rows carry no volume adds no launch. */
typedef struct {
  const float* gain;  /* [t] linear gains, NULL = all 1.0 */
  int32_t t;          /* the item's number of ids */
} piper_hip_volume;   /* 16 bytes */
/* Host-only (no device needed). volume_check: PIPER_HIP_ERR_ARG with a message that names the field and the index.
 * volume_frames: gf of an item with `t` ids from the frames per id actually used, F = max(Σ d, 1) (Σ d = 0 gives gain[0]). `volume` NULL
 * is all 1.0; its t different from `t` is PIPER_HIP_ERR_SHAPE. *frames receives F; frame_gain may be NULL to ask for F alone, otherwise it
 * holds max_frames entries (fewer than F is PIPER_HIP_ERR_SHAPE).
 * volume_from_f32: the sequential twin of the kernels, v from gf and x. n must equal frames · hop, otherwise PIPER_HIP_ERR_SHAPE; hop in
 * [1, 65536]. */
int piper_hip_volume_check(const piper_hip_volume* volume);
int piper_hip_volume_frames(const piper_hip_volume* volume, const int32_t* durations, int32_t t, float* frame_gain, int64_t max_frames,
                            int64_t* frames);
int piper_hip_volume_from_f32(const float* frame_gain, int64_t frames, int32_t hop, const float* x, size_t n, float* y);
/* Per-op: `count` device floats and a device frame_gain[frames] → `count` device floats. `*out` convention of the other ops; count must
 * equal frames · hop (PIPER_HIP_ERR_SHAPE otherwise), hop in [1, 65536], count may be 0. The pointers need no alignment beyond a float's. */
int piper_hip_volume_f32(piper_hip_ctx* ctx, const float* x, size_t count, const float* frame_gain, int64_t frames, int32_t hop, float** out,
                         piper_hip_stream stream);
/* The volume of the NEXT staging call on slot id `slot`, with the lifecycle of piper_hip_voice_slot_prosody: entry i is for item i, items
 * past `n` have none; the arrays are copied here; n = 0 clears the assignment; n outside 0 … 256 is PIPER_HIP_ERR_ARG; every entry is
 * checked here on the host (a refusal leaves the assignment in place as it was). The staging calls prepare, prepare_batch,
 * prepare_batch_bounded, stream_begin, stream_begin_batch, synthesize* (slot 0) and stream_pool_join* (where `slot` is the work slot) take
 * the assignment and clear it, whether or not they succeed; an entry whose t differs from its item's t is PIPER_HIP_ERR_SHAPE there, and
 * nothing is staged. Unlike the duration fields of prosody, a volume is allowed on
 * items with supplied durations: it does not touch them. It combines freely with prosody (including fit), speakers, level, loudness,
 * output rates and mixed formats. Every later collect, collect_pcm16, collect_pcm16_rate and collect_g711 of that staging delivers v, on plain, ragged and
 * bounded slots; on bounded slots lengths and the frame-to-id map are read from device memory, and nothing new waits for the GPU.
 * Debug tap "vol.gain" [1, F] per item (piper_hip_voice_tap): gf compacted to the item's true F, on a slot whose last staging carried a
 * volume; otherwise PIPER_HIP_ERR_ARG; on a bounded slot that has not been collected PIPER_HIP_ERR_UNSUPPORTED, like the other taps. */
int piper_hip_voice_slot_volume(piper_hip_voice* v, int slot, const piper_hip_volume* items, int n);

/* ---- Equaliser: a biquad cascade on the device (DESIGN.md §4 "Equaliser") ----
 * A high-pass for rumble, a presence lift for small loudspeakers, a telephone band ahead of 8 kHz G.711: a spectral stage that a host
 * cannot add afterwards without giving up the device's output formats, and that must sit in front of the loudness measurement and the
 * limiter. It is one more stage of the output chain on whole items — generator → volume → EQ → loudness gain → level → resampler →
 * PCM / G.711 / mixed — and it changes nothing for a request that does not ask for it. Every later stage reads the EQ's output in place of
 * its input, its own contract unchanged: the loudness measurement and piper_hip_voice_loudness measure it, the limiter reads it, the peak
 * of normalize = 1 and piper_hip_voice_peaks are taken over it. The fp32 audio in the plan and the `audio` tap stay raw.
 * The EQ is a contract, bit for bit. All of it is in double, every operation rounded on its own (no FMA), the fp32 fields widened:
 *   params     n sections in 1 … 4, each {type, f0_hz, q, gain_db}; type 1 lowpass, 2 highpass, 3 bandpass (0 dB peak), 4 notch, 5 peaking,
 *              6 lowshelf, 7 highshelf. f0_hz finite in [10, 0.45·rate], q finite in [0.1, 30], gain_db finite in [−30, 30] for peaking
 *              and the shelves and exactly 0 for the other types; rate in [8000, 48000]: the rate of the samples being filtered, the
 *              voice's own rate on every voice route. Anything else is PIPER_HIP_ERR_ARG with a message that names the field and the index.
 *   design     w0 = 2.0·M_PI·f0 / fs,  c = cos(w0),  s = sin(w0),  α = s / (2.0·Q),  A = pow(10.0, gain_db / 40.0),  r = 2.0·sqrt(A)·α
 *              (evaluated left to right as written, the RBJ Audio-EQ-Cookbook):
 *              lowpass    b = [(1.0 − c)/2.0, 1.0 − c, (1.0 − c)/2.0]                a = [1.0 + α, −2.0·c, 1.0 − α]
 *              highpass   b = [(1.0 + c)/2.0, −(1.0 + c), (1.0 + c)/2.0]             a = [1.0 + α, −2.0·c, 1.0 − α]
 *              bandpass   b = [α, 0.0, −α]                                           a = [1.0 + α, −2.0·c, 1.0 − α]
 *              notch      b = [1.0, −2.0·c, 1.0]                                     a = [1.0 + α, −2.0·c, 1.0 − α]
 *              peaking    b = [1.0 + α·A, −2.0·c, 1.0 − α·A]                         a = [1.0 + α/A, −2.0·c, 1.0 − α/A]
 *              lowshelf   b = [A·((A + 1.0) − (A − 1.0)·c + r), 2.0·A·((A − 1.0) − (A + 1.0)·c), A·((A + 1.0) − (A − 1.0)·c − r)]
 *                         a = [(A + 1.0) + (A − 1.0)·c + r, −2.0·((A − 1.0) + (A + 1.0)·c), (A + 1.0) + (A − 1.0)·c − r]
 *              highshelf  b = [A·((A + 1.0) + (A − 1.0)·c + r), −2.0·A·((A − 1.0) + (A + 1.0)·c), A·((A + 1.0) + (A − 1.0)·c − r)]
 *                         a = [(A + 1.0) − (A − 1.0)·c + r, 2.0·((A − 1.0) − (A + 1.0)·c), (A + 1.0) − (A − 1.0)·c − r]
 *              then b_i = b_i / a0 and a_i = a_i / a0: coefficients {b0, b1, b2, a1, a2}. A peaking section at 0 dB has b = a, b0 = 1 exactly.
 *   recurrence sections in order, each in transposed direct form II: y = b0·v + s1;  s1 = (b1·v − a1·y) + s2;  s2 = b2·v − a2·y;  v = y.
 *              v starts as x[n] widened (a non-finite x reads as 0); the output is y[n] = (float)v. The state is D = 2·n doubles, section i
 *              at (s1, s2) = (2i, 2i + 1).
 *   blocks     B = 64 samples; block k covers [64k, 64k + 64) ∩ [0, N). A [D][D] is the zero-input transition of one sample (column j: unit
 *              state j stepped once with v = 0). P_0 = A^64 by six squarings, P_{l+1} = P_l·P_l. In every matrix product and matrix-vector
 *              product the sum runs over ascending j, starting from the j = 0 product, each product and each sum rounded; P·S + T adds T
 *              after the sum.
 *              E[k] = the state after running block k from zero state over its true length. T_0[k] = E[k], T_{l+1}[m] = P_l·T_l[2m] +
 *              T_l[2m+1]. Start state of block k: S = 0, then for each set bit l of k, highest first, S ← P_l·S + T_l[(k >> l) − 1].
 *              Block k is run from S and its samples are output.
 * The block form differs from the plain sequential recurrence only by rounding (about 1e-12 of max|y| for a moderate set). A 0 dB
 * peaking EQ gives y = x bit for bit on every finite sample but −0, which becomes +0.
 * Streams (single, group, pool, mixed pool) need hop % 64 == 0 (every preset: hop 256), otherwise stream_set_eq is
 * PIPER_HIP_ERR_UNSUPPORTED. A row keeps as its carry one aggregate per set bit of its block count k (T_l[(k >> l) − 1]); a step folds the
 * carry into the start state of each of its blocks and pushes each block's E, merging equal levels as a binary counter does, so the
 * concatenated steps of a row equal the whole-item result bit for bit, on every format. The EQ adds no delay and changes no sample count,
 * capacity or emit rule; it runs behind the volume and in front of the level. A pool row taken by a new occupant starts at block 0 with
 * an empty carry and never reads its predecessor's. A stream without an EQ has no buffer and no launch. */
#define PIPER_HIP_EQ_MAX_SECTIONS 4
#define PIPER_HIP_EQ_BLOCK        64
#define PIPER_HIP_EQ_LOWPASS      1
#define PIPER_HIP_EQ_HIGHPASS     2
#define PIPER_HIP_EQ_BANDPASS     3
#define PIPER_HIP_EQ_NOTCH        4
#define PIPER_HIP_EQ_PEAKING      5
#define PIPER_HIP_EQ_LOWSHELF     6
#define PIPER_HIP_EQ_HIGHSHELF    7
typedef struct {
  int32_t type;     /* PIPER_HIP_EQ_LOWPASS … PIPER_HIP_EQ_HIGHSHELF */
  float f0_hz;
  float q;
  float gain_db;    /* peaking and shelves; exactly 0 otherwise */
} piper_hip_eq_section;
typedef struct {
  int32_t n;        /* sections in use, 1 … PIPER_HIP_EQ_MAX_SECTIONS */
  piper_hip_eq_section section[PIPER_HIP_EQ_MAX_SECTIONS];
} piper_hip_eq;
/* Host-only (no device needed). eq_check: the rules above at `rate`. eq_design: coeffs[i] = {b0, b1, b2, a1, a2} of section i, eq->n rows.
 * eq_from_f32: the host twin of the kernels, the same block tree: n host floats → n host floats (n may be 0). */
int piper_hip_eq_check(const piper_hip_eq* eq, int32_t rate);
int piper_hip_eq_design(const piper_hip_eq* eq, int32_t rate, double coeffs[][5]);
int piper_hip_eq_from_f32(const piper_hip_eq* eq, int32_t rate, const float* x, size_t n, float* y);
/* Per-op: `count` device floats sampled at `rate` → `count` device floats. `*out` convention of the other ops; count may be 0; the
 * pointers need no alignment beyond a float's. */
int piper_hip_eq_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t rate, const piper_hip_eq* eq, float** out,
                     piper_hip_stream stream);
/* Whole items: the EQ of slot id `slot`, state of the slot id like slot_level: it persists until replaced, NULL clears it. Every later
 * collect, collect_pcm16, collect_pcm16_rate, collect_g711 and the synthesize twins (slot 0) on that slot deliver the chain above, on
 * plain, ragged and bounded slots; on bounded slots the lengths are read from device memory and nothing new waits for the GPU. Collects
 * with different EQs may follow one launch in any order: the EQ'd items, and the loudness measured over them, are recomputed when the
 * slot's EQ changes. The EQ is checked here at the voice's rate (PIPER_HIP_ERR_ARG). */
int piper_hip_voice_slot_eq(piper_hip_voice* v, int slot, const piper_hip_eq* eq);
/* Streams: the EQ of the stream on `slot`, for every row of it. Allowed exactly where stream_set_level is: after stream_begin,
 * stream_begin_batch or stream_pool_open, before the slot's first step, and for a pool also before its first join; later it is
 * PIPER_HIP_ERR_ARG. It combines with stream_set_rate, stream_set_mixed and stream_set_level in either order, and a new begin / open clears
 * it. The design is built and uploaded here. stream_eq reports what the slot holds (PIPER_HIP_ERR_ARG if none). */
int piper_hip_voice_stream_set_eq(piper_hip_voice* v, int slot, const piper_hip_eq* eq);
int piper_hip_voice_stream_eq(piper_hip_voice* v, int slot, piper_hip_eq* out);

/* ---- Join: trim, fade and gap a batch into one programme on the device (DESIGN.md §4 "Join") ----
 * A text is a batch of sentences, and what a host plays is ONE piece of audio with a pause between them (Piper's --sentence-silence).
 * Putting it together on the host means floats down, a scan for the model's quiet head and tail, a second copy with silences, and the
 * resampler or compander on one core; on a bounded slot the host does not even know where an item ends before the device tells it. So
 * the join is one more stage of the whole-item output chain — generator → volume → EQ → loudness gain → level → join → resampler →
 * PCM / G.711 — and it changes nothing for a request that does not ask for it. It turns the NB items of a slot into one signal, the
 * programme:   lead silence, item 0 (trimmed, faded), gap 0, item 1, …, item NB − 1, tail silence.
 * Every later stage treats the programme as a single item of a length only the device knows. In particular, at an output rate other
 * than the voice's the programme is resampled as ONE signal; it is NOT the concatenation of the per-item resamples.
 * The join is a contract, bit for bit:
 *   counts     S(ms) = (int64) floor((double)ms · rate / 1000.0 + 0.5), the float widened first; rate = the rate of the samples being
 *              joined, on voice routes the voice's own. P = S(trim_pad_ms), Fd = S(fade_ms).
 *   kept range item i has N_i samples x. trim = 0: [s, t) = [0, N_i). trim = 1: a = the least index with fabsf(x[n]) > trim_threshold,
 *              e = the greatest (the compare is fp32 and false for NaN; ±Inf is above every threshold). None: s = t = 0, the item is
 *              empty and its gap is still emitted. Otherwise s = max(0, a − P), t = min(N_i, e + 1 + P).
 *   fades      only at an edge that was cut. g(k) = (float)((double)(k + 1) / (double)(Fd + 1)). Head, if s > 0: for k in
 *              [0, min(Fd, t − s)): y[s + k] = fl(x[s + k] · g(k)). Tail, if t < N_i: for k in [0, min(Fd, t − s)):
 *              y[t − 1 − k] = fl(y[t − 1 − k] · g(k)), applied after the head where they overlap. Every other kept sample is copied bit
 *              for bit.
 *   layout     S(lead_ms) samples of +0.0f; for each item its kept samples, and after every item but the last S(gap_i) zeros;
 *              S(tail_ms) zeros after the last item. gap_i = gaps[i] where the caller gave one (i < n_gaps), else gap_ms.
 *              start_i = the programme index of item i's first kept sample, len_i = t − s, total = the programme length.
 *   downstream collect delivers the `total` floats; collect_pcm16 / _rate / _g711 apply their contracts to the programme as one item of
 *              `total` samples: normalize = 1 takes ONE peak over the programme and piper_hip_voice_peaks reports one value; the delivered
 *              count is piper_hip_resample_count(rate, out_rate, total).
 *   identities the neutral join (all three silences 0, trim = 0) of one item reproduces the un-joined collect bit for bit on every sink;
 *              of a batch it reproduces the back-to-back items bit for bit on the sinks at the voice's own rate.
 * Anything outside the ranges below is PIPER_HIP_ERR_ARG with a message that names the field. */
#define PIPER_HIP_JOIN_MAX_ITEMS 256
typedef struct {
  float lead_ms, gap_ms, tail_ms;   /* each finite in [0, 10000] */
  int32_t trim;                     /* 0 or 1 */
  float trim_threshold;             /* finite, >= 0: linear amplitude of the signal that enters the join */
  float trim_pad_ms;                /* finite in [0, 1000] */
  float fade_ms;                    /* finite in [0, 100] */
} piper_hip_join;
/* Host-only (no device needed). join_check: the rules above; gaps (NULL with n = 0, else n values in 0 … 256): each finite in
 * [0, 10000]. join_counts: the S() values at `rate` (rate ≥ 1; any output pointer may be NULL). join_capacity: the no-trim upper bound
 * on total, lead + Σ N_i + the gaps + tail. join_from_f32: the host twin of the kernels: item i is x[item_off[i] … + item_len[i]), the
 * programme goes to y[max] (a shorter y is PIPER_HIP_ERR_SHAPE; only `total` samples are written), start / len ([n_items], optional)
 * and total receive the report. n_items in 1 … 256; items of length 0 are allowed. */
int piper_hip_join_check(const piper_hip_join* join, const float* gaps, int n);
int piper_hip_join_counts(const piper_hip_join* join, int32_t rate, int64_t* lead, int64_t* gap, int64_t* tail, int64_t* pad, int64_t* fade);
int piper_hip_join_capacity(const piper_hip_join* join, const float* gaps, int n_gaps, int32_t rate, const int64_t* item_samples, int n_items,
                            int64_t* samples);
int piper_hip_join_from_f32(const piper_hip_join* join, const float* gaps, int n_gaps, int32_t rate, const float* x, const int64_t* item_off,
                            const int64_t* item_len, int n_items, float* y, int64_t max, int64_t* start, int64_t* len, int64_t* total);
/* Per-op: arbitrary device floats x (4-byte alignment suffices), item i at x[item_off[i] … + item_len[i]) (host arrays) → the programme
 * in device memory: `*out` convention of the other ops, a caller's buffer holds piper_hip_join_capacity samples. start_host / len_host
 * ([n_items], optional) and total_host receive the report; the call waits for the device before it returns, whatever `stream` is
 * (the report is its answer). A capacity that does not fit an int is PIPER_HIP_ERR_SHAPE. */
int piper_hip_join_f32(piper_hip_ctx* ctx, const float* x, const int64_t* item_off, const int64_t* item_len, int n_items, int32_t rate,
                       const piper_hip_join* join, const float* gaps, int n_gaps, float** out, int64_t* start_host, int64_t* len_host,
                       int64_t* total_host, piper_hip_stream stream);
/* Whole items: the join of slot id `slot`, state of the slot id like slot_level / slot_eq: it persists until replaced, join = NULL clears
 * it; checked at the voice's rate. Every later collect, collect_pcm16, collect_pcm16_rate, collect_g711 and the synthesize twins (slot 0,
 * one item; their n_samples is the programme's count) on that slot deliver the programme, on plain, ragged and bounded slots. On a
 * bounded slot nothing new waits for the GPU: trims and offsets are decided on the device, where the lengths live. Collects with
 * different joins, or with and without one, may follow one launch in any order. The fp32 audio in the plan, the `audio` tap,
 * prepared_samples, durations, piper_hip_voice_loudness and prosody_report are unchanged. Streams have no join: a stream row is one item.
 * join_capacity: the samples a collect on the prepared slot needs room for at `out_rate` (0 = the voice's own):
 * piper_hip_resample_count of the no-trim bound, a bounded slot's items taken at their frame capacity; a shorter buffer is
 * PIPER_HIP_ERR_SHAPE and leaves the slot collectable, and a bound that does not fit an int is PIPER_HIP_ERR_SHAPE.
 * join_report: after a joined collect, start / len of each item ([max_items] ≥ the batch size, optional) and total, at the voice's rate;
 * PIPER_HIP_ERR_ARG if the slot was not collected with a join since its last launch. */
int piper_hip_voice_slot_join(piper_hip_voice* v, int slot, const piper_hip_join* join, const float* gaps, int n_gaps);
int piper_hip_voice_join_capacity(piper_hip_voice* v, int slot, int32_t out_rate, int64_t* samples);
int piper_hip_voice_join_report(const piper_hip_voice* v, int slot, int64_t* start, int64_t* len, int max_items, int64_t* total);

/* ---- Pitch: per-item semitone shift on the device, on whole-item routes (DESIGN.md §4 "Pitch") ----
 * SSML <prosody pitch>, the `pitch` field of a speech API's audio config: the one control of a TTS front end that a host had to apply
 * with a tool of its own, floats down, behind the device's whole output chain. An engine that owns the durations needs no overlap-add
 * and no search: to raise the pitch by ρ = 2^(st/12) it synthesises ρ times slower (length_scale, on the device already) and plays the
 * result ρ times faster. The only new arithmetic is a variable-ratio resampler, one more stage of the whole-item output chain —
 * generator → volume → pitch → EQ → loudness gain → level → join → resampler → PCM / G.711 — which changes nothing for a request that
 * does not ask for it. Formants move with the pitch (this is not a formant-preserving shift). The stage is a contract, bit for bit:
 *   parameters semitones is a finite float in [−12, 12]; keep_tempo is 0 or 1. Anything else is PIPER_HIP_ERR_ARG with a message that names
 *              the field.
 *   step       ρ = exp2((double)semitones / 12.0).  Q = (uint64) floor(ρ·2^32 + 0.5), a 32.32 fixed-point step in [2^31, 2^33].
 *              ρq = Q / 2^32, exact in double. Q == 2^32 is not a filter (semitones ±0 and anything that rounds there): the item passes
 *              bit for bit and N' = N.
 *   count      N' = ceil(N·2^32 / Q), for N < 2^30, in 64-bit integers.
 *   positions  output j reads input position u = j·Q (uint64): n = u >> 32, frac = u & 0xffffffff. p = frac >> 25 (128 phases).
 *              α = (float)((frac >> 1) & 0xffffff) · 2^−24, which is exact.
 *   filter     designed in double, once per Q. P = 2·((24·max(Q, 2^32) + 2^32 − 1) >> 32) taps: 48 for ρ ≤ 1, up to 96 at +12 semitones.
 *              fc = 0.93·min(1, 1/ρq). Rows p = 0 … 128 inclusive, taps t = 0 … P − 1: tau = t − (P/2 − 1) − p/128, h = fc·sinc(fc·tau),
 *              times the Kaiser window of "Output rate" (β = 9, half-width P/2, 0 for |tau| ≥ P/2). Every row is divided by its own sum
 *              in double and rounded once to fp32: the table c[129][P], at most 49 536 bytes.
 *   sample     y0 = Σ_t c[p][t]·x[n − (P/2 − 1) + t], y1 the same sum with c[p + 1]; x reads as 0 outside [0, N). Both sums are accumulated
 *              in fp32 in ascending t from 0.0f, each product rounded, then each sum (no FMA).  y[j] = fl(y0 + fl(α·fl(y1 − y0))).
 *   voice      the pitched item of a slot has F' = ceil(N' / hop) frames; samples [N', F'·hop) are +0.0f, a tail of less than one hop
 *              (under 12 ms). So every later stage keeps its interface: rows of frames × hop, lengths in frames on the device.
 *   tempo      rf = (float)ρq. keep_tempo = 1: the staging call uses length_scale' = fl(ls·rf) for that item, ls = the utterance's
 *              length_scale with 0 taken as 1.0; nothing else changes — the prosody rule and a bounded route's max_frames see the frames
 *              the model actually generates. keep_tempo = 1 on an item with supplied durations is PIPER_HIP_ERR_ARG: the caller owns
 *              those. keep_tempo = 0 is plain varispeed: the item comes out 1/ρ as long.
 *   chain      volume shapes the un-pitched frames it was computed for; every stage after the pitch sees the pitched items: the EQ, the
 *              loudness measurement and piper_hip_voice_loudness, the limiter, the peaks of normalize = 1 and piper_hip_voice_peaks, the
 *              join with join_report and join_capacity, the resampler, PCM and G.711.
 * One second of a 0.5 sine at 200, 1000 and 4000 Hz (22 050 Hz), shifted by −12 … +12 semitones, comes out at f·ρq with an SNR of
 * 92 … 114 dB against the ideal sine and a gain within 2e-5 of 1.
 * Streams have no pitch: stream_begin, stream_begin_batch and stream_pool_join* with a pitch pending on their slot return
 * PIPER_HIP_ERR_UNSUPPORTED, stage nothing and clear the pitch. */
typedef struct {
  float semitones;      /* finite, in [−12, 12] */
  int32_t keep_tempo;   /* 1: scale the predicted durations by ρ so that the item keeps its length; 0: varispeed */
} piper_hip_pitch;      /* 8 bytes */
/* Host-only (no device needed). pitch_check: the rules above. pitch_info: Q, P and rf of a shift (any output pointer may be NULL).
 * pitch_count: N' for n_in in [0, 2^30), a negative status code otherwise. pitch_taps: the [129][P] table (a shorter buffer is
 * PIPER_HIP_ERR_SHAPE); it exists for Q == 2^32 as well, where no route applies it. pitch_from_f32: the host twin of the kernel: n host
 * floats → N' host floats in y[max_out] (a shorter y is PIPER_HIP_ERR_SHAPE and nothing is written); *n_out receives N'. */
int piper_hip_pitch_check(const piper_hip_pitch* pitch);
int piper_hip_pitch_info(float semitones, uint64_t* step, int32_t* taps, float* length_factor);
int64_t piper_hip_pitch_count(float semitones, int64_t n_in);
int piper_hip_pitch_taps(float semitones, float* table, size_t max_floats);
int piper_hip_pitch_from_f32(float semitones, const float* x, size_t n, float* y, size_t max_out, size_t* n_out);
/* Per-op: `count` device floats (below 2^30) → N' device floats, no padding. `*out` convention of the other ops; *out_count receives N';
 * count may be 0; the pointers need no alignment beyond a float's. */
int piper_hip_pitch_f32(piper_hip_ctx* ctx, const float* x, size_t count, float semitones, float** out, size_t* out_count,
                        piper_hip_stream stream);
/* The pitch of the NEXT staging call on slot id `slot`, with the lifecycle of piper_hip_voice_slot_prosody and slot_volume: entry i is
 * for item i, items past `n` have none; n = 0 clears the assignment; n outside 0 … 256 is PIPER_HIP_ERR_ARG; every entry is checked here
 * on the host, with a message that names the entry and the field (a refusal leaves the assignment in place as it was). The staging calls
 * prepare, prepare_batch, prepare_batch_bounded and synthesize* (slot 0) take the assignment and clear it, whether or not they succeed.
 * An entry that resolves to Q == 2^32 with keep_tempo 0 is no pitch; if no item has one, the plan carries no pitch and launches nothing
 * new. Every later collect, collect_pcm16, collect_pcm16_rate and collect_g711 of that staging delivers the pitched items, on plain,
 * ragged and bounded slots; on bounded slots the lengths are read from device memory and nothing new waits for the GPU. The tables live
 * in the plan's device memory, one per distinct Q of the batch, uploaded by the staging call. prepared_samples, durations,
 * prosody_report, the `audio` tap and the plan's fp32 audio stay raw.
 * pitch_samples: the samples every item of the prepared slot delivers at the voice's rate, F'·hop (per_item [max_items] ≥ the batch
 * size, optional), and their sum; on a bounded slot the capacity before collect and the true values after it. Collect buffers are
 * checked against it. Without a pitch it reports what prepared_samples reports. */
int piper_hip_voice_slot_pitch(piper_hip_voice* v, int slot, const piper_hip_pitch* items, int n);
int piper_hip_voice_pitch_samples(piper_hip_voice* v, int slot, int64_t* per_item, int max_items, int64_t* total);

/* ---- Multi-speaker voices: speaker-conditioned synthesis (DESIGN.md §4 "Speakers") ----
 * A multi-speaker Piper voice carries a speaker table `emb_g` [S, gin] and three kinds of k = 1 `cond` convs over g = emb_g[sid] [gin, 1]
 * (the graph's `sid` input, read by PiperMetalRuntime.synthesize next to `scales`, PiperMetalRuntime.swift:62-80; in the graph a Gather
 * and Conv / Add nodes, GraphExecutor.swift:653-666, 1739-1810, 741-779):
 *   duration predictor   x = dp.pre(x) + dp.cond(g)                                                     hidden channels
 *   flow coupling f, WaveNet layer l
 *                        acts = tanh(a + g_l[:H]) · sigmoid(b + g_l[H:]), [a;b] = in_layers[l](x),
 *                        g_l = cond_layer(g)[2H·l : 2H·(l+1)]                                           2·hidden per layer
 *   generator            x = dec.conv_pre(z) + dec.cond(g)                                              up_initial
 * g has length 1 in time, so each of these is a per-item, per-channel constant added where the conv's own bias is added. The EFFECTIVE
 * BIAS of a conditioned conv is e[c] = fl(b[c] + fl(bc[c] + d[c])): d[c] the fp32 dot product of cond row c with g (any summation order), bc
 * the cond bias, b the conv's own bias; the consumer adds e exactly where it adds b in a voice without speakers, as one float. The rows
 * of one item in the order dp.pre (hidden; no such rows with dp_present = 0); for f in 0 … n_flows − 1, for l in 0 … wn_layers − 1: 2·hidden each; dec.conv_pre (up_initial)
 * form its SPEAKER ROW of Ctot = hidden + n_flows·wn_layers·2·hidden + up_initial floats (medium 6 592, high 6 848, x_low 3 424).
 * A speaker is a short mix g = Σ_k w_k · emb_g[id_k], 1 ≤ n ≤ 4, accumulated in fp32 from 0.0f in ascending k (product rounded, then the
 * sum): n = 1, w = 1.0 is the table row itself, the plain `sid`.
 * Everything here is opt-in: a voice nobody attached a table to builds the schedules, step names and buffers it built before these
 * symbols existed, and every refusal of a multi-speaker file stays at its entry point (piper_hip_onnx_infer_config,
 * piper_hip_voice_check_json, piper_hip_onnx_verify_graph). */
typedef struct {
  int32_t n_speakers; /* 1 … 65 536 */
  int32_t gin;        /* 4 … 1024, a multiple of 4 (Piper: 512) */
} piper_hip_speaker_config;
/* The speaker blob: packed fp32 like the voice blob, host-only entry points with the conventions of their voice twins. Tensor order:
 * emb_g.weight [S, gin]; dp.cond.weight [hidden, gin, 1], dp.cond.bias (only with cfg->dp_present); for each coupling f:
 * flow.flows.{2f}.enc.cond_layer.weight [2·hidden·wn_layers, gin, 1], .bias; dec.cond.weight [up_initial, gin, 1], dec.cond.bias.
 * The synthetic rule is piper_hip_voice_synthetic_blob's (tensor i of THIS blob takes index i), cond weights with fan_in = gin, emb_g
 * with fan_in = 1 (unit variance, like nn.Embedding). The voice blob, its layout and piper_hip_voice_config do not change. */
int piper_hip_speaker_blob_floats(const piper_hip_voice_config* cfg, const piper_hip_speaker_config* scfg, size_t* n_floats);
int piper_hip_speaker_blob_layout(const piper_hip_voice_config* cfg, const piper_hip_speaker_config* scfg, piper_hip_tensor_info* out,
                                  int max_entries, int* n_entries);
int piper_hip_speaker_synthetic_blob(const piper_hip_voice_config* cfg, const piper_hip_speaker_config* scfg, uint64_t seed, float* host_blob,
                                     size_t n_floats);
/* Give the voice its speaker table: once, before the voice's first prepare / predict / stream (later or twice: PIPER_HIP_ERR_ARG). Packs
 * the table, the cond weights [Ctot, gin], the cond biases and the conditioned convs' own biases for the request-path kernel
 * (csrc/speaker.hip); the blob is not retained. `on_device` as for piper_hip_voice_create. */
int piper_hip_voice_attach_speakers(piper_hip_voice* v, const piper_hip_speaker_config* scfg, const float* blob, int on_device);
int piper_hip_voice_num_speakers(const piper_hip_voice* v); /* 0 without a table (and for a NULL voice) */
typedef struct {
  int32_t n;        /* 1 … 4 mix entries */
  int32_t ids[4];   /* rows of emb_g */
  float weights[4];
} piper_hip_speaker;
/* The speakers of a slot id: entry i is for item i of every later prepare*, stream_begin* and synthesize* (slot 0) on that slot; for
 * stream_pool_join it is the assignment of `work_slot`. Items past `n` take the last entry; n = 0 (spk may be NULL) resets to the default,
 * speaker 0 alone. The assignment persists until replaced. A bad id, an entry's n outside 1 … 4, or a non-finite weight is
 * PIPER_HIP_ERR_ARG, checked here on the host (the device never indexes past the table); n outside 0 … 256 is PIPER_HIP_ERR_ARG; a voice
 * without a table is PIPER_HIP_ERR_UNSUPPORTED. The speakers reach the device with the ids and lengths of a prepare (plan inputs): one
 * launch per plan ("spk.rows", the first step) computes the speaker rows of all its items — the predictor plan the dp.pre rows, the main
 * plan the flow and generator rows — and a graph replay needs no host work. A stream carries each item's conv_pre row with its latent:
 * a pool row keeps its speaker until it is freed. */
int piper_hip_voice_slot_speakers(piper_hip_voice* v, int slot, const piper_hip_speaker* spk, int n);
/* piper_hip_voice_predict_durations (which has no slot) with speakers[n], one per utterance (NULL: speaker 0 alone; on a voice without a
 * table a non-NULL array is PIPER_HIP_ERR_UNSUPPORTED). */
int piper_hip_voice_predict_durations_speakers(piper_hip_voice* v, const piper_hip_utterance* utts, int n, const piper_hip_speaker* speakers,
                                               int32_t* durations_out, float* logw_out, int max_entries);
/* Multi-speaker `.onnx` files, opt-in. piper_hip_onnx_infer_config, piper_hip_onnx_build_blob, piper_hip_voice_check_json and
 * piper_hip_onnx_verify_graph refuse such a file exactly as before; a verifier for the conditioned graph does not exist yet, so the main
 * blob of such a file comes from piper_hip_onnx_build_blob_unchecked and the caller vouches for the graph.
 *   speaker_config          n_speakers = 0 (and gin = 0) when the file has no `emb_g.weight`; otherwise every cond tensor's presence and
 *                           shape is checked against `cfg`: PIPER_HIP_ERR_SHAPE naming the tensor.
 *   infer_config_speakers   infer_config without the refusal of `emb_g` / `cond` initializers.
 *   build_speaker_blob      the cond tensors in the order above, folding weight_g / weight_v pairs as the main loader does.
 *   check_json_speakers     check_json with num_speakers == n_speakers required instead of ≤ 1 (a missing or 0 count reads as 1). */
int piper_hip_onnx_speaker_config(const piper_hip_onnx* m, const piper_hip_voice_config* cfg, piper_hip_speaker_config* scfg);
int piper_hip_onnx_infer_config_speakers(const piper_hip_onnx* m, piper_hip_voice_config* cfg);
int piper_hip_onnx_build_speaker_blob(const piper_hip_onnx* m, const piper_hip_voice_config* cfg, const piper_hip_speaker_config* scfg,
                                      float* host_blob, size_t n_floats);
int piper_hip_voice_check_json_speakers(const piper_hip_voice_config* cfg, const piper_hip_speaker_config* scfg,
                                        const piper_hip_piper_json_info* info);

/* ---- Streaming pool: joins with predicted durations that never wait (DESIGN.md §4 "Bounded pool joins") ----
 * stream_pool_join with durations == NULL stalls the host until the predicted frame counts are back. The bounded join takes the route of
 * prepare_batch_bounded instead: the caller bounds the frames per item, the counts stay on the device, and the join enqueues its work and
 * returns.
 *   Accepted utterances  exactly what prepare_batch_bounded accepts: durations == NULL, noise == NULL (noise_mode DEVICE draws it on the
 *                        device), the same max_frames range; every refusal of that call carries over with its status.
 *   Refused joins        as stream_pool_join(_formats): more items than free rows = PIPER_HIP_ERR_SHAPE; work_slot == slot, a work slot
 *                        holding a pool, fmts on a pool that is not mixed, a format the pool refuses = PIPER_HIP_ERR_ARG (or the format's
 *                        own status). A refused join leaves nothing joined and the pool intact.
 *   Host waits           none: no stream or event synchronisation, no blocking copy. Two waits of the existing code remain: the one a join
 *                        makes for the adopts still queued before it REGROWS a row store, and whatever prepare_batch_bounded does to
 *                        recycle the work slot (its stream is waited for before its staging is rewritten; a bucket seen for the first
 *                        time builds its plans).
 *   Work slot            runs the bounded encoder, predictor, generate_path and flow. Every row store of the join is sized for the work
 *                        plan's frame bucket (the bucket of max_frames), which is the row's stride. Afterwards the work slot is a bounded
 *                        slot whose lengths are still on the device; it may be reused at once. piper_hip_voice_durations(work_slot) and
 *                        prepared_samples answer with the true values once the join has resolved, unless the slot was prepared again.
 *   Row state            a row taken by a bounded join is taken from the join on (it counts against stream_pool_free_rows) but has no
 *                        known length until it is resolved.
 *   Resolution           at the start of the next stream_next_batch* call of any flavour, or in stream_pool_item_samples: the host waits
 *                        for the join's event — which the step's stream would have waited for anyway — and reads the frame count the
 *                        device reported. F ≤ max_frames: the row is an ordinary active row with that F; windows, emit rule per format
 *                        and history are those of any other row. F > max_frames: the row is free again and marked failed until it is
 *                        taken again; it never delivers, the other items of the join are unaffected and the step returns OK. An item
 *                        whose prosody asks for `fit` (piper_hip_voice_slot_prosody on the work slot) never gets there: its durations
 *                        are compressed to max_frames on the device and the row resolves to an ordinary active row.
 *   Order                a bounded join is active from the next step on, like any join: the step waits for the joins made before it,
 *                        so the pool stays deterministic.
 *   stream_drop          on a row that is still pending frees it; the next join may take it (its adopt runs behind the pending one).
 *   Closing              stream_pool_close, voice_destroy and a prepare* / stream_pool_open on the slot wait for joins in flight first.
 *   Rates and formats    on a pool with an output rate the counts are J(N) at that rate. On a mixed pool the joining items' filter
 *                        tables are uploaded in the join, never inside a step, the packed buffer is regrown from the rows' shares of a
 *                        step as in stream_pool_join_formats, and stream_step_capacity_bytes counts a pending row's share. */
/* stream_pool_join for utterances whose durations are PREDICTED, without the host round trip: the caller bounds the frames per item as in
 * prepare_batch_bounded. Nothing in this call waits for the GPU. fmts: NULL, or n formats on a mixed pool (as stream_pool_join_formats;
 * non-NULL on a pool that is not mixed is PIPER_HIP_ERR_ARG). items_out[n] = the rows taken. There is no samples_out: the counts are
 * not known yet (piper_hip_voice_stream_pool_item_samples). */
int piper_hip_voice_stream_pool_join_bounded(piper_hip_voice* v, int slot, const piper_hip_utterance* utts, int n, int work_slot,
                                             int max_frames, const piper_hip_stream_format* fmts, int* items_out);
/* Total samples row `item`'s occupant will deliver, at the row's rate (J(N) on a rated or mixed row). Waits for the join that filled the
 * row if its front is still running. PIPER_HIP_ERR_SHAPE (message naming wanted and allowed frames) when the predictor exceeded the
 * join's max_frames: that item delivers nothing and its row is free. PIPER_HIP_ERR_ARG for a row that never held an item or is out of range. */
int piper_hip_voice_stream_pool_item_samples(piper_hip_voice* v, int slot, int item, int64_t* samples);
/* Joins of this pool whose front has not finished yet (hipEventQuery; never waits). ≥ 0, or a negative status. */
int piper_hip_voice_stream_pool_joins_pending(piper_hip_voice* v, int slot);

/* ---- Per-phoneme prosody: length, pause and noise control on every route (DESIGN.md §4 "Prosody") ----
 * The three `scales` of PiperMetalRuntime.synthesize (PiperMetalRuntime.swift:62-80) shape a whole utterance. A TTS host also wants a pause
 * after a clause (SSML <break>), a slower or faster word (<prosody rate>), a ceiling on one runaway duration of the stochastic predictor
 * and a flatter or livelier word. All of these are per-phoneme-id controls on two things the library computes itself: the frames per id
 * and the prior noise per frame; on the bounded routes neither ever reaches the host. The arithmetic is a contract; its integer part
 * holds bit for bit:
 *   w0 = fl(expf(logw) · length_scale)                        what the predictor's last step computes without prosody
 *   w1 = fl(w0 · length[t])
 *   c  = ceilf(w1);  d0 = c > 0 ? (c < 1e6 ? (int32)c : 1000000) : 0      NaN → 0
 *   d1 = max_frames[t] > 0 ? min(d0, max_frames[t]) : d0
 *   d  = max(d1, min_frames[t])                               ids past the item's length: 0
 *   fit (bounded routes, fit ≠ 0):  S = Σ d in int64;  if S > cap:  d[t] = (int32)((int64)d[t] · cap / S)   (floor)
 *         cap = the call's max_frames. Σ d ≤ cap follows. The bound is hard, so fitting may go below min_frames.
 *         wanted = S, fitted = 1. Otherwise d is unchanged, wanted = S, fitted = 0.
 *   then the rule of every route: the frame count is max(Σ d, 1), frame f belongs to the smallest t with cum[t] > f
 *   ns[t] = fl(noise_scale · noise[t])
 *   z_p[c][f] = m_p[c][t(f)] + fl(fl(nz[c][f] · expf(logs_p[c][t(f)])) · ns[t(f)])
 * Multiplying by 1.0f is exact, so an all-neutral prosody (1.0 for length and noise, 0 for the frame fields, or NULL arrays) gives the
 * result of the same request without prosody bit for bit. Without `fit` a bounded request over its bound fails as it does without prosody.
 * A request that carries prosody runs plans of its own (step names "dp.affine_exp_ceil_prosody" and "expand_noise_prosody" in the places
 * of "dp.affine_exp_ceil" and "expand_noise", the per-id arrays as plan inputs [NB][T] staged with the ids); a request without finds the
 * plans, step lists, buffers and kernel arguments it found before these symbols existed. The predictor plan of a request with prosody
 * keeps w0 as tap "dp.w" [1,T]; "dp.w.row" and "dp.dur.row" are the same buffer and "dp.dur" as whole bucket rows [T] per item, not
 * compacted to the item's length: both are 0 past it. "predict:" selectors of piper_hip_voice_tap and piper_hip_voice_time_subset address
 * the predictor plan the slot's last prepare ran. piper_hip_voice_predict_durations has no slot and ignores prosody. */
typedef struct {
  const float*   length;      /* [t] multiplier on the id's duration w; NULL = all 1.0 */
  const int32_t* min_frames;  /* [t] floor on the id's frames (a pause: raise the blank after a word); NULL = all 0 */
  const int32_t* max_frames;  /* [t] ceiling on the id's frames, 0 = none; NULL = none */
  const float*   noise;       /* [t] multiplier on noise_scale for the frames of this id; NULL = all 1.0 */
  int32_t t;                  /* entries of every non-NULL array; must equal the utterance's t */
  int32_t fit;                /* bounded routes only: compress instead of failing when the frames exceed the call's max_frames */
} piper_hip_prosody;          /* 40 bytes */
/* Host-only. length and noise finite and in [0, 1000]; frame values in [0, 1 000 000]; max_frames[i] ≠ 0 requires min_frames[i] ≤
 * max_frames[i]; t ≥ 1. Any violation is PIPER_HIP_ERR_ARG with a message naming the field and the index. */
int piper_hip_prosody_check(const piper_hip_prosody* p);
/* Host-only: the rule above from w0 [t] on. p may be NULL (neutral); p->t ≠ t is PIPER_HIP_ERR_SHAPE. Fitting happens when p->fit ≠ 0,
 * cap > 0 and the total exceeds cap. frames_out [t]; *wanted (optional) = S. */
int piper_hip_prosody_frames(const piper_hip_prosody* p, const float* w0, int32_t t, int64_t cap, int32_t* frames_out, int64_t* wanted);
/* The prosody of the NEXT staging call on slot id `slot`: entry i is for item i; items past `n` have none. Staging calls are prepare,
 * prepare_batch, prepare_batch_bounded, stream_begin, stream_begin_batch, synthesize* (slot 0) and stream_pool_join* (the slot is the
 * work_slot). The staging call takes the assignment and clears it, whether or not it succeeds; the arrays are copied here, so the caller's
 * memory may go away at once. n = 0 clears the assignment; n outside 0 … 256 is PIPER_HIP_ERR_ARG; every entry passes the checks of
 * piper_hip_prosody_check here, on the host, with a message naming the entry, the field and the index.
 * Checked by the staging call (a refused call stages nothing): t different from the item's t = PIPER_HIP_ERR_SHAPE; on an item with
 * supplied durations any non-NULL length, min_frames or max_frames, or fit ≠ 0 = PIPER_HIP_ERR_ARG (the caller owns those durations; noise
 * alone applies — which is also all a voice with dp_present = 0 can take); fit ≠ 0 on a route without a frame bound (prepare,
 * prepare_batch, stream_begin*, the plain pool joins) = PIPER_HIP_ERR_ARG. */
int piper_hip_voice_slot_prosody(piper_hip_voice* v, int slot, const piper_hip_prosody* items, int n);
/* Where piper_hip_voice_durations answers (after prepare on the unbounded routes, after collect or the resolution of a bounded join on the
 * others): per item the frames the rule wanted before fitting (S) and whether fitting happened. piper_hip_voice_durations reports the
 * frames actually used, so the fitted ones. Either array may be NULL; at most max_items entries are written. */
int piper_hip_voice_prosody_report(const piper_hip_voice* v, int slot, int64_t* wanted_frames, int32_t* fitted, int max_items);

/* Debug taps ⇔ GraphExecutor.execute(maxNodeIndex:) returning intermediates (GraphExecutor.swift:75-152):
 * copy a named intermediate of the slot's last run to host. Names: "enc_out" [H,T], "m_p" [inter,T],
 * "logs_p" [inter,T], "z_p" [inter,F], "z" [inter,F], "dec_pre" [up_initial,F] — per batch item, compacted to the item's
 * true T / F (the bucket's padding is not copied), items back to back. With predicted durations, "logw" [1,T] of the
 * predictor is available through piper_hip_voice_predict_durations.
 * Generator taps (fp32 tensors [C_u, F · up_rates[0..u]] of stage u; a name exists only where the slot's schedule keeps that tensor
 * until the plan has run, any other name is PIPER_HIP_ERR_ARG):
 *   "dec.s{u}.up"            the stage's ConvTranspose output (every schedule, fp32 and bf16);
 *   "dec.s{u}.rb{j}.c{d}"    ResBlock j after dilation step d. bf16 and the fp32 per-conv schedule: the last three steps, except the
 *                            closing step of the last ResBlock where the MRF mean is folded into its epilogue. fp32 merged schedule:
 *                            the last two steps (ping-pong buffers); a step fused inside a pair launch has no tensor, so a ResBlock2
 *                            stage that runs as one pair launch keeps "c1" only;
 *   "dec.s{u}.mean_lrelu"    fp32 per-conv schedule: lrelu(MRF mean) as the next stage reads it (slope 0.1; last stage 0.01);
 *   "dec.s{u}.mean_act"      bf16, u < n_ups − 1: the bf16 image of lrelu(MRF mean, 0.1) as raw bits, [C_u / 8][len][8] bf16 words
 *                            (4 floats per position and channel group);
 *   "dec.mean"               bf16: the last stage's fp32 MRF mean;
 *   "audio"                  the waveform rows [1][F·hop] of the plan (every plan kind), items at F_b·hop samples.
 * Step selector. Name grammar:   ["predict:"] <tensor> ["@" <step name>]   |   ["predict:"] "@steps"
 *                                ["window:"] <tensor>                       |   "window:@steps"
 *   "<tensor>@<step name>"   the tensor as it stands right after the named step of the slot's schedule (step names: what
 *                            piper_hip_voice_profile reports). The call waits for the slot's stream, runs the schedule's launches eagerly
 *                            from the first step through the named one (the inputs staged by prepare are still in place), copies out as
 *                            above, then runs the remaining steps, so every buffer ends in the state a full run leaves. An unknown step
 *                            name is PIPER_HIP_ERR_ARG; a plan whose inputs do not persist (a generator-only stream window) and a bounded
 *                            slot that has not been collected yet are PIPER_HIP_ERR_UNSUPPORTED.
 *   Work buffers of the front half, reused layer after layer and therefore only meaningful with "@": "front.x", "front.x1", "front.att",
 *   "front.y" [hidden,T], "front.qkv" [3·hidden,T], "front.ff" [ffn,T], "front.stats" [2·inter,T] (m_p ; logs_p), "front.zp",
 *   "front.zflip" [inter,F] (the two buffers the halves of the flow's latent travel through), "front.h", "front.acts", "front.skip"
 *   [hidden,F]; of the duration predictor: "dp.a0", "dp.a1", "dp.cond" [hidden,T], "dp.hsp" [3·bins − 1,T], "dp.z" [2,T], "dp.logw" [1,T],
 *   "dp.dur" [1,T] (the int32 frames per id as raw bits).
 *   "predict:<tensor>[@<step>]"  addresses the encoder + duration-predictor plan the slot's last prepare ran, with the slot's true lengths:
 *                            the plan a bounded prepare left attached to the slot id, else the one prepare_batch ran if the cache still
 *                            holds it, else the first cached plan of the slot's form (with or without prosody), bucket T and batch size;
 *                            PIPER_HIP_ERR_ARG when none is cached. Another request that has run the plan since has left its own values.
 *   "@steps"                 the schedule's launch names in order, one per line, one character code per float.
 *   "window:<tensor>"        on a slot that holds a single stream, a group or a streaming pool: the tensor in the generator window plan of
 *                            the slot's LATEST stream step. Items are that step's generator rows 0 … NBg − 1 (one for a single stream),
 *                            each compacted to its window length Fc of that step; a row with Fc = 0 (finished, dropped, free, pad)
 *                            contributes nothing, so n_floats = Σ C · Fc_r · positions per frame. "window:audio" is the window's
 *                            waveform before the chunk is cut out of it. PIPER_HIP_ERR_ARG when no step has run on the slot since it was
 *                            prepared or opened, when the plan has been evicted from the cache, or when another stream has run the plan
 *                            since (its tensors are no longer this step's). "window:<tensor>@<step>" is PIPER_HIP_ERR_UNSUPPORTED, as
 *                            above; "window:@steps" lists the window plan's launches.
 *   "@routes"                one line per launch of the schedule: step name, tab, the route records of the step's most recent enqueue
 *                            (piper_hip_routes_arm; "; " between the records of one launch), one character code per float. Also
 *                            "predict:@routes" and "window:@routes". A captured graph replays the kernels it was captured with, so the
 *                            records hold for replays; a plan enqueued while the context was not armed reports nothing behind the tabs.
 *                            Reading them runs nothing and changes no tensor.
 * A voice with a speaker table (piper_hip_voice_attach_speakers) adds, per batch item at a fixed length: "spk.g" [gin], the mixed speaker
 * vector, and "spk.bias" [Ctot], the item's speaker row — a plan writes the rows it computes and leaves the others 0.0: the slot's plan the
 * flow and generator rows, "predict:spk.bias" the dp.pre rows. */
int piper_hip_voice_tap(piper_hip_voice* v, int slot, const char* name, float* host, size_t max_floats,
                        size_t* n_floats);
/* GPU milliseconds of the slot's last completed launch (hipEvent pair on the slot's stream) ⇔
 * RunTimings.gpuMs (GraphExecutor.swift:29-38). */
int piper_hip_voice_last_gpu_ms(piper_hip_voice* v, int slot, double* ms);
/* Stream of a slot (for external event timing / profiling). */
piper_hip_stream piper_hip_voice_slot_stream(piper_hip_voice* v, int slot);
/* Per-kernel timing of the slot's schedule: runs the schedule eagerly `iters` times with a hipEvent pair
 * around every launch and reports the median per launch; fills up to `max_entries` entries in schedule order. */
typedef struct {
  char name[48];
  double avg_us;     /* MEDIAN launch duration over the profiled passes (robust against a stalled pass) */
  double flops;      /* algorithmic FLOPs of this launch (SURVEY.md Appendix A recipe) */
  double bytes;      /* algorithmic bytes of this launch (same recipe) */
} piper_hip_kernel_stat;
int piper_hip_voice_profile(piper_hip_voice* v, int slot, int iters, piper_hip_kernel_stat* out, int max_entries,
                            int* n_entries);

/* Time a subset of the slot's schedule the way it runs in production: the launches whose name contains `name_filter`
 * ("" = all; "a|b|c" = the launches named exactly a, b or c) are captured into their own HIP graph and replayed `iters` times between two hipEvents on the slot's
 * stream. avg_launch_us = elapsed / (iters · n_launches) — kernel time plus the dispatch boundary, no per-kernel event
 * overhead; flops/bytes are the algorithmic totals of the subset (SURVEY.md Appendix A recipe). A filter that starts with "predict:"
 * times launches of the predictor plan the slot's last prepare ran instead (the plan piper_hip_voice_tap's "predict:" addresses;
 * PIPER_HIP_ERR_ARG when none is cached). */
int piper_hip_voice_time_subset(piper_hip_voice* v, int slot, const char* name_filter, int iters, double* avg_launch_us,
                                int* n_launches, double* flops, double* bytes);

/* ---- multi-GPU: the path's one collective --------------------------------------------------------------------
 * Utterances are independent, so N GPUs are N replicas of the voice, one process per GPU; the only exchange is the one-shot
 * broadcast of the voice blob from the rank that parsed the .onnx (PiperMetalRuntime.init(modelPath:) does that parse once per
 * process, PiperMetalRuntime.swift:37-41 → ONNXModel.init). These wrap rccl.h so that a host without torch.distributed (the Swift CLI, a C++
 * server) can do it: rank 0 calls comm_unique_id and hands the 128 bytes to the other ranks by any side channel (a file, a
 * socket, an environment variable), every rank calls comm_create (collective), uploads / allocates n_floats on its GPU,
 * calls comm_broadcast_f32 (collective, in place, returns when the data is there) and piper_hip_voice_create(on_device = 1).
 * comm_max_f64 / comm_barrier are what a bench needs for the "MAX over ranks between two barriers" timing rule.
 * RCCL is bound at run time: without librccl.so.1 these return PIPER_HIP_ERR_UNAVAILABLE and the rest of the library works. */
#define PIPER_HIP_COMM_ID_BYTES 128
int piper_hip_comm_unique_id(void* id_out /* PIPER_HIP_COMM_ID_BYTES */);
int piper_hip_comm_create(piper_hip_ctx* ctx, const void* id, int rank, int world, piper_hip_comm** out);
void piper_hip_comm_destroy(piper_hip_comm* c);
int piper_hip_comm_rank(const piper_hip_comm* c);
int piper_hip_comm_world(const piper_hip_comm* c); /* ncclCommCount: what the communicator says */
int piper_hip_comm_broadcast_f32(piper_hip_comm* c, float* device_buf, size_t count, int root);
int piper_hip_comm_max_f64(piper_hip_comm* c, double* value); /* in/out: all-reduce MAX of one double */
int piper_hip_comm_barrier(piper_hip_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* PIPER_HIP_H */
