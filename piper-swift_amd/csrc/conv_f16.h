// conv_f16.h — internal interface of the fp16-operand Conv1d / ConvTranspose1d kernel (conv_f16.hip).
//
// PIPER_HIP_PRECISION_F16: the layouts, the fp32 epilogue and the MFMA count of conv_bf16.h on v_mfma_f32_32x32x16_f16 — 11 significand
// bits per operand against bf16's 8. The numeric contract (include/piper_hip.h states it for hosts):
//   activations  x' = fp16_rne(clamp(x, −65504, 65504)): one v_med3_f32 before a round-to-nearest-even conversion, so that an outlier
//                costs a bounded error and never an inf. The image is the C8 geometry of conv_bf16.h with fp16 elements.
//   weights      one power-of-two scale per output channel: m = max|w[co,·,·]| (ConvTranspose: over all C_in and K),
//                e = 14 − ⌊log₂ m⌋ (0 for a zero row), w' = fp16_rne(w · 2^e), max|w'| ∈ [2¹⁴, 2¹⁵). The scaling is exact and keeps every
//                weight that matters out of fp16's subnormal range. The fragment image is conv_bf16.h's (same element counts, same
//                readable pad), a float scale[Cout] = 2^−e travels with it (ConvTranspose: indexed by co, not by the (phase, co) row).
//   epilogue     fp32 accumulator · 2^−e (exact), then bias, residual and MRF mean in fp32 where conv_bf16 adds them.
//   bound        per output, against the unrounded operands: (2·2⁻¹¹ + 2⁻²²)·Σ|w||x| plus fp32 accumulation — with no clamped element
//                and activations that are zero or ≥ 2⁻¹⁴ in magnitude (whether the MFMA honours fp16 subnormal inputs is not relied on).
#pragma once
#include "conv_bf16x3.h"  // conv_bf16.h and conv_reach / convt_reach

namespace ph {

struct ConvF16Args : ConvBf16Args {  // x / act: fp16 C8 images, w: the fp16 fragment image
  const float* wscale = nullptr;     // [Cout] 2^−e per output channel
};

// w fp32 [Cout][Cin][K] → fragment image of packed_conv_bf16_elems(…) fp16 elements + scale[Cout] (a row-max reduction, then a scaled round)
int pack_conv_weights_f16(hipStream_t s, const float* w, int Cout, int Cin, int K, uint16_t* packed, float* scale);
// w fp32 [Cin][Cout][K] → fragment image with rows (phase, co), packed_convt_bf16_elems(…) elements + scale[Cout]
int pack_convt_weights_f16(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, int pad, uint16_t* packed, float* scale);
// pack_act_c8 / pack_mean3_c8 (conv_bf16.h) onto an fp16 image: the two places a schedule enters the image from fp32
int pack_act_c8_f16(hipStream_t s, const float* x, int N, int C, int L, float alpha, uint16_t* act, int64_t row = 0, const int* len_ptr = nullptr);
int pack_mean3_c8_f16(hipStream_t s, const float* a, const float* b, const float* c, int N, int C, int L, float alpha, uint16_t* act, int64_t row,
                      const int* len_ptr, int len_mul);

// The geometry is conv_bf16_eligible / convt_bf16_eligible; on top of it the smallest tile's input window must fit LDS.
// row_tiles = 32-row tiles of the GEMM (ConvTranspose: of one phase, Cout / 32); reach = window positions beyond the tile's columns.
bool conv_f16_fits(int row_tiles, int Cin, int reach);

int launch_conv_f16(piper_hip_ctx* ctx, hipStream_t s, const ConvF16Args& a);
int launch_conv_f16_multi(piper_hip_ctx* ctx, hipStream_t s, const ConvF16Args* convs, int count);  // the kBf16Multi contract

// ---- rb_pair_f16.hip: two chained ResBlock convs in one kernel on the fp16 pipe (C ∈ {32, 64, 128}, odd kernels, both reaches ≤ kC8Halo,
// L % 4 == 0, the window within 160 KB of LDS). RbPairBf16Args::form as in rb_pair_bf16x3.hip:
//   1: a ResBlock1 pair                 y = x + conv_b(lrelu(conv_a(lrelu x) + ba)) + bb
//   2: ResBlock2 steps (i, i+1)         x1 = x + conv_a(lrelu x) + ba ;  y = x1 + conv_b(lrelu x1) + bb      (x1 stays fp32)
// launch_rb_pair_bf16_multi's contract; wa / wb are fp16 fragment images, `act` an fp16 C8 image. Column tiles are 256 − 2·(conv b's reach)
// outputs wide.
struct RbPairF16Args : RbPairBf16Args {
  const float* sa = nullptr;  // [C] 2^−e per output channel of conv a
  const float* sb = nullptr;  // … of conv b
};
bool rb_pair_f16_eligible(int C, int Ka, int dila, int Kb, int dilb, int L, int form);
int launch_rb_pair_f16_multi(piper_hip_ctx* ctx, hipStream_t s, const RbPairF16Args* pairs, int count);  // ≤ 3 pairs, same N, C, L, form

}  // namespace ph
