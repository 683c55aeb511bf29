// conv_bf16x3.h — internal interface of the split-bf16 Conv1d / ConvTranspose1d kernel (conv_bf16x3.hip).
//
// PIPER_HIP_PRECISION_BF16X3: every fp32 operand a is carried as two bf16 values, a_hi = bf16(a) and a_lo = bf16(a − a_hi) (the
// residual is exact in fp32), and the contraction is  W_hi·X_hi + W_hi·X_lo + W_lo·X_hi  — three bf16 MFMAs into one fp32
// accumulator; the lo·lo term (≤ 2⁻¹⁶ relative) is dropped. Everything that conv_bf16.h keeps in fp32 stays fp32.
//
// Operand images are PLANAR: an image of conv_bf16.h ("hi"), then a second image of exactly the same layout ("lo").
//   activations  two C8 planes; the lo plane starts N · (C/8) · row · 8 elements behind the hi plane (= c8_elems(N, C, L) when
//                row = c8_row_len(L)); both are zero outside [0, L)
//   weights      two fragment images, each with its own kBf16WeightPad; the lo image starts packed_*_bf16_elems(…) elements
//                behind the hi image
// The argument struct is ConvBf16Args: x / act / w point at the hi plane, the kernel derives the lo plane from the shape.
#pragma once
#include "conv_bf16.h"

namespace ph {

inline int64_t c8x2_elems(int64_t N, int64_t C, int64_t L) { return 2 * c8_elems(N, C, L); }  // bf16 elements of both planes

// w fp32 → both fragment images, 2 · packed_conv_bf16_elems / packed_convt_bf16_elems elements (hi: round to nearest even; lo: the
// rounded residual)
int pack_conv_weights_bf16x3(hipStream_t s, const float* w, int Cout, int Cin, int K, uint16_t* packed);
int pack_convt_weights_bf16x3(hipStream_t s, const float* w, int Cin, int Cout, int K, int stride, int pad, uint16_t* packed);
// fp32 [N][C][L] → both planes of lrelu(x, alpha) (interior only: the image must have been zeroed once); row 0 ⇒ c8_row_len(L)
int pack_act_c8x2(hipStream_t s, const float* x, int N, int C, int L, float alpha, uint16_t* act, int64_t row = 0, const int* len_ptr = nullptr);

// The geometry is conv_bf16_eligible / convt_bf16_eligible; on top of it both planes of the smallest tile's input window must fit LDS.
// row_tiles = 32-row tiles of the GEMM (ConvTranspose: of one phase, Cout / 32); reach = window positions beyond the tile's columns.
bool conv_bf16x3_fits(int row_tiles, int Cin, int reach);
inline int conv_reach(int K, int dil) { return (K - 1) * dil; }
inline int convt_reach(int K, int stride, int pad) { return (stride - 1 + pad) / stride + K / stride - 1; }

int launch_conv_bf16x3(piper_hip_ctx* ctx, hipStream_t s, const ConvBf16Args& a);
int launch_conv_bf16x3_multi(piper_hip_ctx* ctx, hipStream_t s, const ConvBf16Args* convs, int count);  // the kBf16Multi contract

// C8 planes of lrelu(((a + b) + c) / 3, alpha): pack_mean3_c8 on planar images (true length of item n = len_ptr[n]·len_mul)
int pack_mean3_c8x2(hipStream_t s, const float* a, const float* b, const float* c, int N, int C, int L, float alpha, uint16_t* act, int64_t row,
                    const int* len_ptr, int len_mul);

// ---- rb_pair_bf16x3.hip: two chained ResBlock convs in one kernel on the fp32 stream, C ∈ {32, 64}, L % 4 == 0, odd kernels, any
// dilations (reach ≤ 64 each side); RbPairBf16Args with wa / wb = the planar fragment images above and `form` = 1 (ResBlock1 pair) or
// 2 (ResBlock2 steps i, i+1); `act` is a planar image. The launch refuses (UNSUPPORTED) whatever rb_pair_bf16x3_eligible refuses.
bool rb_pair_bf16x3_eligible(int C, int Ka, int dila, int Kb, int dilb, int L, int form);
int launch_rb_pair_bf16x3_multi(piper_hip_ctx* ctx, hipStream_t s, const RbPairBf16Args* pairs, int count);  // ≤ 3 pairs, same N, C, L, form

}  // namespace ph
