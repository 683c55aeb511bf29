// flow_fold.hip — multiplies the linear tail of a reverse flow coupling out, once per voice, into the matrix conv_k1_tail_kernel reads.
//
// Graph per ResidualCouplingLayer (reverse), behind the last gated conv of its WaveNet:
//   skip  = skip_acc + W_rs·acts + b_rs ;  m = W_post·skip + b_post ;  x1new = x1 − m ;  Flip ;  h' = W_pre'·x0' + b_pre'   (x0' = Flip(x1new))
// With A1 = W_post·W_rs, c1 = W_post·b_rs + b_post and P = W_pre' with the Flip applied to its columns (P[o][r] = W_pre'[o][half − 1 − r]):
//   x1new = x1 − (A1·acts + W_post·skip_acc + c1)
//   h'    = P·x1 − (P·A1)·acts − (P·W_post)·skip_acc + (b_pre' − P·c1)
// Products in float64, rounded to fp32 once. The identity on x1 stays in the launch's epilogue (res − v): the x1new rows carry zeros
// over the x1 segment. Column order of the x1 segment: ascending PHYSICAL rows of z (x1 row r lives in channel base + sign·r), so the
// kernel's loads stay base + lane + immediate whatever the coupling's channel map is.
#include "conv.h"

namespace ph {
namespace {

constexpr int kFoldBlock = 256;

// A1 [half][H] and c1 [half] (column H of the same row)
__global__ __launch_bounds__(kFoldBlock) void fold_a1_kernel(const float* __restrict__ w_post, const float* __restrict__ b_post, const float* __restrict__ w_rs,
                                                             const float* __restrict__ b_rs, double* __restrict__ a1, int H, int half) {
  const int idx = blockIdx.x * kFoldBlock + threadIdx.x;
  if (idx >= half * (H + 1)) return;
  const int r = idx / (H + 1), c = idx % (H + 1);
  double acc = 0.0;
  if (c < H) {
    for (int k = 0; k < H; k++) acc += (double)w_post[r * H + k] * (double)w_rs[k * H + c];
  } else {
    for (int k = 0; k < H; k++) acc += (double)w_post[r * H + k] * (double)(b_rs ? b_rs[k] : 0.0f);
    acc += (double)(b_post ? b_post[r] : 0.0f);
  }
  a1[idx] = acc;
}

// PW = P·W_post [H][H]
__global__ __launch_bounds__(kFoldBlock) void fold_pw_kernel(const float* __restrict__ w_pre, const float* __restrict__ w_post, double* __restrict__ pw, int H, int half) {
  const int idx = blockIdx.x * kFoldBlock + threadIdx.x;
  if (idx >= H * H) return;
  const int o = idx / H, k = idx % H;
  double acc = 0.0;
  for (int r = 0; r < half; r++) acc += (double)w_pre[o * half + (half - 1 - r)] * (double)w_post[r * H + k];
  pw[idx] = acc;
}

// The fragment image [row tile][step][64] (lane = 16·k + i: row i of the tile, channel k of the step's quad) and the bias. Steps of wave
// w: its NX quads of x1, then NS of skip_acc, then NA of acts — the order conv_k1_tail_kernel loads and multiplies them in.
__global__ __launch_bounds__(kFoldBlock) void fold_image_kernel(const float* __restrict__ w_rs, const float* __restrict__ w_post, const float* __restrict__ w_pre,
                                                                const float* __restrict__ b_pre, const double* __restrict__ a1, const double* __restrict__ pw,
                                                                float* __restrict__ image, float* __restrict__ bias, int H, int half, int seam, int x1_sign) {
  const int rows = half + (seam ? H : 0);
  const int NX = seam ? half / 32 : 0, NS = H / 32, NA = H / 32, NT = NX + NS + NA, nsteps = 8 * NT;
  const int idx = blockIdx.x * kFoldBlock + threadIdx.x;
  if (idx < rows) {  // bias: c1 ; b_pre' − P·c1
    double b;
    if (idx < half) b = a1[idx * (H + 1) + H];
    else {
      const int o = idx - half;
      b = (double)(b_pre ? b_pre[o] : 0.0f);
      for (int r = 0; r < half; r++) b -= (double)w_pre[o * half + (half - 1 - r)] * a1[r * (H + 1) + H];
    }
    bias[idx] = (float)b;
  }
  if (idx >= (rows / 16) * nsteps * 64) return;
  const int lane = idx & 63, step = (idx >> 6) % nsteps, mt = (idx >> 6) / nsteps;
  const int row = 16 * mt + (lane & 15), kq = lane >> 4;
  const int wave = step / NT, i = step % NT;
  double v;
  if (i < NX) {  // x1 by ascending physical row p ↔ x1 row r
    const int p = 4 * (wave * NX + i) + kq;
    const int r = x1_sign > 0 ? p : half - 1 - p;
    v = row < half ? 0.0 : (double)w_pre[(row - half) * half + (half - 1 - r)];
  } else if (i < NX + NS) {  // skip_acc
    const int c = 4 * (wave * NS + i - NX) + kq;
    v = row < half ? (double)w_post[row * H + c] : -pw[(row - half) * H + c];
  } else {  // acts
    const int c = 4 * (wave * NA + i - NX - NS) + kq;
    if (row < half) v = a1[row * (H + 1) + c];
    else {
      const int o = row - half;
      v = 0.0;
      for (int k = 0; k < H; k++) v -= pw[o * H + k] * (double)w_rs[k * H + c];
    }
  }
  image[idx] = (float)v;
}

}  // namespace

int fold_flow_tail(hipStream_t s, const float* w_rs, const float* b_rs, const float* w_post, const float* b_post, const float* w_pre, const float* b_pre,
                   int H, int half, int x1_sign, double* scratch, float* image, float* bias) {
  const int seam = w_pre != nullptr;
  if (H % 32 || half % 32 || !w_rs || !w_post || !scratch || !image || !bias) PH_FAIL(PIPER_HIP_ERR_ARG, "fold_flow_tail: H=%d half=%d", H, half);
  double* a1 = scratch;
  double* pw = scratch + (size_t)half * (H + 1);
  hipLaunchKernelGGL(fold_a1_kernel, dim3((unsigned)ceil_div(half * (H + 1), kFoldBlock)), dim3(kFoldBlock), 0, s, w_post, b_post, w_rs, b_rs, a1, H, half);
  if (seam) hipLaunchKernelGGL(fold_pw_kernel, dim3((unsigned)ceil_div(H * H, kFoldBlock)), dim3(kFoldBlock), 0, s, w_pre, w_post, pw, H, half);
  const size_t n = flow_tail_image_floats(H, half, seam);
  hipLaunchKernelGGL(fold_image_kernel, dim3((unsigned)ceil_div((int64_t)n, kFoldBlock)), dim3(kFoldBlock), 0, s, w_rs, w_post, w_pre, b_pre, a1, pw, image, bias, H,
                     half, seam, x1_sign);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PH_FAIL(PIPER_HIP_ERR_LAUNCH, "fold_flow_tail launch failed: %s", hipGetErrorString(e));
  return PIPER_HIP_OK;
}

}  // namespace ph
namespace ph { namespace { PH_WARM(flow_fold, fold_a1_kernel); } }
