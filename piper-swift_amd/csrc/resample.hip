// resample.hip — fp32 waveform at the voice's rate → 8–48 kHz, fp32 or 16-bit PCM, on the device (include/piper_hip.h "Output rate").
//
// The conversion is a contract, tested bit for bit against a numpy restatement (tests/resample_ref.py):
//   ratio     g = gcd(in, out), L = out / g, M = in / g; output j sits at input position j·M / L.
//   filter    Kaiser-windowed sinc, P = 2·⌈24·max(L, M) / L⌉ taps per phase, cutoff fc = 0.93·min(1, L / M), β = 9; designed in double,
//             every phase divided by its own sum, rounded once to fp32: the table c[L][P] (rs_design below).
//   sample    u = j·M (64-bit), n = u div L, p = u mod L; y[j] = Σ_t c[p][t] · x[n − (P/2 − 1) + t], x = 0 outside [0, N), accumulated in
//             fp32 in ascending t from 0.0f, each product rounded, then each sum (no FMA: the library is built with -ffp-contract=off).
//   to int16  exactly pcm16.hip's conversion of y (gain; peak mode with the peak of the fp32 waveform at the voice's rate).
//
// A block is one row by a tile of consecutive outputs: the tile's input span (tile · M / L + P samples) is staged into LDS once, by 16-byte
// loads where the source is aligned, zeros (outside the item) and the stream's history (before the chunk) resolved while staging; every
// thread then runs the P-term sums of its outputs out of LDS, two adjacent outputs per thread so that int16 leaves in 4-byte stores — four
// where the sink is one G.711 byte per sample (include/piper_hip.h "G.711 output"), which then leave as one dword as well.
// Coefficients come from the table in global memory (at most 121 KB, cache-resident), through LDS when L ≤ 3. Nothing is atomic or
// order-dependent. The destination may be a page-locked host buffer seen through its device mapping.
#include "resample.h"

#include <algorithm>
#include <cmath>
#include <memory>

#include "pcm16.h"

namespace ph {
namespace {

constexpr int kRsTile = 1024;       // outputs per tile: two pairs per thread (int16, fp32), one quad per thread (G.711 bytes)
constexpr int kRsTileMin = 64;      // rs_geometry halves the tile down to this at most; a thread's pair or quad never straddles a tile
static_assert(kRsTile % 4 == 0 && kRsTileMin % 4 == 0 && kRsTile % kRsTileMin == 0 && ((kRsTile / kRsTileMin) & (kRsTile / kRsTileMin - 1)) == 0,
              "every tile rs_geometry can choose is a multiple of 4: a byte quad is one aligned dword inside one tile");
constexpr int kRsLdsPhases = 3;     // the table goes through LDS up to this many phases
constexpr size_t kRsLdsMax = 64 << 10;  // LDS of a block: the tile is halved before this is exceeded (two blocks per CU hold 80 KB each)

// What a row's samples are made of: sample g of the item is x[g − s] for g in [s, e), hist[g − (s − kRsHist)] for g in [s − kRsHist, s)
// when hist is given (a stream step past the item's first), and 0 everywhere else.
struct RsSrc {
  const float* x;
  const float* hist;
  int64_t s, e;
  int64_t j0, count;  // outputs [j0, j0 + count)
};

__device__ __forceinline__ float rs_at(const RsSrc& r, int64_t g) {
  if (g < 0 || g >= r.e) return 0.0f;
  if (g >= r.s) return r.x[g - r.s];
  const int64_t h = g - r.s + kRsHist;
  return (r.hist && h >= 0) ? r.hist[h] : 0.0f;
}

// LDS floats of a block: the table when it is staged, then the tile's input span
__host__ __device__ inline int rs_coef_floats(int L, int P) { return L <= kRsLdsPhases ? (L * P + 3) & ~3 : 0; }

// The row's outputs → dst[0 … count). E = bytes of an output: 4 = fp32 y, 2 = int16 through `c`, 1 = the G.711 byte (c.law) of that int16.
// CL: the table has been staged into LDS.
// Outputs are numbered v = (j − j0) + lead, lead = the elements between dst and the 4-byte-aligned address at or below it (int16: 0 or 1,
// bytes: dst & 3), so that a v which is a multiple of W = 4 / E (fp32: 2) is a 4-byte-aligned address: a thread owns the W outputs
// (v … v + W − 1) and stores them as one word where all are outputs of this row, one by one at the row's head and tail — the bytes beside
// them belong to another row of a packed output, which another block writes at the same time.
template <int E, bool CL>
__device__ __forceinline__ void rs_row(const RsSrc r, const RsFilter f, const PcmCvt c, void* dst, int tile, float* lds) {
  constexpr bool F32 = E == 4;
  constexpr int W = E == 1 ? 4 : 2;
  if (r.count <= 0) return;  // (the whole block: an empty item)
  const int tid = threadIdx.x, half = f.P >> 1;
  float* xs = lds + rs_coef_floats(f.L, f.P);
  if (CL)
    for (int i = tid; i < f.L * f.P; i += 256) lds[i] = f.taps[i];  // (the first tile's barrier covers it)
  const int lead = F32 ? 0 : E == 2 ? (int)(((uintptr_t)dst >> 1) & 1) : (int)((uintptr_t)dst & 3);
  const int64_t vend = r.count + lead;
  for (int64_t v0 = (int64_t)blockIdx.x * tile; v0 < vend; v0 += (int64_t)gridDim.x * tile) {
    const int64_t ja = r.j0 + (v0 > lead ? v0 - lead : 0), jb = r.j0 + (v0 + tile < vend ? v0 + tile : vend) - lead;  // the tile's outputs [ja, jb)
    const int64_t ua = ja * f.M, na = ua / f.L;
    const int pa = (int)(ua - na * f.L);
    const int64_t nb = ((jb - 1) * f.M) / f.L;
    // the samples the tile reads are [na − (half − 1), nb + half]; the staged span starts up to 3 earlier, where x is 16-byte aligned
    int64_t g0 = na - (half - 1);
    g0 -= ((int64_t)((uintptr_t)r.x >> 2) + (g0 - r.s)) & 3;
    const int span = (int)(nb + half - g0) + 1;
    __syncthreads();  // the previous tile has been read
    for (int q = tid; q < (span + 3) >> 2; q += 256) {
      const int64_t g = g0 + 4 * q;
      float4 v;
      if (g >= r.s && g + 4 <= r.e) {
        v = *(const float4*)(r.x + (g - r.s));
      } else {
        v.x = rs_at(r, g); v.y = rs_at(r, g + 1); v.z = rs_at(r, g + 2); v.w = rs_at(r, g + 3);
      }
      *(float4*)(xs + 4 * q) = v;
    }
    __syncthreads();
    for (int q = tid; q < tile / W; q += 256) {
      const int64_t v = v0 + W * q;
      float y[W] = {};
      bool ok[W];
#pragma unroll
      for (int k = 0; k < W; k++) {
        ok[k] = v + k >= lead && v + k < vend;
        if (!ok[k]) continue;
        const int64_t j = r.j0 + v + k - lead;
        const int urel = (int)(j - ja) * f.M + pa;  // j·M − na·L: below tile · M + L
        const int dn = urel / f.L, p = urel - dn * f.L;
        const float* xp = xs + (int)(na - (half - 1) - g0) + dn;
        const float* cp = (CL ? lds : f.taps) + p * f.P;
        float acc = 0.0f;
        for (int t = 0; t < f.P; t += 2) {  // P is even; ascending t, product and sum rounded separately
          const float2 cc = *(const float2*)(cp + t);
          acc = acc + cc.x * xp[t];
          acc = acc + cc.y * xp[t + 1];
        }
        y[k] = acc;
      }
      const int64_t o = v - lead;  // index of the thread's first sample in dst
      if (F32) {
        if (ok[0]) ((float*)dst)[o] = y[0];
        if (ok[1]) ((float*)dst)[o + 1] = y[1];
      } else if (E == 2) {
        if (ok[0] && ok[1]) {
          *(unsigned*)((int16_t*)dst + o) = pcm_pair(y[0], y[1], c);
        } else {
          if (ok[0]) ((int16_t*)dst)[o] = (int16_t)pcm_cvt(y[0], c);
          if (ok[1]) ((int16_t*)dst)[o + 1] = (int16_t)pcm_cvt(y[1], c);
        }
      } else if (ok[0] && ok[W - 1]) {  // (the outputs are a range: first and last inside means all inside)
        *(unsigned*)((uint8_t*)dst + o) = g711_quad(y[0], y[1], y[W / 2], y[W - 1], c);
      } else {
#pragma unroll
        for (int k = 0; k < W; k++)
          if (ok[k]) ((uint8_t*)dst)[o + k] = (uint8_t)g711_cvt(pcm_cvt(y[k], c), c.law);
      }
    }
  }
}

__device__ __forceinline__ int64_t rs_count_dev(int64_t n, const RsFilter f) { return (n * f.L + f.M - 1) / f.M; }

// Plan audio [NB][row] → the items back to back at J(len·hop). blockIdx.y = item; its offset is the sum of the J before it (NB ≤ 256 = one
// per thread), so plain, ragged and bounded slots — whose lengths only the device knows — take the same launch. lensF == nullptr: one
// item of n_flat samples (the per-op entry points).
template <int E, bool CL>
__global__ __launch_bounds__(256) void resample_items_kernel(const float* __restrict__ audio, int64_t row, const int* __restrict__ lensF, int F,
                                                             int hop, int64_t n_flat, const RsFilter f, float gain,
                                                             const float* __restrict__ peaks, float* __restrict__ peaks_host, void* out,
                                                             int tile, int law) {
  extern __shared__ float4 rs_lds[];
  __shared__ long long part[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  long long before = (lensF && tid < b) ? rs_count_dev((int64_t)clamp_len(lensF[tid], F) * hop, f) : 0;
  for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off);
  if ((tid & 63) == 0) part[tid >> 6] = before;
  __syncthreads();
  const int64_t at = part[0] + part[1] + part[2] + part[3];
  const int64_t n = lensF ? (int64_t)clamp_len(lensF[b], F) * hop : n_flat;
  PcmCvt c;
  c.gain = gain; c.scale = 1.0f; c.norm = 0; c.law = law;
  if (peaks) {
    const float peak = peaks[b];
    c.scale = (float)(32767.0 / (double)fmaxf(0.01f, peak));
    c.norm = 1;
    if (peaks_host && blockIdx.x == 0 && tid == 0) peaks_host[b] = peak;
  }
  RsSrc r;
  r.x = audio + (int64_t)b * row; r.hist = nullptr; r.s = 0; r.e = n; r.j0 = 0; r.count = rs_count_dev(n, f);
  rs_row<E, CL>(r, f, c, (char*)out + at * E, tile, (float*)rs_lds);
}

// One stream step: row blockIdx.y's chunk sits behind the halo skip of its plan audio, what came before it in the row's history. The
// row's first block also leaves the last kRsHist samples of (history ++ chunk) as the next step's history, in the other buffer.
template <int E, bool CL>
__global__ __launch_bounds__(256) void resample_step_kernel(const float* __restrict__ audio, int64_t row, const RsStepRow* __restrict__ desc,
                                                            const float* __restrict__ hist_old, float* __restrict__ hist_new, const RsFilter f,
                                                            float gain, void* __restrict__ out, int tile, int law) {
  extern __shared__ float4 rs_lds[];
  const RsStepRow d = desc[blockIdx.y];
  // A row without a chunk leaves no history behind although the buffers change roles for the whole stream. That is sound because no row
  // rests for a step and then goes on: a finished or dropped row never resumes, and the session that takes a free row starts at s = 0,
  // where no history is read. A stream that could pause a row would have to carry its history over here.
  if (d.n_in == 0) return;
  RsSrc r;
  r.x = audio + (int64_t)blockIdx.y * row + d.skip;
  r.hist = d.s > 0 ? hist_old + (int64_t)blockIdx.y * kRsHist : nullptr;  // a row's first step sees nothing of the row's previous occupant
  r.s = d.s; r.e = d.s + d.n_in; r.j0 = d.j0; r.count = d.count;
  if (blockIdx.x == 0 && threadIdx.x < kRsHist) {
    const int i = threadIdx.x, at = d.n_in - kRsHist + i;
    hist_new[(int64_t)blockIdx.y * kRsHist + i] = at >= 0 ? r.x[at] : (r.hist ? r.hist[i + d.n_in] : 0.0f);
  }
  PcmCvt c;
  c.gain = gain; c.scale = 1.0f; c.norm = 0; c.law = law;
  rs_row<E, CL>(r, f, c, (char*)out + (int64_t)d.off * E, tile, (float*)rs_lds);
}

// One step of a mixed-format stream (include/piper_hip.h "Mixed formats"): row blockIdx.y brings its own filter, sink and gain in its
// descriptor, and the block runs the body the uniform launch of that format runs — rs_row<E, false> behind a filter (the table read from
// global memory at every L), pcm_span at the voice's own rate. Every branch below is formed from the descriptor, which the whole block
// reads at one address: no wave diverges on the sink. Rows are packed at 4-byte-aligned BYTE offsets, so rs_row's lead is 0 and pcm_span's
// head is empty; neither is special-cased. History as in resample_step_kernel, for the rows that have a filter; its soundness argument
// holds unchanged, because a row keeps its format from its first step to its last.
__global__ __launch_bounds__(256) void mixed_step_kernel(const float* __restrict__ audio, int64_t row, const MixStepRow* __restrict__ desc,
                                                         const float* __restrict__ hist_old, float* __restrict__ hist_new,
                                                         void* __restrict__ out) {
  extern __shared__ float4 rs_lds[];
  const MixStepRow d = desc[blockIdx.y];
  if (d.n_in == 0) return;
  const float* x = audio + (int64_t)blockIdx.y * row + d.skip;
  void* dst = (char*)out + d.off;
  PcmCvt c;
  c.gain = d.gain; c.scale = 1.0f; c.norm = 0; c.law = d.law;
  if (d.L == 0) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
    if (d.elem == 4) pcm_span(x, (float*)dst, (int64_t)d.n_in, tid, nth, c);
    else if (d.elem == 2) pcm_span(x, (int16_t*)dst, (int64_t)d.n_in, tid, nth, c);
    else pcm_span(x, (uint8_t*)dst, (int64_t)d.n_in, tid, nth, c);
    return;
  }
  RsSrc r;
  r.x = x;
  r.hist = d.s > 0 ? hist_old + (int64_t)blockIdx.y * kRsHist : nullptr;  // a row's first step sees nothing of the row's previous occupant
  r.s = d.s; r.e = d.s + d.n_in; r.j0 = d.j0; r.count = d.count;
  if (blockIdx.x == 0 && threadIdx.x < kRsHist) {
    const int i = threadIdx.x, at = d.n_in - kRsHist + i;
    hist_new[(int64_t)blockIdx.y * kRsHist + i] = at >= 0 ? r.x[at] : (r.hist ? r.hist[i + d.n_in] : 0.0f);
  }
  const RsFilter f{d.taps, d.L, d.M, d.P};
  if (d.elem == 4) rs_row<4, false>(r, f, c, dst, d.tile, (float*)rs_lds);
  else if (d.elem == 2) rs_row<2, false>(r, f, c, dst, d.tile, (float*)rs_lds);
  else rs_row<1, false>(r, f, c, dst, d.tile, (float*)rs_lds);
}

// The tile and the dynamic LDS of a launch with filter f
void rs_geometry(const RsFilter& f, int* tile, size_t* lds_bytes) {
  int t = kRsTile;
  for (;;) {
    const size_t floats = (size_t)rs_coef_floats(f.L, f.P) + (size_t)ceil_div((int64_t)t * f.M, f.L) + f.P + 8;
    *lds_bytes = ((floats + 3) & ~(size_t)3) * sizeof(float);
    if (*lds_bytes <= kRsLdsMax || t <= kRsTileMin) break;
    t >>= 1;
  }
  *tile = t;
}

// ---- filter design (host, double)

double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

const int kRates[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000};

int gcd_int(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

}  // namespace

int rs_design(int in_rate, int out_rate, const RsDesign** out) {
  if (in_rate <= 0 || out_rate <= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "resample: rates %d -> %d", in_rate, out_rate);
  if (std::find(std::begin(kRates), std::end(kRates), out_rate) == std::end(kRates))
    PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "resample: output rate %d (supported: 8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)", out_rate);
  const int g = gcd_int(in_rate, out_rate), L = out_rate / g, M = in_rate / g;
  const int64_t P = 2 * ceil_div((int64_t)24 * std::max(L, M), L);
  if (L > 640 || P > 256) PH_FAIL(PIPER_HIP_ERR_UNSUPPORTED, "resample: %d -> %d needs %d phases of %lld taps (at most 640 of 256)", in_rate, out_rate, L, (long long)P);
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::unique_ptr<RsDesign>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto& slot = cache[{in_rate, out_rate}];
  if (!slot) {
    std::unique_ptr<RsDesign> d(new RsDesign());
    d->in = in_rate; d->out = out_rate; d->L = L; d->M = M; d->P = (int)P;
    d->taps.resize((size_t)L * P);
    const double pi = 3.14159265358979323846, fc = 0.93 * std::min(1.0, (double)L / (double)M), half = (double)(P / 2), i0b = bessel_i0(9.0);
    std::vector<double> c((size_t)P);
    for (int p = 0; p < L; p++) {
      double sum = 0.0;
      for (int t = 0; t < P; t++) {
        const double tau = (double)(t - ((int)P / 2 - 1)) - (double)p / (double)L;
        const double a = fc * tau;
        const double h = fc * (a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a));
        const double r = tau / half;
        const double w = std::fabs(tau) < half ? bessel_i0(9.0 * std::sqrt(1.0 - r * r)) / i0b : 0.0;
        c[t] = h * w;
        sum += c[t];
      }
      for (int t = 0; t < P; t++) d->taps[(size_t)p * P + t] = (float)(c[t] / sum);
    }
    slot = std::move(d);
  }
  *out = slot.get();
  return PIPER_HIP_OK;
}

hipError_t launch_resample_items(hipStream_t q, const float* audio, int64_t row, const int* lensF, int F, int hop, int NB, int64_t n_flat,
                                 const RsFilter& f, float gain, const float* peaks, float* peaks_host, void* out, int elem, int law) {
  if (NB < 1 || NB > 256 || (!lensF && NB != 1)) return hipErrorInvalidValue;  // the offset of an item is summed by one block of 256 threads
  int tile;
  size_t lds;
  rs_geometry(f, &tile, &lds);
  const int64_t n_max = lensF ? (int64_t)F * hop : n_flat;
  const int64_t outs = ceil_div(n_max * f.L, f.M) + (elem == 1 ? 3 : 1);  // (a destination that is not 4-byte aligned shifts the tiles: by one int16, by up to three bytes)
  const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(outs, tile), 1), 1024), NB);
  const bool cl = f.L <= kRsLdsPhases;
  if (elem != 4 && elem != 2 && elem != 1) return hipErrorInvalidValue;
#define RS_ITEMS(E, CL) \
  hipLaunchKernelGGL((resample_items_kernel<E, CL>), grid, dim3(256), lds, q, audio, row, lensF, F, hop, n_flat, f, gain, peaks, peaks_host, out, tile, law)
  if (elem == 4) { if (cl) RS_ITEMS(4, true); else RS_ITEMS(4, false); }
  else if (elem == 2) { if (cl) RS_ITEMS(2, true); else RS_ITEMS(2, false); }
  else { if (cl) RS_ITEMS(1, true); else RS_ITEMS(1, false); }
#undef RS_ITEMS
  return hipGetLastError();
}

hipError_t launch_resample_step(hipStream_t q, int NBg, int max_count, const float* audio, int64_t row, const RsStepRow* desc,
                                const float* hist_old, float* hist_new, const RsFilter& f, float gain, void* out, int law) {
  int tile;
  size_t lds;
  rs_geometry(f, &tile, &lds);
  const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div((int64_t)max_count + (law ? 3 : 1), tile), 1), 1024), NBg);
  const bool cl = f.L <= kRsLdsPhases;
#define RS_STEP(E, CL) \
  hipLaunchKernelGGL((resample_step_kernel<E, CL>), grid, dim3(256), lds, q, audio, row, desc, hist_old, hist_new, f, gain, out, tile, law)
  if (law) { if (cl) RS_STEP(1, true); else RS_STEP(1, false); }
  else { if (cl) RS_STEP(2, true); else RS_STEP(2, false); }
#undef RS_STEP
  return hipGetLastError();
}

void mix_step_plan(MixStepRow* rows, int NBg, int pack_blocks, int* grid_x, size_t* lds_bytes) {
  int64_t gx = 1;
  size_t lds = 0;
  for (int r = 0; r < NBg; r++) {
    MixStepRow& d = rows[r];
    if (d.n_in == 0) continue;
    if (d.L == 0) {
      gx = std::max<int64_t>(gx, pack_blocks);
      continue;
    }
    size_t bytes;
    rs_geometry(RsFilter{d.taps, d.L, d.M, d.P}, &d.tile, &bytes);
    lds = std::max(lds, bytes);  // (a multiple of 16: the base of every row's span is 16-byte aligned)
    gx = std::max(gx, ceil_div((int64_t)d.count + 3, d.tile));
  }
  *grid_x = (int)std::min<int64_t>(gx, 1024);
  *lds_bytes = lds;
}

hipError_t launch_mixed_step(hipStream_t q, int NBg, int grid_x, size_t lds_bytes, const float* audio, int64_t row, const MixStepRow* desc,
                             const float* hist_old, float* hist_new, void* out) {
  if (NBg < 1 || grid_x < 1 || lds_bytes > kRsLdsMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mixed_step_kernel, dim3(grid_x, NBg), dim3(256), lds_bytes, q, audio, row, desc, hist_old, hist_new, out);
  return hipGetLastError();
}

namespace { PH_WARM(resample, (resample_items_kernel<2, false>)); }

}  // namespace ph

using namespace ph;

// ---- host-only entry points: these work without a device

PH_EXPORT int piper_hip_resample_info(int32_t in_rate, int32_t out_rate, int32_t* L, int32_t* M, int32_t* taps) {
  const RsDesign* d = nullptr;
  const int rc = rs_design(in_rate, out_rate, &d);
  if (rc) return rc;
  if (L) *L = d->L;
  if (M) *M = d->M;
  if (taps) *taps = d->P;
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_resample_taps(int32_t in_rate, int32_t out_rate, float* table, size_t max_floats) {
  const RsDesign* d = nullptr;
  const int rc = rs_design(in_rate, out_rate, &d);
  if (rc) return rc;
  if (!table) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_taps: null table");
  if (max_floats < d->taps.size()) PH_FAIL(PIPER_HIP_ERR_SHAPE, "resample_taps: buffer holds %zu < %zu floats", max_floats, d->taps.size());
  memcpy(table, d->taps.data(), d->taps.size() * sizeof(float));
  return PIPER_HIP_OK;
}

PH_EXPORT int64_t piper_hip_resample_count(int32_t in_rate, int32_t out_rate, int64_t n_in) {
  const RsDesign* d = nullptr;
  const int rc = rs_design(in_rate, out_rate, &d);
  if (rc) return rc;
  if (n_in < 0 || n_in > ((int64_t)1 << 50)) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_count: %lld input samples", (long long)n_in);
  return rs_count(*d, n_in);
}

PH_EXPORT int64_t piper_hip_resample_step_bound(int32_t in_rate, int32_t out_rate, int64_t n_in) {
  const RsDesign* d = nullptr;
  const int rc = rs_design(in_rate, out_rate, &d);
  if (rc) return rc;
  if (n_in < 0 || n_in > ((int64_t)1 << 50)) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_step_bound: %lld input samples", (long long)n_in);
  return rs_step_bound(*d, n_in);
}

// ---- per-op

namespace {
// x[count] → *out — the fp32 y (elem 4), int16 (elem 2) or G.711 bytes by `law` (elem 1) —, the table uploaded behind a pool block that
// is returned at the context's next sync point
int resample_op(piper_hip_ctx* ctx, const char* who, const float* x, size_t count, int in_rate, int out_rate, float gain, void** out, size_t elem,
                int law, size_t* out_count, piper_hip_stream stream) {
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: null output pointer", who);
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: null input", who);
  if (!(gain >= 0.0f) || !std::isfinite(gain)) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: gain %g is negative or not finite", who, (double)gain);
  if (((uintptr_t)*out & (elem - 1)) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "%s: the output buffer is not %zu-byte aligned", who, elem);
  if (count > ((size_t)1 << 40)) PH_FAIL(PIPER_HIP_ERR_SHAPE, "%s: %zu samples", who, count);
  const RsDesign* d = nullptr;
  int rc = rs_design(in_rate, out_rate, &d);
  if (rc) return rc;
  const size_t n_out = (size_t)rs_count(*d, (int64_t)count);
  if (!*out) {
    if ((rc = ctx->pool.alloc(n_out * elem, out))) return rc;
  }
  if (out_count) *out_count = n_out;
  if (n_out == 0) return PIPER_HIP_OK;
  void* tab = nullptr;
  if ((rc = ctx->pool.alloc(d->taps.size() * sizeof(float), &tab))) return rc;
  defer_free(ctx, tab);
  StreamScope ss(ctx, stream);
  PH_HIP(hipMemcpyAsync(tab, d->taps.data(), d->taps.size() * sizeof(float), hipMemcpyHostToDevice, ss.s), PIPER_HIP_ERR_LAUNCH);
  const RsFilter f{(const float*)tab, d->L, d->M, d->P};
  (void)launch_resample_items(ss.s, x, 0, nullptr, 0, 1, 1, (int64_t)count, f, gain == 0.0f ? 1.0f : gain, nullptr, nullptr, *out, (int)elem, law);
  return ss.finish(who);
}
}  // namespace

PH_EXPORT int piper_hip_resample_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float** out,
                                     size_t* out_count, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (in_rate == out_rate && in_rate > 0) {  // not a filter: a copy
    if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_f32: null output pointer");
    if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_f32: null input");
    if (((uintptr_t)*out & 3) != 0) PH_FAIL(PIPER_HIP_ERR_ARG, "resample_f32: the output buffer is not 4-byte aligned");
    if (!*out) {
      void* p = nullptr;
      const int rc = ctx->pool.alloc(count * sizeof(float), &p);
      if (rc) return rc;
      *out = (float*)p;
    }
    if (out_count) *out_count = count;
    if (count == 0) return PIPER_HIP_OK;
    StreamScope ss(ctx, stream);
    PH_HIP(hipMemcpyAsync(*out, x, count * sizeof(float), hipMemcpyDeviceToDevice, ss.s), PIPER_HIP_ERR_LAUNCH);
    return ss.finish("resample_f32");
  }
  return resample_op(ctx, "resample_f32", x, count, in_rate, out_rate, 1.0f, (void**)out, sizeof(float), 0, out_count, stream);
}

PH_EXPORT int piper_hip_resample_pcm16_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float gain,
                                           int16_t** out, size_t* out_count, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);
  if (in_rate == out_rate && in_rate > 0) {  // not a filter: bit for bit the un-resampled call
    const int rc = piper_hip_pcm16_f32(ctx, x, count, gain, out, stream);
    if (!rc && out_count) *out_count = count;
    return rc;
  }
  return resample_op(ctx, "resample_pcm16_f32", x, count, in_rate, out_rate, gain, (void**)out, sizeof(int16_t), 0, out_count, stream);
}

// ---- G.711 (include/piper_hip.h "G.711 output")

PH_EXPORT int piper_hip_g711_f32(piper_hip_ctx* ctx, const float* x, size_t count, int32_t in_rate, int32_t out_rate, float gain, int law,
                                 uint8_t** out, size_t* out_count, piper_hip_stream stream) {
  PH_CHECK_CTX(ctx);  // stays first: without a device this returns UNAVAILABLE before any other field of ctx is touched
  if (law != PIPER_HIP_G711_MULAW && law != PIPER_HIP_G711_ALAW) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_f32: law %d (1 = mu-law, 2 = A-law)", law);
  if (in_rate != out_rate || in_rate <= 0)
    return resample_op(ctx, "g711_f32", x, count, in_rate, out_rate, gain, (void**)out, 1, law, out_count, stream);
  // not a filter: the byte of every sample of piper_hip_pcm16_f32
  if (!out) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_f32: null output pointer");
  if (!x && count) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_f32: null input");
  if (!(gain >= 0.0f) || !std::isfinite(gain)) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_f32: gain %g is negative or not finite", (double)gain);
  if (!*out) {
    void* p = nullptr;
    const int rc = ctx->pool.alloc(count, &p);
    if (rc) return rc;
    *out = (uint8_t*)p;
  }
  if (out_count) *out_count = count;
  if (count == 0) return PIPER_HIP_OK;
  StreamScope ss(ctx, stream);
  (void)launch_pcm16_flat(ss.s, x, (int64_t)count, gain == 0.0f ? 1.0f : gain, *out, law, ctx->num_cus);
  return ss.finish("g711_f32");
}
