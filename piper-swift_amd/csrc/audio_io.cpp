// audio_io.cpp — float waveform → 16-bit PCM / mono WAV file, the last hop after synthesize (host-only).
//
// Same sample conversion as the reference's CLI writer (WavFileWriter.swift:20-30): clamp to [−1, 1] in double, multiply by
// 32767.0, truncate toward zero; header layout of its writeHeaderPlaceholder / finalize (RIFF, fmt chunk 16 bytes, PCM,
// 1 channel, 16 bits, data chunk).
//
// G.711 (include/piper_hip.h "G.711 output"): the two laws in the table-search form of the contract, their decodes, and a WAV writer for
// companded bytes (format tags 7 and 6, an 18-byte fmt chunk and a fact chunk, as the RIFF specification asks of non-PCM formats).
#include <cstdio>

#include "common.h"

using namespace ph;

PH_EXPORT int piper_hip_pcm16_from_f32(const float* samples, size_t n, int16_t* pcm) {
  if ((!samples || !pcm) && n) PH_FAIL(PIPER_HIP_ERR_ARG, "pcm16_from_f32: null argument");
  for (size_t i = 0; i < n; i++) {
    double x = (double)samples[i];
    x = x != x ? 0.0 : (x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x));  // NaN → silence rather than undefined conversion
    const long v = (long)(x * 32767.0);                            // C cast truncates toward zero like Swift's Int(_:)
    pcm[i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
  }
  return PIPER_HIP_OK;
}

namespace {
// RIFF / fmt (16 bytes, PCM, 1 channel, 16 bits) / data header of n samples
void wav_header(uint8_t h[44], size_t n, int32_t sample_rate) {
  const uint32_t data_bytes = (uint32_t)(n * 2), riff = 36 + data_bytes, rate = (uint32_t)sample_rate, byte_rate = rate * 2;
  auto u32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; i++) h[at + i] = (uint8_t)(v >> (8 * i)); };
  auto u16 = [&](int at, uint32_t v) { h[at] = (uint8_t)v; h[at + 1] = (uint8_t)(v >> 8); };
  memcpy(h, "RIFF", 4); u32(4, riff); memcpy(h + 8, "WAVE", 4);
  memcpy(h + 12, "fmt ", 4); u32(16, 16); u16(20, 1); u16(22, 1); u32(24, rate); u32(28, byte_rate); u16(32, 2); u16(34, 16);
  memcpy(h + 36, "data", 4); u32(40, data_bytes);
}
}  // namespace

PH_EXPORT int piper_hip_wav_write(const char* path, const float* samples, size_t n, int32_t sample_rate) {
  if (!path || (!samples && n)) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write: null argument");
  if (sample_rate <= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write: sample_rate %d", sample_rate);
  if (n > 0x7fffffffu / 2) PH_FAIL(PIPER_HIP_ERR_SHAPE, "wav_write: %zu samples do not fit a RIFF file", n);
  FILE* f = fopen(path, "wb");
  if (!f) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write: cannot create '%s'", path);
  uint8_t h[44];
  wav_header(h, n, sample_rate);
  bool ok = fwrite(h, 1, 44, f) == 44;
  std::vector<int16_t> pcm(n < 65536 ? n : 65536);
  for (size_t at = 0; ok && at < n; at += pcm.size()) {
    const size_t m = n - at < pcm.size() ? n - at : pcm.size();
    piper_hip_pcm16_from_f32(samples + at, m, pcm.data());
    ok = fwrite(pcm.data(), 2, m, f) == m;  // little-endian host (x86-64)
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write: short write to '%s'", path);
  return PIPER_HIP_OK;
}

// The same file from samples that are 16-bit PCM already (the device's conversion, at whatever rate it delivered).
PH_EXPORT int piper_hip_wav_write_pcm16(const char* path, const int16_t* pcm, size_t n, int32_t sample_rate) {
  if (!path || (!pcm && n)) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_pcm16: null argument");
  if (sample_rate <= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_pcm16: sample_rate %d", sample_rate);
  if (n > 0x7fffffffu / 2) PH_FAIL(PIPER_HIP_ERR_SHAPE, "wav_write_pcm16: %zu samples do not fit a RIFF file", n);
  FILE* f = fopen(path, "wb");
  if (!f) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_pcm16: cannot create '%s'", path);
  uint8_t h[44];
  wav_header(h, n, sample_rate);
  bool ok = fwrite(h, 1, 44, f) == 44;
  ok = ok && fwrite(pcm, 2, n, f) == n;  // little-endian host (x86-64)
  ok = (fclose(f) == 0) && ok;
  if (!ok) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_pcm16: short write to '%s'", path);
  return PIPER_HIP_OK;
}

// ---- G.711

namespace {
uint8_t g711_mulaw(int s) {
  static const int end[8] = {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF};
  const int v = s >> 2;  // arithmetic shift
  const bool neg = v < 0;
  const int a = neg ? -v : v, m = (a < 8159 ? a : 8159) + 33;
  int seg = 0;
  while (seg < 8 && end[seg] < m) seg++;
  const int code = seg == 8 ? 0x7F : (seg << 4) | ((m >> (seg + 1)) & 15);
  return (uint8_t)(code ^ (neg ? 0x7F : 0xFF));
}

uint8_t g711_alaw(int s) {
  static const int end[8] = {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF};
  const int v = s >> 3;
  const bool neg = v < 0;
  const int m = neg ? -v - 1 : v;
  int seg = 0;
  while (seg < 8 && end[seg] < m) seg++;  // (m ≤ 4095: at most 7)
  const int code = (seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15);
  return (uint8_t)(code ^ (neg ? 0x55 : 0xD5));
}

int16_t g711_mulaw_decode(uint8_t b) {
  const int u = ~b & 0xFF;
  const int t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);
  return (int16_t)((u & 0x80) ? 0x84 - t : t - 0x84);
}

int16_t g711_alaw_decode(uint8_t b) {
  const int a = b ^ 0x55, seg = (a & 0x70) >> 4;
  int t = (a & 15) << 4;
  t = seg == 0 ? t + 8 : seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1);
  return (int16_t)((a & 0x80) ? t : -t);
}

bool g711_law_ok(int law) { return law == PIPER_HIP_G711_MULAW || law == PIPER_HIP_G711_ALAW; }
}  // namespace

PH_EXPORT int piper_hip_g711_from_pcm16(int law, const int16_t* pcm, size_t n, uint8_t* out) {
  if (!g711_law_ok(law)) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_from_pcm16: law %d (1 = mu-law, 2 = A-law)", law);
  if ((!pcm || !out) && n) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_from_pcm16: null argument");
  if (law == PIPER_HIP_G711_MULAW) for (size_t i = 0; i < n; i++) out[i] = g711_mulaw(pcm[i]);
  else for (size_t i = 0; i < n; i++) out[i] = g711_alaw(pcm[i]);
  return PIPER_HIP_OK;
}

PH_EXPORT int piper_hip_g711_to_pcm16(int law, const uint8_t* in, size_t n, int16_t* pcm) {
  if (!g711_law_ok(law)) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_to_pcm16: law %d (1 = mu-law, 2 = A-law)", law);
  if ((!in || !pcm) && n) PH_FAIL(PIPER_HIP_ERR_ARG, "g711_to_pcm16: null argument");
  if (law == PIPER_HIP_G711_MULAW) for (size_t i = 0; i < n; i++) pcm[i] = g711_mulaw_decode(in[i]);
  else for (size_t i = 0; i < n; i++) pcm[i] = g711_alaw_decode(in[i]);
  return PIPER_HIP_OK;
}

// RIFF / fmt (18 bytes: tag 7 or 6, 1 channel, 8 bits, cbSize 0) / fact (n) / data, padded to an even length
PH_EXPORT int piper_hip_wav_write_g711(const char* path, int law, const uint8_t* bytes, size_t n, int32_t sample_rate) {
  if (!g711_law_ok(law)) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_g711: law %d (1 = mu-law, 2 = A-law)", law);
  if (!path || (!bytes && n)) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_g711: null argument");
  if (sample_rate <= 0) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_g711: sample_rate %d", sample_rate);
  if (n > 0x7fffff00u) PH_FAIL(PIPER_HIP_ERR_SHAPE, "wav_write_g711: %zu samples do not fit a RIFF file", n);
  FILE* f = fopen(path, "wb");
  if (!f) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_g711: cannot create '%s'", path);
  uint8_t h[58];
  const uint32_t data_bytes = (uint32_t)n, pad = data_bytes & 1, rate = (uint32_t)sample_rate;
  auto u32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; i++) h[at + i] = (uint8_t)(v >> (8 * i)); };
  auto u16 = [&](int at, uint32_t v) { h[at] = (uint8_t)v; h[at + 1] = (uint8_t)(v >> 8); };
  memcpy(h, "RIFF", 4); u32(4, 50 + data_bytes + pad); memcpy(h + 8, "WAVE", 4);
  memcpy(h + 12, "fmt ", 4); u32(16, 18); u16(20, law == PIPER_HIP_G711_MULAW ? 7 : 6); u16(22, 1); u32(24, rate); u32(28, rate); u16(32, 1); u16(34, 8);
  u16(36, 0);
  memcpy(h + 38, "fact", 4); u32(42, 4); u32(46, data_bytes);
  memcpy(h + 50, "data", 4); u32(54, data_bytes);
  bool ok = fwrite(h, 1, 58, f) == 58;
  ok = ok && fwrite(bytes, 1, n, f) == n;
  const uint8_t zero = 0;
  if (pad) ok = ok && fwrite(&zero, 1, 1, f) == 1;
  ok = (fclose(f) == 0) && ok;
  if (!ok) PH_FAIL(PIPER_HIP_ERR_ARG, "wav_write_g711: short write to '%s'", path);
  return PIPER_HIP_OK;
}
