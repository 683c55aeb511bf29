/* piper_hip_cli.c — the bench / one-shot modes of the reference's command line (Sources/PiperCLI/PiperCLI.swift) over the C-ABI, in plain C.
 *
 *   --scale-bench            PiperCLI.runScaleBench (PiperCLI.swift:381-551): the fixture utterance tiled by each scale factor, truncated at
 *                            --max-phonemes, `--warmup` untimed + `--iters` timed calls of synthesize per factor, ONE JSON object on stdout with the
 *                            reference's keys (backend, mode, model_path, sample_rate, warmup, iters, max_phonemes, scale_factors,
 *                            base_test_phonemes, results[{factor, phoneme_count, ms_mean, ms_p50, ms_p95, ms_max}]); with
 *                            PIPER_BENCH_GPU_TIMING=1 also gpu_ms_mean, cpu_user_ms_mean, cpu_sys_ms_mean, gpu_busy_fraction_mean, max_rss_max
 *                            (PiperCLI.swift:288, 395, 524-537). Same flags: --warmup (1) --iters (3) --scale-factors (1,2,4,8,16) --max-phonemes (4096)
 *                            --model voice.onnx [--config voice.onnx.json].
 *   --phoneme-ids a,b,c …    one utterance → --output file.wav (16-bit, WavFileWriter.swift:20-60); the espeak-ng front end of the reference CLI is
 *                            out of scope, so the ids are the input. --output-raw file.raw writes the s16le stream instead (or as
 *                            well), converted on the device (piper_hip_voice_synthesize_pcm16; after --output, collect_pcm16 on the
 *                            slot that ran): --volume V scales it (linear, default 1),
 *                            --normalize applies Piper's peak normalisation (audio_float_to_int16). Both flags act on --output-raw only.
 *                            --output-rate N (8000 … 48000) resamples on the device (piper_hip_voice_collect_pcm16_rate): --output-raw is
 *                            then s16le at N Hz, and --output a WAV whose header carries N (piper_hip_wav_write_pcm16).
 *                            --output-encoding s16le|mulaw|alaw (default s16le): G.711 bytes companded on the device
 *                            (piper_hip_voice_collect_g711 / synthesize_g711) — --output-raw is then one byte per sample, --output a
 *                            G.711 WAV at the output rate (piper_hip_wav_write_g711); combinable with --output-rate, --volume and
 *                            --normalize (with a law the last two act on --output as well: the file holds the same bytes).
 *                            --drive X --ceiling Y --release-ms Z: a look-ahead limiter on the device in front of every output above
 *                            (piper_hip_voice_slot_level on slot 0; a flag left out takes its default 1, 1, 50). Not with --normalize.
 *                            --loudness LUFS [--max-gain-db X]: BS.1770 integrated loudness measured on the device and the utterance
 *                            brought to that target in front of the limiter and every output above (piper_hip_voice_slot_loudness on
 *                            slot 0; X defaults to 20); the measured loudness and the gain go to stderr. Not with --normalize.
 *                            --id-volume I:J=G[,I:J=G…]: a volume per phoneme id, ids I … J − 1 at the linear gain G (0 … 16) and the
 *                            others at 1.0, ramped between ids on the device in front of the loudness gain, the limiter and every
 *                            output above (piper_hip_voice_slot_volume on slot 0).
 *                            --eq TYPE:F0:Q[:GAIN_DB], up to four times: a biquad section of the equaliser on the device (TYPE lowpass,
 *                            highpass, bandpass, notch, peaking, lowshelf or highshelf; GAIN_DB for peaking and the shelves), in front
 *                            of the loudness gain, the limiter and every output above (piper_hip_voice_slot_eq on slot 0).
 *                            --phoneme-ids A/B/…: several id lists separated by '/', the sentences of one text. They run as ONE
 *                            piper_hip_voice_prepare_batch and leave as ONE programme joined on the device (piper_hip_voice_slot_join on
 *                            slot 0), with --sentence-silence SECONDS (Piper's flag) between them, --lead-ms X / --tail-ms X of silence
 *                            around them and --trim-silence THRESHOLD[:PAD_MS[:FADE_MS]] cutting each sentence's quiet head and tail
 *                            (linear amplitude; the cut edges fade). Any of the four flags joins a single list too. Each sentence's
 *                            start in the programme is printed on stderr. One list without these flags behaves as before.
 *                            --pitch ST[/ST…]: a shift in semitones (−12 … 12) for every sentence, or one per sentence, applied on the
 *                            device behind the volume and in front of the EQ and every output above (piper_hip_voice_slot_pitch on
 *                            slot 0). The tempo is kept: the predicted durations are scaled so that the sentence keeps its length (so
 *                            this needs --predict, or a real voice); --pitch-varispeed turns that off: the sentence comes out 1/ρ as
 *                            long, with pinned durations too.
 *   --speaker N              both modes: speaker N of a multi-speaker voice (the graph's `sid`; piper_hip_voice_attach_speakers +
 *                            piper_hip_voice_slot_speakers). With --model the file's speaker table is loaded (opt-in: without the flag such a
 *                            file is refused; its node graph is NOT verified — no verifier for the conditioned graph exists yet); without
 *                            --model the synthetic voice gets a synthetic table of --speakers rows (8).
 * Without --model the synthetic voice of the tests is used (--quality medium|high|low|x_low; low and x_low are the 16 kHz tier); its duration predictor has random weights, so frames per id are
 * pinned to --pin-frames (3, the bench's convention) unless --predict asks for the predictor (the only mode a real voice has).
 *
 * build: gcc -std=c99 -O2 -Iinclude examples/piper_hip_cli.c -Lpiper-swift_amd/lib -lpiper_hip -Wl,-rpath,$PWD/piper-swift_amd/lib -o piper_hip_cli
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <time.h>

#include "piper_hip.h"

static const int64_t kFixture[14] = {1, 20, 0, 120, 0, 61, 0, 24, 0, 59, 0, 100, 0, 2}; /* bench/fixtures/test_summary.json:8 */

#define CHECK(call)                                                                \
  do {                                                                             \
    int rc_ = (call);                                                              \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, piper_hip_last_error()); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static const char* arg_value(int argc, char** argv, const char* key) {
  for (int i = 1; i + 1 < argc; i++)
    if (strcmp(argv[i], key) == 0) return argv[i + 1];
  return NULL;
}
static int has_flag(int argc, char** argv, const char* key) {
  for (int i = 1; i < argc; i++)
    if (strcmp(argv[i], key) == 0) return 1;
  return 0;
}
static int parse_csv_i64(const char* s, int64_t* out, int cap) {
  int n = 0;
  while (*s && n < cap) {
    char* end = NULL;
    const long long v = strtoll(s, &end, 10);
    if (end == s) return -1;
    out[n++] = v;
    s = end;
    while (*s == ',' || *s == ' ') s++;
  }
  return n;
}
static double now_ms(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static double tv_ms(struct timeval tv) { return tv.tv_sec * 1e3 + tv.tv_usec * 1e-3; }
static int cmp_double(const void* a, const void* b) { return (*(const double*)a > *(const double*)b) - (*(const double*)a < *(const double*)b); }
/* linear-interpolated percentile of the sorted sample, as PiperCLI.swift:428-436 */
static double percentile(double* sorted, int n, double p) {
  const double k = (n - 1) * (p / 100.0);
  const int f = (int)k;
  const int c = (k > f) ? f + 1 : f;
  return f == c ? sorted[f] : sorted[f] + (sorted[c] - sorted[f]) * (k - f);
}

typedef struct {
  piper_hip_voice* voice;
  float noise_scale, length_scale, noise_w;
  int predict, pin_frames;
  float* audio;
  int64_t audio_cap;
  float* id_gain; /* --id-volume: one gain per id of the utterance, NULL without the flag */
  piper_hip_pitch pitch[PIPER_HIP_JOIN_MAX_ITEMS]; /* --pitch: one per sentence */
  int n_pitch;                                     /* 0 without the flag */
} runner;

/* --pitch: the pitch of the staging call that follows (the assignment is that call's alone, so it is made before each) */
static int stage_pitch(runner* r) {
  return r->n_pitch ? piper_hip_voice_slot_pitch(r->voice, 0, r->pitch, r->n_pitch) : 0;
}

/* --id-volume: the volume of the staging call that follows (the assignment is that call's alone, so it is made before each) */
static int stage_volume(runner* r, int t) {
  piper_hip_volume vol;
  if (!r->id_gain) return 0;
  vol.gain = r->id_gain; vol.t = t;
  return piper_hip_voice_slot_volume(r->voice, 0, &vol, 1);
}

/* "I:J=G[,I:J=G…]" → gain[t], 1.0 where no range names the id; 0 on success */
static int parse_id_volume(const char* s, float* gain, int t) {
  for (int i = 0; i < t; i++) gain[i] = 1.0f;
  while (*s) {
    char* end = NULL;
    const long a = strtol(s, &end, 10);
    if (end == s || *end != ':') return -1;
    s = end + 1;
    const long b = strtol(s, &end, 10);
    if (end == s || *end != '=') return -1;
    s = end + 1;
    const float g = strtof(s, &end);
    if (end == s || a < 0 || b < a || b > t) return -1;
    for (long i = a; i < b; i++) gain[i] = g;
    s = end;
    if (*s == ',') s++;
    else if (*s) return -1;
  }
  return 0;
}

/* PiperMetalRuntime.synthesize(phonemeIDs:noiseScale:lengthScale:noiseW:) on slot 0; *samples = waveform length */
static int run_one(runner* r, const int64_t* ids, int t, int64_t* samples) {
  piper_hip_utterance u;
  memset(&u, 0, sizeof u);
  u.phoneme_ids = ids; u.t = t; u.noise_scale = r->noise_scale; u.seed = 1234; /* the reference's fixed seed (GraphExecutor.swift:2658) */
  u.length_scale = r->length_scale; u.noise_w = r->noise_w; u.noise_mode = PIPER_HIP_NOISE_DEVICE;
  int32_t* dur = NULL;
  if (!r->predict) {
    dur = (int32_t*)malloc(sizeof(int32_t) * (size_t)t);
    for (int i = 0; i < t; i++) dur[i] = r->pin_frames;
    u.durations = dur;
  }
  int rc = stage_volume(r, t);
  if (rc >= 0) rc = stage_pitch(r);
  if (rc >= 0) rc = piper_hip_voice_prepare(r->voice, &u, 0);
  free(dur);
  if (rc < 0) return rc;
  int64_t n = 0;
  if ((rc = piper_hip_voice_pitch_samples(r->voice, 0, NULL, 0, &n)) < 0) return rc; /* (without a pitch: prepared_samples) */
  if (n > r->audio_cap) {
    free(r->audio);
    r->audio = (float*)malloc(sizeof(float) * (size_t)n);
    r->audio_cap = n;
  }
  if ((rc = piper_hip_voice_launch(r->voice, 0)) < 0) return rc;
  if ((rc = piper_hip_voice_collect(r->voice, 0, r->audio, n)) < 0) return rc;
  *samples = n;
  return 0;
}

/* The utterance as 16-bit samples converted on the device — law != 0: as G.711 bytes, through the _g711 twins of the calls named here.
 * *pcm is malloc'ed; the caller frees it, after a failure too.
 * ran != 0: run_one has just run this utterance on slot 0 and its waveform is still in the plan, so piper_hip_voice_collect_pcm16 converts
 * that. Otherwise pinned durations go through piper_hip_voice_synthesize_pcm16 in one call; with --predict the length is the predictor's,
 * so the slot is prepared (once), asked for it, launched and collected as PCM. */
static int run_one_pcm16(runner* r, const int64_t* ids, int t, const piper_hip_pcm_params* prm, int ran, int in_rate, int rate, int law, void** pcm,
                         int64_t* samples) {
  const size_t elem = law ? 1 : sizeof(int16_t);
  piper_hip_utterance u;
  memset(&u, 0, sizeof u);
  u.phoneme_ids = ids; u.t = t; u.noise_scale = r->noise_scale; u.seed = 1234;
  u.length_scale = r->length_scale; u.noise_w = r->noise_w; u.noise_mode = PIPER_HIP_NOISE_DEVICE;
  int rc;
  int64_t cap = 0;
  *pcm = NULL;
  int32_t* pinned = NULL;
  if (!ran && !r->predict && !r->n_pitch) {
    int32_t* dur = (int32_t*)malloc(sizeof(int32_t) * (size_t)t);
    for (int i = 0; i < t; i++) dur[i] = r->pin_frames;
    u.durations = dur;
    cap = piper_hip_voice_num_samples(r->voice, &u);
    if (cap >= 0 && rate != in_rate) cap = piper_hip_resample_count(in_rate, rate, cap);
    rc = cap < 0 ? (int)cap : 0;
    if (!rc) *pcm = malloc(elem * (size_t)(cap > 0 ? cap : 1));
    if (!rc) rc = stage_volume(r, t);
    if (!rc) rc = law ? piper_hip_voice_synthesize_g711(r->voice, &u, prm, law, rate, (uint8_t*)*pcm, cap, samples)
                      : piper_hip_voice_synthesize_pcm16_rate(r->voice, &u, prm, rate, (int16_t*)*pcm, cap, samples);
    free(dur);
    return rc;
  }
  if (!ran && !r->predict) { /* a pitch: the length is the library's to say, so the slot is prepared and asked */
    pinned = (int32_t*)malloc(sizeof(int32_t) * (size_t)t);
    for (int i = 0; i < t; i++) pinned[i] = r->pin_frames;
    u.durations = pinned;
  }
  rc = ran ? 0 : stage_volume(r, t);
  if (!ran && rc >= 0) rc = stage_pitch(r);
  if (!ran && rc >= 0) rc = piper_hip_voice_prepare(r->voice, &u, 0);
  free(pinned);
  if (rc < 0) return rc;
  if ((rc = piper_hip_voice_pitch_samples(r->voice, 0, NULL, 0, &cap)) < 0) return rc;
  if (rate != in_rate && (cap = piper_hip_resample_count(in_rate, rate, cap)) < 0) return (int)cap;
  *pcm = malloc(elem * (size_t)(cap > 0 ? cap : 1));
  if (!ran && (rc = piper_hip_voice_launch(r->voice, 0)) < 0) return rc;
  rc = law ? piper_hip_voice_collect_g711(r->voice, 0, prm, law, rate, (uint8_t*)*pcm, cap)
           : piper_hip_voice_collect_pcm16_rate(r->voice, 0, prm, rate, (int16_t*)*pcm, cap);
  if (rc < 0) return rc;
  *samples = cap;
  return 0;
}

/* Several sentences (or one under a join flag): one prepare_batch on slot 0, joined on the device into ONE programme, converted (and
 * resampled, as one signal) there. *pcm is malloc'ed; the caller frees it, after a failure too. The starts go to stderr. */
static int run_programme(runner* r, const int64_t* ids, const int* off, const int* len, int n_lists, const piper_hip_join* join,
                         const piper_hip_pcm_params* prm, int in_rate, int rate, int law, void** pcm, int64_t* samples) {
  piper_hip_utterance u[PIPER_HIP_JOIN_MAX_ITEMS];
  int64_t start[PIPER_HIP_JOIN_MAX_ITEMS], total = 0, cap = 0;
  int32_t* dur = NULL;
  int rc;
  *pcm = NULL;
  memset(u, 0, sizeof u);
  if (!r->predict) {
    int t_max = 0;
    for (int i = 0; i < n_lists; i++) t_max = len[i] > t_max ? len[i] : t_max;
    dur = (int32_t*)malloc(sizeof(int32_t) * (size_t)t_max);
    for (int i = 0; i < t_max; i++) dur[i] = r->pin_frames;
  }
  for (int i = 0; i < n_lists; i++) {
    u[i].phoneme_ids = ids + off[i]; u[i].t = len[i]; u[i].noise_scale = r->noise_scale; u[i].seed = 1234;
    u[i].length_scale = r->length_scale; u[i].noise_w = r->noise_w; u[i].noise_mode = PIPER_HIP_NOISE_DEVICE;
    u[i].durations = dur;
  }
  rc = piper_hip_voice_slot_join(r->voice, 0, join, NULL, 0);
  if (rc >= 0) rc = stage_pitch(r);
  if (rc >= 0) rc = piper_hip_voice_prepare_batch(r->voice, u, n_lists, 0);
  free(dur);
  if (rc < 0) return rc;
  if ((rc = piper_hip_voice_join_capacity(r->voice, 0, rate, &cap)) < 0) return rc;
  *pcm = malloc((law ? 1 : sizeof(int16_t)) * (size_t)(cap > 0 ? cap : 1));
  if ((rc = piper_hip_voice_launch(r->voice, 0)) < 0) return rc;
  rc = law ? piper_hip_voice_collect_g711(r->voice, 0, prm, law, rate, (uint8_t*)*pcm, cap)
           : piper_hip_voice_collect_pcm16_rate(r->voice, 0, prm, rate, (int16_t*)*pcm, cap);
  if (rc < 0) return rc;
  if ((rc = piper_hip_voice_join_report(r->voice, 0, start, NULL, PIPER_HIP_JOIN_MAX_ITEMS, &total)) < 0) return rc;
  for (int i = 0; i < n_lists; i++) fprintf(stderr, "sentence %d starts at %.3f s\n", i, (double)start[i] / in_rate);
  *samples = rate == in_rate ? total : piper_hip_resample_count(in_rate, rate, total);
  return 0;
}

/* --eq TYPE:F0:Q[:GAIN_DB] → one section; nonzero on a malformed argument (the library checks the values) */
static int parse_eq_section(const char* s, piper_hip_eq_section* out) {
  static const char* const names[7] = {"lowpass", "highpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf"};
  char name[16];
  float f0 = 0.0f, q = 0.0f, g = 0.0f;
  const int k = sscanf(s, "%15[^:]:%f:%f:%f", name, &f0, &q, &g);
  if (k < 3) return 1;
  for (int i = 0; i < 7; i++)
    if (strcmp(name, names[i]) == 0) {
      out->type = PIPER_HIP_EQ_LOWPASS + i;
      out->f0_hz = f0; out->q = q; out->gain_db = k == 4 ? g : 0.0f;
      return 0;
    }
  return 1;
}

int main(int argc, char** argv) {
  const char* model = arg_value(argc, argv, "--model");
  const char* config = arg_value(argc, argv, "--config");
  const char* quality = arg_value(argc, argv, "--quality");
  static const char* const quality_names[4] = {"medium", "high", "low", "x_low"}; /* piper_hip_voice_config_preset's numbering */
  static const char* const synthetic_names[4] = {"synthetic:medium", "synthetic:high", "synthetic:low", "synthetic:x_low"};
  int preset = 0;
  if (quality) {
    for (preset = 0; preset < 4 && strcmp(quality, quality_names[preset]) != 0; preset++) {}
    if (preset == 4) { fprintf(stderr, "--quality %s: expected medium, high, low or x_low\n", quality); return 2; }
  }
  const int scale_bench = has_flag(argc, argv, "--scale-bench");
  const char* ids_arg = arg_value(argc, argv, "--phoneme-ids");
  const char* enc = arg_value(argc, argv, "--output-encoding");
  const int law = !enc || strcmp(enc, "s16le") == 0 ? 0 : strcmp(enc, "mulaw") == 0 ? PIPER_HIP_G711_MULAW : strcmp(enc, "alaw") == 0 ? PIPER_HIP_G711_ALAW : -1;
  if (law < 0) { fprintf(stderr, "--output-encoding %s: expected s16le, mulaw or alaw\n", enc); return 2; }
  if (!scale_bench && !ids_arg) {
    fprintf(stderr, "usage: %s --scale-bench [--warmup N] [--iters N] [--scale-factors 1,2,4,8,16] [--max-phonemes N]\n"
                    "       %s --phoneme-ids 1,20,0,… --output out.wav | --output-raw out.s16le [--volume V] [--normalize] [--output-rate N]\n"
                    "                [--output-encoding s16le|mulaw|alaw] [--drive X] [--ceiling Y] [--release-ms Z]\n"
                    "                [--loudness LUFS [--max-gain-db X]] [--id-volume I:J=G[,I:J=G...]] [--eq TYPE:F0:Q[:GAIN_DB] ...]\n"
                    "                [--phoneme-ids A/B/... --sentence-silence SECONDS --lead-ms X --tail-ms X --trim-silence THRESHOLD[:PAD_MS[:FADE_MS]]]\n"
                    "                [--pitch ST[/ST...] [--pitch-varispeed]]\n"
                    "       common: [--model voice.onnx [--config voice.onnx.json]] [--quality medium|high|low|x_low] [--predict] [--pin-frames N]\n"
                    "               [--speaker N [--speakers S]]\n", argv[0], argv[0]);
    return 2;
  }

  piper_hip_voice_config cfg;
  size_t n_floats = 0;
  float* blob = NULL;
  runner r;
  memset(&r, 0, sizeof r);
  r.noise_scale = 0.667f; r.length_scale = 1.0f; r.noise_w = 0.8f; /* PiperConfig defaults; the voice's .onnx.json overrides them */
  r.predict = has_flag(argc, argv, "--predict");
  r.pin_frames = arg_value(argc, argv, "--pin-frames") ? atoi(arg_value(argc, argv, "--pin-frames")) : 3;
  /* --speaker N: the `sid` of a multi-speaker voice (PiperMetalRuntime.synthesize reads it next to the scales, PiperMetalRuntime.swift:62-80).
   * Opt-in: without the flag a multi-speaker file is refused as before. */
  const char* speaker_arg = arg_value(argc, argv, "--speaker");
  const int speaker = speaker_arg ? atoi(speaker_arg) : -1;
  if (speaker_arg && speaker < 0) { fprintf(stderr, "--speaker %s: expected a speaker id >= 0\n", speaker_arg); return 2; }
  piper_hip_speaker_config scfg;
  float* sblob = NULL;
  memset(&scfg, 0, sizeof scfg);
  if (model) {
    piper_hip_onnx* m = NULL;
    CHECK(piper_hip_onnx_open(model, &m));
    if (speaker_arg) {
      CHECK(piper_hip_onnx_infer_config_speakers(m, &cfg));
      CHECK(piper_hip_onnx_speaker_config(m, &cfg, &scfg));
      if (scfg.n_speakers < 1) { fprintf(stderr, "--speaker: %s is a single-speaker voice\n", model); return 2; }
    } else {
      CHECK(piper_hip_onnx_infer_config(m, &cfg));
    }
    CHECK(piper_hip_voice_blob_floats(&cfg, &n_floats));
    blob = (float*)malloc(n_floats * sizeof(float));
    if (scfg.n_speakers) { /* no verifier for the conditioned graph exists yet: the caller vouches that this is a standard multi-speaker Piper VITS */
      size_t sn = 0;
      CHECK(piper_hip_onnx_build_blob_unchecked(m, &cfg, blob, n_floats));
      CHECK(piper_hip_speaker_blob_floats(&cfg, &scfg, &sn));
      sblob = (float*)malloc(sn * sizeof(float));
      CHECK(piper_hip_onnx_build_speaker_blob(m, &cfg, &scfg, sblob, sn));
    } else {
      CHECK(piper_hip_onnx_build_blob(m, &cfg, blob, n_floats)); /* verifies the graph first */
    }
    piper_hip_onnx_close(m);
    r.predict = 1; /* a real voice decides its own durations */
    if (config) { /* PiperConfig (PiperConfig.swift:3-47): sample rate and the three inference scales */
      FILE* fj = fopen(config, "rb");
      if (!fj) { fprintf(stderr, "cannot open %s\n", config); return 1; }
      fseek(fj, 0, SEEK_END);
      const long len = ftell(fj);
      fseek(fj, 0, SEEK_SET);
      char* text = (char*)malloc((size_t)len + 1);
      if (fread(text, 1, (size_t)len, fj) != (size_t)len) { fprintf(stderr, "cannot read %s\n", config); return 1; }
      text[len] = 0;
      fclose(fj);
      piper_hip_piper_json_info info;
      const int jrc = piper_hip_piper_json(text, &info);
      free(text);
      CHECK(jrc);
      if (scfg.n_speakers) CHECK(piper_hip_voice_check_json_speakers(&cfg, &scfg, &info));
      if (info.sample_rate > 0) cfg.sample_rate = info.sample_rate;
      r.noise_scale = info.noise_scale; r.length_scale = info.length_scale; r.noise_w = info.noise_w;
    }
  } else {
    CHECK(piper_hip_voice_config_preset(preset, &cfg));
    CHECK(piper_hip_voice_blob_floats(&cfg, &n_floats));
    blob = (float*)malloc(n_floats * sizeof(float));
    CHECK(piper_hip_voice_synthetic_blob(&cfg, 1234, blob, n_floats));
    if (speaker_arg) { /* the synthetic voice with a synthetic table of --speakers rows (8), gin 512 */
      size_t sn = 0;
      scfg.n_speakers = arg_value(argc, argv, "--speakers") ? atoi(arg_value(argc, argv, "--speakers")) : 8;
      scfg.gin = 512;
      CHECK(piper_hip_speaker_blob_floats(&cfg, &scfg, &sn));
      sblob = (float*)malloc(sn * sizeof(float));
      CHECK(piper_hip_speaker_synthetic_blob(&cfg, &scfg, 4321, sblob, sn));
    }
  }
  piper_hip_ctx* ctx = NULL;
  CHECK(piper_hip_create(0, &ctx));
  CHECK(piper_hip_voice_create(ctx, &cfg, blob, 0, &r.voice));
  free(blob);
  if (sblob) { /* the table before the first prepare, then slot 0's speaker for every utterance of this run */
    piper_hip_speaker spk;
    memset(&spk, 0, sizeof spk);
    spk.n = 1; spk.ids[0] = speaker; spk.weights[0] = 1.0f;
    CHECK(piper_hip_voice_attach_speakers(r.voice, &scfg, sblob, 0));
    free(sblob);
    CHECK(piper_hip_voice_slot_speakers(r.voice, 0, &spk, 1)); /* an id past the table: PIPER_HIP_ERR_ARG */
  }

  if (!scale_bench) { /* one shot: ids → WAV */
    int64_t ids[4096];
    /* several id lists separated by '/': the sentences of one text (one list: exactly the former behaviour) */
    int list_off[PIPER_HIP_JOIN_MAX_ITEMS], list_len[PIPER_HIP_JOIN_MAX_ITEMS], n_lists = 0, t = 0;
    {
      char* copy = (char*)malloc(strlen(ids_arg) + 1);
      strcpy(copy, ids_arg);
      for (char* part = copy; part && n_lists < PIPER_HIP_JOIN_MAX_ITEMS;) {
        char* bar = strchr(part, '/');
        if (bar) *bar = 0;
        const int k = parse_csv_i64(part, ids + t, 4096 - t);
        if (k < 1) { t = 0; break; }
        list_off[n_lists] = t; list_len[n_lists] = k; n_lists++;
        t += k;
        part = bar ? bar + 1 : NULL;
        if (part && n_lists == PIPER_HIP_JOIN_MAX_ITEMS) t = 0; /* more sentences than a join takes */
      }
      free(copy);
    }
    const char* out = arg_value(argc, argv, "--output");
    const char* out_raw = arg_value(argc, argv, "--output-raw");
    if (t < 1 || (!out && !out_raw)) { fprintf(stderr, "--phoneme-ids needs a comma-separated list and --output or --output-raw a path\n"); return 2; }
    int64_t n = 0;
    double gpu = 0.0;
    const int rate = arg_value(argc, argv, "--output-rate") ? atoi(arg_value(argc, argv, "--output-rate")) : cfg.sample_rate;
    piper_hip_pcm_params prm;
    prm.gain = arg_value(argc, argv, "--volume") ? (float)atof(arg_value(argc, argv, "--volume")) : 1.0f;
    prm.normalize = has_flag(argc, argv, "--normalize");
    if (arg_value(argc, argv, "--drive") || arg_value(argc, argv, "--ceiling") || arg_value(argc, argv, "--release-ms")) {
      piper_hip_level lv; /* slot 0's level: every collect below delivers the limited samples */
      lv.drive = arg_value(argc, argv, "--drive") ? (float)atof(arg_value(argc, argv, "--drive")) : 0.0f;
      lv.ceiling = arg_value(argc, argv, "--ceiling") ? (float)atof(arg_value(argc, argv, "--ceiling")) : 0.0f;
      lv.release_ms = arg_value(argc, argv, "--release-ms") ? (float)atof(arg_value(argc, argv, "--release-ms")) : 0.0f;
      CHECK(piper_hip_voice_slot_level(r.voice, 0, &lv));
    }
    const char* loud_arg = arg_value(argc, argv, "--loudness");
    if (loud_arg) {
      piper_hip_loudness ld; /* slot 0's loudness target: every collect below delivers the utterance at that loudness */
      ld.target_lufs = (float)atof(loud_arg);
      ld.max_gain_db = arg_value(argc, argv, "--max-gain-db") ? (float)atof(arg_value(argc, argv, "--max-gain-db")) : 0.0f;
      if (ld.target_lufs == 0.0f) { fprintf(stderr, "--loudness %s: expected a target in LUFS, -70 ... -1\n", loud_arg); return 2; }
      CHECK(piper_hip_voice_slot_loudness(r.voice, 0, &ld));
    }
    { /* --eq, up to four times: slot 0's equaliser, sections in the order given */
      piper_hip_eq eq;
      memset(&eq, 0, sizeof eq);
      for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--eq") != 0) continue;
        if (i + 1 == argc) { fprintf(stderr, "--eq: expected TYPE:F0:Q[:GAIN_DB] after the flag\n"); return 2; }
        if (eq.n == PIPER_HIP_EQ_MAX_SECTIONS) { fprintf(stderr, "--eq: at most %d sections\n", PIPER_HIP_EQ_MAX_SECTIONS); return 2; }
        if (parse_eq_section(argv[i + 1], &eq.section[eq.n]) != 0) {
          fprintf(stderr, "--eq %s: expected TYPE:F0:Q[:GAIN_DB], TYPE lowpass|highpass|bandpass|notch|peaking|lowshelf|highshelf\n", argv[i + 1]);
          return 2;
        }
        eq.n++;
      }
      if (eq.n) CHECK(piper_hip_voice_slot_eq(r.voice, 0, &eq));
    }
    const char* idvol_arg = arg_value(argc, argv, "--id-volume");
    if (idvol_arg) { /* slot 0's volume for the utterance: ids I … J − 1 at gain G, ramped between ids on the device */
      r.id_gain = (float*)malloc(sizeof(float) * (size_t)t);
      piper_hip_volume vol;
      int bad = parse_id_volume(idvol_arg, r.id_gain, t) != 0;
      if (bad) fprintf(stderr, "--id-volume %s: expected I:J=G[,I:J=G...] with 0 <= I <= J <= %d ids\n", idvol_arg, t);
      vol.gain = r.id_gain; vol.t = t;
      if (!bad && piper_hip_volume_check(&vol) < 0) { /* a gain outside [0, 16] */
        fprintf(stderr, "--id-volume %s: %s\n", idvol_arg, piper_hip_last_error());
        bad = 1;
      }
      if (bad) { /* leave as the success path does */
        free(r.id_gain);
        piper_hip_voice_destroy(r.voice);
        piper_hip_destroy(ctx);
        return 2;
      }
    }
    const char* pitch_arg = arg_value(argc, argv, "--pitch");
    if (pitch_arg) { /* one shift for every sentence, or one per sentence; the tempo kept unless --pitch-varispeed */
      const int keep = !has_flag(argc, argv, "--pitch-varispeed");
      int k = 0, bad = 0;
      for (const char* s = pitch_arg; !bad;) {
        char* end = NULL;
        const float st = strtof(s, &end);
        if (end == s || k == PIPER_HIP_JOIN_MAX_ITEMS) { bad = 1; break; }
        r.pitch[k].semitones = st; r.pitch[k].keep_tempo = keep;
        k++;
        if (*end == '/') s = end + 1;
        else { bad = *end != 0; break; }
      }
      if (!bad && k != 1 && k != n_lists) bad = 1;
      if (bad) { fprintf(stderr, "--pitch %s: expected ST or ST/ST/... with one value per sentence (%d)\n", pitch_arg, n_lists); return 2; }
      for (; k < n_lists; k++) r.pitch[k] = r.pitch[0];
      r.n_pitch = n_lists;
      for (int i = 0; i < r.n_pitch; i++)
        if (piper_hip_pitch_check(&r.pitch[i]) < 0) { fprintf(stderr, "--pitch %s: %s\n", pitch_arg, piper_hip_last_error()); return 2; }
    }
    const char* sil_arg = arg_value(argc, argv, "--sentence-silence");
    const char* trim_arg = arg_value(argc, argv, "--trim-silence");
    if (n_lists > 1 || sil_arg || trim_arg || arg_value(argc, argv, "--lead-ms") || arg_value(argc, argv, "--tail-ms")) {
      /* the programme: the sentences as one batch, joined, converted and resampled on the device */
      piper_hip_join jn;
      void* pcm = NULL;
      int failed = 0;
      memset(&jn, 0, sizeof jn);
      jn.gap_ms = sil_arg ? (float)(atof(sil_arg) * 1000.0) : 0.0f;
      jn.lead_ms = arg_value(argc, argv, "--lead-ms") ? (float)atof(arg_value(argc, argv, "--lead-ms")) : 0.0f;
      jn.tail_ms = arg_value(argc, argv, "--tail-ms") ? (float)atof(arg_value(argc, argv, "--tail-ms")) : 0.0f;
      if (trim_arg) {
        jn.trim = 1;
        if (sscanf(trim_arg, "%f:%f:%f", &jn.trim_threshold, &jn.trim_pad_ms, &jn.fade_ms) < 1) {
          fprintf(stderr, "--trim-silence %s: expected THRESHOLD[:PAD_MS[:FADE_MS]]\n", trim_arg);
          return 2;
        }
      }
      if (piper_hip_join_check(&jn, NULL, 0) < 0) { fprintf(stderr, "%s\n", piper_hip_last_error()); return 2; }
      if (idvol_arg) { fprintf(stderr, "--id-volume is for a single sentence without a join\n"); return 2; }
      const int prc = run_programme(&r, ids, list_off, list_len, n_lists, &jn, &prm, cfg.sample_rate, rate, law, &pcm, &n);
      if (prc < 0) {
        fprintf(stderr, "the programme failed (%d): %s\n", prc, piper_hip_last_error());
        failed = 1;
      } else {
        (void)piper_hip_voice_last_gpu_ms(r.voice, 0, &gpu);
        if (out && (law ? piper_hip_wav_write_g711(out, law, (const uint8_t*)pcm, (size_t)n, rate)
                        : piper_hip_wav_write_pcm16(out, (const int16_t*)pcm, (size_t)n, rate)) < 0) {
          fprintf(stderr, "cannot write %s: %s\n", out, piper_hip_last_error());
          failed = 1;
        }
        if (out_raw && !failed) {
          FILE* fr = fopen(out_raw, "wb");
          failed = !fr || fwrite(pcm, law ? 1 : sizeof(int16_t), (size_t)n, fr) != (size_t)n;
          if (fr && fclose(fr) != 0) failed = 1;
          if (failed) fprintf(stderr, "cannot write %s\n", out_raw);
        }
        if (!failed)
          fprintf(stderr, "%d sentences, %lld samples (%.3f s at %d Hz) as %s, %.3f ms on the GPU -> %s\n", n_lists, (long long)n, (double)n / rate, rate,
                  enc ? enc : "s16le", gpu, out_raw ? out_raw : out);
      }
      free(pcm);
      free(r.id_gain);
      piper_hip_voice_destroy(r.voice);
      piper_hip_destroy(ctx);
      return failed;
    }
    if (out) {
      CHECK(run_one(&r, ids, t, &n));
      CHECK(piper_hip_voice_last_gpu_ms(r.voice, 0, &gpu));
      if (law) { /* the slot that ran, companded (and resampled) on the device */
        void* wg = NULL;
        int wrc = run_one_pcm16(&r, ids, t, &prm, 1, cfg.sample_rate, rate, law, &wg, &n);
        if (wrc >= 0) wrc = piper_hip_wav_write_g711(out, law, (const uint8_t*)wg, (size_t)n, rate);
        free(wg); /* after a failure too */
        CHECK(wrc);
      } else if (rate == cfg.sample_rate) {
        CHECK(piper_hip_wav_write(out, r.audio, (size_t)n, cfg.sample_rate));
      } else { /* the slot that ran, resampled and converted on the device */
        void* wpcm = NULL;
        int wrc = run_one_pcm16(&r, ids, t, NULL, 1, cfg.sample_rate, rate, 0, &wpcm, &n);
        if (wrc >= 0) wrc = piper_hip_wav_write_pcm16(out, (const int16_t*)wpcm, (size_t)n, rate);
        free(wpcm); /* after a failure too */
        CHECK(wrc);
      }
      fprintf(stderr, "%lld samples (%.3f s at %d Hz), %.3f ms on the GPU -> %s\n", (long long)n, (double)n / rate, rate, gpu, out);
    }
    if (out_raw) { /* s16le or G.711 bytes, the samples converted on the device */
      void* pcm = NULL;
      int failed = 0;
      const int prc = run_one_pcm16(&r, ids, t, &prm, out != NULL, cfg.sample_rate, rate, law, &pcm, &n);
      if (prc < 0) {
        fprintf(stderr, "--output-raw failed (%d): %s\n", prc, piper_hip_last_error());
        failed = 1;
      } else {
        (void)piper_hip_voice_last_gpu_ms(r.voice, 0, &gpu);
        FILE* fr = fopen(out_raw, "wb");
        failed = !fr || fwrite(pcm, law ? 1 : sizeof(int16_t), (size_t)n, fr) != (size_t)n;
        if (fr && fclose(fr) != 0) failed = 1;
        if (failed) fprintf(stderr, "cannot write %s\n", out_raw);
        else fprintf(stderr, "%lld samples (%.3f s at %d Hz) as %s, %.3f ms on the GPU -> %s\n", (long long)n, (double)n / rate, rate, enc ? enc : "s16le", gpu, out_raw);
      }
      free(pcm);
      if (failed) { /* leave as the success path does */
        free(r.audio);
        piper_hip_voice_destroy(r.voice);
        piper_hip_destroy(ctx);
        return 1;
      }
    }
    if (loud_arg) { /* what the device measured on the utterance that ran, and the gain it applied */
      float lufs = 0.0f, g = 1.0f;
      CHECK(piper_hip_voice_loudness(r.voice, 0, &lufs, &g, 1));
      fprintf(stderr, "loudness %.4f LUFS, gain %.6g\n", (double)lufs, (double)g);
    }
    free(r.audio);
    free(r.id_gain);
    piper_hip_voice_destroy(r.voice);
    piper_hip_destroy(ctx);
    return 0;
  }

  const int warmup = arg_value(argc, argv, "--warmup") ? atoi(arg_value(argc, argv, "--warmup")) : 1;
  const int iters = arg_value(argc, argv, "--iters") ? atoi(arg_value(argc, argv, "--iters")) : 3;
  const int max_phonemes = arg_value(argc, argv, "--max-phonemes") ? atoi(arg_value(argc, argv, "--max-phonemes")) : 4096;
  int64_t factors[64];
  const int nf = parse_csv_i64(arg_value(argc, argv, "--scale-factors") ? arg_value(argc, argv, "--scale-factors") : "1,2,4,8,16", factors, 64);
  if (nf < 1 || iters < 1 || warmup < 0 || max_phonemes < 1 || max_phonemes > 4096) { fprintf(stderr, "bad --scale-factors / --iters / --warmup / --max-phonemes\n"); return 2; }
  const char* tenv = getenv("PIPER_BENCH_GPU_TIMING");
  const int want_timings = tenv && strcmp(tenv, "1") == 0;

  printf("{\n  \"backend\": \"piper-hip\",\n  \"base_test_phonemes\": 14,\n  \"iters\": %d,\n  \"max_phonemes\": %d,\n  \"mode\": \"scale-bench\",\n  \"model_path\": \"%s\",\n  \"results\": [\n",
         iters, max_phonemes, model ? model : synthetic_names[preset]);
  int64_t* ids = (int64_t*)malloc(sizeof(int64_t) * 4096);
  double* wall = (double*)malloc(sizeof(double) * (size_t)iters);
  for (int fi = 0; fi < nf; fi++) {
    const int f = factors[fi] < 1 ? 1 : (int)factors[fi];
    long long want = 14LL * f;
    const int t = (int)(want > max_phonemes ? max_phonemes : want); /* tiled, then truncated at --max-phonemes (PiperCLI.swift:467-473) */
    for (int i = 0; i < t; i++) ids[i] = kFixture[i % 14];
    int64_t n = 0;
    for (int w = 0; w < warmup; w++) CHECK(run_one(&r, ids, t, &n));
    double gpu_sum = 0.0, user_sum = 0.0, sys_sum = 0.0, rss_max = 0.0;
    for (int it = 0; it < iters; it++) {
      struct rusage ru0, ru1;
      getrusage(RUSAGE_SELF, &ru0);
      const double t0 = now_ms();
      CHECK(run_one(&r, ids, t, &n));
      wall[it] = now_ms() - t0;
      getrusage(RUSAGE_SELF, &ru1);
      double g = 0.0;
      CHECK(piper_hip_voice_last_gpu_ms(r.voice, 0, &g));
      gpu_sum += g;
      user_sum += tv_ms(ru1.ru_utime) - tv_ms(ru0.ru_utime);
      sys_sum += tv_ms(ru1.ru_stime) - tv_ms(ru0.ru_stime);
      if ((double)ru1.ru_maxrss > rss_max) rss_max = (double)ru1.ru_maxrss;
    }
    double mean = 0.0, mx = 0.0;
    for (int it = 0; it < iters; it++) { mean += wall[it]; if (wall[it] > mx) mx = wall[it]; }
    mean /= iters;
    qsort(wall, (size_t)iters, sizeof(double), cmp_double);
    printf("    {\"factor\": %d, \"phoneme_count\": %d, \"ms_mean\": %.4f, \"ms_p50\": %.4f, \"ms_p95\": %.4f, \"ms_max\": %.4f", f, t, mean, percentile(wall, iters, 50.0),
           percentile(wall, iters, 95.0), mx);
    if (want_timings)
      printf(", \"gpu_ms_mean\": %.4f, \"cpu_user_ms_mean\": %.4f, \"cpu_sys_ms_mean\": %.4f, \"gpu_busy_fraction_mean\": %.4f, \"max_rss_max\": %.0f", gpu_sum / iters,
             user_sum / iters, sys_sum / iters, mean > 0.0 ? gpu_sum / iters / mean : 0.0, rss_max);
    /* beyond the reference's keys: what the audio was worth (audio-s per wall-s) */
    printf(", \"audio_sec\": %.4f, \"rtf_inv\": %.1f}%s\n", (double)n / cfg.sample_rate, mean > 0.0 ? (double)n / cfg.sample_rate / (mean * 1e-3) : 0.0, fi + 1 < nf ? "," : "");
  }
  printf("  ],\n  \"sample_rate\": %d,\n  \"scale_factors\": [", cfg.sample_rate);
  for (int fi = 0; fi < nf; fi++) printf("%s%lld", fi ? ", " : "", (long long)factors[fi]);
  printf("],\n  \"warmup\": %d\n}\n", warmup);
  free(ids); free(wall); free(r.audio);
  piper_hip_voice_destroy(r.voice);
  piper_hip_destroy(ctx);
  return 0;
}
