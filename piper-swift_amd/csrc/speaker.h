// speaker.h — internal interface of the speaker-row kernel (speaker.hip; piper_hip.h "Multi-speaker voices").
#pragma once
#include "common.h"

namespace ph {

// What piper_hip_voice_attach_speakers leaves on the device: the table and, row for row in speaker-row order, the cond weights, the
// cond biases and the conditioned convs' own biases.
struct SpeakerTables {
  const float* emb = nullptr;    // [S][gin]
  const float* w = nullptr;      // [Ctot][gin]
  const float* bc = nullptr;     // [Ctot] cond bias
  const float* b_own = nullptr;  // [Ctot] bias of the conv the row conditions
  int S = 0, gin = 0, Ctot = 0;
};

// Rows [row0, row0 + rows) of the speaker rows of N items in ONE launch: per item g = Σ_k w_k · emb[id_k] from spk[i] (a
// piper_hip_speaker in device memory; n and the ids are clamped to the table, so a stale or zeroed record reads legal memory), then
// e[c] = b_own[c] + (bc[c] + W[c]·g) → bias_out[i·Ctot + c]. g_out (optional) [N][gin] receives g.
int launch_speaker_rows(hipStream_t s, const SpeakerTables& t, const piper_hip_speaker* spk, int N, int row0, int rows, float* g_out,
                        float* bias_out);

}  // namespace ph
