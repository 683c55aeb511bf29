// PiperHIPRuntime — PiperMetalRuntime (Sources/PiperMetal/PiperMetalRuntime.swift:62-115 in the reference) over the voice-level C-ABI:
// one static schedule replayed as a HIP graph per request instead of a 2 755-node interpreted walk. UNTESTED GLUE (see Package.swift).
import CPiperHIP
import Foundation

/// Piper's four published qualities, numbered as piper_hip_voice_config_preset numbers them. low and xLow are the 16 kHz tier: low is the
/// medium geometry at 16 000 Hz, xLow has 96 channels (two heads of head_dim 48) in front of the medium generator.
public enum PiperHIPQuality: Int32, CaseIterable {
    case medium = 0, high = 1, low = 2, xLow = 3

    /// The name Piper's voice list and `voice.onnx.json` ("audio.quality") use: "medium", "high", "low", "x_low".
    public var name: String { ["medium", "high", "low", "x_low"][Int(rawValue)] }
    public init?(name: String) {
        guard let q = PiperHIPQuality.allCases.first(where: { $0.name == name }) else { return nil }
        self = q
    }

    /// The geometry of the quality (piper_hip_voice_config_preset): what piper_hip_onnx_infer_config returns for a voice of that quality.
    public func config() throws -> piper_hip_voice_config {
        var cfg = piper_hip_voice_config()
        try HIPBackend.check(piper_hip_voice_config_preset(rawValue, &cfg))
        return cfg
    }
}

public final class PiperHIPRuntime {
    private let backend: HIPBackend
    private var voice: OpaquePointer?
    public let sampleRate: Int32
    public let hop: Int

    /// A Piper voice file: the ONNX loader (host-only C++) infers the geometry, folds weight norm and lays the weights out in the order
    /// of include/piper_hip_voice_layout.h; `voice.onnx.json` supplies the sample rate (PiperConfig.swift:3-47).
    /// `speakers: true` takes a multi-speaker voice (`emb_g` + cond convs) instead of refusing it: the speaker table is loaded and attached
    /// (piper_hip_voice_attach_speakers) and `slotSpeakers` chooses who speaks. No verifier for the conditioned graph exists yet, so the
    /// weights of such a file are taken unchecked (piper_hip_onnx_build_blob_unchecked): the caller vouches that it is a standard Piper VITS.
    public init(modelPath: String, device: Int32 = 0, speakers: Bool = false) throws {
        backend = try HIPBackend(device: device)
        var model: OpaquePointer?
        try HIPBackend.check(piper_hip_onnx_open(modelPath, &model))
        defer { piper_hip_onnx_close(model) }
        var cfg = piper_hip_voice_config()
        var scfg = piper_hip_speaker_config()
        if speakers {
            try HIPBackend.check(piper_hip_onnx_infer_config_speakers(model, &cfg))
            try HIPBackend.check(piper_hip_onnx_speaker_config(model, &cfg, &scfg))   // n_speakers = 0: a single-speaker file
        } else {
            try HIPBackend.check(piper_hip_onnx_infer_config(model, &cfg))
        }
        if let json = try? String(contentsOfFile: modelPath + ".json", encoding: .utf8) {
            var info = piper_hip_piper_json_info()
            try HIPBackend.check(piper_hip_piper_json(json, &info))
            if scfg.n_speakers > 0 {
                try HIPBackend.check(piper_hip_voice_check_json_speakers(&cfg, &scfg, &info))   // num_speakers == table rows
            } else {
                try HIPBackend.check(piper_hip_voice_check_json(&cfg, &info))   // num_symbols vs n_vocab, single speaker
            }
            cfg.sample_rate = info.sample_rate
        }
        var n = 0
        try HIPBackend.check(piper_hip_voice_blob_floats(&cfg, &n))
        var blob = [Float](repeating: 0, count: n)
        if scfg.n_speakers > 0 {
            try HIPBackend.check(piper_hip_onnx_build_blob_unchecked(model, &cfg, &blob, n))
        } else {
            try HIPBackend.check(piper_hip_onnx_build_blob(model, &cfg, &blob, n))
        }
        try HIPBackend.check(piper_hip_voice_create(backend.ctx, &cfg, blob, 0, &voice))
        if scfg.n_speakers > 0 {                                               // before the voice's first prepare
            var sn = 0
            try HIPBackend.check(piper_hip_speaker_blob_floats(&cfg, &scfg, &sn))
            var sblob = [Float](repeating: 0, count: sn)
            try HIPBackend.check(piper_hip_onnx_build_speaker_blob(model, &cfg, &scfg, &sblob, sn))
            try HIPBackend.check(piper_hip_voice_attach_speakers(voice, &scfg, sblob, 0))
        }
        sampleRate = cfg.sample_rate
        var h = 1                                                              // hop = Π upsample rates (256 for Piper)
        withUnsafeBytes(of: &cfg.up_rates) { r in for i in 0..<Int(cfg.n_ups) { h *= Int(r.load(fromByteOffset: 4 * i, as: Int32.self)) } }
        hop = h
    }
    deinit { piper_hip_voice_destroy(voice) }

    /// Rows of the voice's speaker table; 0 for a single-speaker voice (piper_hip_voice_num_speakers).
    public var numSpeakers: Int32 { piper_hip_voice_num_speakers(voice) }

    /// The speakers of a slot's items from now on (piper_hip_voice_slot_speakers) — the graph's `sid`, read by PiperMetalRuntime.synthesize
    /// next to the scales (PiperMetalRuntime.swift:62-80). Entry i is for item i of every later prepare / stream begin on the slot (a pool
    /// join: of its work slot), the last entry for items past the list, an empty list = speaker 0 alone again. An entry is a mix of one to
    /// four (id, weight) pairs: g = Σ weight · emb_g[id]; [(id, 1)] is the plain speaker id.
    public func slotSpeakers(slot: Int32, speakers: [[(id: Int32, weight: Float)]]) throws {
        var recs = speakers.map { mix -> piper_hip_speaker in
            var s = piper_hip_speaker()
            s.n = Int32(mix.count)                                             // outside 1 … 4: refused by the library
            withUnsafeMutableBytes(of: &s.ids) { p in for (k, e) in mix.prefix(4).enumerated() { p.storeBytes(of: e.id, toByteOffset: 4 * k, as: Int32.self) } }
            withUnsafeMutableBytes(of: &s.weights) { p in for (k, e) in mix.prefix(4).enumerated() { p.storeBytes(of: e.weight, toByteOffset: 4 * k, as: Float.self) } }
            return s
        }
        try HIPBackend.check(piper_hip_voice_slot_speakers(voice, slot, &recs, Int32(recs.count)))
    }
    public func slotSpeaker(slot: Int32, id: Int32) throws { try slotSpeakers(slot: slot, speakers: [[(id: id, weight: 1.0)]]) }

    /// Per-phoneme prosody of one utterance (piper_hip_prosody): multipliers on the id's duration and on noise_scale, a floor (a pause) and a
    /// ceiling (0 = none) on the id's frames — nil = neutral — and `fit` (bounded routes: compress to the bound instead of failing). The
    /// reference shapes an utterance with the three scales alone (PiperMetalRuntime.swift:62-80).
    public struct Prosody {
        public var length: [Float]?
        public var minFrames: [Int32]?
        public var maxFrames: [Int32]?
        public var noise: [Float]?
        public var count: Int32
        public var fit: Bool
        public init(count: Int32, length: [Float]? = nil, minFrames: [Int32]? = nil, maxFrames: [Int32]? = nil, noise: [Float]? = nil, fit: Bool = false) {
            self.count = count; self.length = length; self.minFrames = minFrames; self.maxFrames = maxFrames; self.noise = noise; self.fit = fit
        }
    }

    /// The record over copies of the arrays that live until `body` returns (the library copies them inside slot_prosody).
    private static func withRecords<R>(_ items: [Prosody], _ body: ([piper_hip_prosody]) throws -> R) rethrows -> R {
        var keepF: [UnsafeMutablePointer<Float>] = [], keepI: [UnsafeMutablePointer<Int32>] = []
        defer { keepF.forEach { $0.deallocate() }; keepI.forEach { $0.deallocate() } }
        func floats(_ a: [Float]?) -> UnsafePointer<Float>? {
            guard let a = a else { return nil }
            let p = UnsafeMutablePointer<Float>.allocate(capacity: max(a.count, 1)); p.initialize(from: a, count: a.count); keepF.append(p)
            return UnsafePointer(p)
        }
        func ints(_ a: [Int32]?) -> UnsafePointer<Int32>? {
            guard let a = a else { return nil }
            let p = UnsafeMutablePointer<Int32>.allocate(capacity: max(a.count, 1)); p.initialize(from: a, count: a.count); keepI.append(p)
            return UnsafePointer(p)
        }
        let recs = items.map { piper_hip_prosody(length: floats($0.length), min_frames: ints($0.minFrames), max_frames: ints($0.maxFrames),
                                                 noise: floats($0.noise), t: $0.count, fit: $0.fit ? 1 : 0) }
        return try body(recs)
    }

    /// piper_hip_prosody_check: throws naming the field and the index of the first violation.
    public static func prosodyCheck(_ p: Prosody) throws {
        try withRecords([p]) { recs in var r = recs[0]; try HIPBackend.check(piper_hip_prosody_check(&r)) }
    }

    /// piper_hip_prosody_frames: the integer frame rule from w0 = exp(logw)·length_scale on (host only) → (frames per id, wanted = Σ before fitting).
    public static func prosodyFrames(_ p: Prosody?, w0: [Float], cap: Int64 = 0) throws -> (frames: [Int32], wanted: Int64) {
        var out = [Int32](repeating: 0, count: w0.count)
        var wanted: Int64 = 0
        try withRecords(p.map { [$0] } ?? []) { recs in
            if var r = recs.first {
                try HIPBackend.check(piper_hip_prosody_frames(&r, w0, Int32(w0.count), cap, &out, &wanted))
            } else {
                try HIPBackend.check(piper_hip_prosody_frames(nil, w0, Int32(w0.count), cap, &out, &wanted))   // no record: neutral
            }
        }
        return (out, wanted)
    }

    /// The prosody of the NEXT staging call on the slot id (piper_hip_voice_slot_prosody): entry i for item i of prepare*, stream_begin*,
    /// synthesize* (slot 0) or a pool join (its work slot). The staging call takes the assignment whether or not it succeeds; an empty list clears it.
    public func slotProsody(slot: Int32, items: [Prosody]) throws {
        try PiperHIPRuntime.withRecords(items) { recs in
            var r = recs
            try HIPBackend.check(piper_hip_voice_slot_prosody(voice, slot, &r, Int32(r.count)))
        }
    }

    /// The volume of the NEXT staging call on the slot id (piper_hip_voice_slot_volume): entry i holds item i's linear gains per id in
    /// [0, 16] (nil: all 1.0, `counts[i]` ids), for prepare*, stream_begin*, synthesize* (slot 0) or a pool join (its work slot). The staging
    /// call takes the assignment whether or not it succeeds; an empty list clears it.
    public func slotVolume(slot: Int32, items: [[Float]?], counts: [Int32]) throws {
        var keep: [UnsafeMutablePointer<Float>] = []
        defer { keep.forEach { $0.deallocate() } }
        var recs: [piper_hip_volume] = []
        for (i, g) in items.enumerated() {
            guard let g = g else { recs.append(piper_hip_volume(gain: nil, t: counts[i])); continue }
            let p = UnsafeMutablePointer<Float>.allocate(capacity: max(g.count, 1)); p.initialize(from: g, count: g.count); keep.append(p)
            recs.append(piper_hip_volume(gain: UnsafePointer(p), t: Int32(g.count)))
        }
        try HIPBackend.check(piper_hip_voice_slot_volume(voice, slot, &recs, Int32(recs.count)))
    }

    /// Per item of the slot: the frames the rule wanted before fitting, and whether the bounded route compressed the item to its bound
    /// (piper_hip_voice_prosody_report); answers where the durations are known.
    public func prosodyReport(slot: Int32) throws -> [(wanted: Int64, fitted: Bool)] {
        let n = Int(piper_hip_voice_batch_size(voice, slot))
        var wanted = [Int64](repeating: 0, count: max(n, 1)), fitted = [Int32](repeating: 0, count: max(n, 1))
        try HIPBackend.check(piper_hip_voice_prosody_report(voice, slot, &wanted, &fitted, Int32(n)))
        return (0..<n).map { (wanted[$0], fitted[$0] != 0) }
    }

    /// PiperMetalRuntime.synthesize(phonemeIDs:noiseScale:lengthScale:noiseW:) — the whole graph on the device: `durations == nil` ⇒ the
    /// voice's stochastic duration predictor runs (part of the plan's HIP graph); `noise_mode = DEVICE` ⇒ both RandomNormalLike tensors are
    /// drawn on the device with the reference's xorshift32 + Box-Muller generator (elementwise.metal:132-163) from `seed`.
    public func synthesize(phonemeIDs: [Int64], noiseScale: Float = 0.667, lengthScale: Float = 1.0, noiseW: Float = 0.8,
                           seed: UInt32 = 1234) throws -> [Float] {
        try phonemeIDs.withUnsafeBufferPointer { ids in
            var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: nil, noise: nil,
                                        noise_scale: noiseScale, noise_mode: Int32(PIPER_HIP_NOISE_DEVICE), seed: seed,
                                        length_scale: lengthScale, noise_w: noiseW, dp_noise: nil)
            try HIPBackend.check(piper_hip_voice_prepare(voice, &u, 0))          // predicts the durations, uploads the inputs
            var total: Int64 = 0
            try HIPBackend.check(piper_hip_voice_prepared_samples(voice, 0, nil, 0, &total))   // Σ predicted frames · hop
            var audio = [Float](repeating: 0, count: Int(total))
            try HIPBackend.check(piper_hip_voice_launch(voice, 0))
            try HIPBackend.check(piper_hip_voice_collect(voice, 0, &audio, total))
            return audio
        }
    }

    /// The same without the host round trip between the duration predictor and the flow (piper_hip_voice_prepare_batch_bounded): the caller bounds
    /// the frames (Piper voices stay below ≈ 6 frames per phoneme id at lengthScale 1), the plan is the bucket of that bound, generate_path runs on the
    /// device and the true length comes back with the waveform. Throws ExecutionError.shapeMismatch when the prediction exceeds the bound.
    public func synthesize(phonemeIDs: [Int64], maxFrames: Int, noiseScale: Float = 0.667, lengthScale: Float = 1.0, noiseW: Float = 0.8,
                           seed: UInt32 = 1234) throws -> [Float] {
        try phonemeIDs.withUnsafeBufferPointer { ids in
            var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: nil, noise: nil,
                                        noise_scale: noiseScale, noise_mode: Int32(PIPER_HIP_NOISE_DEVICE), seed: seed,
                                        length_scale: lengthScale, noise_w: noiseW, dp_noise: nil)
            try HIPBackend.check(piper_hip_voice_prepare_batch_bounded(voice, &u, 1, 0, Int32(maxFrames)))   // nothing waits for the GPU here
            try HIPBackend.check(piper_hip_voice_launch(voice, 0))
            var cap: Int64 = 0
            try HIPBackend.check(piper_hip_voice_prepared_samples(voice, 0, nil, 0, &cap))       // capacity: bucket(maxFrames) · hop
            var audio = [Float](repeating: 0, count: Int(cap))
            try HIPBackend.check(piper_hip_voice_collect(voice, 0, &audio, cap))
            var total: Int64 = 0
            try HIPBackend.check(piper_hip_voice_prepared_samples(voice, 0, nil, 0, &total))     // the true length now
            audio.removeLast(audio.count - Int(total))
            return audio
        }
    }

    /// The reference's `overrides` (GraphExecutor.swift:101-104): pinned durations and an injected noise tensor — the parity entry.
    public func synthesize(phonemeIDs: [Int64], durations: [Int32], noise: [Float]?, noiseScale: Float) throws -> [Float] {
        var n: Int64 = 0
        return try phonemeIDs.withUnsafeBufferPointer { ids in try durations.withUnsafeBufferPointer { dur in
            try (noise ?? []).withUnsafeBufferPointer { nz in
                var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: dur.baseAddress,
                                            noise: noise == nil ? nil : nz.baseAddress, noise_scale: noiseScale,
                                            noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234, length_scale: 1.0, noise_w: 0.8, dp_noise: nil)
                var audio = [Float](repeating: 0, count: Int(piper_hip_voice_num_samples(voice, &u)))
                try HIPBackend.check(piper_hip_voice_synthesize(voice, &u, &audio, Int64(audio.count), &n))
                return audio
            }
        } }
    }

    /// PiperMetalRuntime.synthesizeStream (PiperMetalRuntime.swift:82-115) with a generator that really decodes incrementally:
    /// encoder + flow once, then one HiFi-GAN window (chunk + receptive-field halo) per call.
    public func synthesizeStream(phonemeIDs: [Int64], durations: [Int32], noiseScale: Float, chunkFrames: Int32 = 64,
                                 onChunk: ([Float]) -> Void) throws {
        try phonemeIDs.withUnsafeBufferPointer { ids in try durations.withUnsafeBufferPointer { dur in
            var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: dur.baseAddress,
                                        noise: nil, noise_scale: noiseScale, noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234,
                                        length_scale: 1.0, noise_w: 0.8, dp_noise: nil)
            let chunks = piper_hip_voice_stream_begin(voice, &u, 0, chunkFrames)      // encoder + flow run here
            if chunks < 0 { try HIPBackend.check(chunks) }
            var buf = [Float](repeating: 0, count: Int(chunkFrames) * hop)
            var n: Int64 = 0
            repeat {
                try HIPBackend.check(piper_hip_voice_stream_next(voice, 0, &buf, Int64(buf.count), &n))
                if n > 0 { onChunk(Array(buf[0..<Int(n)])) }
            } while n > 0
        } }
    }

    /// Batched streaming (piper_hip_voice_stream_begin_batch): a group of utterances on one slot, encoder + flow once for the group, then
    /// every active item's next chunk in one generator launch per step. `onStep` receives one array per item (empty once it has finished);
    /// `durations[i] == nil` = predicted by the voice's duration predictor.
    public func synthesizeStreamBatch(phonemeIDs: [[Int64]], durations: [[Int32]?], noiseScale: Float, chunkFrames: Int32 = 64,
                                      slot: Int32 = 0, onStep: ([[Float]]) -> Void) throws {
        let n = phonemeIDs.count
        let ids = phonemeIDs.map { ContiguousArray($0) }
        let durs = durations.map { $0.map { ContiguousArray($0) } }
        var utts = [piper_hip_utterance]()
        var steps: Int32 = 0
        try withExtendedLifetime((ids, durs)) {
            for i in 0..<n {
                let ip = ids[i].withUnsafeBufferPointer { $0.baseAddress }       // storage kept alive by withExtendedLifetime
                let dp = durs[i]?.withUnsafeBufferPointer { $0.baseAddress }
                utts.append(piper_hip_utterance(phoneme_ids: ip, t: Int32(ids[i].count), durations: dp, noise: nil, noise_scale: noiseScale,
                                                noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234, length_scale: 1.0, noise_w: 0.8,
                                                dp_noise: nil))
            }
            steps = piper_hip_voice_stream_begin_batch(voice, &utts, Int32(n), slot, chunkFrames)   // encoder + flow of the group
            if steps < 0 { try HIPBackend.check(steps) }
        }
        var buf = [Float](repeating: 0, count: n * Int(chunkFrames) * hop)
        var counts = [Int64](repeating: 0, count: n)
        while true {
            try HIPBackend.check(piper_hip_voice_stream_next_batch(voice, slot, &buf, Int64(buf.count), &counts))
            if counts.allSatisfy({ $0 == 0 }) { return }
            var out = [[Float]](), off = 0
            for c in counts {
                out.append(Array(buf[off..<off + Int(c)]))
                off += Int(c)
            }
            onStep(out)
        }
    }

    /// The client of item `item` of the batched stream on `slot` went away: later steps skip it.
    public func streamDrop(slot: Int32, item: Int32) throws {
        try HIPBackend.check(piper_hip_voice_stream_drop(voice, slot, item))
    }

    /// A streaming pool (piper_hip_voice_stream_pool_open): `capacity` rows on `slot` that sessions join and leave while the stream runs.
    /// The pool itself has no counterpart in PiperMetalRuntime; the closest role is synthesizeStream.
    public func streamPoolOpen(slot: Int32, capacity: Int32, chunkFrames: Int32 = 64) throws {
        try HIPBackend.check(piper_hip_voice_stream_pool_open(voice, slot, capacity, chunkFrames))
    }

    /// New sessions for the pool on `slot`: encoder + flow run on `workSlot`, the latents move into free rows. Returns, per utterance, the
    /// row it took (its item id for streamPoolStep / streamDrop) and the samples it will deliver in all. `durations[i] == nil` = predicted.
    public func streamPoolJoin(slot: Int32, workSlot: Int32, phonemeIDs: [[Int64]], durations: [[Int32]?], noiseScale: Float,
                               seeds: [UInt32]? = nil) throws -> [(item: Int32, samples: Int64)] {
        let n = phonemeIDs.count
        let ids = phonemeIDs.map { ContiguousArray($0) }
        let durs = durations.map { $0.map { ContiguousArray($0) } }
        var utts = [piper_hip_utterance]()
        var items = [Int32](repeating: 0, count: n)
        var samples = [Int64](repeating: 0, count: n)
        try withExtendedLifetime((ids, durs)) {
            for i in 0..<n {
                let ip = ids[i].withUnsafeBufferPointer { $0.baseAddress }       // storage kept alive by withExtendedLifetime
                let dp = durs[i]?.withUnsafeBufferPointer { $0.baseAddress }
                utts.append(piper_hip_utterance(phoneme_ids: ip, t: Int32(ids[i].count), durations: dp, noise: nil, noise_scale: noiseScale,
                                                noise_mode: Int32(PIPER_HIP_NOISE_DEVICE), seed: seeds?[i] ?? 1234, length_scale: 1.0,
                                                noise_w: 0.8, dp_noise: nil))
            }
            try HIPBackend.check(piper_hip_voice_stream_pool_join(voice, slot, &utts, Int32(n), workSlot, &items, &samples))
        }
        return (0..<n).map { (items[$0], samples[$0]) }
    }

    /// The next chunk of every active session of the pool on `slot` (piper_hip_voice_stream_next_batch), keyed by item; empty = idle.
    public func streamPoolStep(slot: Int32, capacity: Int32, chunkFrames: Int32 = 64) throws -> [Int32: [Float]] {
        var buf = [Float](repeating: 0, count: Int(capacity) * Int(chunkFrames) * hop)
        var counts = [Int64](repeating: 0, count: Int(capacity))
        try HIPBackend.check(piper_hip_voice_stream_next_batch(voice, slot, &buf, Int64(buf.count), &counts))
        var out = [Int32: [Float]](), off = 0
        for (item, c) in counts.enumerated() where c > 0 {
            out[Int32(item)] = Array(buf[off..<off + Int(c)])
            off += Int(c)
        }
        return out
    }

    public func streamPoolFreeRows(slot: Int32) throws -> Int32 {
        let rc = piper_hip_voice_stream_pool_free_rows(voice, slot)
        if rc < 0 { try HIPBackend.check(rc) }
        return rc
    }

    public func streamPoolClose(slot: Int32) throws {
        try HIPBackend.check(piper_hip_voice_stream_pool_close(voice, slot))
    }

    // ---- 16-bit PCM converted on the device (include/piper_hip.h "16-bit PCM straight from the device") ----

    /// piper_hip_voice_collect_pcm16 on a launched slot: the items back to back as int16. normalize = false: the samples
    /// piper_hip_pcm16_from_f32 gives for what collect returns; true: Piper's peak normalisation per item (peaks(slot:) afterwards).
    public func collectPCM16(slot: Int32, gain: Float = 1.0, normalize: Bool = false) throws -> [Int16] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        var cap: Int64 = 0
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, nil, 0, &cap))      // a bounded slot: its capacity
        var pcm = [Int16](repeating: 0, count: Int(cap))
        try HIPBackend.check(piper_hip_voice_collect_pcm16(voice, slot, &prm, &pcm, cap))
        var total: Int64 = 0
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, nil, 0, &total))    // the true length now
        pcm.removeLast(pcm.count - Int(total))
        return pcm
    }

    /// synthesize(phonemeIDs:durations:noise:noiseScale:) ending in int16 (piper_hip_voice_synthesize_pcm16).
    public func synthesizePCM16(phonemeIDs: [Int64], durations: [Int32], noise: [Float]?, noiseScale: Float, gain: Float = 1.0,
                                normalize: Bool = false) throws -> [Int16] {
        var n: Int64 = 0
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        return try phonemeIDs.withUnsafeBufferPointer { ids in try durations.withUnsafeBufferPointer { dur in
            try (noise ?? []).withUnsafeBufferPointer { nz in
                var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: dur.baseAddress,
                                            noise: noise == nil ? nil : nz.baseAddress, noise_scale: noiseScale,
                                            noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234, length_scale: 1.0, noise_w: 0.8, dp_noise: nil)
                var pcm = [Int16](repeating: 0, count: Int(piper_hip_voice_num_samples(voice, &u)))
                try HIPBackend.check(piper_hip_voice_synthesize_pcm16(voice, &u, &prm, &pcm, Int64(pcm.count), &n))
                return pcm
            }
        } }
    }

    /// max |x| of each item of the slot after a collectPCM16(normalize: true) of its latest run.
    public func peaks(slot: Int32) throws -> [Float] {
        var out = [Float](repeating: 0, count: Int(piper_hip_voice_batch_size(voice, slot)))
        try HIPBackend.check(piper_hip_voice_peaks(voice, slot, &out, Int32(out.count)))
        return out
    }

    /// The next chunk of the single stream on `slot` as int16 (piper_hip_voice_stream_next_pcm16); empty at the end of the stream.
    public func streamNextPCM16(slot: Int32, chunkFrames: Int32 = 64, gain: Float = 1.0) throws -> [Int16] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [Int16](repeating: 0, count: Int(chunkFrames) * hop)
        var n: Int64 = 0
        try HIPBackend.check(piper_hip_voice_stream_next_pcm16(voice, slot, &prm, &buf, Int64(buf.count), &n))
        return Array(buf[0..<Int(n)])
    }

    /// The next chunk of every active item of the group (`rows` = its size) or pool (`rows` = its capacity) on `slot` as int16
    /// (piper_hip_voice_stream_next_batch_pcm16), keyed by item; empty = the group has ended / the pool is idle. Float and PCM steps may alternate.
    public func streamNextBatchPCM16(slot: Int32, rows: Int32, chunkFrames: Int32 = 64, gain: Float = 1.0) throws -> [Int32: [Int16]] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [Int16](repeating: 0, count: Int(rows) * Int(chunkFrames) * hop)
        var counts = [Int64](repeating: 0, count: Int(rows))
        try HIPBackend.check(piper_hip_voice_stream_next_batch_pcm16(voice, slot, &prm, &buf, Int64(buf.count), &counts))
        var out = [Int32: [Int16]](), off = 0
        for (item, c) in counts.enumerated() where c > 0 {
            out[Int32(item)] = Array(buf[off..<off + Int(c)])
            off += Int(c)
        }
        return out
    }

    // ---- Output rate: resampled to 8–48 kHz PCM on the device (include/piper_hip.h "Output rate") ----

    /// J(n): the samples `n` samples at the voice's rate yield at `rate` (piper_hip_resample_count).
    public func resampleCount(_ n: Int64, rate: Int32) throws -> Int64 {
        let j = piper_hip_resample_count(sampleRate, rate, n)
        if j < 0 { try HIPBackend.check(Int32(j)) }
        return j
    }

    /// collectPCM16 at `rate` (piper_hip_voice_collect_pcm16_rate): item b at J(its true samples), in any order with collect / collectPCM16.
    public func collectPCM16(slot: Int32, rate: Int32, gain: Float = 1.0, normalize: Bool = false) throws -> [Int16] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        let nb = Int(piper_hip_voice_batch_size(voice, slot))
        var per = [Int64](repeating: 0, count: max(nb, 1))
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, &per, Int32(nb), nil))   // a bounded slot: the capacity per item
        var cap: Int64 = 0
        for b in 0..<nb { cap += try resampleCount(per[b], rate: rate) }
        var pcm = [Int16](repeating: 0, count: Int(cap))
        try HIPBackend.check(piper_hip_voice_collect_pcm16_rate(voice, slot, &prm, rate, &pcm, cap))
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, &per, Int32(nb), nil))   // the true lengths now
        var total: Int64 = 0
        for b in 0..<nb { total += try resampleCount(per[b], rate: rate) }
        pcm.removeLast(pcm.count - Int(total))
        return pcm
    }

    /// synthesizePCM16 at `rate` (piper_hip_voice_synthesize_pcm16_rate).
    public func synthesizePCM16(phonemeIDs: [Int64], durations: [Int32], noise: [Float]?, noiseScale: Float, rate: Int32, gain: Float = 1.0,
                                normalize: Bool = false) throws -> [Int16] {
        var n: Int64 = 0
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        return try phonemeIDs.withUnsafeBufferPointer { ids in try durations.withUnsafeBufferPointer { dur in
            try (noise ?? []).withUnsafeBufferPointer { nz in
                var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: dur.baseAddress,
                                            noise: noise == nil ? nil : nz.baseAddress, noise_scale: noiseScale,
                                            noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234, length_scale: 1.0, noise_w: 0.8, dp_noise: nil)
                var pcm = [Int16](repeating: 0, count: Int(try resampleCount(piper_hip_voice_num_samples(voice, &u), rate: rate)))
                try HIPBackend.check(piper_hip_voice_synthesize_pcm16_rate(voice, &u, &prm, rate, &pcm, Int64(pcm.count), &n))
                return pcm
            }
        } }
    }

    /// The output rate of the stream on `slot` (piper_hip_voice_stream_set_rate): after its begin / open, before its first step (a pool:
    /// and its first join). The PCM steps then deliver at `rate`; the float steps are refused.
    public func streamSetRate(slot: Int32, rate: Int32) throws {
        try HIPBackend.check(piper_hip_voice_stream_set_rate(voice, slot, rate))
    }

    /// The level of slot id `slot`'s whole-item collects (piper_hip_voice_slot_level): it persists until replaced; nil clears it.
    public func slotLevel(slot: Int32, level: piper_hip_level?) throws {
        if var lv = level {
            try HIPBackend.check(piper_hip_voice_slot_level(voice, slot, &lv))
        } else {
            try HIPBackend.check(piper_hip_voice_slot_level(voice, slot, nil))
        }
    }

    /// The loudness target of slot id `slot`'s whole-item collects (piper_hip_voice_slot_loudness): it persists until replaced; nil
    /// clears it. Every later collect* and synthesize* on the slot id delivers the items at that BS.1770 loudness, in front of the level.
    public func slotLoudness(slot: Int32, loudness: piper_hip_loudness?) throws {
        if var ld = loudness {
            try HIPBackend.check(piper_hip_voice_slot_loudness(voice, slot, &ld))
        } else {
            try HIPBackend.check(piper_hip_voice_slot_loudness(voice, slot, nil))
        }
    }

    /// The equaliser of slot id `slot`'s whole-item collects (piper_hip_voice_slot_eq): it persists until replaced; nil clears it.
    /// Every later collect* and synthesize* on the slot id delivers the EQ'd items, behind the volume and in front of the loudness gain.
    public func slotEq(slot: Int32, eq: piper_hip_eq?) throws {
        if var e = eq {
            try HIPBackend.check(piper_hip_voice_slot_eq(voice, slot, &e))
        } else {
            try HIPBackend.check(piper_hip_voice_slot_eq(voice, slot, nil))
        }
    }

    /// Per item of the slot's latest launch: the integrated loudness of the raw samples, measured on the device, and the gain the
    /// slot's target implies, 1 without one (piper_hip_voice_loudness). Waits for the slot.
    public func loudness(slot: Int32) throws -> (lufs: [Float], gain: [Float]) {
        let n = Int(piper_hip_voice_batch_size(voice, slot))
        var lufs = [Float](repeating: 0, count: max(n, 1)), gain = lufs
        try HIPBackend.check(piper_hip_voice_loudness(voice, slot, &lufs, &gain, Int32(n)))
        return (Array(lufs[0..<n]), Array(gain[0..<n]))
    }

    /// The join of slot id `slot`'s whole-item collects (piper_hip_voice_slot_join): it persists until replaced; nil clears it. Every
    /// later collect* and synthesize* on the slot id delivers ONE programme: the items trimmed, faded and separated by silences.
    public func slotJoin(slot: Int32, join: piper_hip_join?, gaps: [Float] = []) throws {
        if var j = join {
            try HIPBackend.check(piper_hip_voice_slot_join(voice, slot, &j, gaps.isEmpty ? nil : gaps, Int32(gaps.count)))
        } else {
            try HIPBackend.check(piper_hip_voice_slot_join(voice, slot, nil, nil, 0))
        }
    }

    /// The samples a collect* of the prepared, joined slot needs room for at `outRate` (0: the voice's own) (piper_hip_voice_join_capacity).
    public func joinCapacity(slot: Int32, outRate: Int32 = 0) throws -> Int64 {
        var n: Int64 = 0
        try HIPBackend.check(piper_hip_voice_join_capacity(voice, slot, outRate, &n))
        return n
    }

    /// Where each item starts in the programme of the slot's latest joined collect, how long it is, and the total, at the voice's rate
    /// (piper_hip_voice_join_report).
    public func joinReport(slot: Int32) throws -> (start: [Int64], len: [Int64], total: Int64) {
        let nb = Int(piper_hip_voice_batch_size(voice, slot))
        var start = [Int64](repeating: 0, count: max(nb, 1)), len = [Int64](repeating: 0, count: max(nb, 1))
        var total: Int64 = 0
        try HIPBackend.check(piper_hip_voice_join_report(voice, slot, &start, &len, Int32(nb), &total))
        return (Array(start.prefix(nb)), Array(len.prefix(nb)), total)
    }

    /// The pitch of the NEXT staging call on slot id `slot` (piper_hip_voice_slot_pitch): entry i for item i, semitones in [−12, 12];
    /// keep_tempo 1 scales the predicted durations so that the item keeps its length, 0 is varispeed. For prepare* and synthesize*
    /// (slot 0); the staging call takes the assignment whether or not it succeeds; an empty list clears it. Streams refuse a pending pitch.
    public func slotPitch(slot: Int32, items: [piper_hip_pitch]) throws {
        try HIPBackend.check(piper_hip_voice_slot_pitch(voice, slot, items.isEmpty ? nil : items, Int32(items.count)))
    }

    /// The samples each item of the prepared slot delivers at the voice's rate, F'·hop under a pitch, and their sum
    /// (piper_hip_voice_pitch_samples): a bounded slot's capacity before collect, the true values after. Collect buffers hold the sum.
    public func pitchSamples(slot: Int32) throws -> (perItem: [Int64], total: Int64) {
        let nb = Int(piper_hip_voice_batch_size(voice, slot))
        var per = [Int64](repeating: 0, count: max(nb, 1))
        var total: Int64 = 0
        try HIPBackend.check(piper_hip_voice_pitch_samples(voice, slot, &per, Int32(nb), &total))
        return (Array(per.prefix(nb)), total)
    }

    /// The EQ of the stream on `slot` (piper_hip_voice_stream_set_eq): where streamSetLevel is allowed, in either order with it.
    public func streamSetEq(slot: Int32, eq: piper_hip_eq) throws {
        var e = eq
        try HIPBackend.check(piper_hip_voice_stream_set_eq(voice, slot, &e))
    }

    /// The EQ the stream on `slot` holds (piper_hip_voice_stream_eq).
    public func streamEq(slot: Int32) throws -> piper_hip_eq {
        var e = piper_hip_eq()
        try HIPBackend.check(piper_hip_voice_stream_eq(voice, slot, &e))
        return e
    }

    /// The level of the stream on `slot` (piper_hip_voice_stream_set_level): where streamSetRate is allowed, in either order with it.
    public func streamSetLevel(slot: Int32, level: piper_hip_level) throws {
        var lv = level
        try HIPBackend.check(piper_hip_voice_stream_set_level(voice, slot, &lv))
    }

    /// The level the stream on `slot` holds, defaults resolved (piper_hip_voice_stream_level).
    public func streamLevel(slot: Int32) throws -> piper_hip_level {
        var lv = piper_hip_level(drive: 0, ceiling: 0, release_ms: 0)
        try HIPBackend.check(piper_hip_voice_stream_level(voice, slot, &lv))
        return lv
    }

    public func streamRate(slot: Int32) throws -> Int32 {
        let r = piper_hip_voice_stream_rate(voice, slot)
        if r < 0 { try HIPBackend.check(r) }
        return r
    }

    /// The int16 samples one step of the stream on `slot` can deliver at its current rate (piper_hip_voice_stream_step_capacity).
    public func streamStepCapacity(slot: Int32) throws -> Int {
        let c = piper_hip_voice_stream_step_capacity(voice, slot)
        if c < 0 { try HIPBackend.check(Int32(c)) }
        return Int(c)
    }

    /// streamNextPCM16 / streamNextBatchPCM16 on a slot with an output rate: the buffer is sized by streamStepCapacity.
    public func streamNextPCM16AtRate(slot: Int32, gain: Float = 1.0) throws -> [Int16] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [Int16](repeating: 0, count: try streamStepCapacity(slot: slot))
        var n: Int64 = 0
        try HIPBackend.check(piper_hip_voice_stream_next_pcm16(voice, slot, &prm, &buf, Int64(buf.count), &n))
        return Array(buf[0..<Int(n)])
    }

    public func streamNextBatchPCM16AtRate(slot: Int32, rows: Int32, gain: Float = 1.0) throws -> [Int32: [Int16]] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [Int16](repeating: 0, count: try streamStepCapacity(slot: slot))
        var counts = [Int64](repeating: 0, count: Int(rows))
        try HIPBackend.check(piper_hip_voice_stream_next_batch_pcm16(voice, slot, &prm, &buf, Int64(buf.count), &counts))
        var out = [Int32: [Int16]](), off = 0
        for (item, c) in counts.enumerated() where c > 0 {
            out[Int32(item)] = Array(buf[off..<off + Int(c)])
            off += Int(c)
        }
        return out
    }

    // ---- G.711 output: μ-law / A-law bytes companded on the device (include/piper_hip.h "G.711 output") ----

    /// collectPCM16 ending in G.711 bytes (piper_hip_voice_collect_g711; law = PIPER_HIP_G711_MULAW or _ALAW) at `rate` (nil: the voice's
    /// own): item b at J(its true samples), in any order with collect / collectPCM16.
    public func collectG711(slot: Int32, law: Int32, rate: Int32? = nil, gain: Float = 1.0, normalize: Bool = false) throws -> [UInt8] {
        let r = rate ?? sampleRate
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        let nb = Int(piper_hip_voice_batch_size(voice, slot))
        var per = [Int64](repeating: 0, count: max(nb, 1))
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, &per, Int32(nb), nil))   // a bounded slot: the capacity per item
        var cap: Int64 = 0
        for b in 0..<nb { cap += r == sampleRate ? per[b] : try resampleCount(per[b], rate: r) }
        var bytes = [UInt8](repeating: 0, count: Int(cap))
        try HIPBackend.check(piper_hip_voice_collect_g711(voice, slot, &prm, law, r, &bytes, cap))
        try HIPBackend.check(piper_hip_voice_prepared_samples(voice, slot, &per, Int32(nb), nil))   // the true lengths now
        var total: Int64 = 0
        for b in 0..<nb { total += r == sampleRate ? per[b] : try resampleCount(per[b], rate: r) }
        bytes.removeLast(bytes.count - Int(total))
        return bytes
    }

    /// synthesizePCM16 ending in G.711 bytes (piper_hip_voice_synthesize_g711).
    public func synthesizeG711(phonemeIDs: [Int64], durations: [Int32], noise: [Float]?, noiseScale: Float, law: Int32, rate: Int32? = nil,
                               gain: Float = 1.0, normalize: Bool = false) throws -> [UInt8] {
        let r = rate ?? sampleRate
        var n: Int64 = 0
        var prm = piper_hip_pcm_params(gain: gain, normalize: normalize ? 1 : 0)
        return try phonemeIDs.withUnsafeBufferPointer { ids in try durations.withUnsafeBufferPointer { dur in
            try (noise ?? []).withUnsafeBufferPointer { nz in
                var u = piper_hip_utterance(phoneme_ids: ids.baseAddress, t: Int32(ids.count), durations: dur.baseAddress,
                                            noise: noise == nil ? nil : nz.baseAddress, noise_scale: noiseScale,
                                            noise_mode: Int32(PIPER_HIP_NOISE_INJECTED), seed: 1234, length_scale: 1.0, noise_w: 0.8, dp_noise: nil)
                let samples = piper_hip_voice_num_samples(voice, &u)
                var bytes = [UInt8](repeating: 0, count: Int(r == sampleRate ? samples : try resampleCount(samples, rate: r)))
                try HIPBackend.check(piper_hip_voice_synthesize_g711(voice, &u, &prm, law, r, &bytes, Int64(bytes.count), &n))
                return bytes
            }
        } }
    }

    /// The next chunk of the single stream on `slot` as G.711 bytes (piper_hip_voice_stream_next_g711), at the slot's rate; empty at the
    /// end of the stream. The law is an argument of the step: PCM and G.711 steps may alternate.
    public func streamNextG711(slot: Int32, law: Int32, gain: Float = 1.0) throws -> [UInt8] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [UInt8](repeating: 0, count: try streamStepCapacity(slot: slot))
        var n: Int64 = 0
        try HIPBackend.check(piper_hip_voice_stream_next_g711(voice, slot, &prm, law, &buf, Int64(buf.count), &n))
        return Array(buf[0..<Int(n)])
    }

    /// The next chunk of every active item of a group or pool as G.711 bytes (piper_hip_voice_stream_next_batch_g711), keyed by item.
    public func streamNextBatchG711(slot: Int32, rows: Int32, law: Int32, gain: Float = 1.0) throws -> [Int32: [UInt8]] {
        var prm = piper_hip_pcm_params(gain: gain, normalize: 0)
        var buf = [UInt8](repeating: 0, count: try streamStepCapacity(slot: slot))
        var counts = [Int64](repeating: 0, count: Int(rows))
        try HIPBackend.check(piper_hip_voice_stream_next_batch_g711(voice, slot, &prm, law, &buf, Int64(buf.count), &counts))
        var out = [Int32: [UInt8]](), off = 0
        for (item, c) in counts.enumerated() where c > 0 {
            out[Int32(item)] = Array(buf[off..<off + Int(c)])
            off += Int(c)
        }
        return out
    }

    // ---- mixed formats (include/piper_hip.h "Mixed formats"): every row of a group or pool in its own rate, encoding and gain

    /// Marks the batched stream on `slot` mixed (piper_hip_voice_stream_set_mixed): right after streamBeginBatch / streamPoolOpen.
    public func streamSetMixed(slot: Int32) throws {
        try HIPBackend.check(piper_hip_voice_stream_set_mixed(voice, slot))
    }

    /// The formats of a mixed group's items, before its first step (piper_hip_voice_stream_item_formats); items past the list take the last.
    public func streamItemFormats(slot: Int32, formats: [piper_hip_stream_format]) throws {
        try HIPBackend.check(piper_hip_voice_stream_item_formats(voice, slot, formats, Int32(formats.count)))
    }

    /// The format of item / row `item` of a mixed slot as the library holds it (piper_hip_voice_stream_item_format).
    public func streamItemFormat(slot: Int32, item: Int32) throws -> piper_hip_stream_format {
        var f = piper_hip_stream_format(out_rate: 0, encoding: 0, gain: 0)
        try HIPBackend.check(piper_hip_voice_stream_item_format(voice, slot, item, &f))
        return f
    }

    /// The bytes one step of the mixed slot can deliver with the rows' current formats (piper_hip_voice_stream_step_capacity_bytes).
    public func streamStepCapacityBytes(slot: Int32) throws -> Int {
        let n = piper_hip_voice_stream_step_capacity_bytes(voice, slot)
        if n < 0 { try HIPBackend.check(Int32(n)) }
        return Int(n)
    }

    /// streamPoolJoin on a mixed pool with one format per utterance (piper_hip_voice_stream_pool_join_formats).
    public func streamPoolJoin(slot: Int32, workSlot: Int32, phonemeIDs: [[Int64]], durations: [[Int32]?], noiseScale: Float,
                               formats: [piper_hip_stream_format], seeds: [UInt32]? = nil) throws -> [(item: Int32, samples: Int64)] {
        let n = phonemeIDs.count
        precondition(formats.count == n, "one format per utterance")
        let ids = phonemeIDs.map { ContiguousArray($0) }
        let durs = durations.map { $0.map { ContiguousArray($0) } }
        var utts = [piper_hip_utterance]()
        var items = [Int32](repeating: 0, count: n)
        var samples = [Int64](repeating: 0, count: n)
        try withExtendedLifetime((ids, durs)) {
            for i in 0..<n {
                let ip = ids[i].withUnsafeBufferPointer { $0.baseAddress }       // storage kept alive by withExtendedLifetime
                let dp = durs[i]?.withUnsafeBufferPointer { $0.baseAddress }
                utts.append(piper_hip_utterance(phoneme_ids: ip, t: Int32(ids[i].count), durations: dp, noise: nil, noise_scale: noiseScale,
                                                noise_mode: Int32(PIPER_HIP_NOISE_DEVICE), seed: seeds?[i] ?? 1234, length_scale: 1.0,
                                                noise_w: 0.8, dp_noise: nil))
            }
            try HIPBackend.check(piper_hip_voice_stream_pool_join_formats(voice, slot, &utts, Int32(n), workSlot, formats, &items, &samples))
        }
        return (0..<n).map { (items[$0], samples[$0]) }
    }

    // ---- bounded pool joins (include/piper_hip.h "Streaming pool: joins with predicted durations that never wait")

    /// streamPoolJoin for utterances whose durations are predicted, without the host round trip
    /// (piper_hip_voice_stream_pool_join_bounded): at most `maxFrames` frames per item, nothing waits for the GPU. `formats`: one per
    /// utterance on a mixed pool, nil otherwise. Returns the rows taken; streamPoolItemSamples tells what each will deliver.
    public func streamPoolJoinBounded(slot: Int32, workSlot: Int32, phonemeIDs: [[Int64]], maxFrames: Int32, noiseScale: Float,
                                      formats: [piper_hip_stream_format]? = nil, seeds: [UInt32]? = nil) throws -> [Int32] {
        let n = phonemeIDs.count
        precondition(formats == nil || formats!.count == n, "one format per utterance")
        let ids = phonemeIDs.map { ContiguousArray($0) }
        var utts = [piper_hip_utterance]()
        var items = [Int32](repeating: 0, count: n)
        try withExtendedLifetime(ids) {
            for i in 0..<n {
                let ip = ids[i].withUnsafeBufferPointer { $0.baseAddress }       // storage kept alive by withExtendedLifetime
                utts.append(piper_hip_utterance(phoneme_ids: ip, t: Int32(ids[i].count), durations: nil, noise: nil, noise_scale: noiseScale,
                                                noise_mode: Int32(PIPER_HIP_NOISE_DEVICE), seed: seeds?[i] ?? 1234, length_scale: 1.0,
                                                noise_w: 0.8, dp_noise: nil))
            }
            if let f = formats {
                try HIPBackend.check(piper_hip_voice_stream_pool_join_bounded(voice, slot, &utts, Int32(n), workSlot, maxFrames, f, &items))
            } else {
                try HIPBackend.check(piper_hip_voice_stream_pool_join_bounded(voice, slot, &utts, Int32(n), workSlot, maxFrames, nil, &items))
            }
        }
        return items
    }

    /// Total samples the occupant of row `item` will deliver, at the row's rate (piper_hip_voice_stream_pool_item_samples); waits for the
    /// join that filled the row if it is still running. Throws the shape error for a bounded item the predictor made longer than its bound.
    public func streamPoolItemSamples(slot: Int32, item: Int32) throws -> Int64 {
        var n: Int64 = 0
        try HIPBackend.check(piper_hip_voice_stream_pool_item_samples(voice, slot, item, &n))
        return n
    }

    /// Joins of the pool whose encoder + flow have not finished yet (piper_hip_voice_stream_pool_joins_pending); never waits.
    public func streamPoolJoinsPending(slot: Int32) throws -> Int32 {
        let rc = piper_hip_voice_stream_pool_joins_pending(voice, slot)
        if rc < 0 { try HIPBackend.check(rc) }
        return rc
    }

    /// The step of a mixed group or pool (piper_hip_voice_stream_next_batch_mixed): per delivering item / row its chunk as raw bytes —
    /// int16 or float32 in host order, or G.711 bytes, by the row's format (streamItemFormat). Empty = end / idle.
    public func streamNextBatchMixed(slot: Int32, rows: Int32) throws -> [Int32: [UInt8]] {
        var buf = [UInt8](repeating: 0, count: max(try streamStepCapacityBytes(slot: slot), 4))
        var counts = [Int64](repeating: 0, count: Int(rows))
        var offs = [Int64](repeating: 0, count: Int(rows))
        // the element sizes are read before the step: a pool row whose session delivers its last chunk is free afterwards
        let elems: [Int] = (0..<rows).map { r in
            guard let f = try? streamItemFormat(slot: slot, item: r) else { return 0 }  // a free pool row
            return f.encoding == PIPER_HIP_ENC_F32 ? 4 : f.encoding == PIPER_HIP_ENC_S16 ? 2 : 1
        }
        try HIPBackend.check(piper_hip_voice_stream_next_batch_mixed(voice, slot, &buf, Int64(buf.count), &counts, &offs))
        var out = [Int32: [UInt8]]()
        for (item, c) in counts.enumerated() where c > 0 {
            out[Int32(item)] = Array(buf[Int(offs[item])..<Int(offs[item]) + Int(c) * elems[item]])
        }
        return out
    }

    /// A mono G.711 WAV (format tag 7 / 6, fact chunk) from bytes that are companded already (piper_hip_wav_write_g711).
    public func writeWav(g711 bytes: [UInt8], law: Int32, rate: Int32, to path: String) throws {
        try HIPBackend.check(piper_hip_wav_write_g711(path, law, bytes, bytes.count, rate))
    }

    /// A mono WAV from samples that are 16-bit PCM already, at the rate they were delivered (piper_hip_wav_write_pcm16).
    public func writeWav(pcm: [Int16], rate: Int32, to path: String) throws {
        try HIPBackend.check(piper_hip_wav_write_pcm16(path, pcm, pcm.count, rate))
    }

    /// WavFileWriter (Sources/PiperCLI/WavFileWriter.swift:20-60): float → int16 with the CLI's x·32767 clamp, RIFF header.
    public func writeWav(_ samples: [Float], to path: String) throws {
        try HIPBackend.check(piper_hip_wav_write(path, samples, samples.count, sampleRate))
    }
}
