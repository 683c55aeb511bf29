// HIPBackend — MetalBackend's per-operator surface (Sources/PiperMetal/Execution/MetalBackend.swift:8-3427 in the reference) over
// the C-ABI of include/piper_hip.h: every method of the Python twin (piper_hip.HipBackend, which the test-suite drives) under the
// reference's method names and argument labels. UNCOMPILED GLUE in this pipeline (no Swift toolchain in the image, SURVEY F5).
import CPiperHIP
import Foundation

/// The reference's error cases (CPUBackend.swift:3-17), so a GraphExecutor arm can catch the same things.
public enum ExecutionError: Error {
    case unsupportedOp(String)
    case typeMismatch(String)
    case shapeMismatch(String)
    case metalUnavailable(String)
}

/// MTLBuffer stand-in: a device pointer owned by the context's pool (freed on deinit, like ARC on MTLBuffer).
public final class HIPBuffer {
    public let ptr: UnsafeMutableRawPointer
    private let ctx: OpaquePointer
    init(_ p: UnsafeMutableRawPointer, ctx: OpaquePointer) { self.ptr = p; self.ctx = ctx }
    deinit { piper_hip_free(ctx, ptr) }
    var f32: UnsafeMutablePointer<Float> { ptr.assumingMemoryBound(to: Float.self) }
}

public final class HIPBackend {
    public let ctx: OpaquePointer

    public init(device: Int32 = 0) throws {
        var c: OpaquePointer?
        try HIPBackend.check(piper_hip_create(device, &c))           // MetalContext.init, MetalContext.swift:9-33
        ctx = c!
    }
    deinit { piper_hip_destroy(ctx) }

    /// int status + thread-local message → the ExecutionError cases of CPUBackend.swift:3-17
    public static func check(_ rc: Int32) throws {
        guard rc != 0 else { return }
        let msg = String(cString: piper_hip_last_error())
        switch rc {
        case -1: throw ExecutionError.shapeMismatch(msg)
        case -2: throw ExecutionError.typeMismatch(msg)
        case -3: throw ExecutionError.unsupportedOp(msg)
        case -4: throw ExecutionError.metalUnavailable(msg)
        default: throw NSError(domain: "HIPBackend", code: Int(rc), userInfo: [NSLocalizedDescriptionKey: msg])
        }
    }

    public func makeCommandBuffer() throws -> UnsafeMutableRawPointer {      // MetalBackend.swift:841-843
        var s: UnsafeMutableRawPointer?
        try Self.check(piper_hip_stream_create(ctx, &s)); return s!
    }
    public func flush(_ cmd: UnsafeMutableRawPointer) throws { try Self.check(piper_hip_stream_sync(ctx, cmd)) }   // :845-855

    public func uploadFloat32(_ data: [Float]) throws -> HIPBuffer {         // MetalBackend.swift:983-993
        var out: UnsafeMutablePointer<Float>?
        try data.withUnsafeBufferPointer { try Self.check(piper_hip_upload_f32(ctx, $0.baseAddress, $0.count, &out)) }
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }
    public func downloadFloat32(_ buf: HIPBuffer, count: Int) throws -> [Float] {   // MetalBackend.swift:963-981
        var host = [Float](repeating: 0, count: count)
        try Self.check(piper_hip_download_f32(ctx, buf.f32, &host, count))
        return host
    }

    /// MetalBackend.conv1dF32 (MetalBackend.swift:1149-1161) — same labels, `commandBuffer:` is a HIP stream or nil.
    public func conv1dF32(input: HIPBuffer, inputShape: [Int], weight: HIPBuffer, weightShape: [Int], bias: HIPBuffer?,
                          stride: Int, dilation: Int, padL: Int, padR: Int, groups: Int,
                          commandBuffer: UnsafeMutableRawPointer? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        guard inputShape.count == 3 else { throw ExecutionError.shapeMismatch("conv1dF32 input must be [N,C,L]") }
        guard weightShape.count == 3 else { throw ExecutionError.shapeMismatch("conv1dF32 weight must be [C_out,C_in,K]") }
        var p = piper_hip_conv1d_params(stride: Int32(stride), dilation: Int32(dilation), pad_l: Int32(padL),
                                        pad_r: Int32(padR), groups: Int32(groups))
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 3)
        try Self.check(piper_hip_conv1d_f32(ctx, input.f32, inputShape.map(Int64.init), weight.f32, weightShape.map(Int64.init),
                                            bias?.f32, &p, &out, &oshape, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), oshape.map(Int.init))
    }

    /// MetalBackend.convTranspose1dF32 (MetalBackend.swift:2812-2895)
    public func convTranspose1dF32(input: HIPBuffer, inputShape: [Int], weight: HIPBuffer, weightShape: [Int], bias: HIPBuffer?,
                                   stride: Int, dilation: Int, padL: Int, padR: Int, outputPadding: Int, groups: Int,
                                   commandBuffer: UnsafeMutableRawPointer? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var p = piper_hip_convtranspose1d_params(stride: Int32(stride), dilation: Int32(dilation), pad_l: Int32(padL), pad_r: Int32(padR),
                                                 output_padding: Int32(outputPadding), groups: Int32(groups))
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 3)
        try Self.check(piper_hip_convtranspose1d_f32(ctx, input.f32, inputShape.map(Int64.init), weight.f32, weightShape.map(Int64.init),
                                                     bias?.f32, &p, &out, &oshape, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), oshape.map(Int.init))
    }

    /// The fused attention core the reference spells as 4 MatMuls + Pad/Reshape/Slice skews + Softmax per layer (GraphExecutor.swift:1862-1929)
    public func relAttentionF32(q: HIPBuffer, k: HIPBuffer, v: HIPBuffer, embRelK: HIPBuffer, embRelV: HIPBuffer, batch: Int, heads: Int,
                                headDim: Int, length: Int, window: Int,
                                commandBuffer: UnsafeMutableRawPointer? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_rel_attention_f32(ctx, q.f32, k.f32, v.f32, embRelK.f32, embRelV.f32, Int64(batch), Int64(heads), Int64(headDim),
                                                   Int64(length), Int64(window), &out, commandBuffer))
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }
    // ---- shared plumbing of the wrappers below ----
    public typealias Stream = UnsafeMutableRawPointer

    private func wrap(_ p: UnsafeMutablePointer<Float>?) -> HIPBuffer { HIPBuffer(UnsafeMutableRawPointer(p!), ctx: ctx) }
    private static func i64(_ a: [Int]) -> [Int64] { a.map(Int64.init) }

    /// MetalBackend.allocateBuffer(length:) (MetalBackend.swift:34-39): `length` BYTES of device memory (≥ 1 byte, like the reference)
    public func allocateBuffer(length: Int) throws -> HIPBuffer {
        var p: UnsafeMutableRawPointer? = nil
        try Self.check(piper_hip_alloc(ctx, max(1, length), &p))
        return HIPBuffer(p!, ctx: ctx)
    }

    /// MetalBackend.matmulF32 (MetalBackend.swift:1232-1323). `useTiledKernel` is accepted for source compatibility and ignored: there is one
    /// kernel. Equal ranks ≥ 2; lead dims equal or 1-broadcast (the executor's expandF32, GraphExecutor.swift:1870-1899, is not needed).
    public func matmulF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], useTiledKernel: Bool = false,
                          commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        guard aShape.count == bShape.count, aShape.count >= 2 else { throw ExecutionError.shapeMismatch("matmulF32 needs equal ranks >= 2") }
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: aShape.count)
        try Self.check(piper_hip_matmul_f32(ctx, a.f32, Self.i64(aShape), b.f32, Self.i64(bShape), Int32(aShape.count), &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }

    /// MetalBackend.softmaxLastDimF32 (MetalBackend.swift:1326-1355)
    public func softmaxLastDimF32(input: HIPBuffer, shape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_softmax_lastdim_f32(ctx, input.f32, Self.i64(shape), Int32(shape.count), &out, commandBuffer))
        return (wrap(out), shape)
    }

    /// MetalBackend.reduceMeanLastDimF32 (MetalBackend.swift:1357-1390): [.., C] → [.., 1]
    public func reduceMeanLastDimF32(input: HIPBuffer, shape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_reduce_mean_lastdim_f32(ctx, input.f32, Self.i64(shape), Int32(shape.count), &out, commandBuffer))
        return (wrap(out), Array(shape.dropLast()) + [1])
    }

    // ---- unary (MetalBackend.swift:1501-1586) ----
    private func unaryF32(_ op: piper_hip_unary_op, input: HIPBuffer, count: Int, alpha: Float = 0, commandBuffer: Stream?) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_unary_f32(ctx, op, input.f32, count, alpha, &out, commandBuffer))
        return wrap(out)
    }
    public func reluF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_RELU, input: input, count: count, commandBuffer: commandBuffer) }
    public func erfF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_ERF, input: input, count: count, commandBuffer: commandBuffer) }
    public func softplusF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_SOFTPLUS, input: input, count: count, commandBuffer: commandBuffer) }
    public func negF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_NEG, input: input, count: count, commandBuffer: commandBuffer) }
    public func expF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_EXP, input: input, count: count, commandBuffer: commandBuffer) }
    public func ceilF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_CEIL, input: input, count: count, commandBuffer: commandBuffer) }
    public func tanhF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_TANH, input: input, count: count, commandBuffer: commandBuffer) }
    public func sigmoidF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_SIGMOID, input: input, count: count, commandBuffer: commandBuffer) }
    public func sqrtF32(input: HIPBuffer, count: Int, commandBuffer: Stream? = nil) throws -> HIPBuffer { try unaryF32(PIPER_HIP_SQRT, input: input, count: count, commandBuffer: commandBuffer) }
    public func leakyReluF32(input: HIPBuffer, count: Int, alpha: Float, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        try unaryF32(PIPER_HIP_LEAKYRELU, input: input, count: count, alpha: alpha, commandBuffer: commandBuffer)
    }

    /// `count` device floats → `count` int16 on the device (piper_hip_pcm16_f32): x · gain, clamp to [−1, 1], × 32767 in double, truncate —
    /// the samples WavFileWriter.swift:20-30 writes. The buffer holds int16 (`count` · 2 bytes).
    public func pcm16F32(input: HIPBuffer, count: Int, gain: Float = 1.0, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Int16>? = nil
        try Self.check(piper_hip_pcm16_f32(ctx, input.f32, count, gain, &out, commandBuffer))
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }

    /// `count` device floats at inRate → J(count) device floats at outRate (piper_hip_resample_f32): the fp32 y of the output-rate contract.
    public func resampleF32(input: HIPBuffer, count: Int, inRate: Int32, outRate: Int32, commandBuffer: Stream? = nil) throws -> (HIPBuffer, Int) {
        var out: UnsafeMutablePointer<Float>? = nil
        var n = 0
        try Self.check(piper_hip_resample_f32(ctx, input.f32, count, inRate, outRate, &out, &n, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), n)
    }

    /// The same ending in int16 (piper_hip_resample_pcm16_f32): y · gain through pcm16F32's arithmetic. The buffer holds J(count) int16.
    public func resamplePcm16F32(input: HIPBuffer, count: Int, inRate: Int32, outRate: Int32, gain: Float = 1.0,
                                 commandBuffer: Stream? = nil) throws -> (HIPBuffer, Int) {
        var out: UnsafeMutablePointer<Int16>? = nil
        var n = 0
        try Self.check(piper_hip_resample_pcm16_f32(ctx, input.f32, count, inRate, outRate, gain, &out, &n, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), n)
    }

    /// `count` device floats at inRate → J(count) G.711 bytes at outRate on the device (piper_hip_g711_f32; law = PIPER_HIP_G711_MULAW or
    /// _ALAW): law(int16 of y · gain). inRate == outRate is not a filter. The buffer holds J(count) bytes.
    public func g711F32(input: HIPBuffer, count: Int, law: Int32, inRate: Int32, outRate: Int32, gain: Float = 1.0,
                        commandBuffer: Stream? = nil) throws -> (HIPBuffer, Int) {
        var out: UnsafeMutablePointer<UInt8>? = nil
        var n = 0
        try Self.check(piper_hip_g711_f32(ctx, input.f32, count, inRate, outRate, gain, law, &out, &n, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), n)
    }

    /// int16 samples → G.711 bytes and back on the host (piper_hip_g711_from_pcm16 / _to_pcm16): the function the device applies.
    public static func g711Encode(_ pcm: [Int16], law: Int32) throws -> [UInt8] {
        var out = [UInt8](repeating: 0, count: pcm.count)
        try check(piper_hip_g711_from_pcm16(law, pcm, pcm.count, &out))
        return out
    }

    public static func g711Decode(_ bytes: [UInt8], law: Int32) throws -> [Int16] {
        var out = [Int16](repeating: 0, count: bytes.count)
        try check(piper_hip_g711_to_pcm16(law, bytes, bytes.count, &out))
        return out
    }

    /// (L, M, taps per phase) of a rate pair and its [L][P] coefficient table (piper_hip_resample_info / _taps; host-only).
    public static func resampleInfo(inRate: Int32, outRate: Int32) throws -> (l: Int32, m: Int32, taps: Int32) {
        var l: Int32 = 0, m: Int32 = 0, p: Int32 = 0
        try check(piper_hip_resample_info(inRate, outRate, &l, &m, &p))
        return (l, m, p)
    }

    public static func resampleTaps(inRate: Int32, outRate: Int32) throws -> [Float] {
        let i = try resampleInfo(inRate: inRate, outRate: outRate)
        var t = [Float](repeating: 0, count: Int(i.l) * Int(i.taps))
        try check(piper_hip_resample_taps(inRate, outRate, &t, t.count))
        return t
    }

    /// The most samples one stream row delivers in a step over `n` input samples (piper_hip_resample_step_bound; host-only).
    public static func resampleStepBound(inRate: Int32, outRate: Int32, n: Int64) throws -> Int64 {
        let b = piper_hip_resample_step_bound(inRate, outRate, n)
        if b < 0 { try check(Int32(b)) }
        return b
    }

    // ---- per-phoneme volume (include/piper_hip.h "Per-phoneme volume") ----

    /// `frames`·`hop` device floats under the envelope of the device gains per frame (piper_hip_volume_f32).
    public func volumeF32(input: HIPBuffer, frameGain: HIPBuffer, frames: Int64, hop: Int32, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_volume_f32(ctx, input.f32, Int(frames) * Int(hop), frameGain.f32, frames, hop, &out, commandBuffer))
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }

    /// The envelope on the host (piper_hip_volume_from_f32), bit for bit what the device computes: x [frames·hop] under the gains per frame.
    public static func volumeFromF32(_ x: [Float], frameGain: [Float], hop: Int32) throws -> [Float] {
        var y = [Float](repeating: 0, count: x.count)
        try check(piper_hip_volume_from_f32(frameGain, Int64(frameGain.count), hop, x, x.count, &y))
        return y
    }

    /// The gain of every frame of an item whose ids last `durations` frames (piper_hip_volume_frames; host-only). gains nil: all 1.0.
    public static func volumeFrames(gains: [Float]?, durations: [Int32]) throws -> [Float] {
        var frames: Int64 = 0
        func run(_ out: UnsafeMutablePointer<Float>?, _ cap: Int64) throws {
            if let g = gains {
                try g.withUnsafeBufferPointer { gp in
                    var rec = piper_hip_volume(gain: gp.baseAddress, t: Int32(g.count))
                    try check(piper_hip_volume_frames(&rec, durations, Int32(durations.count), out, cap, &frames))
                }
            } else {
                try check(piper_hip_volume_frames(nil, durations, Int32(durations.count), out, cap, &frames))
            }
        }
        try run(nil, 0)
        var gf = [Float](repeating: 0, count: Int(frames))
        try gf.withUnsafeMutableBufferPointer { try run($0.baseAddress, frames) }
        return gf
    }

    /// InvalidArgument naming the field and the index for gains outside [0, 16] (piper_hip_volume_check; host-only).
    public static func volumeCheck(gains: [Float]) throws {
        try gains.withUnsafeBufferPointer { gp in
            var rec = piper_hip_volume(gain: gp.baseAddress, t: Int32(gains.count))
            try check(piper_hip_volume_check(&rec))
        }
    }

    // ---- level control (include/piper_hip.h "Level control") ----

    /// `count` device floats sampled at `rate` → `count` limited device floats (piper_hip_level_f32): the look-ahead limiter.
    public func levelF32(input: HIPBuffer, count: Int, rate: Int32, level: piper_hip_level, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        var lv = level
        try Self.check(piper_hip_level_f32(ctx, input.f32, count, rate, &lv, &out, commandBuffer))
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }

    /// The limiter on the host (piper_hip_level_from_f32), bit for bit what the device computes.
    public static func levelFromF32(_ x: [Float], level: piper_hip_level, rate: Int32) throws -> [Float] {
        var lv = level
        var y = [Float](repeating: 0, count: x.count)
        try check(piper_hip_level_from_f32(&lv, rate, x, x.count, &y))
        return y
    }

    /// InvalidArgument naming the field for a level outside the contract (piper_hip_level_check; host-only).
    public static func levelCheck(_ level: piper_hip_level) throws {
        var lv = level
        try check(piper_hip_level_check(&lv))
    }

    /// The fp32 release step per block of `level` at `rate` (piper_hip_level_info; host-only).
    public static func levelInfo(_ level: piper_hip_level, rate: Int32) throws -> Float {
        var lv = level
        var rel: Float = 0
        try check(piper_hip_level_info(&lv, rate, &rel))
        return rel
    }

    /// The limited samples that are final when samples [0, e) of a longer item are known (piper_hip_level_ready; host-only).
    public static func levelReady(_ e: Int64) throws -> Int64 {
        let r = piper_hip_level_ready(e)
        if r < 0 { try check(Int32(r)) }
        return r
    }

    /// The most limited samples one stream row delivers in a step over `n` input samples (piper_hip_level_step_bound; host-only).
    public static func levelStepBound(_ n: Int64) throws -> Int64 {
        let b = piper_hip_level_step_bound(n)
        if b < 0 { try check(Int32(b)) }
        return b
    }

    // ---- loudness (include/piper_hip.h "Loudness") ----

    /// `count` device floats sampled at `rate` → their BS.1770 integrated loudness in LUFS, measured on the device
    /// (piper_hip_loudness_f32); −∞ for an item too short to measure. The call blocks: the value is final when it returns.
    public func loudnessF32(input: HIPBuffer, count: Int, rate: Int32) throws -> Float {
        var lufs: Float = 0
        try Self.check(piper_hip_loudness_f32(ctx, input.f32, count, rate, &lufs, nil))
        return lufs
    }

    /// BS.1770 integrated loudness of host floats (piper_hip_loudness_from_f32): the sequential double twin of the kernels.
    public static func loudnessFromF32(_ x: [Float], rate: Int32) throws -> Float {
        var lufs: Float = 0
        try check(piper_hip_loudness_from_f32(rate, x, x.count, &lufs))
        return lufs
    }

    /// InvalidArgument naming the field for a loudness target outside the contract (piper_hip_loudness_check; host-only).
    public static func loudnessCheck(_ loudness: piper_hip_loudness) throws {
        var ld = loudness
        try check(piper_hip_loudness_check(&ld))
    }

    /// The K-weighting biquads at `rate`, three coefficients each, a[0] = 1 (piper_hip_loudness_coeffs; host-only).
    public static func loudnessCoeffs(rate: Int32) throws -> (shelfB: [Double], shelfA: [Double], hpB: [Double], hpA: [Double]) {
        var sb = [Double](repeating: 0, count: 3), sa = sb, hb = sb, ha = sb
        try check(piper_hip_loudness_coeffs(rate, &sb, &sa, &hb, &ha))
        return (sb, sa, hb, ha)
    }

    /// The fp32 gain `loudness` implies for an item measured at `lufs` (piper_hip_loudness_gain; host-only); 1 for −∞.
    public static func loudnessGain(_ loudness: piper_hip_loudness, lufs: Float) throws -> Float {
        var ld = loudness
        var g: Float = 1
        try check(piper_hip_loudness_gain(&ld, lufs, &g))
        return g
    }

    // ---- equaliser (include/piper_hip.h "Equaliser") ----

    /// `count` device floats sampled at `rate` → the same number of EQ'd device floats (piper_hip_eq_f32): up to four biquads in double,
    /// bit for bit the host twin.
    public func eqF32(input: HIPBuffer, count: Int, rate: Int32, eq: piper_hip_eq, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        var e = eq
        try Self.check(piper_hip_eq_f32(ctx, input.f32, count, rate, &e, &out, commandBuffer))
        return HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx)
    }

    /// The equaliser on the host (piper_hip_eq_from_f32), bit for bit what the device computes.
    public static func eqFromF32(_ x: [Float], eq: piper_hip_eq, rate: Int32) throws -> [Float] {
        var e = eq
        var y = [Float](repeating: 0, count: x.count)
        try check(piper_hip_eq_from_f32(&e, rate, x, x.count, &y))
        return y
    }

    /// InvalidArgument naming the field and the section for an EQ outside the contract at `rate` (piper_hip_eq_check; host-only).
    public static func eqCheck(_ eq: piper_hip_eq, rate: Int32) throws {
        var e = eq
        try check(piper_hip_eq_check(&e, rate))
    }

    /// {b0, b1, b2, a1, a2} of every section in use (piper_hip_eq_design; host-only).
    public static func eqDesign(_ eq: piper_hip_eq, rate: Int32) throws -> [[Double]] {
        var e = eq
        var rows = [(Double, Double, Double, Double, Double)](repeating: (0, 0, 0, 0, 0), count: Int(PIPER_HIP_EQ_MAX_SECTIONS))
        try check(piper_hip_eq_design(&e, rate, &rows))
        return rows.prefix(Int(max(0, min(eq.n, PIPER_HIP_EQ_MAX_SECTIONS)))).map { [$0.0, $0.1, $0.2, $0.3, $0.4] }
    }

    // ---- join (include/piper_hip.h "Join") ----

    /// Items of device floats (item i at input[itemOff[i] ..< itemOff[i] + itemLen[i]]) → ONE programme in device memory
    /// (piper_hip_join_f32): trimmed, faded, with silences; bit for bit the host twin. Waits for the device: the report is its answer.
    public func joinF32(input: HIPBuffer, itemOff: [Int64], itemLen: [Int64], rate: Int32, join: piper_hip_join, gaps: [Float] = [],
                        commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, start: [Int64], len: [Int64], total: Int64) {
        var out: UnsafeMutablePointer<Float>? = nil
        var j = join
        var start = [Int64](repeating: 0, count: itemOff.count), len = [Int64](repeating: 0, count: itemOff.count)
        var total: Int64 = 0
        try Self.check(piper_hip_join_f32(ctx, input.f32, itemOff, itemLen, Int32(itemOff.count), rate, &j, gaps.isEmpty ? nil : gaps,
                                          Int32(gaps.count), &out, &start, &len, &total, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), start, len, total)
    }

    /// The join on the host (piper_hip_join_from_f32), bit for bit what the device computes.
    public static func joinFromF32(_ x: [Float], itemOff: [Int64], itemLen: [Int64], rate: Int32, join: piper_hip_join,
                                   gaps: [Float] = []) throws -> (programme: [Float], start: [Int64], len: [Int64]) {
        var j = join
        var cap: Int64 = 0
        try check(piper_hip_join_capacity(&j, gaps.isEmpty ? nil : gaps, Int32(gaps.count), rate, itemLen, Int32(itemLen.count), &cap))
        var y = [Float](repeating: 0, count: Int(max(cap, 1)))
        var start = [Int64](repeating: 0, count: itemOff.count), len = [Int64](repeating: 0, count: itemOff.count)
        var total: Int64 = 0
        try check(piper_hip_join_from_f32(&j, gaps.isEmpty ? nil : gaps, Int32(gaps.count), rate, x, itemOff, itemLen, Int32(itemOff.count), &y, cap,
                                          &start, &len, &total))
        return (Array(y.prefix(Int(total))), start, len)
    }

    /// InvalidArgument naming the field for a join outside the contract (piper_hip_join_check; host-only).
    public static func joinCheck(_ join: piper_hip_join, gaps: [Float] = []) throws {
        var j = join
        try check(piper_hip_join_check(&j, gaps.isEmpty ? nil : gaps, Int32(gaps.count)))
    }

    /// The S() sample counts of the join at `rate` (piper_hip_join_counts; host-only).
    public static func joinCounts(_ join: piper_hip_join, rate: Int32) throws -> (lead: Int64, gap: Int64, tail: Int64, pad: Int64, fade: Int64) {
        var j = join
        var c: (Int64, Int64, Int64, Int64, Int64) = (0, 0, 0, 0, 0)
        try check(piper_hip_join_counts(&j, rate, &c.0, &c.1, &c.2, &c.3, &c.4))
        return c
    }

    // ---- pitch (include/piper_hip.h "Pitch") ----

    /// `count` device floats → N' device floats shifted by `semitones` in [−12, 12] (piper_hip_pitch_f32): the variable-ratio resampler
    /// of the pitch contract, bit for bit the host twin; no padding.
    public func pitchF32(input: HIPBuffer, count: Int, semitones: Float, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, count: Int) {
        var out: UnsafeMutablePointer<Float>? = nil
        var n = 0
        try Self.check(piper_hip_pitch_f32(ctx, input.f32, count, semitones, &out, &n, commandBuffer))
        return (HIPBuffer(UnsafeMutableRawPointer(out!), ctx: ctx), n)
    }

    /// The pitch on the host (piper_hip_pitch_from_f32), bit for bit what the device computes.
    public static func pitchFromF32(_ x: [Float], semitones: Float) throws -> [Float] {
        let want = piper_hip_pitch_count(semitones, Int64(x.count))
        if want < 0 { try check(Int32(want)) }
        var y = [Float](repeating: 0, count: Int(max(want, 1)))
        var n = 0
        try check(piper_hip_pitch_from_f32(semitones, x, x.count, &y, Int(want), &n))
        return Array(y.prefix(n))
    }

    /// (Q, taps, length factor) of a shift: the 32.32 step, P and rf = (float)(Q / 2^32) (piper_hip_pitch_info; host-only).
    public static func pitchInfo(semitones: Float) throws -> (step: UInt64, taps: Int32, lengthFactor: Float) {
        var q: UInt64 = 0, p: Int32 = 0, f: Float = 0
        try check(piper_hip_pitch_info(semitones, &q, &p, &f))
        return (q, p, f)
    }

    /// N': the samples an item of `count` samples yields under a shift (piper_hip_pitch_count; host-only).
    public static func pitchCount(semitones: Float, count: Int64) throws -> Int64 {
        let n = piper_hip_pitch_count(semitones, count)
        if n < 0 { try check(Int32(n)) }
        return n
    }

    /// InvalidArgument naming the field for a pitch outside the contract (piper_hip_pitch_check; host-only).
    public static func pitchCheck(_ pitch: piper_hip_pitch) throws {
        var p = pitch
        try check(piper_hip_pitch_check(&p))
    }

    // ---- binary with NumPy broadcasting, output rank ≤ 4 (MetalBackend.swift:2099-2134, 2592-2610) ----
    private func binaryBroadcastF32(_ op: piper_hip_binary_op, a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int],
                                    commandBuffer: Stream?) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 4)
        var orank: Int32 = 0
        try Self.check(piper_hip_binary_broadcast_f32(ctx, op, a.f32, Self.i64(aShape), Int32(aShape.count), b.f32, Self.i64(bShape), Int32(bShape.count),
                                                      &out, &oshape, &orank, commandBuffer))
        return (wrap(out), oshape.prefix(Int(orank)).map(Int.init))
    }
    public func addF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try binaryBroadcastF32(PIPER_HIP_ADD, a: a, aShape: aShape, b: b, bShape: bShape, commandBuffer: commandBuffer)
    }
    public func subF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try binaryBroadcastF32(PIPER_HIP_SUB, a: a, aShape: aShape, b: b, bShape: bShape, commandBuffer: commandBuffer)
    }
    public func mulF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try binaryBroadcastF32(PIPER_HIP_MUL, a: a, aShape: aShape, b: b, bShape: bShape, commandBuffer: commandBuffer)
    }
    public func divF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try binaryBroadcastF32(PIPER_HIP_DIV, a: a, aShape: aShape, b: b, bShape: bShape, commandBuffer: commandBuffer)
    }
    public func powF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try binaryBroadcastF32(PIPER_HIP_POW, a: a, aShape: aShape, b: b, bShape: bShape, commandBuffer: commandBuffer)
    }

    // ---- layout ops of the skew and of the flow coupling ----
    /// MetalBackend.padConstantF32 (MetalBackend.swift:780-839): pads = [begin_0 … begin_{r-1}, end_0 … end_{r-1}], rank ≤ 4
    public func padConstantF32(input: HIPBuffer, shape: [Int], pads: [Int], constant: Float, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        guard pads.count == 2 * shape.count else { throw ExecutionError.shapeMismatch("padConstantF32: pads must hold 2·rank entries") }
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: shape.count)
        try Self.check(piper_hip_pad_constant_f32(ctx, input.f32, Self.i64(shape), Int32(shape.count), Self.i64(pads), constant, &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }
    /// MetalBackend.transposeF32 (MetalBackend.swift:995-1060)
    public func transposeF32(input: HIPBuffer, shape: [Int], perm: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: shape.count)
        try Self.check(piper_hip_transpose_f32(ctx, input.f32, Self.i64(shape), Int32(shape.count), perm.map(Int32.init), &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }
    /// One-axis slice with any non-zero step; the reference's family sliceAxis1NCLF32 / sliceAxis2NCLF32 / slice2DAxis1F32Step1 /
    /// sliceRank4Axis3F32Step1 / slice1DF32Step1 / reverseRank3Axis1F32 (MetalBackend.swift:1702-1980) are calls of this with their axis.
    public func sliceF32(input: HIPBuffer, shape: [Int], axis: Int, start: Int, end: Int, step: Int = 1, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: shape.count)
        try Self.check(piper_hip_slice_f32(ctx, input.f32, Self.i64(shape), Int32(shape.count), Int32(axis), Int64(start), Int64(end), Int64(step), &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }
    public func sliceAxis1NCLF32(input: HIPBuffer, shape: [Int], start: Int, step: Int, count: Int, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try sliceF32(input: input, shape: shape, axis: 1, start: start, end: start + step * count, step: step, commandBuffer: commandBuffer)   // :1702
    }
    public func sliceAxis2NCLF32(input: HIPBuffer, shape: [Int], start: Int, step: Int, count: Int, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try sliceF32(input: input, shape: shape, axis: 2, start: start, end: start + step * count, step: step, commandBuffer: commandBuffer)   // :1730
    }
    public func sliceRank4Axis3F32Step1(input: HIPBuffer, shape: [Int], start: Int, end: Int, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try sliceF32(input: input, shape: shape, axis: 3, start: start, end: end, commandBuffer: commandBuffer)                               // :1873
    }
    /// VITS `Flip`: reverse the channel axis of [N, C, L] (MetalBackend.swift:1803-1871)
    public func reverseRank3Axis1F32(input: HIPBuffer, shape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        try sliceF32(input: input, shape: shape, axis: 1, start: shape[1] - 1, end: -1, step: -1, commandBuffer: commandBuffer)
    }
    /// MetalBackend.concat2Axis1NCLF32 (MetalBackend.swift:1597-1641)
    public func concat2Axis1NCLF32(a: HIPBuffer, aShape: [Int], b: HIPBuffer, bShape: [Int], commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 3)
        try Self.check(piper_hip_concat2_axis1_f32(ctx, a.f32, Self.i64(aShape), b.f32, Self.i64(bShape), &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }
    /// MetalBackend.split2Axis1NCLF32 (MetalBackend.swift:1643-1700)
    public func split2Axis1NCLF32(input: HIPBuffer, inputShape: [Int], c0: Int, c1: Int, commandBuffer: Stream? = nil) throws
        -> (out0: HIPBuffer, out0Shape: [Int], out1: HIPBuffer, out1Shape: [Int]) {
        guard inputShape.count == 3, c0 + c1 == inputShape[1] else { throw ExecutionError.shapeMismatch("split2Axis1NCLF32: c0 + c1 must equal C") }
        var o0: UnsafeMutablePointer<Float>? = nil, o1: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_split2_axis1_f32(ctx, input.f32, Self.i64(inputShape), Int64(c0), &o0, &o1, commandBuffer))
        return (wrap(o0), [inputShape[0], c0, inputShape[2]], wrap(o1), [inputShape[0], c1, inputShape[2]])
    }
    /// MetalBackend.expandF32 (MetalBackend.swift:2438-2458)
    public func expandF32(input: HIPBuffer, inShape: [Int], outShape: [Int], commandBuffer: Stream? = nil) throws -> HIPBuffer {
        guard inShape.count == outShape.count else { throw ExecutionError.shapeMismatch("expandF32 needs equal ranks") }
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_expand_f32(ctx, input.f32, Self.i64(inShape), Self.i64(outShape), Int32(inShape.count), &out, commandBuffer))
        return wrap(out)
    }

    /// MetalBackend.randomNormalLike(shape:seed:) (MetalBackend.swift:3398-3426): the reference's xorshift32 + Box-Muller generator
    public func randomNormalLike(shape: [Int], seed: UInt64 = 1234, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_random_normal_like_f32(ctx, shape.reduce(1, *), seed, &out, commandBuffer))
        return wrap(out)
    }

    // ---- bf16-operand contractions (build extension; same contract as the f32 ones) ----
    public func conv1dBF16(input: HIPBuffer, inputShape: [Int], weight: HIPBuffer, weightShape: [Int], bias: HIPBuffer?, stride: Int, dilation: Int,
                           padL: Int, padR: Int, groups: Int, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var p = piper_hip_conv1d_params(stride: Int32(stride), dilation: Int32(dilation), pad_l: Int32(padL), pad_r: Int32(padR), groups: Int32(groups))
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 3)
        try Self.check(piper_hip_conv1d_bf16(ctx, input.f32, Self.i64(inputShape), weight.f32, Self.i64(weightShape), bias?.f32, &p, &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }
    public func convTranspose1dBF16(input: HIPBuffer, inputShape: [Int], weight: HIPBuffer, weightShape: [Int], bias: HIPBuffer?, stride: Int, dilation: Int,
                                    padL: Int, padR: Int, outputPadding: Int, groups: Int, commandBuffer: Stream? = nil) throws -> (out: HIPBuffer, outShape: [Int]) {
        var p = piper_hip_convtranspose1d_params(stride: Int32(stride), dilation: Int32(dilation), pad_l: Int32(padL), pad_r: Int32(padR),
                                                 output_padding: Int32(outputPadding), groups: Int32(groups))
        var out: UnsafeMutablePointer<Float>? = nil
        var oshape = [Int64](repeating: 0, count: 3)
        try Self.check(piper_hip_convtranspose1d_bf16(ctx, input.f32, Self.i64(inputShape), weight.f32, Self.i64(weightShape), bias?.f32, &p, &out, &oshape, commandBuffer))
        return (wrap(out), oshape.map(Int.init))
    }

    // ---- fused blocks (results equal the composition of the ops above; tests/test_gpu_ops.py) ----
    /// out = LN_c(x + y)·gamma + beta (the Add + ReduceMean … Div chain, GraphExecutor.swift:2071-2125); y may be nil
    public func addLayerNormF32(x: HIPBuffer, y: HIPBuffer?, gamma: HIPBuffer, beta: HIPBuffer, batch: Int, channels: Int, length: Int, eps: Float = 1e-5,
                                commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_add_layernorm_f32(ctx, x.f32, y?.f32, gamma.f32, beta.f32, Int64(batch), Int64(channels), Int64(length), eps, &out, commandBuffer))
        return wrap(out)
    }
    /// attention core + output projection + residual + LayerNorm of an encoder layer in one launch (PIPER_HIP_ERR_UNSUPPORTED outside its geometry)
    public func attentionBlockF32(q: HIPBuffer, k: HIPBuffer, v: HIPBuffer, embRelK: HIPBuffer, embRelV: HIPBuffer, wO: HIPBuffer, bO: HIPBuffer, x: HIPBuffer,
                                  gamma: HIPBuffer, beta: HIPBuffer, batch: Int, heads: Int, headDim: Int, length: Int, window: Int, eps: Float = 1e-5,
                                  commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_attention_block_f32(ctx, q.f32, k.f32, v.f32, embRelK.f32, embRelV.f32, wO.f32, bO.f32, x.f32, gamma.f32, beta.f32, Int64(batch),
                                                     Int64(heads), Int64(headDim), Int64(length), Int64(window), eps, &out, commandBuffer))
        return wrap(out)
    }
    /// One WaveNet layer of the flow: gate conv + tanh·sigmoid + res/skip conv. Returns (x_out — nil when `last` —, skip_out).
    public func wavenetLayerF32(x: HIPBuffer, skipIn: HIPBuffer?, wIn: HIPBuffer, bIn: HIPBuffer, wRs: HIPBuffer, bRs: HIPBuffer, batch: Int, channels: Int,
                                length: Int, kernel: Int, dilation: Int, last: Bool, commandBuffer: Stream? = nil) throws -> (xOut: HIPBuffer?, skipOut: HIPBuffer) {
        var xo: UnsafeMutablePointer<Float>? = nil, so: UnsafeMutablePointer<Float>? = nil
        try Self.check(piper_hip_wavenet_layer_f32(ctx, x.f32, skipIn?.f32, wIn.f32, bIn.f32, wRs.f32, bRs.f32, Int64(batch), Int64(channels), Int64(length),
                                                   Int64(kernel), Int64(dilation), last ? 1 : 0, &xo, &so, commandBuffer))
        return (last ? nil : wrap(xo), wrap(so))
    }
    /// HiFi-GAN ResBlock1 (type 1: weights c1_0, c2_0, c1_1, …) / ResBlock2 (type 2) over all its dilations
    public func hifiganResblockF32(type: Int, x: HIPBuffer, batch: Int, channels: Int, length: Int, kernel: Int, dilations: [Int], weights: [HIPBuffer],
                                   biases: [HIPBuffer], slope: Float = 0.1, commandBuffer: Stream? = nil) throws -> HIPBuffer {
        var out: UnsafeMutablePointer<Float>? = nil
        let w: [UnsafePointer<Float>?] = weights.map { UnsafePointer($0.f32) }
        let b: [UnsafePointer<Float>?] = biases.map { UnsafePointer($0.f32) }
        try Self.check(piper_hip_hifigan_resblock_f32(ctx, Int32(type), x.f32, Int64(batch), Int64(channels), Int64(length), Int64(kernel), dilations.map(Int32.init),
                                                      Int32(dilations.count), w, b, slope, &out, commandBuffer))
        return wrap(out)
    }
}
