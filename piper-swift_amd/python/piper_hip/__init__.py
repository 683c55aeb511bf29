"""ctypes shim over lib/libpiper_hip.so (include/piper_hip.h).

Host-side mirror of the reference's operator interface for this path: `HipBackend` exposes the
`MetalBackend` per-op methods (Sources/PiperMetal/Execution/MetalBackend.swift) with the same names
and argument meaning — buffer + shape in, (buffer, shape) out, optional stream standing in for
`commandBuffer:` — and raises `ExecutionError` subclasses where the Swift code `throws`.

There is NO CPU fallback here: if the shared library is missing, or no gfx950 device is present,
construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libpiper_hip.so"))
LIB_NORT_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libpiper_hip_nort.so"))  # linked with -no-hip-rt

# ---- errors: ExecutionError (CPUBackend.swift:3-17) ----


class ExecutionError(RuntimeError):
    code = None


class ShapeMismatch(ExecutionError):
    code = -1


class TypeMismatch(ExecutionError):
    code = -2


class UnsupportedOp(ExecutionError):
    code = -3


class DeviceUnavailable(ExecutionError):  # ExecutionError.metalUnavailable
    code = -4


class AllocationFailed(ExecutionError):
    code = -5


class LaunchFailed(ExecutionError):
    code = -6


class InvalidArgument(ExecutionError):
    code = -7


_ERRORS = {c.code: c for c in (ShapeMismatch, TypeMismatch, UnsupportedOp, DeviceUnavailable, AllocationFailed,
                               LaunchFailed, InvalidArgument)}

RELU, LEAKYRELU, TANH, SIGMOID, EXP, NEG, SQRT, SOFTPLUS, CEIL, ERF = range(10)
ADD, SUB, MUL, DIV, POW = range(5)

c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)
c_vp = C.c_void_p


class Conv1dParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("stride", "dilation", "pad_l", "pad_r", "groups")]


class ConvTranspose1dParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("stride", "dilation", "pad_l", "pad_r", "output_padding", "groups")]


class VoiceConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vocab", "hidden", "n_heads", "n_layers", "ffn", "ffn_kernel", "window",
                                         "inter", "n_flows", "wn_layers", "wn_kernel", "up_initial", "n_ups")] + [
        ("up_rates", C.c_int32 * 4), ("up_kernels", C.c_int32 * 4), ("resblock_type", C.c_int32), ("n_rb", C.c_int32),
        ("rb_kernels", C.c_int32 * 3), ("rb_n_dil", C.c_int32), ("rb_dilations", (C.c_int32 * 3) * 3),
        ("sample_rate", C.c_int32), ("dp_present", C.c_int32), ("dp_kernel", C.c_int32), ("dp_dds_layers", C.c_int32),
        ("dp_n_flows", C.c_int32), ("dp_bins", C.c_int32), ("dp_tail_bound", C.c_float)]

    @property
    def hop(self):
        h = 1
        for i in range(self.n_ups):
            h *= self.up_rates[i]
        return h


class TensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("kind", C.c_int32), ("rank", C.c_int32), ("shape", C.c_int64 * 3),
                ("fan_in", C.c_int64), ("offset", C.c_uint64), ("count", C.c_uint64)]


class OnnxTensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("data_type", C.c_int32), ("rank", C.c_int32), ("dims", C.c_int64 * 8),
                ("count", C.c_int64)]


class PiperJsonInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("num_symbols", C.c_int32), ("num_speakers", C.c_int32),
                ("noise_scale", C.c_float), ("length_scale", C.c_float), ("noise_w", C.c_float)]


class Utterance(C.Structure):
    _fields_ = [("phoneme_ids", c_i64p), ("t", C.c_int32), ("durations", c_i32p), ("noise", c_f32p),
                ("noise_scale", C.c_float), ("noise_mode", C.c_int32), ("seed", C.c_uint32), ("length_scale", C.c_float),
                ("noise_w", C.c_float), ("dp_noise", c_f32p)]


NOISE_MODES = {"injected": 0, "device": 1}


class SpeakerConfig(C.Structure):
    """piper_hip_speaker_config: the speaker table's rows and the width gin of a speaker vector (multiple of 4, 4 … 1024)."""
    _fields_ = [("n_speakers", C.c_int32), ("gin", C.c_int32)]


class Speaker(C.Structure):
    """piper_hip_speaker: a mix g = Σ_k weights[k] · emb_g[ids[k]] of 1 … 4 table rows."""
    _fields_ = [("n", C.c_int32), ("ids", C.c_int32 * 4), ("weights", C.c_float * 4)]


def _speaker(s):
    """int → that speaker alone; {id: weight} or [(id, weight), …] → a mix; a Speaker is passed through. What does not fit the record is
    handed on out of range, for the library to refuse."""
    if isinstance(s, Speaker):
        return s
    pairs = [(int(s), 1.0)] if isinstance(s, (int, np.integer)) else list(s.items() if isinstance(s, dict) else s)
    out = Speaker()
    out.n = len(pairs)
    for k, (i, w) in enumerate(pairs[:4]):
        out.ids[k], out.weights[k] = int(i), float(w)
    return out


def _speakers(speakers):
    return (Speaker * len(speakers))(*[_speaker(s) for s in speakers])


class Prosody(C.Structure):
    """piper_hip_prosody (40 bytes): per-id multipliers on the duration and on noise_scale, a floor and a ceiling on the id's frames (NULL =
    neutral), the number of ids, and `fit` (bounded routes: compress to the bound instead of failing)."""
    _fields_ = [("length", c_f32p), ("min_frames", c_i32p), ("max_frames", c_i32p), ("noise", c_f32p), ("t", C.c_int32), ("fit", C.c_int32)]


def _prosody(p, t=None):
    """None → the neutral record of t ids; a dict(length=, min_frames=, max_frames=, noise=, fit=) of arrays (a missing or None field is
    neutral; t = the arrays' length, else `t`); a Prosody is passed through. Returns (record, the arrays that must outlive the call)."""
    if isinstance(p, Prosody):
        return p, ()
    p = dict(p or {})
    arrs = {k: (None if p.get(k) is None else np.ascontiguousarray(p[k], dt))
            for k, dt in (("length", np.float32), ("min_frames", np.int32), ("max_frames", np.int32), ("noise", np.float32))}
    sizes = [a.size for a in arrs.values() if a is not None]
    n = int(p["t"]) if p.get("t") is not None else (sizes[0] if sizes else int(t or 0))
    if any(s != n for s in sizes):
        raise InvalidArgument("prosody: arrays of %s entries, t = %d" % (sorted(set(sizes)), n))
    rec = Prosody(*[None if arrs[k] is None else arrs[k].ctypes.data_as(c_f32p if arrs[k].dtype == np.float32 else c_i32p)
                    for k in ("length", "min_frames", "max_frames", "noise")], n, int(p.get("fit") or 0))
    return rec, tuple(arrs.values())


def prosody_check(p):
    """piper_hip_prosody_check: raises InvalidArgument naming the field and the index of the first violation."""
    rec, _keep = _prosody(p)
    _check(load_library().piper_hip_prosody_check(C.byref(rec)))


def prosody_frames(p, w0, cap=0):
    """piper_hip_prosody_frames: the integer frame rule from w0 = exp(logw)·length_scale on (host only). Returns (frames int32 [t], wanted):
    wanted = Σ frames before fitting; fitting happens with p's fit, cap > 0 and wanted > cap."""
    w0 = np.ascontiguousarray(w0, np.float32)
    rec, _keep = (None, ()) if p is None else _prosody(p, w0.size)
    out = np.empty(w0.size, np.int32)
    wanted = C.c_int64()
    _check(load_library().piper_hip_prosody_frames(None if rec is None else C.byref(rec), w0.ctypes.data_as(c_f32p), w0.size, int(cap),
                                                   out.ctypes.data_as(c_i32p), C.byref(wanted)))
    return out, int(wanted.value)


class Volume(C.Structure):
    """piper_hip_volume (16 bytes): one linear gain per phoneme id in [0, 16] (NULL = all 1.0) and the number of ids."""
    _fields_ = [("gain", c_f32p), ("t", C.c_int32)]


def _volume(g, t=None):
    """None → the all-1.0 record of t ids; an array of gains (t = its length); a Volume is passed through. Returns (record, the array
    that must outlive the call)."""
    if isinstance(g, Volume):
        return g, None
    if g is None:
        return Volume(None, int(t or 0)), None
    arr = np.ascontiguousarray(g, np.float32).reshape(-1)
    return Volume(arr.ctypes.data_as(c_f32p), arr.size), arr


def volume_check(g, t=None):
    """piper_hip_volume_check: raises InvalidArgument naming the field and the index of the first violation. Host-only. g None (all 1.0)
    needs t, the number of ids."""
    if g is None and t is None:
        raise InvalidArgument("volume_check: a volume without gains needs t, the number of ids")
    rec, _keep = _volume(g, t)
    _check(load_library().piper_hip_volume_check(C.byref(rec)))


def volume_frames(g, durations):
    """piper_hip_volume_frames: the gain of every frame, gf [F], F = max(Σ d, 1), of an item whose ids last `durations` frames (host only).
    g: the gains per id, a Volume, or None (all 1.0)."""
    d = np.ascontiguousarray(durations, np.int32).reshape(-1)
    rec, _keep = (None, None) if g is None else _volume(g)
    lib, frames = load_library(), C.c_int64()
    ref = None if rec is None else C.byref(rec)
    _check(lib.piper_hip_volume_frames(ref, d.ctypes.data_as(c_i32p), d.size, None, 0, C.byref(frames)))
    out = np.empty(frames.value, np.float32)
    _check(lib.piper_hip_volume_frames(ref, d.ctypes.data_as(c_i32p), d.size, out.ctypes.data_as(c_f32p), out.size, C.byref(frames)))
    return out


def volume_from_f32(samples, frame_gain, hop):
    """The envelope on the host (piper_hip_volume_from_f32), bit for bit what the device computes: samples [frames·hop] under the gains
    per frame."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    gf = np.ascontiguousarray(frame_gain, np.float32).reshape(-1)
    y = np.empty_like(x)
    _check(load_library().piper_hip_volume_from_f32(gf.ctypes.data_as(c_f32p), gf.size, int(hop), x.ctypes.data_as(c_f32p), x.size,
                                                    y.ctypes.data_as(c_f32p)))
    return y


class PcmParams(C.Structure):
    """piper_hip_pcm_params: linear gain (0 = 1.0) and the peak-normalisation flag of the 16-bit PCM entry points."""
    _fields_ = [("gain", C.c_float), ("normalize", C.c_int32)]


c_i16p = C.POINTER(C.c_int16)
c_u8p = C.POINTER(C.c_uint8)

# G.711 laws (include/piper_hip.h "G.711 output")
G711_MULAW, G711_ALAW = 1, 2


def _law(law):
    """"mulaw" / "alaw" (or PIPER_HIP_G711_*) → the constant; anything else is passed on for the library to refuse."""
    return {"mulaw": G711_MULAW, "ulaw": G711_MULAW, "pcmu": G711_MULAW, "alaw": G711_ALAW, "pcma": G711_ALAW}.get(
        law.lower() if isinstance(law, str) else law, law if isinstance(law, int) else -1)


# encodings of a mixed stream's rows (include/piper_hip.h "Mixed formats")
ENC_S16, ENC_MULAW, ENC_ALAW, ENC_F32 = 0, 1, 2, 3
_ENCODINGS = {"s16": ENC_S16, "pcm16": ENC_S16, "mulaw": ENC_MULAW, "ulaw": ENC_MULAW, "pcmu": ENC_MULAW, "alaw": ENC_ALAW, "pcma": ENC_ALAW,
              "f32": ENC_F32, "float32": ENC_F32}
ENC_DTYPES = {ENC_S16: np.int16, ENC_MULAW: np.uint8, ENC_ALAW: np.uint8, ENC_F32: np.float32}


class StreamFormat(C.Structure):
    """piper_hip_stream_format: the output format of one row of a mixed stream. out_rate 0 = the voice's own rate; gain 0 = 1.0."""
    _fields_ = [("out_rate", C.c_int32), ("encoding", C.c_int32), ("gain", C.c_float)]

    @property
    def dtype(self):
        return ENC_DTYPES[int(self.encoding)]

    def __repr__(self):
        return "StreamFormat(rate=%d, encoding=%d, gain=%g)" % (self.out_rate, self.encoding, self.gain)


def stream_format(rate=None, encoding="s16", gain=1.0):
    """A StreamFormat from rate= (None or 0: the voice's own), encoding= "s16" | "mulaw" | "alaw" | "f32" (or ENC_*), gain=. What can be
    told here without a voice is: an unknown encoding, a negative or non-finite gain and a gain other than 1 on an f32 row raise
    InvalidArgument, a rate outside the output-rate list UnsupportedOp — the statuses the library gives for the same formats."""
    enc = _ENCODINGS.get(encoding.lower()) if isinstance(encoding, str) else (int(encoding) if int(encoding) in ENC_DTYPES else None)
    if enc is None:
        raise InvalidArgument("stream_format: encoding %r (s16, mulaw, alaw or f32)" % (encoding,))
    gain = float(gain)
    if not (gain >= 0.0) or gain == float("inf"):
        raise InvalidArgument("stream_format: gain %r is negative or not finite" % gain)
    if enc == ENC_F32 and gain not in (0.0, 1.0):
        raise InvalidArgument("stream_format: an f32 row has no gain (got %r)" % gain)
    rate = int(rate or 0)
    if rate and rate not in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000):
        raise UnsupportedOp("stream_format: output rate %d (supported: 8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)" % rate)
    return StreamFormat(rate, enc, gain)


def _formats(formats):
    """[StreamFormat | dict | None] → a ctypes array (None: the default format)"""
    fs = [f if isinstance(f, StreamFormat) else stream_format(**(f or {})) for f in formats]
    return (StreamFormat * max(len(fs), 1))(*fs)


class Level(C.Structure):
    """piper_hip_level: the look-ahead limiter of include/piper_hip.h "Level control". A zero field takes its default: {1, 1, 50 ms}."""
    _fields_ = [("drive", C.c_float), ("ceiling", C.c_float), ("release_ms", C.c_float)]

    def __repr__(self):
        return "Level(drive=%g, ceiling=%g, release_ms=%g)" % (self.drive, self.ceiling, self.release_ms)


def _level(level):
    """Level | (drive, ceiling, release_ms) | dict → a Level"""
    if isinstance(level, Level):
        return level
    if isinstance(level, dict):
        return Level(float(level.get("drive", 0.0)), float(level.get("ceiling", 0.0)), float(level.get("release_ms", 0.0)))
    d, c, r = level
    return Level(float(d), float(c), float(r))


KEEP = object()  # level=KEEP / loudness=KEEP / eq=KEEP / join=KEEP: leave the slot id's level / loudness / EQ / join as it is

JOIN_MAX_ITEMS = 256


class Join(C.Structure):
    """piper_hip_join: lead / gap / tail silences in ms, trim (0 / 1) with its linear threshold and pad, fade in ms
    (include/piper_hip.h "Join"). Join(gap_ms=200, trim=1, trim_threshold=0.01) also works: fields left out are 0."""
    _fields_ = [("lead_ms", C.c_float), ("gap_ms", C.c_float), ("tail_ms", C.c_float), ("trim", C.c_int32),
                ("trim_threshold", C.c_float), ("trim_pad_ms", C.c_float), ("fade_ms", C.c_float)]

    def __repr__(self):
        return "Join(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_)


def _join(join, gaps=None):
    """Join | dict (which may carry gaps=[...]) | None → (Join or None, C array of gaps or None, their number)"""
    if join is None:
        return None, None, 0
    if isinstance(join, dict):
        d = dict(join)
        if "gaps" in d:
            g = d.pop("gaps")
            gaps = g if gaps is None else gaps
        d["trim"] = int(d.get("trim", 0))
        join = Join(**d)
    g = [] if gaps is None else [float(x) for x in gaps]
    return join, ((C.c_float * len(g))(*g) if g else None), len(g)

EQ_LOWPASS, EQ_HIGHPASS, EQ_BANDPASS, EQ_NOTCH, EQ_PEAKING, EQ_LOWSHELF, EQ_HIGHSHELF = range(1, 8)
EQ_MAX_SECTIONS = 4
_EQ_TYPES = {"lowpass": 1, "highpass": 2, "bandpass": 3, "notch": 4, "peaking": 5, "lowshelf": 6, "highshelf": 7}


class EqSection(C.Structure):
    """piper_hip_eq_section: one biquad of include/piper_hip.h "Equaliser"."""
    _fields_ = [("type", C.c_int32), ("f0_hz", C.c_float), ("q", C.c_float), ("gain_db", C.c_float)]


class Eq(C.Structure):
    """piper_hip_eq: up to four sections run in order. Eq([(type, f0, q, gain_db), ...]) also works; a type may be a name
    ("lowpass", "highpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf") and gain_db may be left out (0)."""
    _fields_ = [("n", C.c_int32), ("section", EqSection * 4)]

    def __init__(self, sections=None, *args):
        super().__init__()
        if sections is None:
            return
        if isinstance(sections, int):  # the ctypes form: Eq(n, section array)
            super().__init__(sections, *args)
            return
        secs = list(sections)
        self.n = len(secs)
        for i, sec in enumerate(secs[:EQ_MAX_SECTIONS]):
            typ, f0, q = sec[0], sec[1], sec[2]
            g = sec[3] if len(sec) > 3 else 0.0
            typ = _EQ_TYPES[typ.lower()] if isinstance(typ, str) else int(typ)
            self.section[i] = EqSection(typ, float(f0), float(q), float(g))

    def sections(self):
        return [(s.type, s.f0_hz, s.q, s.gain_db) for s in self.section[:max(0, min(self.n, EQ_MAX_SECTIONS))]]

    def __repr__(self):
        return "Eq(%r)" % (self.sections(),)


def _eq(eq):
    """Eq | [(type, f0, q[, gain_db])] → an Eq"""
    return eq if isinstance(eq, Eq) else Eq(eq)


class Loudness(C.Structure):
    """piper_hip_loudness: the BS.1770 target of include/piper_hip.h "Loudness". A zero field takes its default: {−16 LUFS, 20 dB}."""
    _fields_ = [("target_lufs", C.c_float), ("max_gain_db", C.c_float)]

    def __repr__(self):
        return "Loudness(target_lufs=%g, max_gain_db=%g)" % (self.target_lufs, self.max_gain_db)


def _loudness(loudness):
    """Loudness | target | (target_lufs, max_gain_db) | dict → a Loudness"""
    if isinstance(loudness, Loudness):
        return loudness
    if isinstance(loudness, dict):
        return Loudness(float(loudness.get("target_lufs", 0.0)), float(loudness.get("max_gain_db", 0.0)))
    if isinstance(loudness, (int, float)):
        return Loudness(float(loudness), 0.0)
    t, m = loudness
    return Loudness(float(t), float(m))


class Pitch(C.Structure):
    """piper_hip_pitch (include/piper_hip.h "Pitch"): semitones in [−12, 12]; keep_tempo 1 scales the predicted durations so that the item
    keeps its length, 0 is varispeed."""
    _fields_ = [("semitones", C.c_float), ("keep_tempo", C.c_int32)]

    def __repr__(self):
        return "Pitch(semitones=%g, keep_tempo=%d)" % (self.semitones, self.keep_tempo)


def _pitch(p):
    """A Pitch from a Pitch, a number (keep_tempo on), a (semitones, keep_tempo) pair or None (no pitch)"""
    if isinstance(p, Pitch):
        return p
    if p is None:
        return Pitch(0.0, 0)
    if isinstance(p, (tuple, list)):
        st, keep = p
        return Pitch(float(st), int(keep))
    return Pitch(float(p), 1)


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("avg_us", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


# every symbol include/piper_hip.h declares: (restype, argtypes)
_PROTOS = {
    "piper_hip_last_error": (C.c_char_p, []),
    "piper_hip_abi_version": (C.c_int, []),
    "piper_hip_config_string": (C.c_int, [C.c_char_p, C.c_size_t]),
    "piper_hip_routes_arm": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_last_routes": (C.c_int, [c_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "piper_hip_device_count": (C.c_int, []),
    "piper_hip_create": (C.c_int, [C.c_int, C.POINTER(c_vp)]),
    "piper_hip_destroy": (None, [c_vp]),
    "piper_hip_alloc": (C.c_int, [c_vp, C.c_size_t, C.POINTER(c_vp)]),
    "piper_hip_free": (C.c_int, [c_vp, c_vp]),
    "piper_hip_upload_f32": (C.c_int, [c_vp, c_f32p, C.c_size_t, C.POINTER(c_vp)]),
    "piper_hip_upload_i64": (C.c_int, [c_vp, c_i64p, C.c_size_t, C.POINTER(c_vp)]),
    "piper_hip_download_f32": (C.c_int, [c_vp, c_vp, c_f32p, C.c_size_t]),
    "piper_hip_stream_create": (C.c_int, [c_vp, C.POINTER(c_vp)]),
    "piper_hip_stream_destroy": (C.c_int, [c_vp, c_vp]),
    "piper_hip_stream_sync": (C.c_int, [c_vp, c_vp]),
    "piper_hip_timer_begin": (C.c_int, [c_vp, c_vp]),
    "piper_hip_timer_end": (C.c_int, [c_vp, c_vp, C.POINTER(C.c_double)]),
    "piper_hip_conv1d_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, c_vp, C.POINTER(Conv1dParams),
                                       C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_convtranspose1d_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, c_vp,
                                                C.POINTER(ConvTranspose1dParams), C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_conv1d_bf16": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, c_vp, C.POINTER(Conv1dParams),
                                        C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_convtranspose1d_bf16": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, c_vp,
                                                 C.POINTER(ConvTranspose1dParams), C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_matmul_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, C.c_int, C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_softmax_lastdim_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int, C.POINTER(c_vp), c_vp]),
    "piper_hip_unary_f32": (C.c_int, [c_vp, C.c_int, c_vp, C.c_size_t, C.c_float, C.POINTER(c_vp), c_vp]),
    "piper_hip_binary_broadcast_f32": (C.c_int, [c_vp, C.c_int, c_vp, c_i64p, C.c_int, c_vp, c_i64p, C.c_int,
                                                 C.POINTER(c_vp), c_i64p, C.POINTER(C.c_int), c_vp]),
    "piper_hip_pad_constant_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int, c_i64p, C.c_float, C.POINTER(c_vp), c_i64p,
                                             c_vp]),
    "piper_hip_slice_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                      C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_transpose_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int, c_i32p, C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_concat2_axis1_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_vp, c_i64p, C.POINTER(c_vp), c_i64p, c_vp]),
    "piper_hip_split2_axis1_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int64, C.POINTER(c_vp), C.POINTER(c_vp), c_vp]),
    "piper_hip_expand_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_i64p, C.c_int, C.POINTER(c_vp), c_vp]),
    "piper_hip_reduce_mean_lastdim_f32": (C.c_int, [c_vp, c_vp, c_i64p, C.c_int, C.POINTER(c_vp), c_vp]),
    "piper_hip_random_normal_like_f32": (C.c_int, [c_vp, C.c_size_t, C.c_uint64, C.POINTER(c_vp), c_vp]),
    "piper_hip_random_draws_u32": (C.c_int, [c_vp, C.c_size_t, C.c_uint64, C.POINTER(c_vp), c_vp]),
    "piper_hip_rel_attention_f32": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_int64, C.c_int64, C.POINTER(c_vp), c_vp]),
    "piper_hip_attention_block_f32": (C.c_int, [c_vp] * 11 + [C.c_int64] * 5 + [C.c_float, C.POINTER(c_vp), c_vp]),
    "piper_hip_add_layernorm_f32": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int64, C.c_int64, C.c_int64, C.c_float,
                                              C.POINTER(c_vp), c_vp]),
    "piper_hip_wavenet_layer_f32": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_int64, C.c_int64, C.c_int, C.POINTER(c_vp), C.POINTER(c_vp), c_vp]),
    "piper_hip_hifigan_resblock_f32": (C.c_int, [c_vp, C.c_int, c_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, c_i32p,
                                                 C.c_int, C.POINTER(c_vp), C.POINTER(c_vp), C.c_float, C.POINTER(c_vp),
                                                 c_vp]),
    "piper_hip_voice_config_preset": (C.c_int, [C.c_int, C.POINTER(VoiceConfig)]),
    "piper_hip_voice_blob_floats": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(C.c_size_t)]),
    "piper_hip_voice_blob_layout": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(TensorInfo), C.c_int,
                                              C.POINTER(C.c_int)]),
    "piper_hip_voice_synthetic_blob": (C.c_int, [C.POINTER(VoiceConfig), C.c_uint64, c_f32p, C.c_size_t]),
    "piper_hip_voice_create": (C.c_int, [c_vp, C.POINTER(VoiceConfig), c_vp, C.c_int, C.POINTER(c_vp)]),
    "piper_hip_onnx_open": (C.c_int, [C.c_char_p, C.POINTER(c_vp)]),
    "piper_hip_onnx_open_memory": (C.c_int, [c_vp, C.c_size_t, C.POINTER(c_vp)]),
    "piper_hip_onnx_close": (None, [c_vp]),
    "piper_hip_onnx_counts": (C.c_int, [c_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "piper_hip_onnx_initializer": (C.c_int, [c_vp, C.c_int, C.POINTER(OnnxTensorInfo)]),
    "piper_hip_onnx_find": (C.c_int, [c_vp, C.c_char_p]),
    "piper_hip_onnx_read_f32": (C.c_int, [c_vp, C.c_int, c_f32p, C.c_size_t]),
    "piper_hip_onnx_infer_config": (C.c_int, [c_vp, C.POINTER(VoiceConfig)]),
    "piper_hip_onnx_build_blob": (C.c_int, [c_vp, C.POINTER(VoiceConfig), c_f32p, C.c_size_t]),
    "piper_hip_onnx_build_blob_unchecked": (C.c_int, [c_vp, C.POINTER(VoiceConfig), c_f32p, C.c_size_t]),
    "piper_hip_onnx_verify_graph": (C.c_int, [c_vp, C.POINTER(VoiceConfig)]),
    "piper_hip_voice_last_build_breakdown": (C.c_int, [c_vp, C.POINTER(C.c_double)]),
    "piper_hip_voice_set_plan_cache": (C.c_int, [c_vp, C.c_int, C.c_size_t]),
    "piper_hip_piper_json": (C.c_int, [C.c_char_p, C.POINTER(PiperJsonInfo)]),
    "piper_hip_voice_check_json": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(PiperJsonInfo)]),
    "piper_hip_pcm16_from_f32": (C.c_int, [c_f32p, C.c_size_t, C.POINTER(C.c_int16)]),
    "piper_hip_wav_write": (C.c_int, [C.c_char_p, c_f32p, C.c_size_t, C.c_int32]),
    "piper_hip_voice_receptive_field": (C.c_int, [c_vp]),
    "piper_hip_voice_stream_begin": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, C.c_int]),
    "piper_hip_voice_stream_next": (C.c_int, [c_vp, C.c_int, c_f32p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_begin_batch": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, C.c_int, C.c_int]),
    "piper_hip_voice_stream_next_batch": (C.c_int, [c_vp, C.c_int, c_f32p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_drop": (C.c_int, [c_vp, C.c_int, C.c_int]),
    "piper_hip_voice_stream_pool_open": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int]),
    "piper_hip_voice_stream_pool_join": (C.c_int, [c_vp, C.c_int, C.POINTER(Utterance), C.c_int, C.c_int, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_pool_free_rows": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_stream_pool_close": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_memory_stats": (C.c_int, [c_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "piper_hip_memory_trim": (C.c_int, [c_vp]),
    "piper_hip_memory_reserve": (C.c_int, [c_vp, C.c_size_t]),
    "piper_hip_voice_set_precision": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_precision": (C.c_int, [c_vp]),
    "piper_hip_voice_destroy": (None, [c_vp]),
    "piper_hip_voice_num_samples": (C.c_int64, [c_vp, C.POINTER(Utterance)]),
    "piper_hip_host_alloc": (C.c_int, [c_vp, C.c_size_t, C.POINTER(C.c_void_p)]),
    "piper_hip_host_free": (C.c_int, [c_vp, C.c_void_p]),
    "piper_hip_comm_unique_id": (C.c_int, [C.c_void_p]),
    "piper_hip_comm_create": (C.c_int, [c_vp, C.c_void_p, C.c_int, C.c_int, C.POINTER(c_vp)]),
    "piper_hip_comm_destroy": (None, [c_vp]),
    "piper_hip_comm_rank": (C.c_int, [c_vp]),
    "piper_hip_comm_world": (C.c_int, [c_vp]),
    "piper_hip_comm_broadcast_f32": (C.c_int, [c_vp, C.c_void_p, C.c_size_t, C.c_int]),
    "piper_hip_comm_max_f64": (C.c_int, [c_vp, C.POINTER(C.c_double)]),
    "piper_hip_comm_barrier": (C.c_int, [c_vp]),
    "piper_hip_voice_prepare": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int]),
    "piper_hip_voice_predict_durations": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, c_i32p, c_f32p, C.c_int]),
    "piper_hip_voice_prepared_samples": (C.c_int, [c_vp, C.c_int, c_i64p, C.c_int, c_i64p]),
    "piper_hip_voice_durations": (C.c_int, [c_vp, C.c_int, c_i32p, C.c_int, C.POINTER(C.c_int)]),
    "piper_hip_voice_prepare_batch": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, C.c_int]),
    "piper_hip_voice_prepare_batch_bounded": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, C.c_int, C.c_int]),
    "piper_hip_voice_batch_size": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_plan_info": (C.c_int, [c_vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_size_t)]),
    "piper_hip_voice_launch": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_collect": (C.c_int, [c_vp, C.c_int, c_f32p, C.c_int64]),
    "piper_hip_voice_synthesize": (C.c_int, [c_vp, C.POINTER(Utterance), c_f32p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_pcm16_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_float, C.POINTER(c_vp), c_vp]),
    "piper_hip_voice_collect_pcm16": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), c_i16p, C.c_int64]),
    "piper_hip_voice_synthesize_pcm16": (C.c_int, [c_vp, C.POINTER(Utterance), C.POINTER(PcmParams), c_i16p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_next_pcm16": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), c_i16p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_next_batch_pcm16": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), c_i16p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_peaks": (C.c_int, [c_vp, C.c_int, c_f32p, C.c_int]),
    "piper_hip_resample_info": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "piper_hip_resample_taps": (C.c_int, [C.c_int32, C.c_int32, c_f32p, C.c_size_t]),
    "piper_hip_resample_count": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    "piper_hip_resample_step_bound": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    "piper_hip_wav_write_pcm16": (C.c_int, [C.c_char_p, c_i16p, C.c_size_t, C.c_int32]),
    "piper_hip_resample_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(c_vp), C.POINTER(C.c_size_t), c_vp]),
    "piper_hip_resample_pcm16_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, C.c_int32, C.c_float, C.POINTER(c_vp), C.POINTER(C.c_size_t),
                                               c_vp]),
    "piper_hip_voice_collect_pcm16_rate": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), C.c_int32, c_i16p, C.c_int64]),
    "piper_hip_voice_synthesize_pcm16_rate": (C.c_int, [c_vp, C.POINTER(Utterance), C.POINTER(PcmParams), C.c_int32, c_i16p, C.c_int64,
                                                        C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_set_rate": (C.c_int, [c_vp, C.c_int, C.c_int32]),
    "piper_hip_voice_stream_rate": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_stream_step_capacity": (C.c_int64, [c_vp, C.c_int]),
    "piper_hip_g711_from_pcm16": (C.c_int, [C.c_int, c_i16p, C.c_size_t, c_u8p]),
    "piper_hip_g711_to_pcm16": (C.c_int, [C.c_int, c_u8p, C.c_size_t, c_i16p]),
    "piper_hip_wav_write_g711": (C.c_int, [C.c_char_p, C.c_int, c_u8p, C.c_size_t, C.c_int32]),
    "piper_hip_g711_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, C.c_int32, C.c_float, C.c_int, C.POINTER(c_vp), C.POINTER(C.c_size_t),
                                     c_vp]),
    "piper_hip_voice_collect_g711": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), C.c_int, C.c_int32, c_u8p, C.c_int64]),
    "piper_hip_voice_synthesize_g711": (C.c_int, [c_vp, C.POINTER(Utterance), C.POINTER(PcmParams), C.c_int, C.c_int32, c_u8p, C.c_int64,
                                                  C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_next_g711": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), C.c_int, c_u8p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_next_batch_g711": (C.c_int, [c_vp, C.c_int, C.POINTER(PcmParams), C.c_int, c_u8p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_level_check": (C.c_int, [C.POINTER(Level)]),
    "piper_hip_level_info": (C.c_int, [C.POINTER(Level), C.c_int32, c_f32p]),
    "piper_hip_level_ready": (C.c_int64, [C.c_int64]),
    "piper_hip_level_step_bound": (C.c_int64, [C.c_int64]),
    "piper_hip_level_from_f32": (C.c_int, [C.POINTER(Level), C.c_int32, c_f32p, C.c_size_t, c_f32p]),
    "piper_hip_level_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, C.POINTER(Level), C.POINTER(c_vp), c_vp]),
    "piper_hip_voice_slot_level": (C.c_int, [c_vp, C.c_int, C.POINTER(Level)]),
    "piper_hip_voice_stream_set_level": (C.c_int, [c_vp, C.c_int, C.POINTER(Level)]),
    "piper_hip_voice_stream_level": (C.c_int, [c_vp, C.c_int, C.POINTER(Level)]),
    "piper_hip_loudness_check": (C.c_int, [C.POINTER(Loudness)]),
    "piper_hip_loudness_coeffs": (C.c_int, [C.c_int32, c_f64p, c_f64p, c_f64p, c_f64p]),
    "piper_hip_loudness_from_f32": (C.c_int, [C.c_int32, c_f32p, C.c_size_t, c_f32p]),
    "piper_hip_loudness_gain": (C.c_int, [C.POINTER(Loudness), C.c_float, c_f32p]),
    "piper_hip_loudness_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, c_f32p, c_vp]),
    "piper_hip_voice_slot_loudness": (C.c_int, [c_vp, C.c_int, C.POINTER(Loudness)]),
    "piper_hip_voice_loudness": (C.c_int, [c_vp, C.c_int, c_f32p, c_f32p, C.c_int]),
    "piper_hip_voice_stream_set_mixed": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_voice_stream_item_formats": (C.c_int, [c_vp, C.c_int, C.POINTER(StreamFormat), C.c_int]),
    "piper_hip_voice_stream_pool_join_formats": (C.c_int, [c_vp, C.c_int, C.POINTER(Utterance), C.c_int, C.c_int, C.POINTER(StreamFormat),
                                                           C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_next_batch_mixed": (C.c_int, [c_vp, C.c_int, c_vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_step_capacity_bytes": (C.c_int64, [c_vp, C.c_int]),
    "piper_hip_voice_stream_item_format": (C.c_int, [c_vp, C.c_int, C.c_int, C.POINTER(StreamFormat)]),
    "piper_hip_voice_tap": (C.c_int, [c_vp, C.c_int, C.c_char_p, c_f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "piper_hip_voice_last_gpu_ms": (C.c_int, [c_vp, C.c_int, C.POINTER(C.c_double)]),
    "piper_hip_voice_slot_stream": (c_vp, [c_vp, C.c_int]),
    "piper_hip_voice_profile": (C.c_int, [c_vp, C.c_int, C.c_int, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int)]),
    "piper_hip_voice_time_subset": (C.c_int, [c_vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                              C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "piper_hip_speaker_blob_floats": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig), C.POINTER(C.c_size_t)]),
    "piper_hip_speaker_blob_layout": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig), C.POINTER(TensorInfo), C.c_int,
                                                C.POINTER(C.c_int)]),
    "piper_hip_speaker_synthetic_blob": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig), C.c_uint64, c_f32p, C.c_size_t]),
    "piper_hip_voice_attach_speakers": (C.c_int, [c_vp, C.POINTER(SpeakerConfig), c_vp, C.c_int]),
    "piper_hip_voice_num_speakers": (C.c_int, [c_vp]),
    "piper_hip_voice_slot_speakers": (C.c_int, [c_vp, C.c_int, C.POINTER(Speaker), C.c_int]),
    "piper_hip_voice_predict_durations_speakers": (C.c_int, [c_vp, C.POINTER(Utterance), C.c_int, C.POINTER(Speaker), c_i32p, c_f32p, C.c_int]),
    "piper_hip_onnx_speaker_config": (C.c_int, [c_vp, C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig)]),
    "piper_hip_onnx_infer_config_speakers": (C.c_int, [c_vp, C.POINTER(VoiceConfig)]),
    "piper_hip_onnx_build_speaker_blob": (C.c_int, [c_vp, C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig), c_f32p, C.c_size_t]),
    "piper_hip_voice_check_json_speakers": (C.c_int, [C.POINTER(VoiceConfig), C.POINTER(SpeakerConfig), C.POINTER(PiperJsonInfo)]),
    "piper_hip_voice_stream_pool_join_bounded": (C.c_int, [c_vp, C.c_int, C.POINTER(Utterance), C.c_int, C.c_int, C.c_int, C.POINTER(StreamFormat),
                                                           C.POINTER(C.c_int)]),
    "piper_hip_voice_stream_pool_item_samples": (C.c_int, [c_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "piper_hip_voice_stream_pool_joins_pending": (C.c_int, [c_vp, C.c_int]),
    "piper_hip_prosody_check": (C.c_int, [C.POINTER(Prosody)]),
    "piper_hip_prosody_frames": (C.c_int, [C.POINTER(Prosody), c_f32p, C.c_int32, C.c_int64, c_i32p, C.POINTER(C.c_int64)]),
    "piper_hip_voice_slot_prosody": (C.c_int, [c_vp, C.c_int, C.POINTER(Prosody), C.c_int]),
    "piper_hip_voice_prosody_report": (C.c_int, [c_vp, C.c_int, C.POINTER(C.c_int64), c_i32p, C.c_int]),
    "piper_hip_volume_check": (C.c_int, [C.POINTER(Volume)]),
    "piper_hip_volume_frames": (C.c_int, [C.POINTER(Volume), c_i32p, C.c_int32, c_f32p, C.c_int64, C.POINTER(C.c_int64)]),
    "piper_hip_volume_from_f32": (C.c_int, [c_f32p, C.c_int64, C.c_int32, c_f32p, C.c_size_t, c_f32p]),
    "piper_hip_volume_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, c_vp, C.c_int64, C.c_int32, C.POINTER(c_vp), c_vp]),
    "piper_hip_voice_slot_volume": (C.c_int, [c_vp, C.c_int, C.POINTER(Volume), C.c_int]),
    "piper_hip_join_check": (C.c_int, [C.POINTER(Join), c_f32p, C.c_int]),
    "piper_hip_join_counts": (C.c_int, [C.POINTER(Join), C.c_int32, c_i64p, c_i64p, c_i64p, c_i64p, c_i64p]),
    "piper_hip_join_capacity": (C.c_int, [C.POINTER(Join), c_f32p, C.c_int, C.c_int32, c_i64p, C.c_int, c_i64p]),
    "piper_hip_join_from_f32": (C.c_int, [C.POINTER(Join), c_f32p, C.c_int, C.c_int32, c_f32p, c_i64p, c_i64p, C.c_int, c_f32p, C.c_int64,
                                          c_i64p, c_i64p, c_i64p]),
    "piper_hip_join_f32": (C.c_int, [c_vp, c_vp, c_i64p, c_i64p, C.c_int, C.c_int32, C.POINTER(Join), c_f32p, C.c_int, C.POINTER(c_vp),
                                     c_i64p, c_i64p, c_i64p, c_vp]),
    "piper_hip_voice_slot_join": (C.c_int, [c_vp, C.c_int, C.POINTER(Join), c_f32p, C.c_int]),
    "piper_hip_voice_join_capacity": (C.c_int, [c_vp, C.c_int, C.c_int32, c_i64p]),
    "piper_hip_voice_join_report": (C.c_int, [c_vp, C.c_int, c_i64p, c_i64p, C.c_int, c_i64p]),
    "piper_hip_eq_check": (C.c_int, [C.POINTER(Eq), C.c_int32]),
    "piper_hip_eq_design": (C.c_int, [C.POINTER(Eq), C.c_int32, c_f64p]),
    "piper_hip_eq_from_f32": (C.c_int, [C.POINTER(Eq), C.c_int32, c_f32p, C.c_size_t, c_f32p]),
    "piper_hip_eq_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_int32, C.POINTER(Eq), C.POINTER(c_vp), c_vp]),
    "piper_hip_voice_slot_eq": (C.c_int, [c_vp, C.c_int, C.POINTER(Eq)]),
    "piper_hip_voice_stream_set_eq": (C.c_int, [c_vp, C.c_int, C.POINTER(Eq)]),
    "piper_hip_voice_stream_eq": (C.c_int, [c_vp, C.c_int, C.POINTER(Eq)]),
    "piper_hip_pitch_check": (C.c_int, [C.POINTER(Pitch)]),
    "piper_hip_pitch_info": (C.c_int, [C.c_float, C.POINTER(C.c_uint64), c_i32p, c_f32p]),
    "piper_hip_pitch_count": (C.c_int64, [C.c_float, C.c_int64]),
    "piper_hip_pitch_taps": (C.c_int, [C.c_float, c_f32p, C.c_size_t]),
    "piper_hip_pitch_from_f32": (C.c_int, [C.c_float, c_f32p, C.c_size_t, c_f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "piper_hip_pitch_f32": (C.c_int, [c_vp, c_vp, C.c_size_t, C.c_float, C.POINTER(c_vp), C.POINTER(C.c_size_t), c_vp]),
    "piper_hip_voice_slot_pitch": (C.c_int, [c_vp, C.c_int, C.POINTER(Pitch), C.c_int]),
    "piper_hip_voice_pitch_samples": (C.c_int, [c_vp, C.c_int, c_i64p, C.c_int, c_i64p]),
}

_lib = None
_runtime = os.environ.get("PIPER_HIP_RUNTIME", "system")  # "system" (ROCm install) or "torch" (PyTorch's bundled copy)


def set_runtime(which):
    """Choose the HIP runtime the library runs on; must be called before the first load_library().

    A process may hold only ONE libamdhip64 that touches the GPU.  "system" loads libpiper_hip.so, which depends on the
    ROCm install's runtime.  "torch" is for processes that also drive the GPU through PyTorch (torch.cuda, RCCL): PyTorch's
    bundled libamdhip64 is made global and libpiper_hip_nort.so (linked with -no-hip-rt) binds to it."""
    global _runtime
    if which not in ("system", "torch"):
        raise ValueError("runtime must be 'system' or 'torch'")
    if _lib is not None and which != _runtime:
        raise RuntimeError("piper_hip: the HIP runtime is already bound to %r" % _runtime)
    _runtime = which


def _library_path():
    if _runtime == "torch":
        import torch
        rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if not os.path.exists(rt):
            raise DeviceUnavailable("PyTorch's HIP runtime not found at %s" % rt)
        C.CDLL(rt, mode=C.RTLD_GLOBAL)  # already loaded by torch; this only promotes it to the global symbol scope
        return LIB_NORT_PATH
    return LIB_PATH


def load_library(path=None):
    """dlopen the C-ABI library and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _library_path()
    if not os.path.exists(p):
        raise DeviceUnavailable(f"{p} not found: build it with `make -C piper-swift_amd` "
                                "(python __graft_entry__.py build). There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def exported_symbols():
    return sorted(_PROTOS)


def _check(rc):
    if rc != 0:
        msg = load_library().piper_hip_last_error().decode("utf-8", "replace")
        raise _ERRORS.get(rc, ExecutionError)(msg or f"piper_hip error {rc}")


def _i64(a):
    arr = (C.c_int64 * len(a))(*[int(v) for v in a])
    return arr


def device_count():
    return load_library().piper_hip_device_count()


class DeviceBuffer:
    """An MTLBuffer stand-in: device pointer + element count, owned by a backend's pool. `count` is in elements of `dtype`: float32
    everywhere but for the result of pcm16F32, whose buffer holds `count` int16 samples (read it with downloadInt16, not downloadFloat32)."""

    def __init__(self, backend, ptr, count, owned=True, dtype=np.float32):
        self.backend, self.ptr, self.count, self.owned, self.dtype = backend, ptr, int(count), owned, np.dtype(dtype)

    def free(self):
        if self.owned and self.ptr:
            _check(self.backend.lib.piper_hip_free(self.backend.ctx, self.ptr))
        self.ptr = None


def _ptr(b):
    if b is None:
        return None
    return b.ptr if isinstance(b, DeviceBuffer) else b


class HipBackend:
    """MetalBackend's hot-path surface (MetalBackend.swift:8-3427) over the C-ABI."""

    def __init__(self, device=0):
        self.lib = load_library()
        ctx = c_vp()
        _check(self.lib.piper_hip_create(device, C.byref(ctx)))
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.lib.piper_hip_destroy(self.ctx)
            self.ctx = None

    def arm_routes(self, on=True):
        """Route records (include/piper_hip.h, piper_hip_routes_arm): while armed, every conv / ResBlock-pair / flow-seam / attention launcher
        of this context notes which kernel variant it chose. Off by default. See last_routes() and HipRuntime.routes()."""
        _check(self.lib.piper_hip_routes_arm(self.ctx, 1 if on else 0))

    def last_routes(self):
        """The route records of the last op call on this context, one "<variant> | <shape>" string per launch ([] when disarmed)."""
        n = C.c_size_t()
        _check(self.lib.piper_hip_last_routes(self.ctx, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(int(n.value), 1))
        _check(self.lib.piper_hip_last_routes(self.ctx, buf, len(buf), None))
        txt = buf.value.decode()
        return txt.split("\n") if txt else []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- buffers (MetalBackend.swift:34-39, 963-993)
    def memory_stats(self):
        r, l = C.c_size_t(), C.c_size_t()
        _check(self.lib.piper_hip_memory_stats(self.ctx, C.byref(r), C.byref(l)))
        return dict(reserved=r.value, live=l.value)

    def memory_reserve(self, nbytes):
        """One slab of device memory up front; later allocations are carved from it (no first-touch stalls under requests)."""
        _check(self.lib.piper_hip_memory_reserve(self.ctx, int(nbytes)))

    def memory_trim(self):
        _check(self.lib.piper_hip_memory_trim(self.ctx))

    def allocateBuffer(self, length):
        p = c_vp()
        _check(self.lib.piper_hip_alloc(self.ctx, length, C.byref(p)))
        return DeviceBuffer(self, p.value, length // 4)

    def uploadFloat32(self, data):
        a = np.ascontiguousarray(data, dtype=np.float32)
        p = c_vp()
        _check(self.lib.piper_hip_upload_f32(self.ctx, a.ctypes.data_as(c_f32p), a.size, C.byref(p)))
        return DeviceBuffer(self, p.value, a.size)

    def downloadFloat32(self, buf, count=None):
        if count is None and isinstance(buf, DeviceBuffer) and buf.dtype != np.float32:
            raise TypeError(f"downloadFloat32: the buffer holds {buf.count} {buf.dtype} elements, not floats")
        n = buf.count if count is None else int(count)
        out = np.empty(n, np.float32)
        _check(self.lib.piper_hip_download_f32(self.ctx, _ptr(buf), out.ctypes.data_as(c_f32p), n))
        return out

    def makeCommandBuffer(self):
        s = c_vp()
        _check(self.lib.piper_hip_stream_create(self.ctx, C.byref(s)))
        return s

    def flush(self, stream):
        _check(self.lib.piper_hip_stream_sync(self.ctx, stream))

    def _out(self, p, shape):
        return DeviceBuffer(self, p.value, int(np.prod(shape)) if len(shape) else 1), [int(s) for s in shape]

    # -- ops
    def conv1dF32(self, input, inputShape, weight, weightShape, bias, stride=1, dilation=1, padL=0, padR=0, groups=1,
                  commandBuffer=None):
        if len(inputShape) != 3:
            raise ShapeMismatch("conv1dF32 input must be [N,C,L]")
        if len(weightShape) != 3:
            raise ShapeMismatch("conv1dF32 weight must be [C_out,C_in,K]")
        prm = Conv1dParams(stride, dilation, padL, padR, groups)
        p, osh = c_vp(), (C.c_int64 * 3)()
        _check(self.lib.piper_hip_conv1d_f32(self.ctx, _ptr(input), _i64(inputShape), _ptr(weight), _i64(weightShape),
                                             _ptr(bias), C.byref(prm), C.byref(p), osh, commandBuffer))
        return self._out(p, list(osh))

    def convTranspose1dF32(self, input, inputShape, weight, weightShape, bias, stride=1, dilation=1, padL=0, padR=0,
                           outputPadding=0, groups=1, commandBuffer=None):
        if len(inputShape) != 3:
            raise ShapeMismatch("convTranspose1dF32 input must be [N,C,L]")
        if len(weightShape) != 3:
            raise ShapeMismatch("convTranspose1dF32 weight must be [C_in,C_out_per_group,K]")
        prm = ConvTranspose1dParams(stride, dilation, padL, padR, outputPadding, groups)
        p, osh = c_vp(), (C.c_int64 * 3)()
        _check(self.lib.piper_hip_convtranspose1d_f32(self.ctx, _ptr(input), _i64(inputShape), _ptr(weight),
                                                      _i64(weightShape), _ptr(bias), C.byref(prm), C.byref(p), osh,
                                                      commandBuffer))
        return self._out(p, list(osh))

    def conv1dBF16(self, input, inputShape, weight, weightShape, bias, stride=1, dilation=1, padL=0, padR=0, groups=1,
                   commandBuffer=None):
        """conv1dF32's contract with bf16 operands / fp32 accumulation (build extension; UnsupportedOp outside its geometry)."""
        if len(inputShape) != 3:
            raise ShapeMismatch("conv1dBF16 input must be [N,C,L]")
        if len(weightShape) != 3:
            raise ShapeMismatch("conv1dBF16 weight must be [C_out,C_in,K]")
        prm = Conv1dParams(stride, dilation, padL, padR, groups)
        p, osh = c_vp(), (C.c_int64 * 3)()
        _check(self.lib.piper_hip_conv1d_bf16(self.ctx, _ptr(input), _i64(inputShape), _ptr(weight), _i64(weightShape),
                                              _ptr(bias), C.byref(prm), C.byref(p), osh, commandBuffer))
        return self._out(p, list(osh))

    def convTranspose1dBF16(self, input, inputShape, weight, weightShape, bias, stride=1, dilation=1, padL=0, padR=0,
                            outputPadding=0, groups=1, commandBuffer=None):
        if len(inputShape) != 3:
            raise ShapeMismatch("convTranspose1dBF16 input must be [N,C,L]")
        if len(weightShape) != 3:
            raise ShapeMismatch("convTranspose1dBF16 weight must be [C_in,C_out,K]")
        prm = ConvTranspose1dParams(stride, dilation, padL, padR, outputPadding, groups)
        p, osh = c_vp(), (C.c_int64 * 3)()
        _check(self.lib.piper_hip_convtranspose1d_bf16(self.ctx, _ptr(input), _i64(inputShape), _ptr(weight),
                                                       _i64(weightShape), _ptr(bias), C.byref(prm), C.byref(p), osh,
                                                       commandBuffer))
        return self._out(p, list(osh))

    def matmulF32(self, a, aShape, b, bShape, commandBuffer=None):
        if len(aShape) < 2 or len(bShape) < 2:
            raise ShapeMismatch(f"matmulF32 requires rank>=2 (got {aShape} x {bShape})")
        if len(aShape) != len(bShape):
            raise ShapeMismatch(f"matmulF32 rank mismatch (got {len(aShape)} vs {len(bShape)})")
        r = len(aShape)
        p, osh = c_vp(), (C.c_int64 * r)()
        _check(self.lib.piper_hip_matmul_f32(self.ctx, _ptr(a), _i64(aShape), _ptr(b), _i64(bShape), r, C.byref(p), osh,
                                             commandBuffer))
        return self._out(p, list(osh))

    def softmaxLastDimF32(self, input, shape, commandBuffer=None):
        if len(shape) < 1:
            raise ShapeMismatch("softmaxLastDimF32 requires non-empty last dim")
        p = c_vp()
        _check(self.lib.piper_hip_softmax_lastdim_f32(self.ctx, _ptr(input), _i64(shape), len(shape), C.byref(p),
                                                      commandBuffer))
        return self._out(p, shape)

    def unaryF32(self, op, input, count, alpha=0.0, commandBuffer=None):
        p = c_vp()
        _check(self.lib.piper_hip_unary_f32(self.ctx, op, _ptr(input), count, alpha, C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, count)

    def reluF32(self, input, count, commandBuffer=None):
        return self.unaryF32(RELU, input, count, 0.0, commandBuffer)

    def leakyReluF32(self, input, count, alpha=0.01, commandBuffer=None):
        return self.unaryF32(LEAKYRELU, input, count, alpha, commandBuffer)

    def tanhF32(self, input, count, commandBuffer=None):
        return self.unaryF32(TANH, input, count, 0.0, commandBuffer)

    def sigmoidF32(self, input, count, commandBuffer=None):
        return self.unaryF32(SIGMOID, input, count, 0.0, commandBuffer)

    def binaryBroadcastF32(self, op, a, aShape, b, bShape, commandBuffer=None):
        r = max(len(aShape), len(bShape))
        p, osh, orank = c_vp(), (C.c_int64 * max(r, 1))(), C.c_int()
        _check(self.lib.piper_hip_binary_broadcast_f32(self.ctx, op, _ptr(a), _i64(aShape), len(aShape), _ptr(b),
                                                       _i64(bShape), len(bShape), C.byref(p), osh, C.byref(orank),
                                                       commandBuffer))
        return self._out(p, list(osh)[:orank.value])

    def addF32(self, a, aShape, b, bShape, commandBuffer=None):
        return self.binaryBroadcastF32(ADD, a, aShape, b, bShape, commandBuffer)

    def subF32(self, a, aShape, b, bShape, commandBuffer=None):
        return self.binaryBroadcastF32(SUB, a, aShape, b, bShape, commandBuffer)

    def mulF32(self, a, aShape, b, bShape, commandBuffer=None):
        return self.binaryBroadcastF32(MUL, a, aShape, b, bShape, commandBuffer)

    def divF32(self, a, aShape, b, bShape, commandBuffer=None):
        return self.binaryBroadcastF32(DIV, a, aShape, b, bShape, commandBuffer)

    def padConstantF32(self, input, shape, pads, value=0.0, commandBuffer=None):
        r = len(shape)
        p, osh = c_vp(), (C.c_int64 * r)()
        _check(self.lib.piper_hip_pad_constant_f32(self.ctx, _ptr(input), _i64(shape), r, _i64(pads), value, C.byref(p),
                                                   osh, commandBuffer))
        return self._out(p, list(osh))

    def sliceF32(self, input, shape, axis, start, end, step=1, commandBuffer=None):
        r = len(shape)
        p, osh = c_vp(), (C.c_int64 * r)()
        _check(self.lib.piper_hip_slice_f32(self.ctx, _ptr(input), _i64(shape), r, axis, start, end, step, C.byref(p), osh,
                                            commandBuffer))
        return self._out(p, list(osh))

    def transposeF32(self, input, shape, perm, commandBuffer=None):
        r = len(shape)
        if len(perm) != r:
            raise ShapeMismatch(f"Transpose perm rank mismatch: perm={perm} shape={shape}")
        p, osh = c_vp(), (C.c_int64 * r)()
        pm = (C.c_int32 * r)(*perm)
        _check(self.lib.piper_hip_transpose_f32(self.ctx, _ptr(input), _i64(shape), r, pm, C.byref(p), osh, commandBuffer))
        return self._out(p, list(osh))

    def concat2Axis1F32(self, a, aShape, b, bShape, commandBuffer=None):
        p, osh = c_vp(), (C.c_int64 * 3)()
        _check(self.lib.piper_hip_concat2_axis1_f32(self.ctx, _ptr(a), _i64(aShape), _ptr(b), _i64(bShape), C.byref(p),
                                                    osh, commandBuffer))
        return self._out(p, list(osh))

    def split2Axis1F32(self, input, shape, c0, commandBuffer=None):
        p0, p1 = c_vp(), c_vp()
        _check(self.lib.piper_hip_split2_axis1_f32(self.ctx, _ptr(input), _i64(shape), c0, C.byref(p0), C.byref(p1),
                                                   commandBuffer))
        n, c, l = shape
        return self._out(p0, [n, c0, l]), self._out(p1, [n, c - c0, l])

    def expandF32(self, input, inShape, outShape, commandBuffer=None):
        p = c_vp()
        _check(self.lib.piper_hip_expand_f32(self.ctx, _ptr(input), _i64(inShape), _i64(outShape), len(outShape),
                                             C.byref(p), commandBuffer))
        return self._out(p, outShape)[0]

    def reduceMeanLastDimF32(self, input, shape, commandBuffer=None):
        p = c_vp()
        _check(self.lib.piper_hip_reduce_mean_lastdim_f32(self.ctx, _ptr(input), _i64(shape), len(shape), C.byref(p),
                                                          commandBuffer))
        return self._out(p, list(shape[:-1]))

    def randomNormalLike(self, shape, seed=1234, commandBuffer=None):
        """MetalBackend.randomNormalLike(shape:seed:) — device buffer of prod(shape) floats."""
        n = int(np.prod(shape)) if len(shape) else 1
        p = c_vp()
        _check(self.lib.piper_hip_random_normal_like_f32(self.ctx, n, int(seed), C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, n)

    def randomDraws(self, count, seed=1234):
        """The raw (u0, u1) 32-bit draws per element, as a host uint32 array [count, 2]."""
        p = c_vp()
        _check(self.lib.piper_hip_random_draws_u32(self.ctx, int(count), int(seed), C.byref(p), None))
        out = np.empty(2 * int(count), np.float32)
        _check(self.lib.piper_hip_download_f32(self.ctx, p, out.ctypes.data_as(c_f32p), 2 * int(count)))
        _check(self.lib.piper_hip_free(self.ctx, p))
        return out.view(np.uint32).reshape(-1, 2)

    def pcm16F32(self, buf, gain=1.0, count=None, out=None, commandBuffer=None):
        """`count` device floats → 16-bit PCM on the device (piper_hip_pcm16_f32): x · gain, clamp to [−1, 1], × 32767 in double, truncate —
        the samples pcm16() gives on the host. Returns a DeviceBuffer of `count` int16 (downloadInt16); `out`: a device address to write to
        (2-byte alignment suffices), returned as it is."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        _check(self.lib.piper_hip_pcm16_f32(self.ctx, _ptr(buf), n, float(gain), C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, n, owned=out is None, dtype=np.int16)

    def level_f32(self, buf, rate, level, count=None, out=None, commandBuffer=None):
        """`count` device floats sampled at `rate` → the same number of limited device floats (piper_hip_level_f32): the look-ahead limiter
        of include/piper_hip.h "Level control". Returns a DeviceBuffer of `count` float32."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        lv = _level(level)
        _check(self.lib.piper_hip_level_f32(self.ctx, _ptr(buf), n, int(rate), C.byref(lv), C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, n, owned=out is None)

    def join_f32(self, buf, item_off, item_len, rate, join, gaps=None, out=None, commandBuffer=None):
        """Items of the device floats `buf` (item i at buf[item_off[i] … + item_len[i])) → ONE programme in device memory
        (piper_hip_join_f32; include/piper_hip.h "Join"): trimmed, faded, with silences. buf and out may be raw device addresses (4-byte
        alignment suffices). Returns (DeviceBuffer of `total` float32, start [n], len [n], total)."""
        off = np.ascontiguousarray(item_off, np.int64).reshape(-1)
        ln = np.ascontiguousarray(item_len, np.int64).reshape(-1)
        assert off.size == ln.size
        jn, g, ng = _join(join, gaps)
        start, length, total = np.zeros(max(off.size, 1), np.int64), np.zeros(max(off.size, 1), np.int64), C.c_int64()
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        _check(self.lib.piper_hip_join_f32(self.ctx, _ptr(buf), off.ctypes.data_as(c_i64p), ln.ctypes.data_as(c_i64p), off.size, int(rate),
                                           C.byref(jn), g, ng, C.byref(p), start.ctypes.data_as(c_i64p), length.ctypes.data_as(c_i64p),
                                           C.byref(total), commandBuffer))
        return DeviceBuffer(self, p.value, total.value, owned=out is None), start[:off.size], length[:off.size], int(total.value)

    def eq_f32(self, buf, rate, eq, count=None, out=None, commandBuffer=None):
        """`count` device floats sampled at `rate` → the same number of EQ'd device floats (piper_hip_eq_f32): the biquad cascade of
        include/piper_hip.h "Equaliser". Returns a DeviceBuffer of `count` float32."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        e = _eq(eq)
        _check(self.lib.piper_hip_eq_f32(self.ctx, _ptr(buf), n, int(rate), C.byref(e), C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, n, owned=out is None)

    def volume(self, buf, frame_gain, hop, count=None, out=None, commandBuffer=None):
        """`count` = frames·hop device floats under the envelope of the device gains per frame `frame_gain` [frames] (piper_hip_volume_f32;
        include/piper_hip.h "Per-phoneme volume"). buf and out may be raw device addresses (4-byte alignment suffices). Returns a
        DeviceBuffer of `count` float32."""
        frames = frame_gain.count
        n = frames * int(hop) if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        _check(self.lib.piper_hip_volume_f32(self.ctx, _ptr(buf), n, _ptr(frame_gain), frames, int(hop), C.byref(p), commandBuffer))
        return DeviceBuffer(self, p.value, n, owned=out is None)

    def loudness_f32(self, buf, rate, count=None, commandBuffer=None):
        """`count` device floats sampled at `rate` → their BS.1770 integrated loudness in LUFS, measured on the device
        (piper_hip_loudness_f32; include/piper_hip.h "Loudness"). −inf for an item too short to measure. With a commandBuffer the value
        is final after its sync: then a one-element float32 array is returned instead of a number."""
        n = buf.count if count is None else int(count)
        out = np.empty(1, np.float32)
        _check(self.lib.piper_hip_loudness_f32(self.ctx, _ptr(buf), n, int(rate), out.ctypes.data_as(c_f32p), commandBuffer))
        return out if commandBuffer is not None else np.float32(out[0])

    def resampleF32(self, buf, inRate, outRate, count=None, out=None, commandBuffer=None):
        """`count` device floats at inRate → J(count) device floats at outRate (piper_hip_resample_f32): the fp32 y of the output-rate
        contract (include/piper_hip.h "Output rate"). Returns a DeviceBuffer of J(count) float32."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        got = C.c_size_t()
        _check(self.lib.piper_hip_resample_f32(self.ctx, _ptr(buf), n, int(inRate), int(outRate), C.byref(p), C.byref(got), commandBuffer))
        return DeviceBuffer(self, p.value, got.value, owned=out is None)

    def pitch_f32(self, buf, semitones, count=None, out=None, commandBuffer=None):
        """`count` device floats → N' device floats shifted by `semitones` (piper_hip_pitch_f32): the contract of include/piper_hip.h
        "Pitch", no padding. Returns a DeviceBuffer of N' float32."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        got = C.c_size_t()
        _check(self.lib.piper_hip_pitch_f32(self.ctx, _ptr(buf), n, float(semitones), C.byref(p), C.byref(got), commandBuffer))
        return DeviceBuffer(self, p.value, got.value, owned=out is None)

    def resamplePcm16F32(self, buf, inRate, outRate, gain=1.0, count=None, out=None, commandBuffer=None):
        """The same ending in 16-bit PCM (piper_hip_resample_pcm16_f32): y · gain through pcm16F32's arithmetic. Returns a DeviceBuffer of
        J(count) int16 (downloadInt16); `out`: a device address to write to (2-byte alignment suffices), returned as it is."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        got = C.c_size_t()
        _check(self.lib.piper_hip_resample_pcm16_f32(self.ctx, _ptr(buf), n, int(inRate), int(outRate), float(gain), C.byref(p), C.byref(got),
                                                     commandBuffer))
        return DeviceBuffer(self, p.value, got.value, owned=out is None, dtype=np.int16)

    def g711F32(self, buf, law, inRate=None, outRate=None, gain=1.0, count=None, out=None, commandBuffer=None):
        """`count` device floats → G.711 bytes on the device (piper_hip_g711_f32): law ("mulaw" / "alaw") of the int16 that pcm16F32 —
        or, with inRate != outRate, resamplePcm16F32 — gives. Returns a DeviceBuffer of J(count) uint8 (downloadUint8); `out`: a device
        address to write to (any byte address), returned as it is."""
        n = buf.count if count is None else int(count)
        p = c_vp(_ptr(out)) if out is not None else c_vp()
        got = C.c_size_t()
        r_in = 1 if inRate is None else int(inRate)
        r_out = r_in if outRate is None else int(outRate)
        _check(self.lib.piper_hip_g711_f32(self.ctx, _ptr(buf), n, r_in, r_out, float(gain), _law(law), C.byref(p), C.byref(got), commandBuffer))
        return DeviceBuffer(self, p.value, got.value, owned=out is None, dtype=np.uint8)

    def downloadUint8(self, buf, count=None):
        """The first `count` bytes of a device buffer of this backend's pool → host array. (Copied as whole floats, as downloadInt16: up to
        three bytes more are read, which a pool block always holds.)"""
        n = buf.count if count is None else int(count)
        out = np.empty((n + 3) // 4 * 4, np.uint8)
        _check(self.lib.piper_hip_download_f32(self.ctx, _ptr(buf), out.ctypes.data_as(c_f32p), (n + 3) // 4))
        return out[:n].copy()

    def downloadInt16(self, buf, count=None):
        """The first `count` int16 of a device buffer of this backend's pool → host array. (Copied as whole floats: an odd count reads one
        sample more, which a pool block — a power of two of at least 256 bytes — always holds.)"""
        n = buf.count if count is None else int(count)
        out = np.empty(n + 1, np.int16)
        _check(self.lib.piper_hip_download_f32(self.ctx, _ptr(buf), out.ctypes.data_as(c_f32p), (n + 1) // 2))
        return out[:n].copy()

    # -- fused
    def relAttentionF32(self, q, k, v, embRelK, embRelV, n, heads, headDim, t, window, commandBuffer=None):
        p = c_vp()
        _check(self.lib.piper_hip_rel_attention_f32(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(embRelK), _ptr(embRelV), n,
                                                    heads, headDim, t, window, C.byref(p), commandBuffer))
        return self._out(p, [n, heads * headDim, t])

    def attentionBlockF32(self, q, k, v, embRelK, embRelV, wO, bO, x, gamma, beta, n, heads, headDim, t, window, eps=1e-5,
                          commandBuffer=None):
        """LN(x + conv_o(rel_attention(q, k, v)))·gamma + beta in one launch."""
        p = c_vp()
        _check(self.lib.piper_hip_attention_block_f32(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(embRelK), _ptr(embRelV), _ptr(wO), _ptr(bO),
                                                      _ptr(x), _ptr(gamma), _ptr(beta), n, heads, headDim, t, window, eps, C.byref(p),
                                                      commandBuffer))
        return self._out(p, [n, heads * headDim, t])

    def addLayerNormF32(self, x, y, gamma, beta, n, c, t, eps=1e-5, commandBuffer=None):
        p = c_vp()
        _check(self.lib.piper_hip_add_layernorm_f32(self.ctx, _ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), n, c, t, eps,
                                                    C.byref(p), commandBuffer))
        return self._out(p, [n, c, t])

    def wavenetLayerF32(self, x, skipIn, wIn, bIn, wRs, bRs, n, c, t, k, dilation, last, commandBuffer=None):
        px, ps = c_vp(), c_vp()
        _check(self.lib.piper_hip_wavenet_layer_f32(self.ctx, _ptr(x), _ptr(skipIn), _ptr(wIn), _ptr(bIn), _ptr(wRs),
                                                    _ptr(bRs), n, c, t, k, dilation, int(bool(last)), C.byref(px),
                                                    C.byref(ps), commandBuffer))
        xo = None if last else self._out(px, [n, c, t])[0]
        return xo, self._out(ps, [n, c, t])[0]

    def hifiganResblockF32(self, type, x, n, c, t, k, dilations, weights, biases, slope=0.1, commandBuffer=None):
        nd = len(dilations)
        d = (C.c_int32 * nd)(*dilations)
        w = (c_vp * len(weights))(*[_ptr(b) for b in weights])
        b = (c_vp * len(biases))(*[_ptr(x_) for x_ in biases])
        p = c_vp()
        _check(self.lib.piper_hip_hifigan_resblock_f32(self.ctx, type, _ptr(x), n, c, t, k, d, nd, w, b, slope, C.byref(p),
                                                       commandBuffer))
        return self._out(p, [n, c, t])[0]


# ---------------------------------------------------------------- voice level (PiperMetalRuntime)

QUALITIES = {"medium": 0, "high": 1, "low": 2, "x_low": 3}


def voice_config(quality="medium"):
    """Piper's four published qualities; low and x_low are the 16 kHz tier (x_low: 96 channels, head_dim 48)."""
    cfg = VoiceConfig()
    _check(load_library().piper_hip_voice_config_preset(QUALITIES[quality], C.byref(cfg)))
    return cfg


def blob_floats(cfg):
    n = C.c_size_t()
    _check(load_library().piper_hip_voice_blob_floats(C.byref(cfg), C.byref(n)))
    return n.value


def blob_layout(cfg):
    lib = load_library()
    n = C.c_int()
    _check(lib.piper_hip_voice_blob_layout(C.byref(cfg), None, 0, C.byref(n)))
    arr = (TensorInfo * n.value)()
    _check(lib.piper_hip_voice_blob_layout(C.byref(cfg), arr, n.value, C.byref(n)))
    return [dict(name=t.name.decode(), kind=t.kind, shape=[int(t.shape[i]) for i in range(t.rank)], fan_in=int(t.fan_in),
                 offset=int(t.offset), count=int(t.count)) for t in arr]


def synthetic_blob(cfg, seed=1234):
    """Host-only (no GPU): the synthetic voice of SURVEY.md §8d."""
    n = blob_floats(cfg)
    blob = np.empty(n, np.float32)
    _check(load_library().piper_hip_voice_synthetic_blob(C.byref(cfg), seed, blob.ctypes.data_as(c_f32p), n))
    return blob


def speaker_config(n_speakers, gin=512):
    """The speaker table of a multi-speaker voice: rows and the width of a speaker vector (Piper: 512)."""
    return SpeakerConfig(int(n_speakers), int(gin))


def speaker_blob_floats(cfg, scfg):
    n = C.c_size_t()
    _check(load_library().piper_hip_speaker_blob_floats(C.byref(cfg), C.byref(scfg), C.byref(n)))
    return n.value


def speaker_blob_layout(cfg, scfg):
    lib = load_library()
    n = C.c_int()
    _check(lib.piper_hip_speaker_blob_layout(C.byref(cfg), C.byref(scfg), None, 0, C.byref(n)))
    arr = (TensorInfo * n.value)()
    _check(lib.piper_hip_speaker_blob_layout(C.byref(cfg), C.byref(scfg), arr, n.value, C.byref(n)))
    return [dict(name=t.name.decode(), kind=t.kind, shape=[int(t.shape[i]) for i in range(t.rank)], fan_in=int(t.fan_in),
                 offset=int(t.offset), count=int(t.count)) for t in arr]


def synthetic_speaker_blob(cfg, scfg, seed=4321):
    """Host-only (no GPU): synthetic speaker table and cond convs, by the rule of synthetic_blob with a seed of its own."""
    n = speaker_blob_floats(cfg, scfg)
    blob = np.empty(n, np.float32)
    _check(load_library().piper_hip_speaker_synthetic_blob(C.byref(cfg), C.byref(scfg), seed, blob.ctypes.data_as(c_f32p), n))
    return blob


def speaker_row_floats(cfg):
    """Ctot: floats of one item's speaker row (dp.pre; the flow's gated convs; dec.conv_pre)."""
    return (cfg.hidden if cfg.dp_present else 0) + cfg.n_flows * cfg.wn_layers * 2 * cfg.hidden + cfg.up_initial


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 opaque bytes (ncclUniqueId) made by ONE rank; every rank of the world passes the same bytes to Comm()."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().piper_hip_comm_unique_id(buf))
    return buf.raw


def config_string():
    """The PIPER_HIP_* tuning switches this process has honoured so far (needs PIPER_HIP_TUNING=1), '' when none."""
    buf = C.create_string_buffer(2048)
    _check(load_library().piper_hip_config_string(buf, len(buf)))
    return buf.value.decode()


def comm_available():
    """True when the library can reach RCCL here (librccl.so.1 loads and ncclGetUniqueId works). Local, not a collective — what
    every rank checks BEFORE the ranks agree to enter piper_hip_comm_* together (bench.py)."""
    try:
        comm_unique_id()
        return True
    except Exception:
        return False


class Comm:
    """piper_hip_comm_*: an RCCL communicator for the one-shot voice-blob broadcast (and the bench's MAX / barrier)."""

    def __init__(self, backend, unique_id, rank, world):
        assert len(unique_id) == COMM_ID_BYTES
        self.lib = backend.lib
        h = c_vp()
        _check(self.lib.piper_hip_comm_create(backend.ctx, C.c_char_p(unique_id), int(rank), int(world), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.piper_hip_comm_destroy(self.h)
            self.h = None

    @property
    def rank(self):
        return self.lib.piper_hip_comm_rank(self.h)

    @property
    def world(self):
        return self.lib.piper_hip_comm_world(self.h)

    def broadcast_f32(self, device_ptr, count, root=0):
        ptr = _ptr(device_ptr)
        if not isinstance(ptr, (C.c_void_p, C._Pointer)):
            ptr = C.c_void_p(int(ptr))  # a raw address (torch.Tensor.data_ptr())
        _check(self.lib.piper_hip_comm_broadcast_f32(self.h, ptr, int(count), int(root)))

    def max(self, value):
        v = C.c_double(float(value))
        _check(self.lib.piper_hip_comm_max_f64(self.h, C.byref(v)))
        return v.value

    def barrier(self):
        _check(self.lib.piper_hip_comm_barrier(self.h))


class OnnxModel:
    """A Piper `.onnx` opened by the library's own protobuf reader (host-only; the role of PiperONNX.ONNXLoader)."""

    def __init__(self, path=None, data=None):
        self.lib = load_library()
        h = c_vp()
        if path is not None:
            _check(self.lib.piper_hip_onnx_open(str(path).encode(), C.byref(h)))
        else:
            buf = (C.c_char * len(data)).from_buffer_copy(data)
            _check(self.lib.piper_hip_onnx_open_memory(buf, len(data), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.piper_hip_onnx_close(self.h)
            self.h = None

    def counts(self):
        ir, op, nn, ni = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        _check(self.lib.piper_hip_onnx_counts(self.h, C.byref(ir), C.byref(op), C.byref(nn), C.byref(ni)))
        return dict(ir_version=ir.value, opset=op.value, nodes=nn.value, initializers=ni.value)

    def initializer(self, index):
        info = OnnxTensorInfo()
        _check(self.lib.piper_hip_onnx_initializer(self.h, index, C.byref(info)))
        return dict(name=info.name.decode(), data_type=info.data_type, dims=[int(d) for d in info.dims[:info.rank]],
                    count=int(info.count))

    def find(self, name):
        return int(self.lib.piper_hip_onnx_find(self.h, name.encode()))

    def read_f32(self, index):
        n = self.initializer(index)["count"]
        out = np.empty(n, np.float32)
        _check(self.lib.piper_hip_onnx_read_f32(self.h, index, out.ctypes.data_as(c_f32p), n))
        return out

    def infer_config(self):
        cfg = VoiceConfig()
        _check(self.lib.piper_hip_onnx_infer_config(self.h, C.byref(cfg)))
        return cfg

    def verify_graph(self, cfg):
        """Raises (UNSUPPORTED, naming the first differing node) unless the node graph is the computation the launch schedule performs."""
        _check(self.lib.piper_hip_onnx_verify_graph(self.h, C.byref(cfg)))

    def build_blob(self, cfg, verify=True):
        blob = np.empty(blob_floats(cfg), np.float32)
        fn = self.lib.piper_hip_onnx_build_blob if verify else self.lib.piper_hip_onnx_build_blob_unchecked
        _check(fn(self.h, C.byref(cfg), blob.ctypes.data_as(c_f32p), blob.size))
        return blob

    def infer_config_speakers(self):
        """infer_config that does not refuse a multi-speaker file (`emb_g` / `cond` initializers)."""
        cfg = VoiceConfig()
        _check(self.lib.piper_hip_onnx_infer_config_speakers(self.h, C.byref(cfg)))
        return cfg

    def speaker_config(self, cfg):
        """The file's speaker table (n_speakers = 0: none); raises ShapeMismatch naming a missing or misshapen cond tensor."""
        scfg = SpeakerConfig()
        _check(self.lib.piper_hip_onnx_speaker_config(self.h, C.byref(cfg), C.byref(scfg)))
        return scfg

    def build_speaker_blob(self, cfg, scfg):
        blob = np.empty(speaker_blob_floats(cfg, scfg), np.float32)
        _check(self.lib.piper_hip_onnx_build_speaker_blob(self.h, C.byref(cfg), C.byref(scfg), blob.ctypes.data_as(c_f32p), blob.size))
        return blob


def load_voice(onnx_path, json_path=None, verify=True, speakers=False):
    """(cfg, blob, json info) of a Piper voice: `<voice>.onnx` + `<voice>.onnx.json` (PiperVoices layout). The node graph is verified
    against the launch schedule (refused otherwise) unless verify=False.
    speakers=True: a multi-speaker voice is taken instead of refused and the result is (cfg, blob, json info, scfg, speaker blob) — for
    HipRuntime(...).attach_speakers(scfg, speaker_blob); scfg.n_speakers == 0 and a None blob for a file without a table. No verifier
    for the conditioned graph exists yet: the main blob of a file WITH a table is built unchecked, whatever `verify` says."""
    m = OnnxModel(onnx_path)
    try:
        if speakers:
            cfg = m.infer_config_speakers()
            scfg = m.speaker_config(cfg)
            info = None
            jp = json_path or (str(onnx_path) + ".json")
            if os.path.exists(jp):
                info = piper_json(open(jp, "r", encoding="utf-8").read())
                if scfg.n_speakers:
                    _check(load_library().piper_hip_voice_check_json_speakers(C.byref(cfg), C.byref(scfg), C.byref(info)))
                else:
                    _check(load_library().piper_hip_voice_check_json(C.byref(cfg), C.byref(info)))
                cfg.sample_rate = info.sample_rate
            if not scfg.n_speakers:
                return cfg, m.build_blob(cfg, verify), info, scfg, None
            return cfg, m.build_blob(cfg, False), info, scfg, m.build_speaker_blob(cfg, scfg)
        cfg = m.infer_config()
        info = None
        jp = json_path or (str(onnx_path) + ".json")
        if os.path.exists(jp):
            info = piper_json(open(jp, "r", encoding="utf-8").read())
            _check(load_library().piper_hip_voice_check_json(C.byref(cfg), C.byref(info)))  # multi-speaker / vocabulary mismatch
            cfg.sample_rate = info.sample_rate
        return cfg, m.build_blob(cfg, verify), info
    finally:
        m.close()


def pcm16(samples):
    a = np.ascontiguousarray(samples, np.float32)
    out = np.empty(a.size, np.int16)
    _check(load_library().piper_hip_pcm16_from_f32(a.ctypes.data_as(c_f32p), a.size, out.ctypes.data_as(C.POINTER(C.c_int16))))
    return out


def wav_write(path, samples, sample_rate=22050):
    a = np.ascontiguousarray(samples, np.float32)
    _check(load_library().piper_hip_wav_write(str(path).encode(), a.ctypes.data_as(c_f32p), a.size, int(sample_rate)))


def wav_write_pcm16(path, pcm, sample_rate=22050):
    """A mono WAV file from samples that are 16-bit PCM already, at the rate they were delivered."""
    a = np.ascontiguousarray(pcm, np.int16)
    _check(load_library().piper_hip_wav_write_pcm16(str(path).encode(), a.ctypes.data_as(c_i16p), a.size, int(sample_rate)))


def g711_encode(pcm, law):
    """int16 samples → G.711 bytes ("mulaw" / "alaw") on the host (piper_hip_g711_from_pcm16): the function the device applies."""
    a = np.ascontiguousarray(pcm, np.int16)
    out = np.empty(a.size, np.uint8)
    _check(load_library().piper_hip_g711_from_pcm16(_law(law), a.ctypes.data_as(c_i16p), a.size, out.ctypes.data_as(c_u8p)))
    return out


def g711_decode(data, law):
    """G.711 bytes → int16 samples on the host (piper_hip_g711_to_pcm16)."""
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
    out = np.empty(a.size, np.int16)
    _check(load_library().piper_hip_g711_to_pcm16(_law(law), a.ctypes.data_as(c_u8p), a.size, out.ctypes.data_as(c_i16p)))
    return out


def wav_write_g711(path, data, law, sample_rate=8000):
    """A mono G.711 WAV file (format tag 7 / 6, fact chunk) from bytes that are companded already."""
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
    _check(load_library().piper_hip_wav_write_g711(str(path).encode(), _law(law), a.ctypes.data_as(c_u8p), a.size, int(sample_rate)))


def resample_info(in_rate, out_rate):
    """(L, M, taps per phase) of the output-rate contract for a rate pair; UnsupportedOp for a pair outside it. Host-only."""
    L, M, P = C.c_int32(), C.c_int32(), C.c_int32()
    _check(load_library().piper_hip_resample_info(int(in_rate), int(out_rate), C.byref(L), C.byref(M), C.byref(P)))
    return L.value, M.value, P.value


def resample_taps(in_rate, out_rate):
    """The [L][P] float32 coefficient table the kernels use for a rate pair. Host-only."""
    L, _, P = resample_info(in_rate, out_rate)
    out = np.empty((L, P), np.float32)
    _check(load_library().piper_hip_resample_taps(int(in_rate), int(out_rate), out.ctypes.data_as(c_f32p), out.size))
    return out


def _count(rc):
    if rc < 0:
        _check(int(rc))
    return int(rc)


def resample_count(in_rate, out_rate, n_in):
    """J(n_in): the samples an item of n_in samples yields at out_rate. Host-only."""
    return _count(load_library().piper_hip_resample_count(int(in_rate), int(out_rate), int(n_in)))


def pitch_check(pitch):
    """Raises InvalidArgument, naming the field, for a pitch outside the contract (piper_hip_pitch_check). Host-only."""
    _check(load_library().piper_hip_pitch_check(C.byref(_pitch(pitch))))


def pitch_info(semitones):
    """(Q, taps, length_factor) of a shift: the 32.32 step, P, and rf = (float)(Q / 2^32) (piper_hip_pitch_info). Host-only."""
    q, p, f = C.c_uint64(), C.c_int32(), C.c_float()
    _check(load_library().piper_hip_pitch_info(float(semitones), C.byref(q), C.byref(p), C.byref(f)))
    return q.value, p.value, np.float32(f.value)


def pitch_count(semitones, n_in):
    """N': the samples an item of n_in samples yields under a shift (piper_hip_pitch_count). Host-only."""
    return _count(load_library().piper_hip_pitch_count(float(semitones), int(n_in)))


def pitch_taps(semitones):
    """The [129][P] float32 coefficient table the kernel uses for a shift (piper_hip_pitch_taps). Host-only."""
    _, P, _ = pitch_info(semitones)
    out = np.empty((129, P), np.float32)
    _check(load_library().piper_hip_pitch_taps(float(semitones), out.ctypes.data_as(c_f32p), out.size))
    return out


def pitch_from_f32(samples, semitones):
    """The host twin of the pitch kernel (piper_hip_pitch_from_f32): n float32 → N' float32. Host-only."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    y = np.empty(pitch_count(semitones, x.size), np.float32)
    got = C.c_size_t()
    _check(load_library().piper_hip_pitch_from_f32(float(semitones), x.ctypes.data_as(c_f32p), x.size, y.ctypes.data_as(c_f32p), y.size,
                                                   C.byref(got)))
    assert got.value == y.size
    return y


def resample_step_bound(in_rate, out_rate, n_in):
    """The most samples one stream row delivers in a step over n_in input samples. Host-only."""
    return _count(load_library().piper_hip_resample_step_bound(int(in_rate), int(out_rate), int(n_in)))


def level_check(level):
    """InvalidArgument naming the field for a level outside the contract (piper_hip_level_check). Host-only."""
    lv = _level(level)
    _check(load_library().piper_hip_level_check(C.byref(lv)))


def level_info(level, rate):
    """The fp32 release step per block of that level at `rate`. Host-only."""
    lv, rel = _level(level), C.c_float()
    _check(load_library().piper_hip_level_info(C.byref(lv), int(rate), C.byref(rel)))
    return np.float32(rel.value)


def level_ready(e):
    """The limited samples that are final when samples [0, e) of a longer item are known. Host-only."""
    return _count(load_library().piper_hip_level_ready(int(e)))


def level_step_bound(n_in):
    """The most limited samples one stream row delivers in a step over n_in input samples. Host-only."""
    return _count(load_library().piper_hip_level_step_bound(int(n_in)))


def join_check(join, gaps=None):
    """InvalidArgument naming the field for a join outside the contract (piper_hip_join_check). Host-only."""
    jn, g, ng = _join(join, gaps)
    _check(load_library().piper_hip_join_check(C.byref(jn) if jn is not None else None, g, ng))


def join_counts(join, rate):
    """dict(lead=, gap=, tail=, pad=, fade=): the S() sample counts of the join at `rate` (piper_hip_join_counts). Host-only."""
    jn, _g, _n = _join(join)
    v = [C.c_int64() for _ in range(5)]
    _check(load_library().piper_hip_join_counts(C.byref(jn), int(rate), *[C.byref(x) for x in v]))
    return dict(zip(("lead", "gap", "tail", "pad", "fade"), (int(x.value) for x in v)))


def join_capacity(join, rate, item_samples, gaps=None):
    """The no-trim upper bound on the programme's samples (piper_hip_join_capacity). Host-only."""
    jn, g, ng = _join(join, gaps)
    n = np.ascontiguousarray(item_samples, np.int64).reshape(-1)
    out = C.c_int64()
    _check(load_library().piper_hip_join_capacity(C.byref(jn), g, ng, int(rate), n.ctypes.data_as(c_i64p), n.size, C.byref(out)))
    return int(out.value)


def join_from_f32(items, join, rate, gaps=None):
    """The join on the host (piper_hip_join_from_f32), bit for bit what the device computes: items = a list of float32 arrays →
    (programme, start [n], len [n], total)."""
    arrs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in items]
    ln = np.array([a.size for a in arrs], np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64) if arrs else np.zeros(0, np.int64)
    x = np.concatenate(arrs + [np.zeros(1, np.float32)])
    jn, g, ng = _join(join, gaps)
    cap = join_capacity(jn, rate, ln, gaps)
    y = np.empty(max(cap, 1), np.float32)
    start, length, total = np.zeros(max(ln.size, 1), np.int64), np.zeros(max(ln.size, 1), np.int64), C.c_int64()
    _check(load_library().piper_hip_join_from_f32(C.byref(jn), g, ng, int(rate), x.ctypes.data_as(c_f32p), off.ctypes.data_as(c_i64p),
                                                  ln.ctypes.data_as(c_i64p), ln.size, y.ctypes.data_as(c_f32p), cap,
                                                  start.ctypes.data_as(c_i64p), length.ctypes.data_as(c_i64p), C.byref(total)))
    return y[:total.value], start[:ln.size], length[:ln.size], int(total.value)


def eq_check(eq, rate):
    """InvalidArgument naming the field and the section for an EQ outside the contract at `rate` (piper_hip_eq_check). Host-only."""
    e = _eq(eq)
    _check(load_library().piper_hip_eq_check(C.byref(e), int(rate)))


def eq_design(eq, rate):
    """[n][5] float64 {b0, b1, b2, a1, a2} per section (piper_hip_eq_design). Host-only."""
    e = _eq(eq)
    out = np.zeros((max(e.n, 1), 5), np.float64)
    _check(load_library().piper_hip_eq_design(C.byref(e), int(rate), out.ctypes.data_as(c_f64p)))
    return out[:e.n]


def eq_from_f32(samples, eq, rate):
    """The equaliser on the host (piper_hip_eq_from_f32), bit for bit what the device computes."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    y = np.empty(max(x.size, 1), np.float32)
    e = _eq(eq)
    _check(load_library().piper_hip_eq_from_f32(C.byref(e), int(rate), x.ctypes.data_as(c_f32p), x.size, y.ctypes.data_as(c_f32p)))
    return y[:x.size]


def level_from_f32(samples, level, rate):
    """The limiter on the host (piper_hip_level_from_f32), bit for bit what the device computes."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    y = np.empty(x.size, np.float32)
    lv = _level(level)
    _check(load_library().piper_hip_level_from_f32(C.byref(lv), int(rate), x.ctypes.data_as(c_f32p), x.size, y.ctypes.data_as(c_f32p)))
    return y


def loudness_check(loudness):
    """InvalidArgument naming the field for a loudness target outside the contract (piper_hip_loudness_check). Host-only."""
    ld = _loudness(loudness)
    _check(load_library().piper_hip_loudness_check(C.byref(ld)))


def loudness_coeffs(rate):
    """(shelf_b, shelf_a, hp_b, hp_a), float64 [3] each: the K-weighting biquads at `rate` (piper_hip_loudness_coeffs). Host-only."""
    c = [np.empty(3, np.float64) for _ in range(4)]
    _check(load_library().piper_hip_loudness_coeffs(int(rate), *[a.ctypes.data_as(c_f64p) for a in c]))
    return tuple(c)


def loudness_from_f32(samples, rate):
    """BS.1770 integrated loudness of host floats in LUFS (piper_hip_loudness_from_f32): the sequential double twin of the kernels."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    out = C.c_float()
    _check(load_library().piper_hip_loudness_from_f32(int(rate), x.ctypes.data_as(c_f32p), x.size, C.byref(out)))
    return np.float32(out.value)


def loudness_gain(loudness, lufs):
    """The fp32 gain that target implies for an item measured at `lufs` (piper_hip_loudness_gain); 1.0 for −inf. Host-only."""
    ld, g = _loudness(loudness), C.c_float()
    _check(load_library().piper_hip_loudness_gain(C.byref(ld), float(lufs), C.byref(g)))
    return np.float32(g.value)


def piper_json(text):
    info = PiperJsonInfo()
    _check(load_library().piper_hip_piper_json(text.encode("utf-8"), C.byref(info)))
    return info


class StreamPool:
    """What HipRuntime.stream_pool returns: join() new sessions, step() for the next chunk of every active one, drop() a session."""

    def __init__(self, rt, slot, capacity, chunk_frames, work_slot):
        self.rt, self.slot, self.capacity, self.chunk_frames, self.work_slot = rt, slot, capacity, chunk_frames, work_slot
        self._buf = np.empty(max(capacity * chunk_frames * rt.cfg.hop, 1), np.float32)
        self._got = (C.c_int64 * capacity)()
        self._off = (C.c_int64 * capacity)()
        self.rate = None
        self.mixed = False
        self.level = None
        self._fmt = {}  # (mixed) row → the StreamFormat of the session in it

    def set_mixed(self):
        """Every row picks its rate, encoding and gain (piper_hip_voice_stream_set_mixed): before the first join. join(formats=[...]) then
        brings the formats and step_mixed() is the pool's step."""
        self.rt.stream_set_mixed(self.slot)
        self.mixed = True
        self._resize()

    def _resize(self):
        """The step buffer for the pool as it stands: the level's per-row bound in place of the chunk, the rate's on top of it."""
        rt = self.rt
        if self.mixed:  # the largest share a row can have: f32 at the highest rate
            per = self.chunk_frames * rt.cfg.hop
            if self.level is not None:
                per = level_step_bound(per)
                per = max(per, resample_step_bound(rt.cfg.sample_rate, 48000, per))
            self._buf = np.empty(max(self.capacity * (per + 1), self._buf.size), np.float32)
        elif self.rate:
            self._buf = np.empty((rt.stream_step_capacity(self.slot) + 1) // 2, np.float32)
        else:
            self._buf = np.empty(max(rt.stream_step_capacity(self.slot), 1), np.float32)

    def set_eq(self, eq):
        """An equaliser on every row (piper_hip_voice_stream_set_eq): before the first join, with set_rate, set_mixed or set_level in
        either order."""
        self.rt.stream_set_eq(self.slot, eq)

    def set_level(self, level):
        """A look-ahead limiter on every row (piper_hip_voice_stream_set_level): before the first join, with set_rate or set_mixed in
        either order."""
        self.rt.stream_set_level(self.slot, level)
        self.level = _level(level)
        self._resize()

    def set_rate(self, rate):
        """Deliver at `rate` Hz (piper_hip_voice_stream_set_rate): before the first join. step() then returns int16 chunks only."""
        self.rt.stream_set_rate(self.slot, rate)
        if int(rate) == self.rt.cfg.sample_rate:  # not a filter: the pool stays as it was opened, float steps included
            self.rate = None
            return
        self.rate = int(rate)
        self._resize()

    def join(self, utterances, noiseScale=0.667, formats=None, prosody=None, volume=None):
        """utterances as for synthesize_stream_batch: (phonemeIDs, durations-or-None, noise-or-None[, dict]). Returns [(item, samples)]:
        the row each session took and the samples it will deliver in all. Active from the next step().
        formats (a mixed pool): one StreamFormat (or dict of stream_format's arguments, or None) per utterance
        (piper_hip_voice_stream_pool_join_formats); without it the sessions join in the default format.
        prosody, volume: one entry per utterance, as for slot_prosody / slot_volume (staged on the work slot); a session with a volume
        delivers every chunk under its envelope, a session without brings none into its row."""
        rt, n = self.rt, len(utterances)
        arr = (Utterance * max(n, 1))()
        keep = []
        for i, item in enumerate(utterances):
            ids, dur, noise = item[:3]
            u, k = rt._utt(ids, dur, noise, noiseScale, **(item[3] if len(item) > 3 else {}))
            arr[i] = u
            keep.append(k)
        items = (C.c_int * max(n, 1))()
        samples = (C.c_int64 * max(n, 1))()
        fa = None
        if formats is not None:
            if len(formats) != n:
                raise InvalidArgument("join: %d formats for %d utterances" % (len(formats), n))
            fa = _formats(formats)
        # one entry per utterance, as for slot_prosody; staged behind every refusal made here, so that the join below is what takes it
        rt._stage_prosody(self.work_slot, prosody, [len(u[0]) for u in utterances])
        rt._stage_volume(self.work_slot, volume, [len(u[0]) for u in utterances])
        if fa is not None:
            _check(rt.lib.piper_hip_voice_stream_pool_join_formats(rt.voice, self.slot, arr, n, self.work_slot, fa, items, samples))
        else:
            _check(rt.lib.piper_hip_voice_stream_pool_join(rt.voice, self.slot, arr, n, self.work_slot, items, samples))
        rt._keep.pop(self.work_slot, None)  # the inputs were copied before the call returned
        if self.mixed:
            for i in range(n):
                self._fmt[int(items[i])] = rt.stream_item_format(self.slot, int(items[i]))
            need = rt.stream_step_capacity_bytes(self.slot)
            if need > self._buf.nbytes:
                self._buf = np.empty((need + 3) // 4, np.float32)
        return [(int(items[i]), int(samples[i])) for i in range(n)]

    def join_bounded(self, utterances, max_frames, noiseScale=0.667, formats=None, prosody=None, volume=None):
        """join() for utterances whose durations are predicted, without the host round trip (piper_hip_voice_stream_pool_join_bounded):
        at most max_frames frames per item, durations and noise None (the dict's noise_mode="device" draws the noise on the device).
        Nothing waits for the GPU. Returns [item, ...], the rows taken; item_samples(item) tells what each will deliver once its length
        is known and raises ShapeMismatch for an item the predictor made longer than max_frames (that row is free again).
        prosody (fit=1 compresses to max_frames), volume: one entry per utterance, as for join(); the gains follow the frames the device
        decides."""
        rt, n = self.rt, len(utterances)
        arr = (Utterance * max(n, 1))()
        keep = []
        for i, item in enumerate(utterances):
            ids, dur, noise = item[:3]
            u, k = rt._utt(ids, dur, noise, noiseScale, **(item[3] if len(item) > 3 else {}))
            arr[i] = u
            keep.append(k)
        items = (C.c_int * max(n, 1))()
        fa = None
        if formats is not None:
            if len(formats) != n:
                raise InvalidArgument("join_bounded: %d formats for %d utterances" % (len(formats), n))
            fa = _formats(formats)
        rt._stage_prosody(self.work_slot, prosody, [len(u[0]) for u in utterances])  # one entry per utterance; fit=1 compresses to max_frames
        rt._stage_volume(self.work_slot, volume, [len(u[0]) for u in utterances])
        _check(rt.lib.piper_hip_voice_stream_pool_join_bounded(rt.voice, self.slot, arr, n, self.work_slot, int(max_frames), fa, items))
        rt._keep.pop(self.work_slot, None)  # the inputs were copied before the call returned
        if self.mixed:
            for i in range(n):
                self._fmt[int(items[i])] = rt.stream_item_format(self.slot, int(items[i]))
            need = rt.stream_step_capacity_bytes(self.slot)
            if need > self._buf.nbytes:
                self._buf = np.empty((need + 3) // 4, np.float32)
        return [int(items[i]) for i in range(n)]

    def item_samples(self, item):
        """Total samples the occupant of row `item` will deliver, at the row's rate (piper_hip_voice_stream_pool_item_samples); waits for
        the join that filled the row if it is still running. ShapeMismatch: a bounded join's item over its max_frames."""
        got = C.c_int64()
        _check(self.rt.lib.piper_hip_voice_stream_pool_item_samples(self.rt.voice, self.slot, int(item), C.byref(got)))
        return int(got.value)

    def joins_pending(self):
        """Joins whose encoder + flow have not finished yet (piper_hip_voice_stream_pool_joins_pending); never waits."""
        return _count(self.rt.lib.piper_hip_voice_stream_pool_joins_pending(self.rt.voice, self.slot))

    def step_mixed(self, raw=False):
        """The step of a mixed pool (piper_hip_voice_stream_next_batch_mixed): a list with one numpy array per row, of the row's dtype
        (int16, uint8 or float32) and empty where the row delivered nothing; all empty when the pool is idle.
        raw=True: (n_samples, byte_off, bytes) as the library returned them instead."""
        rt = self.rt
        buf = self._buf.view(np.uint8)
        _check(rt.lib.piper_hip_voice_stream_next_batch_mixed(rt.voice, self.slot, buf.ctypes.data_as(c_vp), buf.size, self._got, self._off))
        counts, offs = [int(x) for x in self._got], [int(x) for x in self._off]
        out, total = [], 0
        for r in range(self.capacity):
            dt = np.dtype(self._fmt[r].dtype if r in self._fmt else np.int16)
            out.append(buf[offs[r]:offs[r] + counts[r] * dt.itemsize].view(dt).copy() if counts[r] else np.empty(0, dt))
            if counts[r]:
                total = offs[r] + counts[r] * dt.itemsize
        return (counts, offs, buf[:total].copy()) if raw else out

    def step(self, pcm=False, gain=1.0, normalize=False, encoding=None):
        """{item: chunk} of every active session; an empty dict when the pool is idle. pcm=True: int16 chunks converted on the device
        (piper_hip_voice_stream_next_batch_pcm16; normalize is refused there — UnsupportedOp — and consumes nothing). encoding "mulaw" /
        "alaw": uint8 chunks of G.711 bytes instead (piper_hip_voice_stream_next_batch_g711), at the pool's rate."""
        rt = self.rt
        if encoding is not None:
            buf = self._buf.view(np.uint8)[:self._buf.size * (4 if self.rate else 1)]
            prm = PcmParams(float(gain), int(bool(normalize)))
            _check(rt.lib.piper_hip_voice_stream_next_batch_g711(rt.voice, self.slot, C.byref(prm), _law(encoding), buf.ctypes.data_as(c_u8p),
                                                                 buf.size, self._got))
        elif pcm:
            buf = self._buf.view(np.int16)[:self._buf.size * (2 if self.rate else 1)]
            prm = PcmParams(float(gain), int(bool(normalize)))
            _check(rt.lib.piper_hip_voice_stream_next_batch_pcm16(rt.voice, self.slot, C.byref(prm), buf.ctypes.data_as(c_i16p), buf.size, self._got))
        else:
            buf = self._buf
            _check(rt.lib.piper_hip_voice_stream_next_batch(rt.voice, self.slot, buf.ctypes.data_as(c_f32p), buf.size, self._got))
        out, off = {}, 0
        for item in range(self.capacity):
            c = int(self._got[item])
            if c:
                out[item] = buf[off:off + c].copy()
                off += c
        return out

    def drop(self, item):
        _check(self.rt.lib.piper_hip_voice_stream_drop(self.rt.voice, self.slot, int(item)))

    @property
    def free_rows(self):
        rc = self.rt.lib.piper_hip_voice_stream_pool_free_rows(self.rt.voice, self.slot)
        if rc < 0:
            _check(rc)
        return rc

    def close(self):
        _check(self.rt.lib.piper_hip_voice_stream_pool_close(self.rt.voice, self.slot))


class HipRuntime:
    """PiperMetalRuntime.synthesize (PiperMetalRuntime.swift:62-80) over the C-ABI, durations/noise injected."""

    def __init__(self, backend, cfg, blob, on_device=False):
        self.backend, self.cfg, self.lib = backend, cfg, backend.lib
        v = c_vp()
        if on_device:
            ptr = blob
        else:
            self._blob = np.ascontiguousarray(blob, np.float32)
            ptr = self._blob.ctypes.data_as(c_vp)
        _check(self.lib.piper_hip_voice_create(backend.ctx, C.byref(cfg), ptr, int(on_device), C.byref(v)))
        self.voice = v
        self._keep = {}
        self._joins = {}  # slot id → (Join, gaps) while the slot id has a join (slot_join)
        self._pinned = []

    def close(self):
        if self.voice:
            self.lib.piper_hip_voice_destroy(self.voice)
            self.voice = None
        for p in self._pinned:
            self.lib.piper_hip_host_free(self.backend.ctx, p)
        self._pinned = []

    def attach_speakers(self, scfg, blob, on_device=False):
        """The speaker table of a multi-speaker voice (piper_hip_voice_attach_speakers): once, before the first prepare."""
        if on_device:
            ptr = _ptr(blob)
        else:
            self._spk_blob = np.ascontiguousarray(blob, np.float32)
            ptr = self._spk_blob.ctypes.data_as(c_vp)
        _check(self.lib.piper_hip_voice_attach_speakers(self.voice, C.byref(scfg), ptr, int(on_device)))

    def num_speakers(self):
        return int(self.lib.piper_hip_voice_num_speakers(self.voice))

    def slot_speakers(self, slot, speakers):
        """The speakers of the slot's items from now on: entry i for item i of every later prepare / stream begin (a pool join: of its work
        slot), the last entry for items past the list, None or [] = speaker 0 alone again. An entry is an id, a {id: weight} mix of up
        to four, or a Speaker."""
        speakers = list(speakers or [])
        arr = _speakers(speakers) if speakers else None
        _check(self.lib.piper_hip_voice_slot_speakers(self.voice, int(slot), arr, len(speakers)))

    def slot_prosody(self, slot, items, ts=None):
        """The prosody of the NEXT staging call on the slot id (piper_hip_voice_slot_prosody): entry i for item i, each a
        dict(length=, min_frames=, max_frames=, noise=, fit=), a Prosody, or None (neutral: needs ts[i], the item's number of ids). The
        library copies the arrays; the staging call takes the assignment whether or not it succeeds. None or [] clears it."""
        items = list(items or [])
        recs, keep = [], []
        for i, p in enumerate(items):
            r, k = _prosody(p, None if ts is None else ts[i])
            recs.append(r)
            keep.append(k)
        arr = (Prosody * len(recs))(*recs) if recs else None
        _check(self.lib.piper_hip_voice_slot_prosody(self.voice, int(slot), arr, len(recs)))

    def _stage_prosody(self, slot, prosody, ts):
        """The `prosody=` keyword of the staging methods: one entry per utterance (None entries neutral), or None for a request without."""
        if prosody is not None:
            self.slot_prosody(slot, prosody, ts)

    def slot_volume(self, slot, items, ts=None):
        """The volume of the NEXT staging call on the slot id (piper_hip_voice_slot_volume): entry i for item i, each an array of linear
        gains per id in [0, 16], a Volume, or None (all 1.0: needs ts[i], the item's number of ids). The library copies the arrays; the
        staging call takes the assignment whether or not it succeeds. None or [] clears it."""
        items = list(items or [])
        recs, keep = [], []
        for i, g in enumerate(items):
            r, k = _volume(g, None if ts is None else ts[i])
            recs.append(r)
            keep.append(k)
        arr = (Volume * len(recs))(*recs) if recs else None
        _check(self.lib.piper_hip_voice_slot_volume(self.voice, int(slot), arr, len(recs)))

    def _stage_volume(self, slot, volume, ts):
        """The `volume=` keyword of the staging methods: one entry per utterance (None entries all 1.0), or None for a request without."""
        if volume is not None:
            self.slot_volume(slot, volume, ts)

    def slot_pitch(self, slot, items):
        """The pitch of the NEXT staging call on the slot id (piper_hip_voice_slot_pitch): entry i for item i, each a number of semitones
        in [−12, 12] (keep_tempo on), a (semitones, keep_tempo) pair, a Pitch, or None (no pitch). The staging call takes the assignment
        whether or not it succeeds. None or [] clears it."""
        recs = [_pitch(p) for p in (items or [])]
        arr = (Pitch * len(recs))(*recs) if recs else None
        _check(self.lib.piper_hip_voice_slot_pitch(self.voice, int(slot), arr, len(recs)))

    def _stage_pitch(self, slot, pitch, n):
        """The `pitch=` keyword of the staging methods: one value for all n utterances, a list with one entry per utterance, or None."""
        if pitch is None:
            return
        if isinstance(pitch, list):
            self.slot_pitch(slot, pitch)
        else:
            self.slot_pitch(slot, [pitch] * n)

    def pitch_samples(self, slot):
        """Samples per batch item the slot delivers at the voice's rate, F'·hop under a pitch (piper_hip_voice_pitch_samples), and their
        sum; a bounded slot: its capacity before collect, the true values after. Without a pitch: prepared_samples."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        per = (C.c_int64 * max(nb, 1))()
        tot = C.c_int64()
        _check(self.lib.piper_hip_voice_pitch_samples(self.voice, slot, per, nb, C.byref(tot)))
        return [int(x) for x in per[:nb]], int(tot.value)

    def prosody_report(self, slot):
        """Per item of the slot: (frames the rule wanted before fitting, fitted?) — piper_hip_voice_prosody_report; answers where
        durations() answers."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        wanted = (C.c_int64 * max(nb, 1))()
        fitted = (C.c_int32 * max(nb, 1))()
        _check(self.lib.piper_hip_voice_prosody_report(self.voice, int(slot), wanted, fitted, nb))
        return [int(x) for x in wanted[:nb]], [int(x) for x in fitted[:nb]]

    def set_precision(self, precision):
        """"f32" (default, the parity configuration) or "bf16" (generator convs on bf16 operands, fp32 accumulate)."""
        code = {"f32": 0, "fp32": 0, "bf16": 1}.get(precision, precision)
        _check(self.lib.piper_hip_voice_set_precision(self.voice, int(code)))
        self._keep.clear()  # prepared slots are dropped by the library

    def _utt(self, ids, durations, noise, noise_scale, noise_mode="injected", seed=1234, length_scale=1.0, noise_w=0.8, dp_noise=None):
        """durations None ⇒ predicted on the device (duration predictor) from length_scale / noise_w / dp_noise."""
        ids = np.ascontiguousarray(ids, np.int64)
        dur = None if durations is None else np.ascontiguousarray(durations, np.int32)
        nz = None if noise is None else np.ascontiguousarray(noise, np.float32)
        dpn = None if dp_noise is None else np.ascontiguousarray(dp_noise, np.float32)
        u = Utterance(ids.ctypes.data_as(c_i64p), len(ids), None if dur is None else dur.ctypes.data_as(c_i32p),
                      None if nz is None else nz.ctypes.data_as(c_f32p), float(noise_scale),
                      NOISE_MODES.get(noise_mode, noise_mode), int(seed) & 0xFFFFFFFF, float(length_scale), float(noise_w),
                      None if dpn is None else dpn.ctypes.data_as(c_f32p))
        return u, (ids, dur, nz, dpn)

    def num_samples(self, ids, durations):
        u, _k = self._utt(ids, durations, None, 0.0)
        return int(self.lib.piper_hip_voice_num_samples(self.voice, C.byref(u)))

    def synthesize(self, phonemeIDs, durations=None, noise=None, noiseScale=0.667, lengthScale=1.0, noiseW=0.8, speaker=None, prosody=None, volume=None,
                   level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP, pitch=None, **kw):
        """PiperMetalRuntime.synthesize(phonemeIDs:noiseScale:lengthScale:noiseW:); `durations` / `noise` / dp_noise are the
        reference's `overrides`. Without durations the frames per id come from the voice's duration predictor.
        speaker (a voice with a speaker table): an id or a {id: weight} mix; it becomes slot 0's assignment (slot_speakers) and stays.
        level: a Level (or tuple / dict) becomes slot 0's level (slot_level) and stays; None clears it. loudness: the same for slot 0's
        loudness target (slot_loudness)."""
        if speaker is not None:
            self.slot_speakers(0, [speaker])
        self._slot_level(0, level)
        self._slot_loudness(0, loudness)
        self._slot_eq(0, eq)
        self._slot_join(0, join)
        if durations is not None and not kw:  # the one-call C entry point
            u, _k = self._utt(phonemeIDs, durations, noise, noiseScale)
            self._stage_prosody(0, None if prosody is None else [prosody], [len(phonemeIDs)])
            self._stage_volume(0, None if volume is None else [volume], [len(phonemeIDs)])
            self._stage_pitch(0, pitch, 1)
            n = self._one_call_room(int(self.lib.piper_hip_voice_num_samples(self.voice, C.byref(u))), pitch)
            out = np.empty(max(n, 1), np.float32)
            got = C.c_int64()
            _check(self.lib.piper_hip_voice_synthesize(self.voice, C.byref(u), out.ctypes.data_as(c_f32p), n, C.byref(got)))
            self._keep.pop(0, None)
            return out[:got.value]
        self.prepare(0, phonemeIDs, durations, noise, noiseScale, length_scale=lengthScale, noise_w=noiseW, prosody=prosody, volume=volume,
                     pitch=pitch, **kw)
        self.launch(0)
        return self.collect(0)

    def prepare(self, slot, phonemeIDs, durations=None, noise=None, noiseScale=0.667, noise_mode="injected", seed=1234, length_scale=1.0,
                noise_w=0.8, dp_noise=None, max_frames=None, prosody=None, volume=None, pitch=None):
        """max_frames (durations must be None): predicted durations WITHOUT the host round trip — the plan is the bucket of that bound and the
        frame count stays on the device until collect (piper_hip_voice_prepare_batch_bounded).
        prosody: the item's per-id prosody (slot_prosody), a dict(length=, min_frames=, max_frames=, noise=, fit=) or a Prosody.
        volume: the item's linear gains per id in [0, 16] (slot_volume): every collect of this staging delivers the samples under that
        envelope (include/piper_hip.h "Per-phoneme volume").
        pitch: semitones in [−12, 12] (the tempo kept: predicted durations only), or a (semitones, keep_tempo) pair (slot_pitch): every
        collect of this staging delivers the pitched item (include/piper_hip.h "Pitch"); pitch_samples(slot) is its length."""
        u, k = self._utt(phonemeIDs, durations, noise, noiseScale, noise_mode, seed, length_scale, noise_w, dp_noise)
        self._stage_prosody(slot, None if prosody is None else [prosody], [len(phonemeIDs)])
        self._stage_volume(slot, None if volume is None else [volume], [len(phonemeIDs)])
        self._stage_pitch(slot, pitch, 1)
        if max_frames is not None:
            rc = self.lib.piper_hip_voice_prepare_batch_bounded(self.voice, C.byref(u), 1, slot, int(max_frames))
        else:
            rc = self.lib.piper_hip_voice_prepare(self.voice, C.byref(u), slot)
        if rc < 0:
            _check(rc)
        tot = C.c_int64()
        _check(self.lib.piper_hip_voice_pitch_samples(self.voice, slot, None, 0, C.byref(tot)))
        self._keep[slot] = (k, int(tot.value), max_frames is not None)
        return rc

    def prepare_batch_bounded(self, slot, utterances, max_frames, noiseScale=0.667, noise_mode="device", seed=1234, length_scale=1.0, noise_w=0.8,
                              prosody=None, volume=None, pitch=None):
        """utterances: list of (phonemeIDs, dp_noise-or-None); durations predicted on the device, at most max_frames frames per item.
        prosody: one entry per utterance (None entries neutral), as for slot_prosody; an entry's fit=1 compresses an item over the bound.
        pitch: one value for all utterances or a list with one per utterance, as for slot_pitch; max_frames bounds the frames the model
        generates, before the pitch."""
        n = len(utterances)
        arr = (Utterance * n)()
        keep = []
        for i, (ids, dpn) in enumerate(utterances):
            u, k = self._utt(ids, None, None, noiseScale, noise_mode, seed, length_scale, noise_w, dpn)
            arr[i] = u
            keep.append(k)
        self._stage_prosody(slot, prosody, [len(u[0]) for u in utterances])
        self._stage_volume(slot, volume, [len(u[0]) for u in utterances])
        self._stage_pitch(slot, pitch, n)
        rc = self.lib.piper_hip_voice_prepare_batch_bounded(self.voice, arr, n, slot, int(max_frames))
        if rc < 0:
            _check(rc)
        tot = C.c_int64()
        _check(self.lib.piper_hip_voice_pitch_samples(self.voice, slot, None, 0, C.byref(tot)))
        self._keep[slot] = (keep, int(tot.value), True)
        return rc

    def prepared_samples(self, slot):
        """samples per batch item of the slot (a bounded slot: its capacity before collect, the true lengths after)."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        per = (C.c_int64 * max(nb, 1))()
        tot = C.c_int64()
        _check(self.lib.piper_hip_voice_prepared_samples(self.voice, slot, per, nb, C.byref(tot)))
        return [int(x) for x in per[:nb]], int(tot.value)

    def durations(self, slot):
        """Frames per id the prepared slot uses (supplied or predicted), items back to back."""
        n = C.c_int()
        _check(self.lib.piper_hip_voice_durations(self.voice, slot, None, 0, C.byref(n)))
        out = np.empty(n.value, np.int32)
        _check(self.lib.piper_hip_voice_durations(self.voice, slot, out.ctypes.data_as(c_i32p), n.value, C.byref(n)))
        return out

    def predict_durations(self, utterances, noise_w=0.8, length_scale=1.0, noise_mode="injected", seed=1234, speakers=None):
        """utterances: list of (phonemeIDs, dp_noise-or-None). Returns (durations, logw) lists per utterance. speakers (a voice with a
        speaker table): one entry per utterance, as for slot_speakers (piper_hip_voice_predict_durations_speakers)."""
        n = len(utterances)
        arr = (Utterance * n)()
        keep = []
        for i, (ids, dpn) in enumerate(utterances):
            u, k = self._utt(ids, None, None, 0.0, noise_mode, seed, length_scale, noise_w, dpn)
            arr[i] = u
            keep.append(k)
        total = sum(len(u[0]) for u in utterances)
        dur = np.empty(total, np.int32)
        lw = np.empty(total, np.float32)
        if speakers is not None:
            _check(self.lib.piper_hip_voice_predict_durations_speakers(self.voice, arr, n, _speakers(list(speakers)), dur.ctypes.data_as(c_i32p),
                                                                       lw.ctypes.data_as(c_f32p), total))
        else:
            _check(self.lib.piper_hip_voice_predict_durations(self.voice, arr, n, dur.ctypes.data_as(c_i32p), lw.ctypes.data_as(c_f32p), total))
        outs, off = [], 0
        for ids, _ in utterances:
            outs.append((dur[off:off + len(ids)].copy(), lw[off:off + len(ids)].copy()))
            off += len(ids)
        return outs

    def stream_set_rate(self, slot, rate):
        """The output rate of the stream on `slot` (piper_hip_voice_stream_set_rate): after its begin / open, before its first step."""
        _check(self.lib.piper_hip_voice_stream_set_rate(self.voice, slot, int(rate)))

    def stream_rate(self, slot):
        return _count(self.lib.piper_hip_voice_stream_rate(self.voice, slot))

    def stream_step_capacity(self, slot):
        """The int16 samples one step of the stream on `slot` can deliver at its current rate."""
        return _count(self.lib.piper_hip_voice_stream_step_capacity(self.voice, slot))

    def slot_level(self, slot, level):
        """The level of slot id `slot`'s whole-item collects (piper_hip_voice_slot_level): it persists until replaced; None clears it."""
        if level is None:
            _check(self.lib.piper_hip_voice_slot_level(self.voice, slot, None))
        else:
            lv = _level(level)
            _check(self.lib.piper_hip_voice_slot_level(self.voice, slot, C.byref(lv)))

    def slot_join(self, slot, join, gaps=None):
        """The join of slot id `slot`'s whole-item collects (piper_hip_voice_slot_join): a Join or a dict (gaps= may be a list of per-item
        gaps in ms); it persists until replaced; None clears it. Every later collect* of the slot delivers ONE programme."""
        jn, g, ng = _join(join, gaps)
        _check(self.lib.piper_hip_voice_slot_join(self.voice, slot, C.byref(jn) if jn is not None else None, g, ng))
        if jn is None:
            self._joins.pop(slot, None)
        else:
            self._joins[slot] = (jn, [float(x) for x in g] if g is not None else None)

    def _slot_join(self, slot, join):
        if join is not KEEP:
            self.slot_join(slot, join)

    def join_capacity(self, slot, rate=None):
        """The samples a collect* of the prepared, joined slot needs room for at `rate` (piper_hip_voice_join_capacity)."""
        out = C.c_int64()
        _check(self.lib.piper_hip_voice_join_capacity(self.voice, slot, 0 if rate is None else int(rate), C.byref(out)))
        return int(out.value)

    def join_report(self, slot):
        """(start [NB], len [NB], total) of the slot's latest joined collect, at the voice's rate (piper_hip_voice_join_report)."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        start, length, total = np.zeros(max(nb, 1), np.int64), np.zeros(max(nb, 1), np.int64), C.c_int64()
        _check(self.lib.piper_hip_voice_join_report(self.voice, slot, start.ctypes.data_as(c_i64p), length.ctypes.data_as(c_i64p), nb, C.byref(total)))
        return start[:nb], length[:nb], int(total.value)

    def _collect_joined(self, slot, dtype, rate, out, call):
        """A collect* of a joined slot: room for join_capacity at `rate`, call(pointer-able array, room), then the programme's count."""
        src = self.cfg.sample_rate
        room = self.join_capacity(slot, rate)
        if out is None:
            out = np.empty(max(room, 1), dtype)
        assert out.dtype == dtype and out.size >= room and out.flags.c_contiguous
        call(out, room)
        if len(self._keep[slot]) > 2 and self._keep[slot][2]:  # bounded: the true lengths are known now
            self._keep[slot] = (self._keep[slot][0], self.pitch_samples(slot)[1], False)
        total = self.join_report(slot)[2]
        return out[:total if rate is None or int(rate) == src else resample_count(src, int(rate), total)]

    def _one_call_room(self, n, pitch=None):
        """samples of slot 0's one-item programme for an utterance of n samples under `pitch` (the synthesize twins)"""
        if pitch is not None:
            hop = self.cfg.hop
            n = -(-pitch_count(_pitch(pitch).semitones, n) // hop) * hop
        if 0 not in self._joins:
            return n
        jn, g = self._joins[0]
        return join_capacity(jn, self.cfg.sample_rate, [n], g)

    def slot_eq(self, slot, eq):
        """The equaliser of slot id `slot`'s whole-item collects (piper_hip_voice_slot_eq): an Eq or a list of (type, f0, q[, gain_db]);
        it persists until replaced; None clears it."""
        if eq is None:
            _check(self.lib.piper_hip_voice_slot_eq(self.voice, slot, None))
        else:
            e = _eq(eq)
            _check(self.lib.piper_hip_voice_slot_eq(self.voice, slot, C.byref(e)))

    def _slot_eq(self, slot, eq):
        if eq is not KEEP:
            self.slot_eq(slot, eq)

    def _slot_level(self, slot, level):
        if level is not KEEP:
            self.slot_level(slot, level)

    def slot_loudness(self, slot, loudness):
        """The loudness target of slot id `slot`'s whole-item collects (piper_hip_voice_slot_loudness): a Loudness, a target in LUFS, a
        (target_lufs, max_gain_db) pair or a dict; it persists until replaced; None clears it."""
        if loudness is None:
            _check(self.lib.piper_hip_voice_slot_loudness(self.voice, slot, None))
        else:
            ld = _loudness(loudness)
            _check(self.lib.piper_hip_voice_slot_loudness(self.voice, slot, C.byref(ld)))

    def _slot_loudness(self, slot, loudness):
        if loudness is not KEEP:
            self.slot_loudness(slot, loudness)

    def loudness(self, slot):
        """(lufs, gain), float32 per item: the BS.1770 integrated loudness of the raw items of the slot's latest launch, measured on the
        device, and the gain the slot's target implies (1.0 without one) — piper_hip_voice_loudness. Waits for the slot."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        lufs, gain = np.empty(max(nb, 1), np.float32), np.empty(max(nb, 1), np.float32)
        _check(self.lib.piper_hip_voice_loudness(self.voice, slot, lufs.ctypes.data_as(c_f32p), gain.ctypes.data_as(c_f32p), nb))
        return lufs[:nb], gain[:nb]

    def stream_set_level(self, slot, level):
        """The level of the stream on `slot` (piper_hip_voice_stream_set_level): after its begin / open, before its first step."""
        lv = _level(level)
        _check(self.lib.piper_hip_voice_stream_set_level(self.voice, slot, C.byref(lv)))

    def stream_set_eq(self, slot, eq):
        """The EQ of the stream on `slot` (piper_hip_voice_stream_set_eq): after its begin / open, before its first step."""
        e = _eq(eq)
        _check(self.lib.piper_hip_voice_stream_set_eq(self.voice, slot, C.byref(e)))

    def stream_eq(self, slot):
        out = Eq()
        _check(self.lib.piper_hip_voice_stream_eq(self.voice, slot, C.byref(out)))
        return out

    def stream_level(self, slot):
        out = Level()
        _check(self.lib.piper_hip_voice_stream_level(self.voice, slot, C.byref(out)))
        return out

    def stream_set_mixed(self, slot):
        """Marks the batched stream on `slot` mixed (piper_hip_voice_stream_set_mixed): every row picks its rate, encoding and gain."""
        _check(self.lib.piper_hip_voice_stream_set_mixed(self.voice, slot))

    def stream_item_formats(self, slot, formats):
        """The formats of a mixed group's items (piper_hip_voice_stream_item_formats): items past the list take the last entry."""
        _check(self.lib.piper_hip_voice_stream_item_formats(self.voice, slot, _formats(formats), len(formats)))

    def stream_item_format(self, slot, item):
        out = StreamFormat()
        _check(self.lib.piper_hip_voice_stream_item_format(self.voice, slot, int(item), C.byref(out)))
        return out

    def stream_step_capacity_bytes(self, slot):
        """The bytes one step of the mixed stream on `slot` can deliver with the rows' current formats."""
        return _count(self.lib.piper_hip_voice_stream_step_capacity_bytes(self.voice, slot))

    def synthesize_stream(self, phonemeIDs, durations, noise=None, noiseScale=0.667, chunkFrames=64, slot=0, pcm=False, gain=1.0, rate=None,
                          encoding=None, prosody=None, volume=None, level=None, eq=None):
        """Generator of waveform chunks (PiperMetalRuntime.synthesizeStream): encoder + flow once, generator per window.
        prosody: the utterance's per-id prosody, as for prepare. volume: the utterance's linear gains per id, as for prepare: every chunk
        leaves under the envelope, and the concatenated chunks equal the whole-item result bit for bit.
        pcm=True: int16 chunks converted on the device (piper_hip_voice_stream_next_pcm16), scaled by `gain`. rate: int16 chunks at that
        output rate (stream_set_rate; implies pcm). encoding "mulaw" / "alaw": uint8 chunks of G.711 bytes instead of int16
        (piper_hip_voice_stream_next_g711), at `rate` or the voice's own."""
        u, keep = self._utt(phonemeIDs, durations, noise, noiseScale)
        self._stage_prosody(slot, None if prosody is None else [prosody], [len(phonemeIDs)])
        self._stage_volume(slot, None if volume is None else [volume], [len(phonemeIDs)])
        n_chunks = self.lib.piper_hip_voice_stream_begin(self.voice, C.byref(u), slot, int(chunkFrames))
        if n_chunks < 0:
            _check(n_chunks)
        law = None if encoding is None else _law(encoding)
        sample = np.uint8 if law is not None else np.int16
        buf = np.empty(int(chunkFrames) * self.cfg.hop, sample if pcm or rate or law is not None else np.float32)
        if eq is not None:  # an equaliser behind the volume (stream_set_eq)
            self.stream_set_eq(slot, eq)
        if level is not None:  # a look-ahead limiter in front of the output stage (stream_set_level)
            self.stream_set_level(slot, level)
            buf = np.empty(self.stream_step_capacity(slot), buf.dtype)
        if rate:
            pcm = True
            self.stream_set_rate(slot, rate)
            buf = np.empty(self.stream_step_capacity(slot), sample)
        got = C.c_int64()
        prm = PcmParams(float(gain), 0)
        while True:
            if law is not None:
                _check(self.lib.piper_hip_voice_stream_next_g711(self.voice, slot, C.byref(prm), law, buf.ctypes.data_as(c_u8p), buf.size,
                                                                 C.byref(got)))
            elif pcm:
                _check(self.lib.piper_hip_voice_stream_next_pcm16(self.voice, slot, C.byref(prm), buf.ctypes.data_as(c_i16p), buf.size, C.byref(got)))
            else:
                _check(self.lib.piper_hip_voice_stream_next(self.voice, slot, buf.ctypes.data_as(c_f32p), buf.size, C.byref(got)))
            if got.value == 0:
                return
            yield buf[:got.value].copy()

    def synthesize_stream_batch(self, utterances, noiseScale=0.667, chunkFrames=64, slot=0, pcm=False, gain=1.0, rate=None, encoding=None,
                                formats=None, prosody=None, volume=None, level=None, eq=None):
        """prosody: one entry per utterance (None entries neutral), as for slot_prosody.
        Batched stream (piper_hip_voice_stream_begin_batch): utterances = list of (phonemeIDs, durations-or-None, noise-or-None[, dict of
        noise_mode / seed / length_scale / noise_w]). Encoder + flow once for the group; yields, per step, a list of len(utterances)
        arrays — the next chunk of every item, empty once the item is finished or dropped (stream_drop). pcm=True: int16 chunks converted on
        the device (piper_hip_voice_stream_next_batch_pcm16), scaled by `gain`. rate: int16 chunks at that output rate (implies pcm).
        encoding "mulaw" / "alaw": uint8 chunks of G.711 bytes instead of int16 (piper_hip_voice_stream_next_batch_g711).
        formats: a mixed group — one StreamFormat (or dict, or None) per item, items past the list take the last; every step's arrays then
        have their item's dtype (piper_hip_voice_stream_next_batch_mixed). pcm, gain, rate and encoding must be left alone with it."""
        n = len(utterances)
        arr = (Utterance * max(n, 1))()
        keep = []
        for i, item in enumerate(utterances):
            ids, dur, noise = item[:3]
            u, k = self._utt(ids, dur, noise, noiseScale, **(item[3] if len(item) > 3 else {}))
            arr[i] = u
            keep.append(k)
        self._stage_prosody(slot, prosody, [len(u[0]) for u in utterances])
        self._stage_volume(slot, volume, [len(u[0]) for u in utterances])
        steps = self.lib.piper_hip_voice_stream_begin_batch(self.voice, arr, n, slot, int(chunkFrames))
        if steps < 0:
            _check(steps)
        if eq is not None:  # an equaliser on every row, behind the volume (stream_set_eq)
            self.stream_set_eq(slot, eq)
        if level is not None:  # a look-ahead limiter on every row, in front of the output stage (stream_set_level)
            self.stream_set_level(slot, level)
        if formats is not None:
            if pcm or rate or encoding is not None or gain != 1.0:
                raise InvalidArgument("synthesize_stream_batch: formats= carries the rate, encoding and gain of every item")
            self.stream_set_mixed(slot)
            self.stream_item_formats(slot, formats)
            dts = [np.dtype(self.stream_item_format(slot, i).dtype) for i in range(n)]
            raw = np.empty(max(self.stream_step_capacity_bytes(slot), 4), np.uint8)
            got, off = (C.c_int64 * n)(), (C.c_int64 * n)()
            while True:
                _check(self.lib.piper_hip_voice_stream_next_batch_mixed(self.voice, slot, raw.ctypes.data_as(c_vp), raw.size, got, off))
                if not any(int(x) for x in got):
                    return
                yield [raw[int(off[i]):int(off[i]) + int(got[i]) * dts[i].itemsize].view(dts[i]).copy() for i in range(n)]
        law = None if encoding is None else _law(encoding)
        sample = np.uint8 if law is not None else np.int16
        buf = np.empty(max(n * int(chunkFrames) * self.cfg.hop, 1), sample if pcm or rate or law is not None else np.float32)
        if level is not None:
            buf = np.empty(self.stream_step_capacity(slot), buf.dtype)
        if rate:
            pcm = True
            self.stream_set_rate(slot, rate)
            buf = np.empty(self.stream_step_capacity(slot), sample)
        got = (C.c_int64 * n)()
        prm = PcmParams(float(gain), 0)
        while True:
            if law is not None:
                _check(self.lib.piper_hip_voice_stream_next_batch_g711(self.voice, slot, C.byref(prm), law, buf.ctypes.data_as(c_u8p), buf.size, got))
            elif pcm:
                _check(self.lib.piper_hip_voice_stream_next_batch_pcm16(self.voice, slot, C.byref(prm), buf.ctypes.data_as(c_i16p), buf.size, got))
            else:
                _check(self.lib.piper_hip_voice_stream_next_batch(self.voice, slot, buf.ctypes.data_as(c_f32p), buf.size, got))
            counts = [int(x) for x in got]
            if not any(counts):
                return
            out, off = [], 0
            for c in counts:
                out.append(buf[off:off + c].copy())
                off += c
            yield out

    def stream_drop(self, slot, item):
        """The client of item `item` of the batched stream on `slot` went away: later steps skip it."""
        _check(self.lib.piper_hip_voice_stream_drop(self.voice, slot, int(item)))

    def stream_pool(self, slot, capacity, chunkFrames=64, work_slot=None, rate=None, mixed=False, level=None, eq=None):
        """A streaming pool (piper_hip_voice_stream_pool_open) of `capacity` rows on `slot`: sessions join and leave while it runs.
        work_slot: the slot id whose plan runs the joins' encoder + flow (default: the next slot id). mixed=True: every joining session
        brings its own format (join(formats=[...]), step_mixed())."""
        if work_slot is None:
            work_slot = slot + 1 if slot + 1 < 16 else slot - 1
        _check(self.lib.piper_hip_voice_stream_pool_open(self.voice, slot, int(capacity), int(chunkFrames)))
        self._keep.pop(slot, None)
        pool = StreamPool(self, slot, int(capacity), int(chunkFrames), int(work_slot))
        if rate:
            pool.set_rate(rate)
        if mixed:
            pool.set_mixed()
        if eq is not None:
            pool.set_eq(eq)
        if level is not None:
            pool.set_level(level)
        return pool

    def prepare_batch(self, slot, utterances, noiseScale=0.667, prosody=None, volume=None, pitch=None):
        """utterances: list of (phonemeIDs, durations, noise-or-None[, dict of noise_mode / seed / length_scale / noise_w / dp_noise]); lengths
        may differ (ragged batch, one bucket). prosody: one entry per utterance (None entries neutral), as for slot_prosody.
        volume: one array of gains per utterance (None entries all 1.0, utterances past the list have none), as for slot_volume.
        pitch: one value for all utterances or a list with one per utterance (None entries no pitch), as for slot_pitch."""
        n = len(utterances)
        arr = (Utterance * n)()
        keep = []
        total = 0
        for i, item in enumerate(utterances):
            ids, dur, noise = item[:3]
            u, k = self._utt(ids, dur, noise, noiseScale, **(item[3] if len(item) > 3 else {}))
            arr[i] = u
            keep.append(k)
        self._stage_prosody(slot, prosody, [len(u[0]) for u in utterances])
        self._stage_volume(slot, volume, [len(u[0]) for u in utterances])
        self._stage_pitch(slot, pitch, n)
        rc = self.lib.piper_hip_voice_prepare_batch(self.voice, arr, n, slot)
        if rc < 0:
            _check(rc)
        tot = C.c_int64()
        _check(self.lib.piper_hip_voice_pitch_samples(self.voice, slot, None, 0, C.byref(tot)))
        self._keep[slot] = (keep, int(tot.value))
        return rc

    def plan_info(self, slot):
        bt, bf, n, by = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
        _check(self.lib.piper_hip_voice_plan_info(self.voice, slot, C.byref(bt), C.byref(bf), C.byref(n), C.byref(by)))
        return dict(bucket_t=bt.value, bucket_f=bf.value, cached_plans=n.value, cached_bytes=by.value)

    def set_plan_cache(self, max_plans, max_bytes=0):
        _check(self.lib.piper_hip_voice_set_plan_cache(self.voice, int(max_plans), int(max_bytes)))

    def last_build_breakdown(self):
        """ms of the phases of the latest plan build (cold prepare): streams, schedule + arena, arena init, eager_pass (always 0, kept
        for the ABI), capture and instantiate (0 after the prepare, filled by the plan's first launch)."""
        a = (C.c_double * 6)()
        _check(self.lib.piper_hip_voice_last_build_breakdown(self.voice, a))
        return dict(zip(("streams_events", "schedule_and_arena", "arena_init", "eager_pass", "capture", "instantiate"), (round(x, 3) for x in a)))

    def launch(self, slot):
        _check(self.lib.piper_hip_voice_launch(self.voice, slot))

    def pinned_empty(self, count):
        """float32 array in page-locked host memory (piper_hip_host_alloc): `collect(slot, out=…)` into it is one DMA. Freed by close()."""
        p = C.c_void_p()
        _check(self.lib.piper_hip_host_alloc(self.backend.ctx, int(count) * 4, C.byref(p)))
        self._pinned.append(p)
        return np.ctypeslib.as_array(C.cast(p, c_f32p), shape=(int(count),))

    def collect(self, slot, want_audio=True, out=None, level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP):
        """level: a Level (or tuple / dict) sets the slot id's level before the call, None clears it (slot_level); it persists.
        loudness: the same for the slot id's loudness target (slot_loudness). join: the same for the slot id's join (slot_join): the
        items then leave as ONE programme (join_report(slot) afterwards)."""
        self._slot_level(slot, level)
        self._slot_loudness(slot, loudness)
        self._slot_eq(slot, eq)
        self._slot_join(slot, join)
        n = self._keep[slot][1]
        if not want_audio:
            _check(self.lib.piper_hip_voice_collect(self.voice, slot, None, 0))
            return None
        if slot in self._joins:
            return self._collect_joined(slot, np.float32, None, out,
                                        lambda o, room: _check(self.lib.piper_hip_voice_collect(self.voice, slot, o.ctypes.data_as(c_f32p), room)))
        if out is None:
            out = np.empty(max(n, 1), np.float32)
        assert out.dtype == np.float32 and out.size >= n and out.flags.c_contiguous
        _check(self.lib.piper_hip_voice_collect(self.voice, slot, out.ctypes.data_as(c_f32p), n))
        if len(self._keep[slot]) > 2 and self._keep[slot][2]:  # bounded: n was the capacity; the true lengths are known now
            n = self.pitch_samples(slot)[1]
            self._keep[slot] = (self._keep[slot][0], n, False)
        return out[:n]

    def collect_pcm16(self, slot, gain=1.0, normalize=False, out=None, rate=None, level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP):
        """collect() with 16-bit PCM converted on the device (piper_hip_voice_collect_pcm16): the items back to back at their true lengths.
        normalize=False: the samples pcm16(collect(slot)) gives; normalize=True: Piper's peak normalisation per item (peaks(slot) afterwards).
        The fp32 waveform stays in the plan: collect / collect_pcm16 may follow in any order. rate: resampled on the device to that output
        rate (piper_hip_voice_collect_pcm16_rate), item b at J(its true samples). level, loudness: as for collect."""
        self._slot_level(slot, level)
        self._slot_loudness(slot, loudness)
        self._slot_eq(slot, eq)
        self._slot_join(slot, join)
        n = self._keep[slot][1]
        if slot in self._joins:  # ONE programme, at `rate` resampled as one signal
            prm = PcmParams(float(gain), int(bool(normalize)))
            r = self.cfg.sample_rate if rate is None else int(rate)
            return self._collect_joined(slot, np.int16, r, out, lambda o, room: _check(self.lib.piper_hip_voice_collect_pcm16_rate(
                self.voice, slot, C.byref(prm), r, o.ctypes.data_as(c_i16p), room)))
        if rate is not None and int(rate) != self.cfg.sample_rate:  # (the voice's own rate is not a filter: the plain call)
            return self._collect_pcm16_rate(slot, gain, normalize, out, int(rate))
        if out is None:
            out = np.empty(max(n, 1), np.int16)
        assert out.dtype == np.int16 and out.size >= n and out.flags.c_contiguous
        prm = PcmParams(float(gain), int(bool(normalize)))
        _check(self.lib.piper_hip_voice_collect_pcm16(self.voice, slot, C.byref(prm), out.ctypes.data_as(c_i16p), n))
        if len(self._keep[slot]) > 2 and self._keep[slot][2]:  # bounded: n was the capacity; the true lengths are known now
            n = self.pitch_samples(slot)[1]
            self._keep[slot] = (self._keep[slot][0], n, False)
        return out[:n]

    def _collect_pcm16_rate(self, slot, gain, normalize, out, rate):
        src = self.cfg.sample_rate
        bounded = len(self._keep[slot]) > 2 and self._keep[slot][2]
        per, total = self.pitch_samples(slot)  # (a bounded slot: the capacity of every item)
        room = sum(resample_count(src, rate, p) for p in per)
        if out is None:
            out = np.empty(max(room, 1), np.int16)
        assert out.dtype == np.int16 and out.size >= room and out.flags.c_contiguous
        prm = PcmParams(float(gain), int(bool(normalize)))
        _check(self.lib.piper_hip_voice_collect_pcm16_rate(self.voice, slot, C.byref(prm), rate, out.ctypes.data_as(c_i16p), room))
        if bounded:  # the true lengths are known now
            per, total = self.pitch_samples(slot)
            self._keep[slot] = (self._keep[slot][0], total, False)
        return out[:sum(resample_count(src, rate, p) for p in per)]

    def synthesize_pcm16(self, phonemeIDs, durations=None, noise=None, noiseScale=0.667, lengthScale=1.0, noiseW=0.8, gain=1.0,
                         normalize=False, rate=None, prosody=None, volume=None, level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP, pitch=None, **kw):
        """synthesize() ending in 16-bit PCM converted on the device (slot 0); rate: at that output rate; prosody: as for prepare;
        level, loudness: as for collect (slot 0)."""
        self._slot_level(0, level)
        self._slot_loudness(0, loudness)
        self._slot_eq(0, eq)
        self._slot_join(0, join)
        pro = None if prosody is None else [prosody]
        vol = None if volume is None else [volume]
        if rate is not None and int(rate) == self.cfg.sample_rate:
            rate = None
        if durations is not None and not kw and rate is not None:  # piper_hip_voice_synthesize_pcm16_rate
            u, _k = self._utt(phonemeIDs, durations, noise, noiseScale)
            n = resample_count(self.cfg.sample_rate, rate, self._one_call_room(int(self.lib.piper_hip_voice_num_samples(self.voice, C.byref(u))), pitch))
            out = np.empty(max(n, 1), np.int16)
            got = C.c_int64()
            prm = PcmParams(float(gain), int(bool(normalize)))
            self._stage_prosody(0, pro, [len(phonemeIDs)])
            self._stage_volume(0, vol, [len(phonemeIDs)])
            self._stage_pitch(0, pitch, 1)
            _check(self.lib.piper_hip_voice_synthesize_pcm16_rate(self.voice, C.byref(u), C.byref(prm), int(rate), out.ctypes.data_as(c_i16p), n,
                                                                  C.byref(got)))
            self._keep.pop(0, None)
            return out[:got.value]
        if durations is not None and not kw:  # the one-call C entry point
            u, _k = self._utt(phonemeIDs, durations, noise, noiseScale)
            n = self._one_call_room(int(self.lib.piper_hip_voice_num_samples(self.voice, C.byref(u))), pitch)
            out = np.empty(max(n, 1), np.int16)
            got = C.c_int64()
            prm = PcmParams(float(gain), int(bool(normalize)))
            self._stage_prosody(0, pro, [len(phonemeIDs)])
            self._stage_volume(0, vol, [len(phonemeIDs)])
            self._stage_pitch(0, pitch, 1)
            _check(self.lib.piper_hip_voice_synthesize_pcm16(self.voice, C.byref(u), C.byref(prm), out.ctypes.data_as(c_i16p), n, C.byref(got)))
            self._keep.pop(0, None)
            return out[:got.value]
        self.prepare(0, phonemeIDs, durations, noise, noiseScale, length_scale=lengthScale, noise_w=noiseW, prosody=prosody, volume=volume,
                     pitch=pitch, **kw)
        self.launch(0)
        return self.collect_pcm16(0, gain, normalize, rate=rate)

    def collect_g711(self, slot, law, gain=1.0, normalize=False, out=None, rate=None, level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP):
        """collect_pcm16 ending in G.711 bytes ("mulaw" / "alaw") companded on the device (piper_hip_voice_collect_g711): one uint8 per
        sample, the items back to back at J(their true samples) at `rate` (default: the voice's own). Every rule of collect_pcm16 holds."""
        self._slot_level(slot, level)
        self._slot_loudness(slot, loudness)
        self._slot_eq(slot, eq)
        self._slot_join(slot, join)
        src = self.cfg.sample_rate
        rate = src if rate is None else int(rate)
        if slot in self._joins:  # ONE programme
            prm = PcmParams(float(gain), int(bool(normalize)))
            return self._collect_joined(slot, np.uint8, rate, out, lambda o, room: _check(self.lib.piper_hip_voice_collect_g711(
                self.voice, slot, C.byref(prm), _law(law), rate, o.ctypes.data_as(c_u8p), room)))
        count = (lambda p: p) if rate == src else (lambda p: resample_count(src, rate, p))
        bounded = len(self._keep[slot]) > 2 and self._keep[slot][2]
        per, total = self.pitch_samples(slot)  # (a bounded slot: the capacity of every item)
        room = sum(count(p) for p in per)
        if out is None:
            out = np.empty(max(room, 1), np.uint8)
        assert out.dtype == np.uint8 and out.size >= room and out.flags.c_contiguous
        prm = PcmParams(float(gain), int(bool(normalize)))
        _check(self.lib.piper_hip_voice_collect_g711(self.voice, slot, C.byref(prm), _law(law), rate, out.ctypes.data_as(c_u8p), room))
        if bounded:  # the true lengths are known now
            per, total = self.pitch_samples(slot)
            self._keep[slot] = (self._keep[slot][0], total, False)
        return out[:sum(count(p) for p in per)]

    def synthesize_g711(self, phonemeIDs, durations, law, noise=None, noiseScale=0.667, gain=1.0, normalize=False, rate=None, prosody=None, volume=None,
                        level=KEEP, loudness=KEEP, eq=KEEP, join=KEEP, pitch=None):
        """synthesize() ending in G.711 bytes companded on the device (piper_hip_voice_synthesize_g711, slot 0), at `rate` or the voice's;
        prosody: as for prepare (with supplied durations: noise alone); level, loudness: as for collect (slot 0)."""
        self._slot_level(0, level)
        self._slot_loudness(0, loudness)
        self._slot_eq(0, eq)
        self._slot_join(0, join)
        src = self.cfg.sample_rate
        rate = src if rate is None else int(rate)
        u, _k = self._utt(phonemeIDs, durations, noise, noiseScale)
        n = self._one_call_room(int(self.lib.piper_hip_voice_num_samples(self.voice, C.byref(u))), pitch)
        if rate != src:
            n = resample_count(src, rate, n)
        out = np.empty(max(n, 1), np.uint8)
        got = C.c_int64()
        prm = PcmParams(float(gain), int(bool(normalize)))
        self._stage_prosody(0, None if prosody is None else [prosody], [len(phonemeIDs)])
        self._stage_volume(0, None if volume is None else [volume], [len(phonemeIDs)])
        self._stage_pitch(0, pitch, 1)
        _check(self.lib.piper_hip_voice_synthesize_g711(self.voice, C.byref(u), C.byref(prm), _law(law), rate, out.ctypes.data_as(c_u8p), n,
                                                        C.byref(got)))
        self._keep.pop(0, None)
        return out[:got.value]

    def peaks(self, slot):
        """max |x| of each item of the slot, after a collect_pcm16(normalize=True) of its latest run (a joined slot: ONE value, the
        programme's)."""
        nb = self.lib.piper_hip_voice_batch_size(self.voice, slot)
        out = np.empty(max(nb, 1), np.float32)
        _check(self.lib.piper_hip_voice_peaks(self.voice, slot, out.ctypes.data_as(c_f32p), nb))
        return out[:1 if slot in self._joins else nb]

    def tap(self, slot, name, max_floats=None):
        """A named intermediate of the slot, items back to back at their true lengths (max_floats None: sized by the library).
        Name grammar (include/piper_hip.h): ["predict:"] <tensor> ["@" <step name>] — "front.x@enc2.ln2_qkv" is the work buffer x right
        after that step (the schedule is replayed up to it, then finished); "predict:" addresses the cached encoder + predictor plan of the
        slot's bucket; the front.* / dp.* work buffers are only meaningful with "@". "window:<tensor>" reads the generator window plan of
        the slot's latest stream step (single stream, group or pool), rows at that step's window lengths. See also steps()."""
        n = C.c_size_t()
        if max_floats is None:
            _check(self.lib.piper_hip_voice_tap(self.voice, slot, name.encode(), None, 0, C.byref(n)))
            max_floats = max(int(n.value), 1)
        out = np.empty(max_floats, np.float32)
        _check(self.lib.piper_hip_voice_tap(self.voice, slot, name.encode(), out.ctypes.data_as(c_f32p), max_floats,
                                            C.byref(n)))
        return out[:n.value]

    def steps(self, slot, predict=False, window=False):
        """Launch names of the slot's schedule in order (predict=True: of the cached encoder + predictor plan of its bucket; window=True:
        of the generator window plan of the slot's latest stream step)."""
        raw = self.tap(slot, ("window:" if window else "predict:" if predict else "") + "@steps")
        return bytes(raw.astype(np.uint8)).decode().split("\n")[:-1]

    def routes(self, slot, predict=False, window=False):
        """[(step name, [route records])] of the slot's schedule, one entry per launch: what each step's launchers chose at its most recent
        enqueue (HipBackend.arm_routes before the plan is prepared; a plan enqueued while disarmed has empty lists). predict / window as
        for steps(). Runs nothing."""
        raw = self.tap(slot, ("window:" if window else "predict:" if predict else "") + "@routes")
        out = []
        for line in bytes(raw.astype(np.uint8)).decode().split("\n")[:-1]:
            name, _, recs = line.partition("\t")
            out.append((name, recs.split("; ") if recs else []))
        return out

    def last_gpu_ms(self, slot):
        ms = C.c_double()
        _check(self.lib.piper_hip_voice_last_gpu_ms(self.voice, slot, C.byref(ms)))
        return ms.value

    def time_subset(self, slot, name_filter, iters=20):
        """Graph replay of the launches whose name contains `name_filter`: (avg µs per launch, launches, flops, bytes). A filter that
        starts with "predict:" times the predictor plan the slot's last prepare ran."""
        us, n, fl, by = C.c_double(), C.c_int(), C.c_double(), C.c_double()
        _check(self.lib.piper_hip_voice_time_subset(self.voice, slot, name_filter.encode(), iters, C.byref(us), C.byref(n),
                                                    C.byref(fl), C.byref(by)))
        return us.value, n.value, fl.value, by.value

    def profile(self, slot, iters=5, max_entries=512):
        arr = (KernelStat * max_entries)()
        n = C.c_int()
        _check(self.lib.piper_hip_voice_profile(self.voice, slot, iters, arr, max_entries, C.byref(n)))
        return [dict(name=a.name.decode(), avg_us=a.avg_us, flops=a.flops, bytes=a.bytes) for a in arr[:n.value]]
