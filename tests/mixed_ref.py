"""The mixed-format contract of include/piper_hip.h ("Mixed formats") restated on top of resample_ref, pcm_ref and g711_ref: from the fp32
chunks of every row and the row's format to the n_samples, byte_off and bytes of every step. Each step of a row is computed the stream's
way — from its chunk and the P − 1 samples before it, nothing else — so the keyword switches can plant the defects a mixed step could
have (test_stream_mixed_ref.py): an offset that is not rounded up, another row's filter, another row's gain, an inherited history."""
from collections import namedtuple

import numpy as np

import g711_ref
import pcm_ref
import resample_ref as rr

F32 = np.float32
Format = namedtuple("Format", "rate enc gain", defaults=(0, "s16", 1.0))  # rate 0 = the voice's own rate
ELEM = {"s16": 2, "mulaw": 1, "alaw": 1, "f32": 4}
DTYPE = {"s16": np.int16, "mulaw": np.uint8, "alaw": np.uint8, "f32": np.float32}
ENC_CODE = {"s16": 0, "mulaw": 1, "alaw": 2, "f32": 3}


def sink(y, f):
    """fp32 samples at the row's rate → the row's elements: the float itself, the PCM contract's int16 of y·gain, or its G.711 byte"""
    y = np.ascontiguousarray(y, F32).reshape(-1)
    if f.enc == "f32":
        return y.copy()
    pcm = pcm_ref.pcm16_reference(y, f.gain)
    return pcm if f.enc == "s16" else g711_ref.table_encode(pcm, f.enc).astype(np.uint8)


def filt(f, in_rate, tables=None):
    """(table, L, M, P) of the row's filter, or None at the voice's own rate. tables: {(in, out): float32 [L][P]} (the library's own in the
    GPU tests); without it the float64 design rounded once."""
    if not f.rate or f.rate == in_rate:
        return None
    L, M, P = rr.ratio(in_rate, f.rate)
    tab = tables[(in_rate, f.rate)] if tables is not None else rr.design(in_rate, f.rate).astype(F32)
    return np.ascontiguousarray(tab, F32).reshape(L, P), L, M, P


def whole(x, f, in_rate, tables=None):
    """the whole-item conversion of an item's fp32 samples at format f"""
    fl = filt(f, in_rate, tables)
    return sink(x if fl is None else rr.apply(x, fl[0], fl[1], fl[2]), f)


def total_samples(n_in, f, in_rate):
    return n_in if not f.rate or f.rate == in_rate else rr.count(n_in, *rr.ratio(in_rate, f.rate)[:2])


def step_bound_bytes(f, in_rate, chunk_samples):
    """a row's share of a step: the per-row bound in elements times the element size, rounded up to 4"""
    n = chunk_samples if not f.rate or f.rate == in_rate else rr.step_bound(chunk_samples, *rr.ratio(in_rate, f.rate))
    return (n * ELEM[f.enc] + 3) & ~3


def row_steps(chunks, f, in_rate, hop, chunk_frames, finished=True, tables=None, inherit=None, as_format=None):
    """The typed chunk of every step of ONE session whose fp32 chunks are `chunks` (finished = the last of them ends the item).
    Planted defects: inherit = fp32 samples of the row's previous occupant that the first step wrongly sees before sample 0;
    as_format = another row's format whose filter / gain / sink is used instead of f's."""
    g = as_format or f
    fl = filt(g, in_rate, tables)
    if fl is None:
        return [sink(c, g) for c in chunks]
    tab, L, M, P = fl
    x = np.concatenate([np.asarray(c, F32) for c in chunks]) if chunks else np.empty(0, F32)
    assert x.size % hop == 0
    frames = x.size // hop
    ranges = rr.stream_ranges(frames if finished else frames + chunk_frames, chunk_frames, hop, L, M, P)[:len(chunks)]
    out, s = [], 0
    for k, (j0, j1) in enumerate(ranges):
        e = s + chunks[k].size
        last = finished and k == len(chunks) - 1
        lo = max(s - (P - 1), 0)
        known = np.full(x.size if last else e, np.nan, F32)  # what the step does not have poisons whatever reads it
        known[lo:e] = x[lo:e]
        if k == 0 and inherit is not None:
            # the defect: sample g < 0 reads the previous occupant's tail. T samples are put in front, T a multiple of M, so that output j
            # of the item is output j + T·L/M of the longer signal, with the same phase
            T = M * (-(-(P - 1) // M))
            tail = np.asarray(inherit, F32)[-T:]
            tail = np.concatenate([np.zeros(T - tail.size, F32), tail])
            y = rr.apply(np.concatenate([tail, known]), tab, L, M, j0 + T * L // M, j1 + T * L // M)
        else:
            y = rr.apply(known, tab, L, M, j0, j1) if j1 > j0 else np.empty(0, F32)
        out.append(sink(y, g))
        s = e
    return out


def layout(counts, elems, round_up=True):
    """byte_off per row and the step's total from the rows' sample counts and element sizes: the first delivering row at 0, every later
    one at the previous delivering row's end rounded up to 4; a row that delivers nothing reports where the next delivering row starts.
    round_up=False plants the defect: rows back to back at any byte."""
    offs, end = [], 0
    for c, el in zip(counts, elems):
        start = (end + 3) & ~3 if round_up else end
        offs.append(start)
        if c:
            end = start + c * el
    return offs, end


def expected(sessions, n_rows, in_rate, hop, chunk_frames, tables=None, round_up=True):
    """sessions: [dict(row=, start=step index of its first chunk, chunks=[fp32 per step], fmt=Format, finished=bool, ...row_steps'
    switches)]. Returns per step (n_samples [n_rows], byte_off [n_rows], bytes uint8 [total], mask bool [total]): mask is False on the
    pad bytes, whose content is unspecified."""
    per = []
    for se in sessions:
        kw = {k: se[k] for k in ("inherit", "as_format") if k in se}
        per.append(row_steps(se["chunks"], se["fmt"], in_rate, hop, chunk_frames, se.get("finished", True), tables, **kw))
    n_steps = max((se["start"] + len(se["chunks"]) for se in sessions), default=0)
    out = []
    for k in range(n_steps):
        parts, elems = [np.empty(0, np.uint8)] * n_rows, [2] * n_rows
        for se, steps in zip(sessions, per):
            i = k - se["start"]
            if 0 <= i < len(steps):
                parts[se["row"]] = steps[i].view(np.uint8)
                elems[se["row"]] = ELEM[(se.get("as_format") or se["fmt"]).enc]
        counts = [p.size // el for p, el in zip(parts, elems)]
        offs, total = layout(counts, elems, round_up)
        data, mask = np.zeros(total, np.uint8), np.zeros(total, bool)
        for p, o in zip(parts, offs):
            data[o:o + p.size] = p
            mask[o:o + p.size] = True
        out.append((counts, offs, data, mask))
    return out


def same_step(got, want):
    """(n_samples, byte_off, bytes) of a step against expected()'s entry: counts, offsets, the total and every byte that is not a pad"""
    (gn, go, gb), (wn, wo, wb, mask) = got, want
    gb = np.asarray(gb, np.uint8)
    return list(gn) == list(wn) and list(go) == list(wo) and gb.size == wb.size and bool(np.array_equal(gb[mask], wb[mask]))
