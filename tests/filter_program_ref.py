"""NumPy restatement of the filter programs (include/oalsfx_hip.h, "filter programs") on top of sweep_ref: sweep_ref with a queue per
voice.  A voice's filter program is a list of sweep records, the current segment first.  A render of F frames is the contract's loop
taken literally: while the queue is not empty and the current segment is spent the head of the queue takes its place; the span is what
is left of the render, or of the current segment where one waits behind it; the span is one call of sweep_ref.filter_one.  So the
restatement IS the render split at every boundary with a set call in between."""
import numpy as np

import biquad_ref as bref
import program_ref as gref
import resample_ref as ref
import sweep_ref as wref

f32 = np.float32
DTYPE = wref.DTYPE
MAX = 8                    # OALSFX_FILTER_PROGRAM_MAX
TILE = 64

MESSAGES = {
    "length": "Filter program length out of range.",
    "active": "A filter program's segment is not active.",
    "started": "A queued filter sweep has already started.",
    "filter": wref.MESSAGES["filter"],
}


def check(program):
    """None, or the text with which oalsfx_batch_set_filter_programs refuses the program, the target's filter apart."""
    if not 1 <= len(program) <= MAX:
        return MESSAGES["length"]
    for j, s in enumerate(program):
        why = wref.check(s)
        if why:
            return why
        if len(program) >= 2 and not int(s["flags"]) & wref.ACTIVE:
            return MESSAGES["active"]
        if j >= 1 and int(s["done"]) != 0:
            return MESSAGES["started"]
    return None


def chain(nodes, frames):
    """oalsfx_host_filter_program: segment k ramps the coefficients nodes[k] to nodes[k + 1] over frames[k] frames."""
    return [wref.make(nodes[k], nodes[k + 1], frames[k])[0] for k in range(len(frames))]


def spent(s):
    return not wref.under_way(s)


def filter_one(record, program, x, channels, how="stated"):
    """One filter record, its program (a list of sweep records, the current one first) and the voice's frames x [F][channels] ->
    (y, the filter afterwards, the program afterwards).  how: "stated", or one of three wrong ways to switch that a kernel might take
    (tests/test_filter_program_ref.py): "late" (the switch one frame late: the boundary frame takes the old segment's `to`, and the
    new segment's indices lag by one), "index" (the index not reset at a switch: the new segment goes on counting where the old one
    stood), "tile" (the segment chosen per 64-frame tile from the tile's first frame)."""
    if how != "stated":
        return _filter_wrong(record, program, x, channels, how)
    frames, t, parts = x.shape[0], 0, []
    program = [s.copy() for s in program]
    while True:
        while len(program) > 1 and spent(program[0]):
            program.pop(0)
        if t == frames:
            break
        s = frames - t if len(program) == 1 else min(frames - t, int(program[0]["frames"]) - int(program[0]["done"]))
        y, record, program[0] = wref.filter_one(record, program[0], x[t:t + s], channels)
        parts.append(y)
        t += s
    y = np.concatenate(parts) if parts else np.zeros((0, channels), f32)
    return y, record, program


def timeline(program, frames):
    """The stated form as data: for each of the `frames` frames (segment number, index inside it), -1 for the segment of a frame that no
    segment ramps (behind the last one's end, or with the last one spent)."""
    seg, idx = np.full(frames, -1), np.zeros(frames, np.int64)
    program, at, t = [s.copy() for s in program], 0, 0
    while True:
        while len(program) - at > 1 and spent(program[at]):
            at += 1
        if t == frames:
            break
        s = program[at]
        left = int(s["frames"]) - int(s["done"]) if wref.under_way(s) else 0
        span = frames - t if len(program) - at == 1 else min(frames - t, left)
        ramp = min(span, left)
        seg[t:t + ramp], idx[t:t + ramp] = at, int(s["done"]) + np.arange(ramp)
        if wref.under_way(s):
            s["done"] = int(s["done"]) + ramp
        t += span
    return seg, idx


def _filter_wrong(record, program, x, channels, how):
    """The voice's frames under a wrong way to switch: the per-frame coefficients formed from a bent timeline, one recurrence over all."""
    frames = x.shape[0]
    seg, idx = timeline(program, frames)
    if how == "late":
        # the frame on which a new segment starts still belongs to the old one, which is past its end there (`to`); the new one starts a
        # frame later, its index a frame behind
        starts = [t for t in range(1, frames) if seg[t] >= 0 and seg[t] != seg[t - 1] and seg[t - 1] >= 0]
        seg2, idx2 = seg.copy(), idx.copy()
        for t in starts:
            end = t + 1
            while end < frames and seg[end] == seg[t]:
                end += 1
            idx2[t + 1:end] = idx[t:end - 1]
            seg2[t] = -2 - seg[t - 1]           # `to` of the old segment
        seg, idx = seg2, idx2
    elif how == "index":
        for t in range(1, frames):
            if seg[t] >= 0 and seg[t - 1] >= 0 and seg[t] != seg[t - 1]:
                end = t
                while end < frames and seg[end] == seg[t]:
                    end += 1
                idx[t:end] = idx[t - 1] + 1 + np.arange(end - t)
    elif how == "tile":
        for base in range(0, frames, TILE):
            end = min(frames, base + TILE)
            if seg[base] >= 0:
                seg[base:end], idx[base:end] = seg[base], idx[base] + np.arange(end - base)
    else:
        raise ValueError(how)
    coef = np.empty((frames, 5), f32)
    plain = bref.coefficients(record)
    for t in range(frames):
        k = int(seg[t])
        if k <= -2:
            coef[t] = program[-2 - k]["to"]
        elif k < 0:
            ramped = seg[:t][seg[:t] >= 0]      # behind the end of the last segment that ramped: its `to`
            coef[t] = program[int(ramped[-1])]["to"] if len(ramped) else plain
        else:
            s = program[k]
            n = int(idx[t])
            coef[t] = (s["from"] + (f32(n) * s["step"]).astype(f32)).astype(f32) if n < int(s["frames"]) else s["to"]
    y, _, _ = wref.process(coef, x, record["x"][:channels], record["y"][:channels])
    return y, record, program


def render(records, programs, resamplers, filters, filter_programs, tables, assets, frames, channels):
    """sweep_ref.render with filter_programs [K][n] lists of sweep records in the sweeps' place.  Returns (out [n][frames][channels], the
    records, the envelope programs, the filters and the filter programs afterwards)."""
    lanes, n = records.shape
    out = np.zeros((n, frames, channels), dtype=f32)
    after, filters_after = records.copy(), filters.copy()
    programs_after = [[None] * n for _ in range(lanes)]
    fp_after = [[None] * n for _ in range(lanes)]
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, after[k][i], programs_after[k][i] = gref.render_voice(records[k][i], programs[k][i], coef, assets[k][i], frames, channels)
            fp_after[k][i] = [s.copy() for s in filter_programs[k][i]]
            if filters[k][i]["flags"] & bref.ACTIVE:
                o, filters_after[k][i], fp_after[k][i] = filter_one(filters[k][i], filter_programs[k][i], o, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = o if lanes == 1 else (acc + o).astype(f32)
        out[i] = acc
    return out, after, programs_after, filters_after, fp_after
