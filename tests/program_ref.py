"""NumPy restatement of the envelope programs (include/oalsfx_hip.h, "envelope programs") on top of resample_ref, polyphony_ref and
biquad_ref: a voice has a program, a list of envelope records, the current segment first and the queued ones behind it.  A render of F
frames walks the contract's loop -- take the head of the queue while the current segment is complete, then render a span of min(F - t,
delay + (ramp_frames - ramp_done)) frames (F - t with an empty queue) with resample_ref.render_one, as a call of that many frames -- and
the voice's output is the concatenation of its spans.  The voices' outputs are then filtered and summed as biquad_ref.render does it."""
import numpy as np

import biquad_ref as bref
import resample_ref as ref
import voice_ref as vref

f32 = np.float32
PROGRAM_MAX = 8        # OALSFX_ENV_PROGRAM_MAX


def complete(e):
    return bool(int(e["flags"]) & vref.ACTIVE) and int(e["delay"]) == 0 and int(e["ramp_done"]) == int(e["ramp_frames"])


def boundaries(program, frames):
    """The frames in (0, frames] at which a render of `frames` frames takes the next segment of `program`: the ends of its spans."""
    at, t = [], 0
    for e in program[:-1]:
        t += int(e["delay"]) + int(e["ramp_frames"]) - int(e["ramp_done"])
        if t > frames:
            break
        at.append(t)
    return at


def render_voice(record, program, coef, asset, frames, channels):
    """One voice: record of sampler_ref.DTYPE, program a sequence of 1 .. PROGRAM_MAX records of voice_ref.DTYPE.  Returns (out
    [frames][channels], the record afterwards, the program afterwards: an array, the current segment first)."""
    assert 1 <= len(program) <= PROGRAM_MAX
    current, queue = np.array(program[0]).copy(), [np.array(e).copy() for e in program[1:]]
    out = np.zeros((frames, channels), f32)
    t = 0
    while True:
        while queue and complete(current):
            current = queue.pop(0)
        if t == frames:
            break
        span = frames - t
        if queue:
            span = min(span, int(current["delay"]) + int(current["ramp_frames"]) - int(current["ramp_done"]))
        out[t:t + span], record, current = ref.render_one(record, current, coef, asset, span, channels)
        t += span
    after = np.zeros(1 + len(queue), vref.DTYPE)
    after[0] = current
    for k, e in enumerate(queue):
        after[1 + k] = e
    return out, record, after


def render(records, programs, resamplers, filters, tables, assets, frames, channels):
    """records [K][n] of sampler_ref.DTYPE, programs[k][i] a sequence of envelope records, resamplers [K][n], filters [K][n] of
    biquad_ref.DTYPE or None, tables {index: coef}, assets[k][i].  Returns (out [n][frames][channels], the records afterwards, the
    programs afterwards [k][i], the filters afterwards or None)."""
    lanes, n = records.shape
    out = np.zeros((n, frames, channels), dtype=f32)
    after = records.copy()
    programs_after = [[None] * n for _ in range(lanes)]
    filters_after = None if filters is None else filters.copy()
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, after[k][i], programs_after[k][i] = render_voice(records[k][i], programs[k][i], coef, assets[k][i], frames, channels)
            if filters is not None and filters[k][i]["flags"] & bref.ACTIVE:
                o, filters_after[k][i] = bref.filter_one(filters[k][i], o, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = o if lanes == 1 else (acc + o).astype(f32)
        out[i] = acc
    return out, after, programs_after, filters_after
