"""NumPy restatement of the sampler streams (include/oalsfx_hip.h, "sampler streams") on top of sampler_ref, voice_ref, resample_ref and
program_ref: a voice has a stream, a list of sampler records, the current one first and the ring's entries behind it, and a count of
the entries taken.  A render of F frames walks the contract's loop -- take the ring's head while the current record is at its end, at
the entry's position plus the excess; then render a span that ends where the one-shot does (or where program_ref's envelope segment
completes) with resample_ref.render_one, as a call of that many frames -- and the voice's output is the concatenation of its spans.
Every record names its asset by its `data` and `frames` fields: `assets` maps asset_key(record) to the PCM array.

`wrong` selects one of the forms a device could take by mistake, which the tests hold against the right one (tests/test_stream_ref.py):
"dropped" loses the overshoot, "late" takes a frame late, "tile" takes at the next 64-frame boundary, "render" at the render's end.
The forms of VALUE_WRONG leave the frames of the takes alone and get a number wrong that only large values show
(tests/test_stream_extremes.py): "over in 16 bits" keeps the low 16 bits of an excess; "start in 32 bits" adds the entry's position and
the excess in 32 bits; "distance in 32 bits" truncates E - P before the division; "one subtraction" wraps an entry's loop by taking its
length off once; "chain drops" hands no excess on behind the first entry of a chain; "whole start" has an entry that ended hand on its
whole start, not the start less E'; "stop takes" takes at delay + n although a STOP fade completed first and left the record short of
its end."""
import numpy as np

import biquad_ref as bref
import filter_program_ref as fref
import program_ref as pref
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref

f32 = np.float32
QUEUE = 8               # OALSFX_STREAM_QUEUE
ONE, FRAC_BITS = sref.ONE, sref.FRAC_BITS
PLAYING, LOOP, LINEAR = sref.PLAYING, sref.LOOP, sref.LINEAR
TILE = 64
VALUE_WRONG = ("over in 16 bits", "start in 32 bits", "distance in 32 bits", "one subtraction", "chain drops", "whole start", "stop takes")


def asset_key(record):
    """What a record's PCM stands under in `assets`: its address and its length (chunkings of one asset share addresses)."""
    return int(record["data"]), int(record["frames"])


def end_of(record):
    return int(record["frames"]) << FRAC_BITS


def at_end(record):
    """No LOOP and position >= E, PLAYING or not: an all-zero record is at its end."""
    return not int(record["flags"]) & LOOP and int(record["position"]) >= end_of(record)


def taken_entry(entry, over, wrong=None):
    """The ring's head as the current record, started `over` further in: (the record, the excess its own end leaves over)."""
    e = np.array(entry).copy()
    q = int(e["position"]) + over
    if wrong == "start in 32 bits":
        q &= 0xFFFFFFFF
    if int(e["flags"]) & LOOP:
        if wrong == "one subtraction":
            first, last = int(e["loop_start"]) << FRAC_BITS, int(e["loop_end"]) << FRAC_BITS
            return _at(e, q - (last - first) if q >= last else q), 0
        return _at(e, int(sref.wrap(q, e))), 0
    if q >= end_of(e):
        e["flags"] = int(e["flags"]) & ~PLAYING
        left = q if wrong == "whole start" else q - end_of(e)
        return _at(e, end_of(e)), 0 if wrong == "chain drops" else left & 0xFFFF if wrong == "over in 16 bits" else left
    return _at(e, q), 0


def _at(e, position):
    e["position"] = position
    return e


def frames_to_end(record, env, wrong=None):
    """(delay + n, the excess of sampler frame n) for a PLAYING one-shot short of its end at a step other than 0, else None."""
    flags, step, p = int(record["flags"]), int(record["step"]), int(record["position"])
    if flags & (PLAYING | LOOP) != PLAYING or step == 0:
        return None
    n = -((p - end_of(record)) // step)          # ceil((E - P) / step), P < E
    if wrong == "distance in 32 bits":
        n = max(-(-((end_of(record) - p) & 0xFFFFFFFF) // step), 1)      # (never more than the right n: the span is cut early, and again)
    assert n >= 1
    delay = int(env["delay"]) if int(env["flags"]) & vref.ACTIVE else 0
    return delay + n, p + n * step - end_of(record)


def render_voice(stream, taken, program, coef, assets, frames, channels, wrong=None):
    """One voice: stream a sequence of 1 .. 1 + QUEUE records of sampler_ref.DTYPE, program a sequence of envelope records.  Returns (out
    [frames][channels], the stream afterwards as an array, taken afterwards, the program afterwards, the frames at which entries were
    taken)."""
    assert 1 <= len(stream) <= 1 + QUEUE
    record, ring = np.array(stream[0]).copy(), [np.array(e).copy() for e in stream[1:]]
    current, queue = np.array(program[0]).copy(), [np.array(e).copy() for e in program[1:]]
    out = np.zeros((frames, channels), f32)
    t, over, takes = 0, 0, []
    hold = 0                                      # wrong forms: no take before this frame
    while True:
        while queue and pref.complete(current):
            current = queue.pop(0)
        while ring and at_end(record) and (t >= hold or t == frames):
            record, over = taken_entry(ring.pop(0), 0 if wrong == "dropped" else over, wrong)
            taken += 1
            takes.append(t)
        if t == frames:
            break
        span = frames - t
        if queue:
            span = min(span, int(current["delay"]) + int(current["ramp_frames"]) - int(current["ramp_done"]))
        excess, ahead = 0, None
        if ring and not at_end(record):
            ahead = frames_to_end(record, current, wrong)
            if ahead is not None:
                span, excess = min(span, ahead[0]), ahead[1]
                if wrong == "over in 16 bits":
                    excess &= 0xFFFF
        elif ring:
            span = min(span, hold - t)             # (a wrong form waiting for its frame)
        before = int(record["position"])
        asset = assets.get(asset_key(record))
        out[t:t + span], record, current = ref.render_one(record, current, coef, asset, span, channels)
        t += span
        reached = before < end_of(record) and at_end(record)
        if wrong == "stop takes" and ring and not reached and ahead is not None and span == ahead[0] and not int(record["flags"]) & PLAYING:
            record, reached = _at(record, end_of(record)), True       # the span was cut for the end, and the end is taken for reached
        over = excess if reached else 0
        if reached and ring and wrong in ("late", "tile", "render"):
            hold = {"late": t + 1, "tile": -(-t // TILE) * TILE, "render": frames}[wrong]
            if wrong != "late":
                over = 0 if hold != t else over   # the frames in between are silence, and the entry starts at its own position
            hold = min(hold, frames)
    after = np.zeros(1 + len(ring), sref.DTYPE)
    after[0] = record
    for k, e in enumerate(ring):
        after[1 + k] = e
    program_after = np.zeros(1 + len(queue), vref.DTYPE)
    program_after[0] = current
    for k, e in enumerate(queue):
        program_after[1 + k] = e
    return out, after, taken, program_after, takes


def render(streams, taken, programs, resamplers, tables, assets, frames, channels, wrong=None, filters=None, filter_programs=None):
    """streams[k][i] a sequence of sampler records, taken [K][n], programs[k][i] a sequence of envelope records, resamplers [K][n], tables
    {index: coef}, assets {asset_key: PCM}.  Returns (out [n][frames][channels], the streams afterwards [k][i], taken afterwards, the
    programs afterwards [k][i]).  One lane: the voice's frames as they are; more: summed ascending from +0.0f, as polyphony_ref does.
    With filters [K][n] of biquad_ref.DTYPE and filter_programs[k][i] lists of sweep records, a voice whose filter is ACTIVE goes through
    filter_program_ref.filter_one over its whole row, spans concatenated, before the sum, and the filters and the filter programs
    afterwards are returned as well."""
    lanes, n = len(streams), len(streams[0])
    out = np.zeros((n, frames, channels), dtype=f32)
    streams_after = [[None] * n for _ in range(lanes)]
    programs_after = [[None] * n for _ in range(lanes)]
    taken_after = np.array(taken, dtype=np.uint32).reshape(lanes, n).copy()
    filters_after = None if filters is None else filters.copy()
    fp_after = None if filters is None else [[[s.copy() for s in p] for p in lane] for lane in filter_programs]
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, streams_after[k][i], t, programs_after[k][i], _ = render_voice(streams[k][i], int(taken_after[k][i]), programs[k][i], coef, assets, frames,
                                                                             channels, wrong)
            taken_after[k][i] = t
            if filters is not None and int(filters[k][i]["flags"]) & bref.ACTIVE:
                o, filters_after[k][i], fp_after[k][i] = fref.filter_one(filters[k][i], filter_programs[k][i], o, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = o if lanes == 1 else (acc + o).astype(f32)
        out[i] = acc
    if filters is not None:
        return out, streams_after, taken_after, programs_after, filters_after, fp_after
    return out, streams_after, taken_after, programs_after


def append(stream, entries):
    """oalsfx_batch_append_streams for one voice: the stream with `entries` behind it, or None where the ring has too little room."""
    if len(stream) - 1 + len(entries) > QUEUE:
        return None
    out = np.zeros(len(stream) + len(entries), sref.DTYPE)
    out[:len(stream)] = stream
    for k, e in enumerate(entries):
        out[len(stream) + k] = e
    return out


def chunks(record, lengths):
    """oalsfx_host_stream_chunks' arithmetic: the one-shot `record` over an asset cut into consecutive chunks of `lengths` frames, each a
    record of its own at position 0 -- the first keeps the record's position, which must lie inside the first chunk."""
    assert sum(lengths) == int(record["frames"]) and not int(record["flags"]) & LOOP
    width = np.dtype(sref.PCM_DTYPE[int(record["format"])]).itemsize * int(record["channels"])
    out, first = np.zeros(len(lengths), sref.DTYPE), 0
    for k, n in enumerate(lengths):
        out[k] = record
        out[k]["data"] = int(record["data"]) + first * width
        out[k]["frames"] = n
        out[k]["position"] = int(record["position"]) if k == 0 else 0
        first += n
    assert int(out[0]["position"]) < int(lengths[0]) << FRAC_BITS
    return out
