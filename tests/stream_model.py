"""A second model of the sampler streams (include/oalsfx_hip.h, "sampler streams"), built unlike tests/stream_ref.py so that the two do not
share a mistake: one output frame after the other, no span and no division that finds an end.  Before every frame -- and once more
behind the last -- the contract's step 1 runs: while the ring holds an entry and the current record is a one-shot at or past its end, the
ring's head becomes the current record, `over` further in, where over = q - E and q is where the frame in front would have read had the
record gone on (P + step in Python's integers; 0 where no frame of this render stepped the record to its end); an entry's own loop is
wrapped with %, and an entry the start lies at or past the end of is left finished and hands start - E' on.  The frame's value and
what it does to the two records come from the scalar models of a render of one frame: tests/voice_model.py (which is
tests/sampler_model.py for an envelope that is not ACTIVE), or resample_ref.render_one for one frame where the voice has a table.  Slow,
and meant to be: tests/test_stream_extremes.py holds it against the restatement."""
import numpy as np

import resample_ref
import voice_model
from sampler_ref import DTYPE
from voice_ref import ACTIVE
from voice_ref import DTYPE as ENV_DTYPE

FRAC_BITS = 12
PLAYING, LOOP = 1, 2
f32 = np.float32


def _end(record):
    return int(record["frames"]) << FRAC_BITS


def _finished_one_shot(record):
    """At its end: no LOOP and position >= E, PLAYING or not."""
    return not int(record["flags"]) & LOOP and int(record["position"]) >= _end(record)


def _complete(e):
    return bool(int(e["flags"]) & ACTIVE) and int(e["delay"]) == 0 and int(e["ramp_done"]) == int(e["ramp_frames"])


def render_voice(stream, taken, program, coef, assets, frames, channels, trace=None):
    """What stream_ref.render_voice returns: (out [frames][channels], the stream afterwards, taken afterwards, the program afterwards, the
    frames at which entries were taken).  trace: a list that receives one dict per take -- "frame"; "hop": 0 for the first take of a
    frame, 1 for the next one in the same chain, ...; "q": where the record taken from stood or would have read (E where nothing ran
    past it); "end": its E; "over"; "start": the entry's position plus over, before any wrap; "wraps": how often the entry's loop was
    passed (None for a one-shot); "ended": whether the entry was left finished and handed an excess on."""
    record, ring = np.array(stream[0]).copy(), [np.array(e).copy() for e in stream[1:]]
    current, queue = np.array(program[0]).copy(), [np.array(e).copy() for e in program[1:]]
    out = np.zeros((frames, channels), f32)
    takes = []
    q = None                    # where the frame in front would have read past the end of the one-shot it finished
    for t in range(frames + 1):
        while queue and _complete(current):
            current = queue.pop(0)
        hop = 0
        while ring and _finished_one_shot(record):
            end = _end(record)
            over = q - end if q is not None else 0
            assert over >= 0
            entry = ring.pop(0)
            taken += 1
            takes.append(t)
            start = int(entry["position"]) + over
            note = dict(frame=t, hop=hop, q=end + over, end=end, over=over, start=start, wraps=None, ended=False)
            q = None
            if int(entry["flags"]) & LOOP:
                l0, l1 = int(entry["loop_start"]) << FRAC_BITS, int(entry["loop_end"]) << FRAC_BITS
                note["wraps"] = (start - l0) // (l1 - l0) if start >= l1 else 0
                entry["position"] = l0 + (start - l0) % (l1 - l0) if start >= l1 else start
            elif start >= _end(entry):
                entry["position"], entry["flags"] = _end(entry), int(entry["flags"]) & ~PLAYING
                q, note["ended"] = start, True
            else:
                entry["position"] = start
            record = entry
            hop += 1
            if trace is not None:
                trace.append(note)
        q = None                # an excess no entry was there for is lost
        if t == frames:
            break
        before, step = int(record["position"]), int(record["step"])
        playing_one_shot = int(record["flags"]) & (PLAYING | LOOP) == PLAYING
        asset = assets.get((int(record["data"]), int(record["frames"])))
        if coef is None:
            o, record, current = voice_model.render_one(record, current, asset, 1, channels)
        else:
            o, record, current = resample_ref.render_one(record, current, coef, asset, 1, channels)
        out[t] = o[0]
        if playing_one_shot and before < _end(record) and int(record["position"]) >= _end(record):
            q = before + step   # this frame's step took the one-shot to its end: the next frame would have read here
    after = np.zeros(1 + len(ring), DTYPE)
    after[0] = record
    for k, e in enumerate(ring):
        after[1 + k] = e
    program_after = np.zeros(1 + len(queue), ENV_DTYPE)
    program_after[0] = current
    for k, e in enumerate(queue):
        program_after[1 + k] = e
    return out, after, taken, program_after, takes
