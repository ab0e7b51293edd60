"""A second model of the voice envelopes (include/oalsfx_hip.h, "voice envelopes"), built unlike tests/voice_ref.py so that the two do not
share a mistake: one output frame after the other, and the state carried from frame to frame is the header's own words -- a delay counter
that is decremented, a ramp index and a glide index that are incremented, PHI a Python integer to which S_g is added frame by frame and
which is wrapped after every add (no closed form), PLAYING cleared at the frame at which the header says so.  Sample arithmetic in
np.float32 scalars, one operation at a time, in the stated order.  A render of F frames is F renders of one frame, so any split gives the
same outputs and records by construction.  Rows whose envelope is not ACTIVE are tests/sampler_model.py's.  Slow, and meant to be:
tests/test_voice_extremes.py holds it against the restatement."""
import numpy as np

import sampler_model
from sampler_model import _samples
from voice_ref import ACTIVE, DTYPE, GLIDE, STOP          # (the record's layout and the flag bits: nothing else comes from the restatement)

FRAC_BITS, SUB_BITS = 12, 16
FINE_BITS = FRAC_BITS + SUB_BITS
PLAYING, LOOP, LINEAR = 1, 2, 4
f32 = np.float32
_idle = {}              # rows without an envelope: (record bytes, id(asset), frames, channels) -> (asset, out, the record afterwards)


def _without_envelope(record, asset, frames, channels):
    """sampler_model.render_one, remembered: the families play the same record under several envelopes that are not ACTIVE."""
    key = (record.tobytes(), id(asset), frames, channels)
    hit = _idle.get(key)
    if hit is None or hit[0] is not asset:
        if len(_idle) > 4096:
            _idle.clear()
        hit = _idle[key] = (asset,) + sampler_model.render_one(record, asset, frames, channels)
    return hit[1].copy(), hit[2].copy()


def render_one(record, env, asset, frames, channels, trace=None):
    """One instance: (out [frames][channels] float32, the sampler's record afterwards, the envelope afterwards).  trace: a dict that
    receives what the arithmetic went through -- "kinds": one letter per output frame (d: delay, p: played, e: not playing or past a
    one-shot's end, s: behind a completed STOP); "g_slope": the largest |g * glide_slope| formed; "S": the largest fine step added;
    "phi": the largest PHI formed, before its wrap; "landed": PHI as the add that ended a one-shot left it, before it became E."""
    eflags = int(env["flags"])
    if not eflags & ACTIVE:
        out, after = _without_envelope(record, asset, frames, channels)
        return out, after, env.copy()
    out = np.zeros((frames, channels), dtype=f32)
    after, env_after = record.copy(), env.copy()
    flags, step = int(record["flags"]), int(record["step"])
    n_frames, width = int(record["frames"]), int(record["channels"])
    first, last = int(record["loop_start"]), int(record["loop_end"])
    end, l0, l1 = n_frames << FINE_BITS, first << FINE_BITS, last << FINE_BITS
    delay, R, n = int(env["delay"]), int(env["ramp_frames"]), int(env["ramp_done"])
    stop, gliding = bool(eflags & STOP), bool(eflags & GLIDE)
    G, g, slope, step_to = int(env["glide_frames"]), int(env["glide_done"]), int(env["glide_slope"]), int(env["step_to"])
    phi = (int(record["position"]) << SUB_BITS) | int(env["sub"])
    s = None
    if flags & PLAYING:
        assert asset.shape == (n_frames, width) and width in (1, channels)
        s = _samples(asset)
    gain = [f32(x) for x in record["gain"][:channels]]
    e_from, e_step, e_to = ([f32(x) for x in env[name][:channels]] for name in ("gain_from", "gain_step", "gain_to"))
    zero, scale = f32(0.0), f32(1.0) / f32(4096.0)
    kinds = []
    seen = dict(g_slope=0, S=0, phi=phi, landed=None)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for f in range(frames):
            if delay > 0:
                delay -= 1                                      # nothing else moves
                kinds.append("d")
            elif stop and n >= R:
                kinds.append("s")                               # the fade has completed: +0.0f, and the sampler stands
            else:
                if flags & PLAYING:
                    if flags & LOOP and phi >= l1:
                        phi = l0 + (phi - l0) % (l1 - l0)
                    if flags & LOOP or phi < end:
                        q = phi >> SUB_BITS
                        i, m = q >> FRAC_BITS, q & 4095
                        j = i + 1
                        if flags & LOOP and j == last:
                            j = first
                        mu = f32(m) * scale
                        v = []
                        for k in range(width):
                            a = s[i, k]
                            if flags & LINEAR:
                                b = zero if j == n_frames and not flags & LOOP else s[j, k]
                                d = b - a
                                t = d * mu
                                v.append(a + t)
                            else:
                                v.append(a)
                        nf = f32(n)
                        for c in range(channels):
                            o = v[c if width > 1 else 0] * gain[c]
                            if n < R:
                                w = nf * e_step[c]
                                e = e_from[c] + w
                            else:
                                e = e_to[c]
                            out[f, c] = o * e
                        kinds.append("p")
                    else:
                        kinds.append("e")
                    # the fine step of this frame's glide index, added; then the wrap
                    if gliding and g < G:
                        bend = g * slope
                        fine = (step << SUB_BITS) + bend
                        seen["g_slope"] = max(seen["g_slope"], abs(bend))
                    elif gliding:
                        fine = step_to << SUB_BITS
                    else:
                        fine = step << SUB_BITS
                    assert fine >= 0
                    phi += fine
                    seen["S"], seen["phi"] = max(seen["S"], fine), max(seen["phi"], phi)
                    if flags & LOOP:
                        if phi >= l1:
                            phi = l0 + (phi - l0) % (l1 - l0)
                    elif phi >= end:
                        seen["landed"] = phi
                        phi = end                               # a one-shot that has reached E: position E, sub 0, finished
                        flags &= ~PLAYING
                else:
                    kinds.append("e")
                if n < R:
                    n += 1
                if gliding and g < G:
                    g += 1
            # what holds "after the render", a render of one frame
            if stop and n == R:
                flags &= ~PLAYING
            if gliding and g == G:
                step = step_to
    assert phi < 1 << 63 and seen["phi"] < 1 << 63
    if int(record["flags"]) & PLAYING:
        after["position"], env_after["sub"] = phi >> SUB_BITS, phi & 0xFFFF
    after["flags"], after["step"] = flags, step
    env_after["delay"], env_after["ramp_done"] = delay, n
    if gliding:
        env_after["glide_done"] = g
    if trace is not None:
        if seen["landed"] is None:
            seen["landed"] = phi
        trace.update(seen, kinds="".join(kinds))
    return out, after, env_after


def render(records, envelopes, assets, frames, channels, traces=None):
    """traces: a list that receives one dict per row (see render_one; empty for a row without an envelope)."""
    assert envelopes.dtype == DTYPE and len(envelopes) == len(records)
    out = np.zeros((len(records), frames, channels), dtype=f32)
    after, env_after = records.copy(), envelopes.copy()
    for r in range(len(records)):
        trace = {} if traces is not None else None
        out[r], after[r], env_after[r] = render_one(records[r], envelopes[r], assets[r], frames, channels, trace)
        if traces is not None:
            traces.append(trace)
    return out, after, env_after
