"""NumPy restatement of the voice filter sweeps (include/oalsfx_hip.h, "voice filter sweeps") on top of biquad_ref and program_ref: a voice
whose filter is ACTIVE and whose sweep is ACTIVE with done < frames takes its five coefficients per frame, from[k] + ((float32)n *
step[k]) at the index n = done + f below the sweep's length R and to[k] from there on, the product and the sum each rounded to float32 by
themselves, and runs them through the voice filters' recurrence.  Afterwards done = min(R, done + F); the sweep that reaches R leaves `to`
in the filter's coefficients and is no longer ACTIVE.  Everything else is biquad_ref's and program_ref's."""
import numpy as np

import biquad_ref as bref
import program_ref as gref
import resample_ref as ref
from oalsfxpp_amd.api import SWEEP_DTYPE

f32 = np.float32
DTYPE = SWEEP_DTYPE
ACTIVE = 1                 # OALSFX_SWEEP_ACTIVE
MAX_FRAMES = 1 << 24       # OALSFX_SWEEP_MAX_FRAMES
TILE = 64

MESSAGES = {
    "flags": "Unknown filter sweep flags.",
    "reserved": "The filter sweep's reserved fields are not 0.",
    "frames": "The filter sweep's frame count is out of range.",
    "done": "The filter sweep is past its end.",
    "finite": "Non-finite filter sweep coefficient.",
    "filter": "The swept voice's filter is not active.",
}


def check(s):
    """None, or the text with which oalsfx_batch_set_sweeps refuses the record, the target's filter apart."""
    flags = int(s["flags"])
    if flags & ~ACTIVE:
        return MESSAGES["flags"]
    if int(s["reserved"]) != 0 or int(np.asarray(s["reserved1"], f32).view(np.uint32)) != 0:
        return MESSAGES["reserved"]
    if not (flags & ACTIVE) <= int(s["frames"]) <= MAX_FRAMES:
        return MESSAGES["frames"]
    if int(s["done"]) > int(s["frames"]):
        return MESSAGES["done"]
    if not (np.isfinite(s["from"]).all() and np.isfinite(s["step"]).all() and np.isfinite(s["to"]).all()):
        return MESSAGES["finite"]
    return None


def make(from_coef, to_coef, frames, done=0):
    """oalsfx_host_filter_sweep: one record, as an array of one."""
    s = np.zeros(1, DTYPE)
    s["flags"], s["frames"], s["done"] = ACTIVE, frames, done
    s["from"], s["to"] = np.asarray(from_coef, f32), np.asarray(to_coef, f32)
    s["step"] = ((s["to"] - s["from"]).astype(f32) / f32(frames)).astype(f32)
    return s


def under_way(sweep):
    return bool(int(sweep["flags"]) & ACTIVE) and int(sweep["done"]) < int(sweep["frames"])


def coefficients(sweep, frames, how="stated"):
    """[frames][5] float32: the coefficients of the `frames` frames behind sweep["done"].  how: "stated", or one of three other ways that
    a kernel might take (tests/test_sweep_ref.py shows that the comparison tells them apart): "running" (c += step from the sweep's first
    frame on), "fma" (the product and the sum rounded once), "tile" (the coefficients of a 64-frame tile's first frame held over the
    tile)."""
    done, length = int(sweep["done"]), int(sweep["frames"])
    a, step, to = (np.asarray(sweep[k], f32) for k in ("from", "step", "to"))
    f = np.arange(frames)
    if how == "tile":
        f = f // TILE * TILE
    n = done + f
    if how == "running":
        run = np.empty((done + frames + 1, 5), f32)
        run[0] = a
        for m in range(done + frames):
            run[m + 1] = run[m] + step
        c = run[np.minimum(n, done + frames)]
    elif how == "fma":
        c = (n[:, None].astype(np.float64) * step.astype(np.float64) + a.astype(np.float64)).astype(f32)
    else:
        c = (a + (n[:, None].astype(f32) * step).astype(f32)).astype(f32)
    c = c.astype(f32)
    c[n >= length] = to
    return c


def process(coef, x, xh, yh):
    """biquad_ref.process with a row of coefficients per frame: coef [F][5], x [F][C], xh and yh [C][2]."""
    x = np.asarray(x, f32)
    xh, yh = np.array(xh, f32), np.array(yh, f32)
    y = np.empty_like(x)
    x1, x2, y1, y2 = xh[:, 0], xh[:, 1], yh[:, 0], yh[:, 1]
    with np.errstate(all="ignore"):
        for f in range(x.shape[0]):
            b0, b1, b2, a1, a2 = coef[f]
            xf = x[f]
            u = ((b0 * xf) + (b1 * x1)) + (b2 * x2)
            yf = (u - (a1 * y1)) - (a2 * y2)
            y[f] = yf
            x2, x1, y2, y1 = x1, xf, y1, yf
    return y, np.stack([x1, x2], axis=-1).astype(f32), np.stack([y1, y2], axis=-1).astype(f32)


def filter_one(record, sweep, x, channels, how="stated"):
    """One filter record, its sweep record and the voice's frames x [F][channels] -> (y, the filter afterwards, the sweep afterwards)."""
    if not under_way(sweep):
        y, after = bref.filter_one(record, x, channels)
        return y, after, sweep.copy()
    frames = x.shape[0]
    after, s_after = record.copy(), sweep.copy()
    y, xh, yh = process(coefficients(sweep, frames, how), x, record["x"][:channels], record["y"][:channels])
    after["x"][:channels], after["y"][:channels] = xh, yh
    s_after["done"] = min(int(sweep["frames"]), int(sweep["done"]) + frames)
    if int(s_after["done"]) == int(sweep["frames"]):
        for k, name in enumerate(bref.COEFFICIENTS):
            after[name] = sweep["to"][k]
        s_after["flags"] = int(sweep["flags"]) & ~ACTIVE
    return y, after, s_after


def render(records, programs, resamplers, filters, sweeps, tables, assets, frames, channels, how="stated"):
    """program_ref.render with sweeps [K][n] of DTYPE beside the filters.  Returns (out [n][frames][channels], the records, the programs,
    the filters and the sweeps afterwards)."""
    lanes, n = records.shape
    out = np.zeros((n, frames, channels), dtype=f32)
    after, filters_after, sweeps_after = records.copy(), filters.copy(), sweeps.copy()
    programs_after = [[None] * n for _ in range(lanes)]
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, after[k][i], programs_after[k][i] = gref.render_voice(records[k][i], programs[k][i], coef, assets[k][i], frames, channels)
            if filters[k][i]["flags"] & bref.ACTIVE:
                o, filters_after[k][i], sweeps_after[k][i] = filter_one(filters[k][i], sweeps[k][i], o, channels, how)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = o if lanes == 1 else (acc + o).astype(f32)
        out[i] = acc
    return out, after, programs_after, filters_after, sweeps_after
