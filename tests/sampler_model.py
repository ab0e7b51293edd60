"""A second model of the samplers (include/oalsfx_hip.h, "samplers"), built unlike tests/sampler_ref.py so that the two do not share a
mistake: one frame after the other, the position a Python integer that is carried forward with q += step and wrapped, never recomputed
as P + f * step; the sample arithmetic in np.float32 scalars, one operation at a time, in the order the header states.  Slow, and meant
to be: tests/test_sampler_extremes.py holds it against the restatement."""
import numpy as np

from sampler_ref import DTYPE, to_float

FRAC_BITS = 12
PLAYING, LOOP, LINEAR = 1, 2, 4
f32 = np.float32
_converted = {}         # id(asset) -> (asset, its samples as float32): an asset is converted once however many records play it


def _samples(asset):
    hit = _converted.get(id(asset))
    if hit is None or hit[0] is not asset:
        hit = _converted[id(asset)] = (asset, to_float(asset))
    return hit[1]


def render_one(record, asset, frames, channels):
    """One instance: (out [frames][channels] float32, the record afterwards)."""
    out = np.zeros((frames, channels), dtype=f32)
    after = record.copy()
    flags = int(record["flags"])
    if not flags & PLAYING:
        return out, after
    n, width, step = int(record["frames"]), int(record["channels"]), int(record["step"])
    assert asset.shape == (n, width) and width in (1, channels)
    s = _samples(asset)
    gain = [f32(g) for g in record["gain"][:channels]]
    end = n << FRAC_BITS
    first, last = int(record["loop_start"]), int(record["loop_end"])
    l0, l1 = first << FRAC_BITS, last << FRAC_BITS
    zero, scale = f32(0.0), f32(1.0) / f32(4096.0)
    q = int(record["position"])
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for f in range(frames + 1):
            if flags & LOOP and q >= l1:
                q = l0 + (q - l0) % (l1 - l0)
            if f == frames:
                break                                   # q is the position after the call
            if flags & LOOP or q < end:
                i, m = q >> FRAC_BITS, q & 4095
                j = i + 1
                if flags & LOOP and j == last:
                    j = first
                mu = f32(m) * scale
                v = []
                for k in range(width):
                    a = s[i, k]
                    if flags & LINEAR:
                        b = zero if j == n and not flags & LOOP else s[j, k]
                        d = b - a
                        t = d * mu
                        v.append(a + t)
                    else:
                        v.append(a)
                for c in range(channels):
                    out[f, c] = v[c if width > 1 else 0] * gain[c]
            q += step
    if not flags & LOOP and q >= end:
        q = end
        after["flags"] = flags & ~PLAYING
    after["position"] = q
    return out, after


def render(records, assets, frames, channels):
    assert records.dtype == DTYPE
    out = np.zeros((len(records), frames, channels), dtype=f32)
    after = records.copy()
    for r in range(len(records)):
        out[r], after[r] = render_one(records[r], assets[r], frames, channels)
    return out, after
