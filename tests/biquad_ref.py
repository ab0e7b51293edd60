"""NumPy restatement of the voice filters (include/oalsfx_hip.h, "voice filters") on top of polyphony_ref: a voice whose filter is ACTIVE is
rendered by itself (resample_ref.render_one), run through y_f = ((((b0 * x_f) + (b1 * x_(f-1))) + (b2 * x_(f-2))) - (a1 * y_(f-1))) -
(a2 * y_(f-2)) over every frame of the render, every operation rounded to float32 by itself, and stands with y where it stood with its
own value: stored at one lane, summed in ascending lanes from +0.0f at two or more.  The histories afterwards are those of the render's
last two frames; channels at and above the channel count are never touched."""
import numpy as np

import resample_ref as ref
from oalsfxpp_amd.api import FILTER_DTYPE

f32 = np.float32
DTYPE = FILTER_DTYPE
ACTIVE, LOAD = 1, 2       # OALSFX_VF_ACTIVE, OALSFX_VF_LOAD
COEFFICIENTS = ("b0", "b1", "b2", "a1", "a2")


def process(coef, x, xh, yh):
    """coef [..., 5] (b0 b1 b2 a1 a2), x [..., F, C], xh and yh [..., C, 2] ([..., 0] the last, [..., 1] the one before), all float32 ->
    (y [..., F, C], the histories afterwards).  The stated order; vectorised over the leading axes."""
    x = np.asarray(x, f32)
    frames = x.shape[-2]
    b0, b1, b2, a1, a2 = (np.asarray(coef, f32)[..., k, None] for k in range(5))        # [..., 1]: against [..., C]
    xh, yh = np.array(xh, f32), np.array(yh, f32)
    y = np.empty_like(x)
    x1, x2, y1, y2 = xh[..., 0], xh[..., 1], yh[..., 0], yh[..., 1]
    with np.errstate(all="ignore"):
        for f in range(frames):
            xf = x[..., f, :]
            u = ((b0 * xf) + (b1 * x1)) + (b2 * x2)
            yf = (u - (a1 * y1)) - (a2 * y2)
            y[..., f, :] = yf
            x2, x1, y2, y1 = x1, xf, y1, yf
    return y, np.stack([x1, x2], axis=-1).astype(f32), np.stack([y1, y2], axis=-1).astype(f32)


def coefficients(record):
    return np.stack([record[k] for k in COEFFICIENTS], axis=-1).astype(f32)


def filter_one(record, x, channels):
    """One record of DTYPE and its voice's frames x [F][channels] -> (y, the record afterwards)."""
    after = record.copy()
    y, xh, yh = process(coefficients(record), x, record["x"][:channels], record["y"][:channels])
    after["x"][:channels], after["y"][:channels] = xh, yh
    return y, after


def render(records, envelopes, resamplers, filters, tables, assets, frames, channels):
    """polyphony_ref.render with filters [K][n] of DTYPE beside the three tables.  Returns (out [n][frames][channels], the records, the
    envelopes and the filters afterwards)."""
    lanes, n = records.shape
    assert envelopes.shape == (lanes, n) and np.shape(resamplers) == (lanes, n) and filters.shape == (lanes, n)
    out = np.zeros((n, frames, channels), dtype=f32)
    after, env_after, filters_after = records.copy(), envelopes.copy(), filters.copy()
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, after[k][i], env_after[k][i] = ref.render_one(records[k][i], envelopes[k][i], coef, assets[k][i], frames, channels)
            if filters[k][i]["flags"] & ACTIVE:
                o, filters_after[k][i] = filter_one(filters[k][i], o, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = o if lanes == 1 else (acc + o).astype(f32)
        out[i] = acc
    return out, after, env_after, filters_after


# ---- other evaluations of the same filter, for tests/test_biquad_abi.py::test_another_order_shows ----
def process_other(coef, x, how):
    """One channel from zero histories, x [F] float32, in one of three other orders: "fma" (a fused multiply-add chain, each step
    rounded once), "grouped" (u - ((a1 * y1) + (a2 * y2))), "from the right" ((b0 * x) + ((b1 * x1) + (b2 * x2)))."""
    b0, b1, b2, a1, a2 = (f32(c) for c in coef)
    fma = lambda a, b, c: f32(np.float64(a) * np.float64(b) + np.float64(c))      # exact product and sum of two floats in double, rounded once
    y = np.empty(len(x), f32)
    x1 = x2 = y1 = y2 = f32(0)
    for f, xf in enumerate(x):
        if how == "fma":
            yf = fma(-a2, y2, fma(-a1, y1, fma(b2, x2, fma(b1, x1, f32(b0 * xf)))))
        elif how == "grouped":
            yf = f32(f32(f32(f32(b0 * xf) + f32(b1 * x1)) + f32(b2 * x2)) - f32(f32(a1 * y1) + f32(a2 * y2)))
        else:
            u = f32(f32(b0 * xf) + f32(f32(b1 * x1) + f32(b2 * x2)))
            yf = f32(f32(u - f32(a1 * y1)) - f32(a2 * y2))
        y[f] = yf
        x2, x1, y2, y1 = x1, xf, y1, yf
    return y
