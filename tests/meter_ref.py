"""The level meters' arithmetic restated in NumPy (include/oalsfx_hip.h, "level meters"): what the device kernel is held to, bit for bit.

Per row and channel: the peak is the largest |x| (a NaN takes no part); the sum of squares is built by LANES lanes -- lane l adds the
squares of its frames f = l, l + LANES, ... in ascending order from +0.0f, block of LANES frames after block --, then the tree s = LANES / 2
.. 1 adds lane l + s into lane l; fp32, product and sum rounded separately.  NumPy's float32 multiply and add round once each and never
fuse, and the loops below fix the order."""
import numpy as np

from downmix_ref import same_bits  # noqa: F401  (the comparison the tests use for float fields)

LANES = 64  # OALSFX_METER_LANES
CARRY = 1   # OALSFX_METER_CARRY
MAX_CHANNELS = 8
UINT32_MAX = 0xFFFFFFFF
DTYPE = np.dtype([("peak", np.float32, (MAX_CHANNELS,)), ("sumsq", np.float32, (MAX_CHANNELS,)), ("peak_hold", np.float32),
                  ("quiet_run", np.uint32), ("nonfinite", np.uint32), ("frames", np.uint32)])


def sumsq(x, lanes=LANES):
    """x: float32 [rows][frames][channels].  Returns float32 [rows][channels] in the stated order with `lanes` lanes (a power of two)."""
    x = np.asarray(x, dtype=np.float32)
    rows, frames, channels = x.shape
    q = np.zeros((rows, lanes, channels), dtype=np.float32)
    with np.errstate(all="ignore"):
        for base in range(0, frames, lanes):       # block after block: every lane takes its next frame
            block = x[:, base:base + lanes]
            q[:, :block.shape[1]] = q[:, :block.shape[1]] + block * block
        s = lanes // 2
        while s >= 1:
            q[:, :s] = q[:, :s] + q[:, s:2 * s]
            s //= 2
    return q[:, 0].copy()


def meter(x, threshold, old=None, lanes=LANES):
    """x: float32 [rows][frames][channels], frames >= 1.  old: the records at the destination (DTYPE, [rows]) for a call with CARRY, None
    for one without.  Returns the records the call writes (DTYPE, [rows])."""
    x = np.asarray(x, dtype=np.float32)
    rows, frames, channels = x.shape
    threshold = np.float32(threshold)
    out = np.zeros(rows, dtype=DTYPE)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        out["peak"][:, :channels] = np.fmax(np.float32(0.0), np.fmax.reduce(a, axis=1, initial=np.float32(0.0)))
        out["sumsq"][:, :channels] = sumsq(x, lanes)
        out["nonfinite"] = (~(a < np.float32(np.inf))).sum(axis=(1, 2))
        loud = (~(a <= threshold)).any(axis=2)                                          # [rows][frames]
    last = np.where(loud.any(axis=1), frames - 1 - np.argmax(loud[:, ::-1], axis=1), -1)
    quiet = (frames - 1 - last).astype(np.int64)                                        # T; `frames` where no frame is loud
    hold = np.fmax.reduce(out["peak"][:, :channels], axis=1)
    if old is None:
        out["quiet_run"] = quiet
        out["peak_hold"] = hold
    else:
        old = np.asarray(old, dtype=DTYPE)
        carried = np.minimum(old["quiet_run"].astype(np.int64) + frames, UINT32_MAX)
        out["quiet_run"] = np.where(quiet == frames, carried, quiet)
        out["peak_hold"] = np.fmax(old["peak_hold"], hold)
    out["frames"] = frames
    return out


def same_records(got, want):
    """Every field equal: the float fields on their bit patterns (NaNs by position), the integer fields exactly."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    return (all(same_bits(got[f], want[f]) for f in ("peak", "sumsq", "peak_hold")) and
            all(np.array_equal(got[f], want[f]) for f in ("quiet_run", "nonfinite", "frames")))


def first_difference(got, want):
    """(row, field) of the first record that differs, for a test's message."""
    for r in range(len(want)):
        for f in DTYPE.names:
            a, b = np.atleast_1d(got[r][f]), np.atleast_1d(want[r][f])
            if a.dtype.kind == "f":
                if not same_bits(a, b):
                    return r, f, a.tolist(), b.tolist()
            elif not np.array_equal(a, b):
                return r, f, a.tolist(), b.tolist()
    return None
