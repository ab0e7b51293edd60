"""NumPy restatement of the samplers (include/oalsfx_hip.h, "samplers"): what the render kernel must write and how it must leave the
records, bit for bit.  Positions are exact unsigned 64-bit integers; sample arithmetic is float32, every operation rounded by itself."""
import numpy as np

FRAC_BITS = 12                                # OALSFX_SAMPLER_FRAC_BITS
ONE = 1 << FRAC_BITS
PCM_U8, PCM_S16, PCM_F32 = 0, 1, 2            # OALSFX_PCM_*
PLAYING, LOOP, LINEAR = 1, 2, 4               # OALSFX_SAMPLER_* flag bits
MAX_CHANNELS = 8
DTYPE = np.dtype([("data", np.uint64), ("position", np.uint64), ("frames", np.uint32), ("loop_start", np.uint32), ("loop_end", np.uint32),
                  ("step", np.uint32), ("format", np.uint32), ("channels", np.uint32), ("flags", np.uint32), ("reserved", np.uint32),
                  ("gain", np.float32, (MAX_CHANNELS,))])
PCM_DTYPE = {PCM_U8: np.uint8, PCM_S16: np.int16, PCM_F32: np.float32}
f32 = np.float32
u64 = np.uint64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_floats(a, b):
    """Bit-exact comparison of two float32 arrays; NaNs compare equal whatever their sign and payload (x86 and gfx950 encode the default
    NaN differently).  Returns (equal, number of differing elements)."""
    a = np.ascontiguousarray(a, dtype=f32).reshape(-1)
    b = np.ascontiguousarray(b, dtype=f32).reshape(-1)
    if a.size != b.size:
        return False, max(a.size, b.size)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return not bad.any(), int(bad.sum())


def to_float(pcm):
    """The conversions of the reference's demo program (src/oalsfxpp_test.cpp:713-735)."""
    if pcm.dtype == np.uint8:
        return (pcm.astype(np.int32) - 128).astype(f32) / f32(128.0)
    if pcm.dtype == np.int16:
        return pcm.astype(f32) / f32(32768.0)
    assert pcm.dtype == np.float32
    return pcm


def wrap(q, record):
    """q: uint64 array (or scalar) of positions."""
    q = np.asarray(q, dtype=u64)
    if not int(record["flags"]) & LOOP:
        return q
    l0, l1 = u64(int(record["loop_start"]) << FRAC_BITS), u64(int(record["loop_end"]) << FRAC_BITS)
    past = q >= l1
    return np.where(past, l0 + (np.where(past, q, l1) - l0) % (l1 - l0), q)


def lerp(a, b, mu):
    """The reference's Math::lerp (src/oalsfxpp.cpp:180-186), each operation rounded to float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return a + ((b - a) * mu)


def render_one(record, asset, frames, channels):
    """One instance: (out [frames][channels] float32, the record afterwards).  `asset`: [asset frames][asset channels] in its PCM type."""
    out = np.zeros((frames, channels), dtype=f32)
    after = record.copy()
    flags = int(record["flags"])
    if not flags & PLAYING:
        return out, after
    n, k = int(record["frames"]), int(record["channels"])
    assert asset.shape == (n, k) and asset.dtype == PCM_DTYPE[int(record["format"])] and k in (1, channels)
    p, step = int(record["position"]), int(record["step"])
    end = n << FRAC_BITS
    q = wrap(u64(p) + np.arange(frames, dtype=u64) * u64(step), record)
    live = np.ones(frames, dtype=bool) if flags & LOOP else q < u64(end)
    i = np.where(live, q >> u64(FRAC_BITS), u64(0)).astype(np.int64)
    m = (q & u64(ONE - 1)).astype(np.int64)
    a = to_float(asset[i])
    if flags & LINEAR:
        j = i + 1
        if flags & LOOP:
            j = np.where(j == int(record["loop_end"]), int(record["loop_start"]), j)
            b = to_float(asset[j])
        else:
            silent = j == n
            b = np.where(silent[:, None], f32(0.0), to_float(asset[np.where(silent, i, j)]))
        mu = m.astype(f32) * f32(1.0 / ONE)
        v = lerp(a, b, mu[:, None])
    else:
        v = a
    if k == 1:
        v = np.repeat(v, channels, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(live[:, None], v * record["gain"][:channels][None, :], f32(0.0)).astype(f32)
    final = int(wrap(u64(p + frames * step), record))
    if not flags & LOOP and final >= end:
        final = end
        after["flags"] = flags & ~PLAYING
    after["position"] = final
    return out, after


def render(records, assets, frames, channels):
    """records: array of DTYPE; assets[r]: the asset record r names (None where it does not play).  Returns (out [n][frames][channels],
    the records afterwards)."""
    out = np.zeros((len(records), frames, channels), dtype=f32)
    after = records.copy()
    for r in range(len(records)):
        out[r], after[r] = render_one(records[r], assets[r], frames, channels)
    return out, after
