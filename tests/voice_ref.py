"""NumPy and Python-integer restatement of the voice envelopes (include/oalsfx_hip.h, "voice envelopes"): what the render kernel must
write and how it must leave the sampler's record and the envelope, bit for bit.  Positions are exact integers (PHI: 28 fractional bits),
checked against 2^63 with Python's unbounded ones; sample arithmetic is float32, every operation rounded by itself."""
import numpy as np

import sampler_ref as sref

ACTIVE, STOP, GLIDE = 1, 2, 4                 # OALSFX_ENV_* flag bits
SUB_BITS = 16                                 # OALSFX_ENV_SUB_BITS
SUB_ONE = 1 << SUB_BITS
FINE_BITS = sref.FRAC_BITS + SUB_BITS
MAX_RAMP, MAX_GLIDE, MAX_STEP = 1 << 24, 1 << 20, 1 << 20
MAX_CHANNELS = sref.MAX_CHANNELS
DTYPE = np.dtype([("flags", np.uint32), ("delay", np.uint32), ("ramp_frames", np.uint32), ("ramp_done", np.uint32),
                  ("gain_from", np.float32, (MAX_CHANNELS,)), ("gain_step", np.float32, (MAX_CHANNELS,)), ("gain_to", np.float32, (MAX_CHANNELS,)),
                  ("glide_frames", np.uint32), ("glide_done", np.uint32), ("glide_slope", np.int32), ("step_to", np.uint32), ("sub", np.uint32),
                  ("reserved", np.uint32, (3,))])
FIELDS = DTYPE.names
OFFSETS = [0, 4, 8, 12, 16, 48, 80, 112, 116, 120, 124, 128, 132]
f32 = np.float32
PLAYING, LOOP, LINEAR = sref.PLAYING, sref.LOOP, sref.LINEAR


# ---- the host helpers' arithmetic ----
def ramp(env, gain_from, gain_to, frames):
    """oalsfx_host_envelope_ramp: step = (to - from) / (float)frames, one subtraction and one division in float32; frames == 0: 0."""
    gain_from, gain_to = np.asarray(gain_from, f32), np.asarray(gain_to, f32)
    c = len(gain_from)
    env["gain_from"][:c], env["gain_to"][:c] = gain_from, gain_to
    with np.errstate(invalid="ignore", over="ignore"):
        env["gain_step"][:c] = (gain_to - gain_from) / f32(frames) if frames else f32(0.0)
    env["ramp_frames"], env["ramp_done"] = frames, 0
    return env


def glide_slope(step, step_to, frames):
    """((int64)(step_to - step) << 16) / frames, truncated toward zero; frames == 0: 0; beyond int32: +-(2^31 - 1)."""
    if not frames:
        return 0
    fine = (step_to - step) * SUB_ONE
    return min(abs(fine) // frames, 2 ** 31 - 1) * (1 if fine >= 0 else -1)


def glide(env, step, step_to, frames):
    """oalsfx_host_envelope_glide."""
    env["flags"] = int(env["flags"]) | GLIDE
    env["glide_frames"], env["glide_done"], env["glide_slope"], env["step_to"] = frames, 0, glide_slope(step, step_to, frames), step_to
    return env


# ---- positions: Python integers ----
def fine_step(step, env_glide, g):
    """S_g.  env_glide: (G, slope, step_to), or None without GLIDE."""
    if env_glide is None:
        return step << SUB_BITS
    G, slope, step_to = env_glide
    return (step << SUB_BITS) + g * slope if g < G else step_to << SUB_BITS


def advance(step, env_glide, g0, frames):
    """The sum of S_(g0 + j) over j < frames, in closed form."""
    if env_glide is None:
        return frames * (step << SUB_BITS)
    G, slope, step_to = env_glide
    m = min(frames, max(G - g0, 0))
    return m * ((step << SUB_BITS) + g0 * slope) + slope * (m * (m - 1) // 2) + (frames - m) * (step_to << SUB_BITS)


def wrap_fine(phi, record):
    """wrapF on a Python integer."""
    if not int(record["flags"]) & LOOP:
        return phi
    l0, l1 = int(record["loop_start"]) << FINE_BITS, int(record["loop_end"]) << FINE_BITS
    return phi if phi < l1 else l0 + (phi - l0) % (l1 - l0)


def fine_positions(record, env_glide, phi0, g0, frames):
    """PHI_f', wrapped, for f' < frames as a uint64 array: the closed form in int64 where every sum stays below 2^62, else in Python's
    integers; either way no sum may reach 2^63."""
    step = int(record["step"])
    total = phi0 + advance(step, env_glide, g0, frames)
    assert 0 <= total < 2 ** 63, "a position sum leaves 63 bits"
    if total < 2 ** 62:
        t = np.arange(frames, dtype=np.int64)
        if env_glide is None:
            off = t * np.int64(step << SUB_BITS)
        else:
            G, slope, step_to = env_glide
            m = np.minimum(t, max(G - g0, 0))
            off = m * np.int64((step << SUB_BITS) + g0 * slope) + np.int64(slope) * (m * (m - 1) // 2) + (t - m) * np.int64(step_to << SUB_BITS)
        assert (off >= 0).all()
        phi = (np.int64(phi0) + off).astype(np.uint64)
        if int(record["flags"]) & LOOP:
            l0, l1 = np.uint64(int(record["loop_start"]) << FINE_BITS), np.uint64(int(record["loop_end"]) << FINE_BITS)
            past = phi >= l1
            phi = np.where(past, l0 + (np.where(past, phi, l1) - l0) % (l1 - l0), phi)
        return phi
    return np.asarray([wrap_fine(phi0 + advance(step, env_glide, g0, t), record) for t in range(frames)], dtype=np.uint64)


def values(record, asset, q, channels):
    """The samplers' frame at every 12-bit position q (uint64): (v * gain [len(q)][channels], live)."""
    flags, n, k = int(record["flags"]), int(record["frames"]), int(record["channels"])
    assert asset.shape == (n, k) and asset.dtype == sref.PCM_DTYPE[int(record["format"])] and k in (1, channels)
    live = np.ones(len(q), dtype=bool) if flags & LOOP else q < np.uint64(n << sref.FRAC_BITS)
    i = np.where(live, q >> np.uint64(sref.FRAC_BITS), np.uint64(0)).astype(np.int64)
    a = sref.to_float(asset[i])
    if flags & LINEAR:
        j = i + 1
        if flags & LOOP:
            j = np.where(j == int(record["loop_end"]), int(record["loop_start"]), j)
            b = sref.to_float(asset[j])
        else:
            silent = j == n
            b = np.where(silent[:, None], f32(0.0), sref.to_float(asset[np.where(silent, i, j)]))
        mu = (q & np.uint64(sref.ONE - 1)).astype(np.int64).astype(f32) * f32(1.0 / sref.ONE)
        v = sref.lerp(a, b, mu[:, None])
    else:
        v = a
    if k == 1:
        v = np.repeat(v, channels, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (v * record["gain"][:channels][None, :]).astype(f32), live


def factors(env, n, channels):
    """e_c for the ramp indices n (int64 array): from + ((float)n * step) below R, to from R on."""
    R = int(env["ramp_frames"])
    with np.errstate(invalid="ignore", over="ignore"):
        ramped = env["gain_from"][:channels][None, :] + (n.astype(f32)[:, None] * env["gain_step"][:channels][None, :])
    return np.where((n < R)[:, None], ramped, env["gain_to"][:channels][None, :]).astype(f32)


def render_one(record, env, asset, frames, channels):
    """One instance: (out [frames][channels] float32, the sampler's record afterwards, the envelope afterwards)."""
    eflags = int(env["flags"])
    if not eflags & ACTIVE:
        out, after = sref.render_one(record, asset, frames, channels)
        return out, after, env.copy()
    out = np.zeros((frames, channels), dtype=f32)
    after, env_after = record.copy(), env.copy()
    flags, step = int(record["flags"]), int(record["step"])
    delay, R, n0 = int(env["delay"]), int(env["ramp_frames"]), int(env["ramp_done"])
    D = min(delay, frames)
    shown = frames - D                                                  # F'
    advanced = min(shown, R - n0) if eflags & STOP else shown           # F''
    env_glide = (int(env["glide_frames"]), int(env["glide_slope"]), int(env["step_to"])) if eflags & GLIDE else None
    g0 = int(env["glide_done"]) if eflags & GLIDE else 0
    env_after["delay"] = delay - D
    env_after["ramp_done"] = min(R, n0 + shown)
    if flags & PLAYING and advanced > 0:
        phi0 = (int(record["position"]) << SUB_BITS) | int(env["sub"])
        phi = fine_positions(record, env_glide, phi0, g0, advanced)
        o, live = values(record, asset, phi >> np.uint64(SUB_BITS), channels)
        e = factors(env, n0 + np.arange(advanced, dtype=np.int64), channels)
        with np.errstate(invalid="ignore", over="ignore"):
            out[D:D + advanced] = np.where(live[:, None], o * e, f32(0.0))
        end = wrap_fine(phi0 + advance(step, env_glide, g0, advanced), record)
        if not flags & LOOP and end >= int(record["frames"]) << FINE_BITS:
            end = int(record["frames"]) << FINE_BITS
            flags &= ~PLAYING
        after["position"], env_after["sub"] = end >> SUB_BITS, end & (SUB_ONE - 1)
    if eflags & GLIDE:
        env_after["glide_done"] = min(env_glide[0], g0 + advanced)
        if env_after["glide_done"] == env_glide[0]:
            after["step"] = env_glide[2]
    if eflags & STOP and env_after["ramp_done"] == R:
        flags &= ~PLAYING
    after["flags"] = flags
    return out, after, env_after


def render(records, envelopes, assets, frames, channels):
    """records: array of sampler_ref.DTYPE; envelopes: array of DTYPE; assets[r]: the asset record r names (None where it never plays).
    Returns (out [n][frames][channels], the records afterwards, the envelopes afterwards)."""
    out = np.zeros((len(records), frames, channels), dtype=f32)
    after, env_after = records.copy(), envelopes.copy()
    for r in range(len(records)):
        out[r], after[r], env_after[r] = render_one(records[r], envelopes[r], assets[r], frames, channels)
    return out, after, env_after


def same_envelopes(got, want):
    """Integers equal, gains equal on their bits (NaNs by position)."""
    return all((sref.same_floats(got[f], want[f])[0] if f.startswith("gain_") else bool((got[f] == want[f]).all())) for f in FIELDS)


def check(env, step):
    """What oalsfx_batch_set_envelopes refuses in one record whose sampler has `step`: the message's key words, or None."""
    flags = int(env["flags"])
    if flags & ~(ACTIVE | STOP | GLIDE):
        return "Unknown envelope flags"
    if env["reserved"].any():
        return "reserved"
    if int(env["ramp_frames"]) > MAX_RAMP:
        return "ramp is longer"
    if int(env["ramp_done"]) > int(env["ramp_frames"]):
        return "ramp_done"
    if int(env["sub"]) >= SUB_ONE:
        return "sub is beyond"
    if flags & GLIDE:
        if int(env["glide_frames"]) > MAX_GLIDE:
            return "glide is longer"
        if int(env["glide_done"]) > int(env["glide_frames"]):
            return "glide_done"
        if int(env["step_to"]) >= MAX_STEP:
            return "step_to"
        if step >= MAX_STEP:
            return "gliding sampler's step"
        if not 0 <= (step << SUB_BITS) + int(env["glide_frames"]) * int(env["glide_slope"]) < 1 << 36:
            return "leaves the range"
    return None


# ---- seeded random record pairs ----
CALLS = (441, 256, 1, 1802)     # the split the tests hold against one render of their sum


def random_pairs(rng, count, channels, calls=CALLS, **kw):
    """`count` sampler records (tests/test_sampler_abi.py: random_records) with an envelope each, the envelopes' kinds taken in turn so
    that every one of them occurs whatever the seed: delays that end inside a call, on a call's boundary and in a later call; ramps of
    0, 1 and more frames that end inside and between calls or never; STOP; ramps and glides already under way; glides up and down that
    end inside and between calls; envelopes that are not ACTIVE; samplers that are not PLAYING.  Returns (records, envelopes, the asset
    of every record, its number in the pool, the pool)."""
    from test_sampler_abi import random_records
    records, assets, keys, pool = random_records(rng, count, channels, **kw)
    total = sum(calls)
    edges = np.cumsum(calls).tolist()
    delays = [0, 0, 5, calls[0], calls[0] - 1, edges[1] + 1, edges[1], 0, total + 7, 0]
    ramps = [0, 1, 64, 300, calls[0], edges[1], edges[2] + 100, total, total + 1000, 700, 37]
    envelopes = np.zeros(count, DTYPE)
    for r in range(count):
        e = envelopes[r]
        kind = r % 16
        if kind == 15:
            # not ACTIVE: every field is noise that must stay as it is
            e["delay"], e["ramp_frames"], e["sub"] = rng.integers(0, 1000, 3)
            e["flags"] = (STOP | GLIDE) & int(rng.integers(0, 8))
            e["gain_to"][:] = rng.uniform(-1, 1, MAX_CHANNELS)
            continue
        flags = ACTIVE
        e["delay"] = delays[(r // 16) % len(delays)] if kind % 2 else 0
        R = ramps[(r // 3) % len(ramps)]
        ramp(e, rng.uniform(-1, 1, channels), rng.uniform(-1, 1, channels), R)
        if kind in (3, 4, 9):
            e["ramp_done"] = int(rng.integers(0, R + 1))
        if kind in (2, 3, 6, 7, 11):
            flags |= STOP
        e["flags"] = flags
        if kind in (4, 5, 6, 7, 8, 9, 10):
            step = int(records[r]["step"])
            G = (0, 1, 100, 441, 697, 1500, total, total + 500)[(r // 16) % 8]
            step_to = int(rng.integers(0, 8 * sref.ONE)) if kind != 10 else 0
            glide(e, step, step_to, G)
            if kind in (8, 9):
                e["glide_done"] = int(rng.integers(0, G + 1))
        if kind in (5, 9, 12):
            e["sub"] = int(rng.integers(0, SUB_ONE))
        if kind == 13:
            records[r]["flags"] = int(records[r]["flags"]) & ~PLAYING
        assert check(e, int(records[r]["step"])) is None
    return records, envelopes, assets, keys, pool
