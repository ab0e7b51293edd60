"""NumPy restatement of the resamplers (include/oalsfx_hip.h, "resamplers"): the value of a frame through a 4- or 8-tap phase table, and
the host helpers that make tables.  Positions, wrapping, envelopes and both records afterwards are voice_ref's, which this module reuses;
an envelope that is not ACTIVE is PHI = position << 16 without a glide, which the header states is the samplers' arithmetic.  Sample
arithmetic is float32, every product and every sum rounded by itself, the taps in ascending order."""
import numpy as np

import sampler_ref as sref
import voice_ref as vref

f32 = np.float32
FIR_TABLES, NONE = 8, -1                      # OALSFX_FIR_TABLES, OALSFX_RESAMPLER_NONE
FRAC_BITS, ONE = sref.FRAC_BITS, sref.ONE
PLAYING, LOOP, LINEAR = sref.PLAYING, sref.LOOP, sref.LINEAR
ACTIVE, STOP, GLIDE = vref.ACTIVE, vref.STOP, vref.GLIDE
SUB_BITS, SUB_ONE, FINE_BITS = vref.SUB_BITS, vref.SUB_ONE, vref.FINE_BITS


# ---- the host helpers ----
def check(taps, phase_bits, coef):
    """oalsfx_host_fir_check: the refusal's text, or None."""
    if taps not in (4, 8):
        return "Unknown FIR tap count."
    if not 0 <= phase_bits <= FRAC_BITS:
        return "FIR phase bits out of range."
    if coef is None:
        return "Null FIR coefficients."
    if not np.isfinite(np.asarray(coef, f32).reshape(-1)[:(1 << phase_bits) * taps]).all():
        return "Non-finite FIR coefficient."
    return None


def cubic(phase_bits):
    """oalsfx_host_fir_cubic: Catmull-Rom at mu = p / P, in double (every term exact there), converted to float once."""
    mu = np.arange(1 << phase_bits, dtype=np.float64) / (1 << phase_bits)
    mu2, mu3 = mu * mu, mu * mu * mu
    return np.stack([-0.5 * mu3 + mu2 - 0.5 * mu, 1.5 * mu3 - 2.5 * mu2 + 1.0, -1.5 * mu3 + 2.0 * mu2 + 0.5 * mu, 0.5 * mu3 - 0.5 * mu2], axis=1).astype(f32)


def sinc_double(taps, phase_bits, cutoff):
    """oalsfx_host_fir_sinc before its conversion to float: h = cutoff * sinc(cutoff * d) * w(d / H), each phase divided by its sum."""
    P, H = 1 << phase_bits, taps // 2
    d = (np.arange(taps, dtype=np.float64) - (H - 1))[None, :] - (np.arange(P, dtype=np.float64) / P)[:, None]
    x = d / H
    h = cutoff * np.sinc(cutoff * d) * (0.42 + 0.5 * np.cos(np.pi * x) + 0.08 * np.cos(2.0 * np.pi * x))
    return h / h.sum(axis=1, keepdims=True)


def sinc(taps, phase_bits, cutoff):
    return sinc_double(taps, phase_bits, cutoff).astype(f32)


def linear_table(phase_bits):
    """Rows (0, 1 - mu, mu, 0): the samplers' LINEAR up to rounding (1 - mu is exact)."""
    mu = (np.arange(1 << phase_bits, dtype=np.float64) / (1 << phase_bits)).astype(f32)
    zero = np.zeros_like(mu)
    return np.stack([zero, f32(1.0) - mu, mu, zero], axis=1).astype(f32)


def nearest_table(phase_bits, taps=4):
    """Rows (0, 1, 0, 0): the samplers' nearest sample, exactly."""
    t = np.zeros((1 << phase_bits, taps), f32)
    t[:, taps // 2 - 1] = 1.0
    return t


# ---- the value of a frame ----
def taps_of(record, asset, i, live, taps):
    """x_k for every frame whose integer position is i (int64; 0 where not live): (x [len(i)][taps][asset channels] float32, in range
    [len(i)][taps])."""
    flags, n = int(record["flags"]), int(record["frames"])
    H = taps // 2
    x = np.zeros((len(i), taps, asset.shape[1]), f32)
    inside = np.zeros((len(i), taps), bool)
    for k in range(taps):
        j = i - (H - 1) + k
        if flags & LOOP:
            l0, l1 = int(record["loop_start"]), int(record["loop_end"])
            ok = live & (j >= 0)
            at = np.where(j >= l1, l0 + (j - l1) % (l1 - l0), j)
        else:
            ok = live & (j >= 0) & (j < n)
            at = j
        at = np.where(ok, at, 0)
        assert ((at >= 0) & (at < n)).all(), "a tap outside the asset"
        x[:, k] = np.where(ok[:, None], sref.to_float(asset[at]), f32(0.0))
        inside[:, k] = ok
    return x, inside


def fir(coef_rows, x):
    """v = (((+0.0f + c_0 x_0) + c_1 x_1) + ...) + c_(T-1) x_(T-1): coef_rows [n][T], x [n][T][K]."""
    v = np.zeros((x.shape[0], x.shape[2]), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[1]):
            v = v + (coef_rows[:, k][:, None] * x[:, k])
    return v.astype(f32)


def values(record, asset, q, channels, coef):
    """The frame at every 12-bit position q (uint64) through the table coef [P][T]: (v * gain [len(q)][channels], live)."""
    flags, n, k = int(record["flags"]), int(record["frames"]), int(record["channels"])
    assert asset.shape == (n, k) and asset.dtype == sref.PCM_DTYPE[int(record["format"])] and k in (1, channels)
    phases, taps = coef.shape
    bits = phases.bit_length() - 1
    assert coef.dtype == f32 and taps in (4, 8) and phases == 1 << bits and bits <= FRAC_BITS
    live = np.ones(len(q), dtype=bool) if flags & LOOP else q < np.uint64(n << FRAC_BITS)
    i = np.where(live, q >> np.uint64(FRAC_BITS), np.uint64(0)).astype(np.int64)
    phase = ((q & np.uint64(ONE - 1)) >> np.uint64(FRAC_BITS - bits)).astype(np.int64)
    x, _ = taps_of(record, asset, i, live, taps)
    v = fir(coef[phase], x)
    if k == 1:
        v = np.repeat(v, channels, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (v * record["gain"][:channels][None, :]).astype(f32), live


def render_one(record, env, coef, asset, frames, channels):
    """One instance: (out [frames][channels] float32, the sampler's record afterwards, the envelope afterwards).  coef None: no table."""
    if coef is None:
        return vref.render_one(record, env, asset, frames, channels)
    eflags = int(env["flags"])
    active = bool(eflags & ACTIVE)
    out = np.zeros((frames, channels), dtype=f32)
    after, env_after = record.copy(), env.copy()
    flags, step = int(record["flags"]), int(record["step"])
    delay, R, n0 = (int(env["delay"]), int(env["ramp_frames"]), int(env["ramp_done"])) if active else (0, 0, 0)
    D = min(delay, frames)
    shown = frames - D
    advanced = min(shown, R - n0) if active and eflags & STOP else shown
    gliding = active and eflags & GLIDE
    env_glide = (int(env["glide_frames"]), int(env["glide_slope"]), int(env["step_to"])) if gliding else None
    g0 = int(env["glide_done"]) if gliding else 0
    if active:
        env_after["delay"] = delay - D
        env_after["ramp_done"] = min(R, n0 + shown)
    if flags & PLAYING and advanced > 0:
        phi0 = (int(record["position"]) << SUB_BITS) | (int(env["sub"]) if active else 0)
        phi = vref.fine_positions(record, env_glide, phi0, g0, advanced)
        o, live = values(record, asset, phi >> np.uint64(SUB_BITS), channels, coef)
        if active:
            with np.errstate(invalid="ignore", over="ignore"):
                o = o * vref.factors(env, n0 + np.arange(advanced, dtype=np.int64), channels)
        out[D:D + advanced] = np.where(live[:, None], o, f32(0.0))
        end = vref.wrap_fine(phi0 + vref.advance(step, env_glide, g0, advanced), record)
        if not flags & LOOP and end >= int(record["frames"]) << FINE_BITS:
            end = int(record["frames"]) << FINE_BITS
            flags &= ~PLAYING
        after["position"] = end >> SUB_BITS
        if active:
            env_after["sub"] = end & (SUB_ONE - 1)
    if gliding:
        env_after["glide_done"] = min(env_glide[0], g0 + advanced)
        if env_after["glide_done"] == env_glide[0]:
            after["step"] = env_glide[2]
    if active and eflags & STOP and env_after["ramp_done"] == R:
        flags &= ~PLAYING
    after["flags"] = flags
    return out, after, env_after


def render(records, envelopes, resamplers, tables, assets, frames, channels):
    """records: array of sampler_ref.DTYPE; envelopes: array of voice_ref.DTYPE; resamplers[r]: a table index or NONE; tables: {index:
    coef [P][T]}; assets[r]: the asset record r names.  Returns (out [n][frames][channels], the records afterwards, the envelopes
    afterwards); the resamplers are nobody's to change."""
    out = np.zeros((len(records), frames, channels), dtype=f32)
    after, env_after = records.copy(), envelopes.copy()
    for r in range(len(records)):
        coef = tables[int(resamplers[r])] if int(resamplers[r]) != NONE else None
        out[r], after[r], env_after[r] = render_one(records[r], envelopes[r], coef, assets[r], frames, channels)
    return out, after, env_after
