"""The voices the voice filters' contract names (include/oalsfx_hip.h, "voice filters"; the kernel: oalsfxpp_amd/csrc/hip/biquad.hip): filters
for polyphony_cases.named_voices, seeded random filters, and the model of a set call.  Everything is data for biquad_ref: arrays
[lanes][instances], lane-major as the batch keeps them.  The coefficients are computed here, in numpy, and not by the library under test."""
import numpy as np

import biquad_ref as bref
import polyphony_cases as pcases

f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)


def low_pass(freq_mult, rcp_q=1.0):
    """The cookbook low-pass in double, rounded once: (b0, b1, b2, a1, a2) / a0."""
    w0 = 2 * np.pi * freq_mult
    alpha = np.sin(w0) / 2 * rcp_q
    b = np.array([(1 - np.cos(w0)) / 2, 1 - np.cos(w0), (1 - np.cos(w0)) / 2, -2 * np.cos(w0), 1 - alpha]) / (1 + alpha)
    return tuple(b.astype(f32))


def band_pass(freq_mult, rcp_q=0.5):
    w0 = 2 * np.pi * freq_mult
    alpha = np.sin(w0) / 2 * rcp_q
    return tuple((np.array([alpha, 0.0, -alpha, -2 * np.cos(w0), 1 - alpha]) / (1 + alpha)).astype(f32))


def filt(coef=IDENTITY, flags=bref.ACTIVE, x=None, y=None):
    """One record of biquad_ref.DTYPE, as an array of one."""
    r = np.zeros(1, bref.DTYPE)
    r["flags"] = flags
    for name, value in zip(bref.COEFFICIENTS, coef):
        r[name] = value
    if x is not None:
        r["x"] = x
    if y is not None:
        r["y"] = y
    return r


def set_model(state, records, lane, instances):
    """What oalsfx_batch_set_lane_filters does to the filters the next render finds, state [lanes][n], changed in place: flags (without
    LOAD) and coefficients always, the histories with LOAD alone."""
    for i, r in zip(instances, records):
        names = bref.DTYPE.names if r["flags"] & bref.LOAD else ("flags",) + bref.COEFFICIENTS
        for name in names:
            state[name][lane, i] = r[name]
        state["flags"][lane, i] &= ~np.uint32(bref.LOAD)


def random_filters(rng, lanes, n, share=0.6, histories=True):
    """Stable low- and band-passes with random corner frequencies; `share` of them ACTIVE; random histories in all eight channels."""
    out = np.zeros((lanes, n), bref.DTYPE)
    for k in range(lanes):
        for i in range(n):
            coef = low_pass(rng.uniform(0.002, 0.45), rng.uniform(0.3, 1.8)) if rng.random() < 0.7 else band_pass(rng.uniform(0.01, 0.4), rng.uniform(0.2, 1.5))
            out[k][i] = filt(coef, bref.ACTIVE if rng.random() < share else 0)[0]
            if histories:
                out[k][i]["x"] = rng.uniform(-1, 1, (8, 2)).astype(f32)
                out[k][i]["y"] = rng.uniform(-1, 1, (8, 2)).astype(f32)
    return out


RINGING = "an active filter on an idle voice rings out of loaded histories"


def named_filters(names, seed=5):
    """Filters [LANES][INSTANCES] for polyphony_cases.named_voices(...)[0]: delays of 1, 63, 64, 65 and 130 frames under a filter, a STOP
    in mid-tile and a one-shot that ends in mid-call and ring on, a filtered voice in the last lane alone, filtered and unfiltered lanes
    mixed in one instance, 4- and 8-tap tables, and, in the instance whose voices are all idle, a filter that rings out of silence."""
    rng = np.random.default_rng(seed)
    where = {names[k][i]: (k, i) for k in range(pcases.LANES) for i in range(pcases.INSTANCES)}
    out = np.zeros((pcases.LANES, pcases.INSTANCES), bref.DTYPE)
    filtered = ("delay 1, T = 4", "delay 63, T = 8", "delay 64, no table", "delay 65, T = 4", "delay 130, T = 8", "a STOP ramp that ends in mid-call",
                "a one-shot that ends in mid-call", "a lone voice in the last lane", "delay 70 and a STOP of 200", "nearest samples, no table", "plain u8", "plain fp32",
                "T = 8, delay 128", "T = 8, delay 449", "an envelope on a voice that does not play")
    for name in filtered:
        out[where[name]] = filt(low_pass(rng.uniform(0.01, 0.3), rng.uniform(0.4, 1.5)))[0]
    # the idle instance 5, lane 1: histories as a sounding voice would have left them
    out[1][5] = filt(low_pass(0.02, 0.2), x=rng.uniform(-0.5, 0.5, (8, 2)).astype(f32), y=rng.uniform(-0.5, 0.5, (8, 2)).astype(f32))[0]
    # an inactive record whose coefficients and histories must not be looked at or touched
    out[2][6] = filt(band_pass(0.1), flags=0, x=np.full((8, 2), 3.0, f32), y=np.full((8, 2), -2.0, f32))[0]
    return out
