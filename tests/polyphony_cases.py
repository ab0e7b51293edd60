"""The voices the polyphony contract names one by one (include/oalsfx_hip.h, "polyphony"; the kernel: oalsfxpp_amd/csrc/hip/polyphony.hip),
and seeded random voices, for the host build of the kernel (tests/test_polyphony_host.py) and for the device
(tests/test_gpu_polyphony.py).  Everything is data for polyphony_ref: arrays [lanes][instances], lane-major as the batch keeps them."""
import numpy as np

import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from test_sampler_abi import rec
from test_voice_abi import env

f32 = np.float32
ONE = sref.ONE
CALLS = (1, 63, 64, 65, 256, 7)        # a call inside a wave, up to one, one wave, one frame more, four waves, a few frames
N = cases.N
LANES, INSTANCES = 4, 8


def by_lanes(flat, lanes, n):
    """A list of lanes * n per-voice items, lane-major, as [lane][instance]."""
    return [list(flat[k * n:(k + 1) * n]) for k in range(lanes)]


def random_voices(rng, n, lanes, channels, enveloped, calls=CALLS, **kw):
    """n * lanes voices of resample_cases.random_rows' kinds.  Returns (records [lanes][n], envelopes [lanes][n], resamplers [lanes][n],
    the asset of every voice [lanes][n], its key in the pool [lanes][n], the pool)."""
    records, envelopes, resamplers, pcm, keys, pool = cases.random_rows(rng, n * lanes, channels, enveloped, calls=calls, **kw)
    shape = (lanes, n)
    return records.reshape(shape), envelopes.reshape(shape), resamplers.reshape(shape), by_lanes(pcm, lanes, n), by_lanes(keys, lanes, n), pool


def named_voices(channels=2, seed=17):
    """LANES voices for each of INSTANCES instances: (names [lanes][n], records (data 0), envelopes, resamplers, the asset of every voice
    [lanes][n]).  The tables are resample_cases.tables()."""
    rng = np.random.default_rng(seed)
    assets = {(fmt, width): cases.asset(rng, fmt, width) for fmt in (sref.PCM_U8, sref.PCM_S16, sref.PCM_F32) for width in sorted({1, channels})}
    gains = lambda: rng.uniform(-1, 1, channels).astype(f32)

    def shot(fmt, width, **kw):
        return dict(dict(format=fmt, channels=width, frames=N, flags=sref.PLAYING | sref.LINEAR, position=(3 << 12) + 77, step=ONE // 8 + 5), **kw)

    def loop(fmt, width, a, b, **kw):
        return shot(fmt, width, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=a, loop_end=b, **dict(dict(position=a << 12), **kw))

    def delayed(D, R=50, flags=vref.ACTIVE):
        e = env(flags=flags, delay=D)
        vref.ramp(e[0], gains(), gains(), R)
        return e

    U8, S16, F32 = sref.PCM_U8, sref.PCM_S16, sref.PCM_F32
    NONE, T4, T8 = ref.NONE, cases.FINE, cases.FINE + 1
    W = channels
    idle = ("not playing", dict(format=S16, channels=1, frames=N, flags=0, data=0), None, NONE)
    gliding = delayed(2, R=0)
    vref.glide(gliding[0], ONE // 2, 2 * ONE, 90)
    voices = [
        # instance 0
        ("delay 0, no table", loop(S16, 1, 2, 31), delayed(0), NONE), ("delay 1, T = 4", loop(U8, W, 0, N), delayed(1), T4),
        ("delay 63, T = 8", loop(F32, 1, 4, 37), delayed(63), T8), ("delay 64, no table", loop(S16, W, 1, 20), delayed(64), NONE),
        # instance 1
        ("delay 65, T = 4", loop(F32, W, 3, 33), delayed(65), T4), ("delay 130, T = 8", loop(U8, 1, 0, N), delayed(130), T8),
        ("a delay longer than the calls", loop(S16, 1, 0, N), delayed(1000), T4), idle,
        # instance 2
        ("a STOP ramp that ends in mid-call", loop(S16, W, 5, 25), delayed(0, R=100, flags=vref.ACTIVE | vref.STOP), T8),
        ("a one-shot that ends in mid-call", shot(U8, 1, position=0, step=ONE // 4), None, T4),
        ("a loop shorter than the taps", loop(F32, W, 5, 6, step=ONE // 3), None, T8), ("a one-shot without a table that ends", shot(S16, 1, position=5 << 12, step=ONE // 2 + 1), None, NONE),
        # instance 3: only the last lane plays
        idle, idle, idle, ("a lone voice in the last lane", loop(U8, W, 0, N, step=ONE + 9), None, NONE),
        # instance 4: a delay with a STOP behind it, a glide, nearest samples
        ("delay 70 and a STOP of 200", loop(F32, 1, 0, N), delayed(70, R=200, flags=vref.ACTIVE | vref.STOP), NONE),
        ("a glide behind a delay of 2", loop(S16, 1, 0, N, step=ONE // 2), gliding, T4),
        ("nearest samples, no table", shot(U8, W, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=N, step=3 * ONE + 1), None, NONE),
        ("an envelope on a voice that does not play", dict(format=S16, channels=1, frames=N, flags=0, data=0), delayed(10, R=80), NONE),
        # instance 5: nothing plays
        idle, idle, idle, idle,
        # instance 6: every lane without a table, no envelope
        ("plain u8", loop(U8, 1, 0, N, step=ONE - 1), None, NONE), ("plain s16", loop(S16, W, 7, 9, step=ONE // 5), None, NONE),
        ("plain fp32", loop(F32, W, 0, N, step=2 * ONE), None, NONE), ("plain one-shot", shot(F32, 1, position=0, step=ONE // 16), None, NONE),
        # instance 7: every lane at 8 taps under an envelope
        ("T = 8, delay 128", loop(S16, 1, 0, N), delayed(128, R=300), T8), ("T = 8, delay 191", loop(U8, W, 2, 30), delayed(191), T8),
        ("T = 8, delay 192", loop(F32, 1, 0, 3), delayed(192, R=1), T8), ("T = 8, delay 449", loop(S16, W, 0, N), delayed(449), T8)]
    assert len(voices) == LANES * INSTANCES
    shape = (LANES, INSTANCES)
    names = [[None] * INSTANCES for _ in range(LANES)]
    pcm = [[None] * INSTANCES for _ in range(LANES)]
    records, envelopes, resamplers = np.zeros(shape, sref.DTYPE), np.zeros(shape, vref.DTYPE), np.full(shape, ref.NONE)
    for at, (what, fields, e, table) in enumerate(voices):
        i, k = divmod(at, LANES)
        r = rec(**fields)
        r["data"] = 0
        r["gain"][:, :channels] *= np.linspace(0.75, -0.5, channels, dtype=f32)
        names[k][i], records[k][i], resamplers[k][i] = what, r[0], table
        if e is not None:
            envelopes[k][i] = e[0]
        pcm[k][i] = assets[(int(r["format"][0]), int(r["channels"][0]))]
    return names, records, envelopes, resamplers, pcm
