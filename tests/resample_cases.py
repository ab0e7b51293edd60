"""The rows the resamplers' contract names one by one (include/oalsfx_hip.h, "resamplers"), and seeded random rows, for the host build
of the kernel (tests/test_resample_host.py) and for the device (tests/test_gpu_resample.py).  Everything is data for resample_ref."""
import numpy as np

import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from test_sampler_abi import rec

f32 = np.float32
ONE = sref.ONE
CALLS = (441, 256, 1, 63)
N = 40          # frames of a named row's asset


def tables():
    """The eight tables of a batch: both tap counts at 12 phase bits, at 0, with zero coefficients, with coefficients that make denormal
    products."""
    odd4, odd8 = np.asarray([[0.125, 0.625, 0.375, -0.125]], f32), np.asarray([[-0.03, 0.11, -0.2, 0.62, 0.58, -0.15, 0.09, -0.02]], f32)
    return {0: ref.cubic(12), 1: ref.sinc(8, 12, 0.9), 2: odd4, 3: odd8, 4: ref.nearest_table(3, 4), 5: ref.nearest_table(3, 8),
            6: (ref.sinc(4, 4, 0.7) * f32(1e-9)).astype(f32), 7: (ref.sinc(8, 4, 0.7) * f32(1e-9)).astype(f32)}


FINE, COARSE, ZEROS, TINY = 0, 2, 4, 6      # the 4-tap table of each kind; the 8-tap one is the next


def asset(rng, fmt, width, frames=N):
    if fmt == sref.PCM_F32:
        return rng.standard_normal((frames, width)).astype(f32)
    info = np.iinfo(sref.PCM_DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, (frames, width)).astype(sref.PCM_DTYPE[fmt])


def named_rows(taps, fmt, width, channels, seed=5):
    """[(what, sampler record (data 0), table, PCM)] for one tap count, one PCM format and one asset width (1 or `channels`)."""
    rng = np.random.default_rng(seed + 10 * taps + fmt + 100 * width)
    H, t8 = taps // 2, taps // 8
    pcm = asset(rng, fmt, width)
    shot = dict(format=fmt, channels=width, frames=N, flags=sref.PLAYING)
    loop = lambda a, b, **kw: dict(shot, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=a, loop_end=b, **kw)
    rows = [("position 0: taps in front of frame 0", dict(shot, position=0, step=ONE // 5 + 3), FINE),
            ("the last H frames of a one-shot", dict(shot, position=((N - 1) << 12) + 100, step=3), FINE),
            ("a one-shot that ends in mid-call", dict(shot, position=(N - 12) << 12, step=ONE // 16 + 1), FINE),
            ("a one-shot that ends in the first frames, pitched up", dict(shot, position=3 << 12, step=3 * ONE + 1), FINE),
            ("a loop of 1 frame", loop(5, 6, position=5 << 12, step=ONE // 3), FINE), ("a loop of 2 frames", loop(5, 7, position=(5 << 12) + 9, step=ONE + 7), FINE),
            ("a loop of 3 frames", loop(5, 8, position=7 << 12, step=2 * ONE + 5), FINE),
            ("a loop of H + 1 frames", loop(9, 9 + H + 1, position=9 << 12, step=ONE - 1), FINE),
            ("a loop of 1 frame at the asset's end", loop(N - 1, N, position=(N - 1) << 12, step=77), FINE),
            ("a loop with loop_end == frames", loop(10, N, position=(N - 2) << 12, step=ONE // 2 + 1), FINE),
            ("a loop with a lead-in, started in front of loop_start", loop(20, 30, position=(3 << 12) + 5, step=ONE - 3), FINE),
            ("a looping voice at i == loop_start reads the lead-in", loop(20, 30, position=20 << 12, step=6), FINE),
            ("a looping voice at i == loop_start == 0 reads +0.0f", loop(0, 10, position=1, step=5), FINE),
            ("a whole-asset loop, pitched up", loop(0, N, position=(N - 1) << 12, step=5 * ONE + 123), FINE),
            ("step 0", dict(shot, position=(7 << 12) + 1234, step=0), FINE), ("step 0 in a loop", loop(6, 9, position=(8 << 12) + 4095, step=0), FINE),
            ("step 2^32 - 1 without a glide", loop(3, 37, position=4 << 12, step=2 ** 32 - 1), FINE),
            ("step 2^32 - 1 on a one-shot", dict(shot, position=0, step=2 ** 32 - 1), FINE),
            ("phase_bits 0", loop(2, 31, position=(4 << 12) + 7, step=ONE + 99), COARSE), ("phase_bits 0 on a one-shot", dict(shot, position=77, step=ONE // 7), COARSE),
            ("phase_bits 12, every phase", loop(0, N, position=0, step=ONE + 1), FINE),
            ("zero coefficients", loop(1, N - 1, position=(2 << 12) + 1, step=ONE // 2 + 3), ZEROS)]
    rows = [(what, fields, table + t8, pcm) for what, fields, table in rows]
    if fmt == sref.PCM_F32:
        special = np.tile(np.asarray([1.0, np.inf, 2.0, -0.0, np.nan, 1e-39, 3e38, -3e38, 0.5, -np.inf, 0.25, 0.75, -1.5, 3.0, 1e-45, -2.0], f32).reshape(-1, 1), (1, width))
        quiet = (rng.standard_normal((N, width)) * 1e-30).astype(f32)
        some = dict(format=fmt, channels=width, frames=16, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=16, position=10 << 12, step=ONE // 4 + 1)
        rows += [("NaN and Inf samples under a zero coefficient", some, ZEROS + t8, special), ("NaN and Inf samples under the filter", dict(some, step=ONE + 5), FINE + t8, special),
                 ("denormal products", loop(0, N, position=0, step=ONE + 17), TINY + t8, quiet), ("denormal samples", dict(some, step=ONE // 2), COARSE + t8, special)]
    records = np.concatenate([rec(**fields) for _, fields, _, _ in rows])
    records["data"] = 0
    records["gain"][:, :channels] *= np.linspace(0.75, -0.5, channels, dtype=f32)
    return [what for what, _, _, _ in rows], records, np.asarray([table for _, _, table, _ in rows]), [p for _, _, _, p in rows]


def random_rows(rng, count, channels, enveloped, calls=CALLS, **kw):
    """`count` rows: a third each at 4 taps, at 8 taps and without a table; with `enveloped` every second row under an envelope of
    voice_ref.random_pairs' kinds.  Returns (records, envelopes, resamplers, the asset of every row, its key, the pool)."""
    kw.setdefault("assets_per_format", 1)
    kw.setdefault("asset_frames", (1, 600))
    records, envelopes, pcm, keys, pool = vref.random_pairs(rng, count, channels, calls=calls, cycle=True, **kw)
    if enveloped:
        envelopes[1::2] = np.zeros(1, vref.DTYPE)
    else:
        envelopes[:] = np.zeros(1, vref.DTYPE)
    four, eight = (FINE, COARSE, ZEROS, TINY), (FINE + 1, COARSE + 1, ZEROS + 1, TINY + 1)
    # (the assets are taken in turn with the pool's period, a multiple of 3: the kind of table moves on by one with every turn of the pool)
    resamplers = np.asarray([(four[(r // 3) % 4], eight[(r // 3) % 4], ref.NONE)[(r + r // len(pool)) % 3] for r in range(count)])
    return records, envelopes, resamplers, pcm, keys, pool
