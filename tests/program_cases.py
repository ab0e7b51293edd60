"""The voices the envelope programs' contract names one by one (include/oalsfx_hip.h, "envelope programs"), and seeded random programs,
for the host build of the kernels (tests/test_program_host.py) and for the device (tests/test_gpu_programs.py).  Built on
polyphony_cases.named_voices: the same records, resamplers and assets, with programs in place of some of the envelopes.  A program is a
list of envelope records, the current segment first; a voice without one has a list of one."""
import numpy as np

import polyphony_cases as pcases
import voice_ref as vref
from test_voice_abi import env

f32 = np.float32
CALLS = pcases.CALLS                     # 1, 63, 64, 65, 256, 7: the calls end at 1, 64, 128, 193, 449 and 456
ENDS = tuple(int(v) for v in np.cumsum(CALLS))


def segment(rng, channels, ramp, delay=0, flags=vref.ACTIVE):
    e = env(flags=flags, delay=delay)
    vref.ramp(e[0], rng.uniform(-1, 1, channels).astype(f32), rng.uniform(-1, 1, channels).astype(f32), ramp)
    return e[0]


def named_programs(channels=2, seed=23):
    """(names, records, programs [lanes][n], resamplers, assets, which: {what: (lane, instance)} of the voices given a program)."""
    names, records, envelopes, resamplers, pcm = pcases.named_voices(channels)
    rng = np.random.default_rng(seed)
    s = lambda ramp, **kw: segment(rng, channels, ramp, **kw)
    programs = [[[envelopes[k][i].copy()] for i in range(pcases.INSTANCES)] for k in range(pcases.LANES)]
    given = {
        # instance 0: every lane loops
        "boundaries at 1, 63, 64, 65 and 128": (0, 0, [s(1), s(62), s(1), s(1), s(63), s(100)]),
        "three boundaries inside one tile": (1, 0, [s(70), s(10), s(10), s(200)]),
        "a boundary on a call's last frame": (2, 0, [s(ENDS[3]), s(50)]),
        "eight segments used up in one call": (3, 0, [s(5, delay=ENDS[3] + 2)] + [s(10) for _ in range(6)] + [s(40)]),
        # instance 1
        "two zero-length segments in a row": (0, 1, [s(30), s(0), s(0), s(40)]),
        "a queued delay": (1, 1, [s(40), s(20, delay=100), s(300)]),
        # instance 2
        "STOP in mid-program": (0, 2, [s(50), s(30, flags=vref.ACTIVE | vref.STOP), s(20), s(10)]),
        "a one-shot that ends inside a later segment": (1, 2, [s(20), s(600), s(5)]),
        "a loop shorter than the taps": (2, 2, [s(33), s(60, delay=5), s(500)]),
        # instance 4: a program on a voice that does not play, and one whose first segment is complete when it is set
        "a program on a voice that does not play": (3, 4, [s(10, delay=3), s(70)]),
        "complete when set": (0, 4, [s(0), s(90, delay=1), s(4)]),
    }
    which = {}
    for what, (k, i, program) in given.items():
        programs[k][i] = program
        which[what] = (k, i)
    return names, records, programs, resamplers, pcm, which


def random_programs(rng, envelopes, channels, share=0.5, longest=90):
    """envelopes [lanes][n] -> programs [lanes][n]: about `share` of the voices get a program of 2 .. 8 random segments, the others keep
    their envelope as a program of one."""
    lanes, n = envelopes.shape
    programs = [[[envelopes[k][i].copy()] for i in range(n)] for k in range(lanes)]
    for k in range(lanes):
        for i in range(n):
            if rng.random() >= share:
                continue
            program = []
            for _ in range(int(rng.integers(2, 9))):
                ramp = int(rng.choice([0, 1, int(rng.integers(2, longest))]))
                delay = int(rng.choice([0, 0, int(rng.integers(1, 40))]))
                flags = vref.ACTIVE | (vref.STOP if rng.random() < 0.1 else 0)
                program.append(segment(rng, channels, ramp, delay=delay, flags=flags))
            programs[k][i] = program
    return programs


def first_segments(programs):
    return np.array([[p[0] for p in lane] for lane in programs], dtype=vref.DTYPE)
