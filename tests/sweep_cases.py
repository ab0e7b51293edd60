"""The voices of the voice filter sweeps' tests (include/oalsfx_hip.h, "voice filter sweeps"; the kernels: oalsfxpp_amd/csrc/hip/sweep.hip),
the same for the host build of the kernels (tests/test_sweep_host.py), for the device (tests/test_gpu_sweeps.py) and for the proof that
the comparison tells wrong kernels apart (tests/test_sweep_ref.py).  Everything is data for sweep_ref: arrays [lanes][instances],
lane-major as the batch keeps them.  The coefficients are computed here, in numpy, and not by the library under test."""
import numpy as np

import biquad_cases as bcases
import biquad_ref as bref
import program_cases as gcases
import resample_ref as ref
import sampler_ref as sref
import sweep_ref as wref
import voice_ref as vref
from test_sampler_abi import rec

f32 = np.float32
ONE = sref.ONE
SIZES = (1, 63, 64, 65, 300)                 # the render sizes, each on a batch of its own
SPLIT = (1, 63, 64, 65, 107)                 # ... and the 300 frames once more in five renders
SHAPES = {1: (9, 1), 2: (5, 3), 6: (6, 2), 7: (7, 3), 8: (8, 2)}      # channels: (instances, lanes)
# (R, done) of the swept voices, taken in turn.  Against renders of 300 frames and their split at 1, 64, 128 and 193: a sweep of one frame
# and of two; one that completes on a tile boundary, which is a render's last frame in the split; one that completes in mid-tile with
# plain frames behind it; one that does not complete; three that start mid-way; one that completes on the 300th frame.
SWEEPS = ((1, 0), (2, 0), (64, 0), (100, 0), (1000, 0), (100, 37), (1000, 500), (300, 0), (128, 0), (64, 32))
ASSET_FRAMES = 97
LONG = 8       # a swept voice with this many frames of ramp left can differ under every wrong form (tests/test_sweep_ref.py)


class Case:
    """records, filters, sweeps, resamplers [lanes][n]; programs and pcm [lanes][n] lists; pool for test_gpu_sampler.Assets; swept: the
    (lane, instance) of the voices with a sweep; what: {(lane, instance): a word on the voice}."""


def design(rng):
    return bcases.low_pass(rng.uniform(0.004, 0.4), rng.uniform(0.3, 1.8)) if rng.random() < 0.7 else bcases.band_pass(rng.uniform(0.01, 0.4), rng.uniform(0.2, 1.5))


def build(channels, seed=900, program=False, n=None):
    """The case of one channel count.  Instance i, lane 0: a swept voice, sweep SWEEPS[i mod 10]; the lanes behind it in turn a filtered
    voice without a sweep, an unfiltered voice under an envelope, an idle voice, and a second swept voice.  program: the swept voices'
    envelopes are programs of three segments that switch inside the renders.  n: another instance count than SHAPES'."""
    n, lanes = (n or SHAPES[channels][0]), SHAPES[channels][1]
    rng = np.random.default_rng(seed + channels)
    case = Case()
    case.channels, case.n, case.lanes = channels, n, lanes
    asset = rng.standard_normal((ASSET_FRAMES, channels)).astype(f32)
    mono = rng.standard_normal((ASSET_FRAMES, 1)).astype(f32)
    case.pool = [(sref.PCM_F32, channels, asset), (sref.PCM_F32, 1, mono)]
    case.records = np.zeros((lanes, n), sref.DTYPE)
    case.records["channels"] = 1               # (an idle voice's record: all zero but for a channel count the batch takes)
    case.filters = np.zeros((lanes, n), bref.DTYPE)
    case.sweeps = np.zeros((lanes, n), wref.DTYPE)
    case.resamplers = np.full((lanes, n), ref.NONE, np.int32)
    case.programs = [[[np.zeros(1, vref.DTYPE)[0]] for _ in range(n)] for _ in range(lanes)]
    case.pcm = [[None] * n for _ in range(lanes)]
    case.keys = [[0] * n for _ in range(lanes)]
    case.swept, case.what = [], {}
    turn = 0

    def voice(k, i):
        key = int(rng.integers(0, 2)) if channels > 1 else 0
        width = case.pool[key][1]
        case.records[k][i] = rec(data=0, format=sref.PCM_F32, channels=width, frames=ASSET_FRAMES, loop_start=0, loop_end=ASSET_FRAMES,
                                 flags=sref.PLAYING | sref.LOOP | sref.LINEAR, position=int(rng.integers(0, ASSET_FRAMES << 12)),
                                 step=int(rng.integers(ONE // 3, 2 * ONE)), gain=0.0)[0]
        case.records[k][i]["gain"][:channels] = rng.uniform(-1, 1, channels).astype(f32)
        case.pcm[k][i], case.keys[k][i] = case.pool[key][2], key

    def filtered(k, i):
        case.filters[k][i] = bcases.filt(design(rng), x=rng.uniform(-1, 1, (8, 2)).astype(f32), y=rng.uniform(-1, 1, (8, 2)).astype(f32))[0]

    def swept(k, i):
        nonlocal turn
        length, done = SWEEPS[turn % len(SWEEPS)]
        turn += 1
        voice(k, i)
        filtered(k, i)
        case.sweeps[k][i] = wref.make(bref.coefficients(case.filters[k][i]), design(rng), length, done)[0]
        if program:
            case.programs[k][i] = [gcases.segment(rng, channels, 40), gcases.segment(rng, channels, 30, delay=5), gcases.segment(rng, channels, 500)]
        case.swept.append((k, i))
        case.what[(k, i)] = f"swept, R = {length}, done = {done}"

    for i in range(n):
        swept(0, i)
        for k in range(1, lanes):
            kind = (i + k) % 4
            if kind == 0:
                voice(k, i)
                filtered(k, i)
                case.what[(k, i)] = "filtered, no sweep"
            elif kind == 1:
                voice(k, i)
                case.programs[k][i] = [gcases.segment(rng, channels, 50)]
                case.what[(k, i)] = "unfiltered, under an envelope"
            elif kind == 2:
                case.what[(k, i)] = "idle"
            else:
                swept(k, i)
    if lanes == 1:
        # one lane: the last two instances a filtered voice without a sweep and an idle one, beside the swept
        case.sweeps[0][n - 2], case.sweeps[0][n - 1] = np.zeros(1, wref.DTYPE)[0], np.zeros(1, wref.DTYPE)[0]
        case.records[0][n - 1], case.filters[0][n - 1] = np.zeros(1, sref.DTYPE)[0], np.zeros(1, bref.DTYPE)[0]
        case.records[0][n - 1]["channels"] = 1
        case.swept = [v for v in case.swept if v[1] < n - 2]
        case.what[(0, n - 2)], case.what[(0, n - 1)] = "filtered, no sweep", "idle"
    return case


def first_segments(case):
    return gcases.first_segments(case.programs)


def swept_voice_outputs(case, sizes, how):
    """{(lane, instance): the swept voice's own filtered frames over the renders `sizes`, side by side} under one form of the ramp."""
    import program_ref as gref
    out = {}
    for k, i in case.swept:
        record, program, f, s, parts = case.records[k][i], case.programs[k][i], case.filters[k][i], case.sweeps[k][i], []
        for frames in sizes:
            x, record, program = gref.render_voice(record, program, None, case.pcm[k][i], frames, case.channels)
            y, f, s = wref.filter_one(f, s, x, case.channels, how)
            parts.append(y)
        out[(k, i)] = np.concatenate(parts)
    return out
