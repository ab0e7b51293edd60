"""The voices of the filter programs' tests (include/oalsfx_hip.h, "filter programs"; the kernels: oalsfxpp_amd/csrc/hip/filter_program.hip),
the same for the host build of the kernels (tests/test_filter_program_host.py), for the device (tests/test_gpu_filter_programs.py) and for
the proof that the comparison tells wrong kernels apart (tests/test_filter_program_ref.py).  Built on sweep_cases: its shapes, sizes and
voices, with the swept voices' single sweeps replaced by programs.  The coefficients are computed here, in numpy, and not by the library
under test."""
import numpy as np

import biquad_ref as bref
import filter_program_ref as fref
import sweep_cases as wcases
import sweep_ref as wref

f32 = np.float32
SIZES = wcases.SIZES                         # (1, 63, 64, 65, 300): the render sizes, each on a batch of its own
SPLIT = wcases.SPLIT                         # (1, 63, 64, 65, 107): ... and the 300 frames once more in five renders
SHAPES = wcases.SHAPES                       # channels: (instances, lanes)
LONG = 8       # a programmed voice with a switch inside the 300 frames and this many ramp frames behind it differs under every wrong form
# The programs, taken in turn: ((frames, done) per segment).  Against renders of 300 frames and their split at 1, 64, 128 and 193: three
# segments of one frame; a switch on a tile boundary that is also a render's last frame in the split; 63 + 1 + 64; switches in mid-tile
# and a last segment that does not finish; seven switches, several inside one tile; a first segment that completes on the 300th frame and
# is replaced in that render (the record afterwards has done == 0); a program that completes on the 300th frame; a first segment that
# starts mid-way; nothing switches inside the 300.
PROGRAMS = (
    ((1, 0), (1, 0), (1, 0)),
    ((64, 0), (64, 0)),
    ((63, 0), (1, 0), (64, 0)),
    ((100, 0), (37, 0), (500, 0)),
    ((10, 0),) * 8,
    ((300, 0), (50, 0)),
    ((128, 0), (172, 0)),
    ((100, 37), (20, 0), (400, 0)),
    ((1000, 0), (10, 0)),
)


def make_program(rng, first_from, shape, continuous):
    """A program of the given shape that starts on the coefficients first_from.  continuous: every segment starts on the bytes the one
    before ends on (oalsfx_host_filter_program's arithmetic, restated: filter_program_ref.chain); else every segment has two designs of
    its own."""
    if continuous:
        nodes = [np.asarray(first_from, f32)] + [np.asarray(wcases.design(rng), f32) for _ in shape]
        program = fref.chain(nodes, [length for length, _ in shape])
    else:
        program = [wref.make(first_from if j == 0 else wcases.design(rng), wcases.design(rng), length)[0] for j, (length, _) in enumerate(shape)]
    for s, (_, done) in zip(program, shape):
        s["done"] = done
    return program


def build(channels, seed=1300, program=False, n=None):
    """sweep_cases.build's case with filter programs: the swept voices -- every lane-0 voice and every fourth voice of the other lanes --
    get the programs of PROGRAMS in turn (starting at another for every channel count), alternately continuous and not; of the voices
    that sweep_cases leaves filtered without a sweep every second gets one plain sweep.  case.filter_programs [lanes][n]: lists of sweep
    records, the current one first (one record for a voice without a program); case.programmed: the (lane, instance) with a program of
    two segments or more; case.shape: {(lane, instance): its PROGRAMS entry}."""
    case = wcases.build(channels, seed=seed, program=program, n=n)
    rng = np.random.default_rng(seed + 50 + channels)
    case.filter_programs = [[[case.sweeps[k][i].copy()] for i in range(case.n)] for k in range(case.lanes)]
    case.programmed, case.shape = [], {}
    turn = channels
    for k, i in case.swept:
        shape = PROGRAMS[turn % len(PROGRAMS)]
        continuous = turn % 2 == 0
        turn += 1
        case.filter_programs[k][i] = make_program(rng, bref.coefficients(case.filters[k][i]), shape, continuous)
        case.sweeps[k][i] = case.filter_programs[k][i][0]
        case.programmed.append((k, i))
        case.shape[(k, i)] = shape
        case.what[(k, i)] = f"programmed, {'continuous' if continuous else 'discontinuous'}, (frames, done) = {shape}"
    plain = [v for v in sorted(case.what) if case.what[v] == "filtered, no sweep"]
    for k, i in plain[::2]:
        case.sweeps[k][i] = wref.make(bref.coefficients(case.filters[k][i]), wcases.design(rng), 150)[0]
        case.filter_programs[k][i] = [case.sweeps[k][i].copy()]
        case.what[(k, i)] = "one plain sweep, R = 150"
    case.swept = []
    return case


def lengths_and_segments(case, lane):
    """(int32 [n], SWEEP_DTYPE [n][8]) of one lane's programs, as oalsfx_batch_set_lane_filter_programs takes them."""
    lengths = np.asarray([len(p) for p in case.filter_programs[lane]], np.int32)
    segments = np.zeros((case.n, fref.MAX), wref.DTYPE)
    for i, p in enumerate(case.filter_programs[lane]):
        segments[i, :len(p)] = p
    return lengths, segments


def switches_inside(shape, frames=300):
    """The frames of the render (below `frames`) on which a later segment of the program starts."""
    at, out = 0, []
    for length, done in shape[:-1]:
        at += length - done
        if at < frames:
            out.append(at)
    return out


def programmed_voice_outputs(case, sizes, how):
    """{(lane, instance): the programmed voice's own filtered frames over the renders `sizes`, side by side} under one way to switch."""
    import program_ref as gref
    out = {}
    for k, i in case.programmed:
        record, program, f, fp, parts = case.records[k][i], case.programs[k][i], case.filters[k][i], case.filter_programs[k][i], []
        for frames in sizes:
            x, record, program = gref.render_voice(record, program, None, case.pcm[k][i], frames, case.channels)
            if how == "stated":
                y, f, fp = fref.filter_one(f, fp, x, case.channels)
            else:
                y, _, _ = fref.filter_one(f, fp, x, case.channels, how)
                _, f, fp = fref.filter_one(f, fp, x, case.channels)     # (the wrong form's outputs of this call, from the stated state)
            parts.append(y)
        out[(k, i)] = np.concatenate(parts)
    return out
