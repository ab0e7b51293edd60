"""GPU: the filter programs (oalsfx_batch_set_filter_programs and its lane form, and the renders while a queue may hold a segment;
include/oalsfx_hip.h, "filter programs") against their restatement (tests/filter_program_ref.py).  Every comparison is on the bit
patterns (NaNs by position) and on the records' bytes: outputs, the samplers, the envelopes or envelope programs, the filters, the
current sweeps and the queues of every voice, read back after every call; there is no tolerance anywhere.
tests/test_filter_program_ref.py shows on these very voices that a switch a frame late, an index not reset and a segment chosen per tile
would each fail the comparison.  No test provokes a device fault: every refusal is decided on the host."""
import os
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import filter_program_cases as fcases
import filter_program_ref as fref
import sampler_ref as sref
import sweep_cases as wcases
import sweep_ref as wref
from harness import ROOT, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch, BatchError, filter_program, filter_sweep_log
from test_gpu_biquad import expect_filters, set_filters
from test_gpu_programs import expect_programs
from test_gpu_resample import FORMAT
from test_gpu_sampler import device_render, expect_output
from test_gpu_sweeps import placed
from test_sampler_abi import rec

pytestmark = pytest.mark.gpu
f32 = np.float32
MINUS_ZERO = 0x80000000
NEW, NEW_ENV = "k_filter_program_rows", "k_filter_program_env_rows"


class Horizons:
    """What the batch knows without reading back: the frames until every filter program stands in its last segment, one
    more; the frames until no sweep is under way.  kernel(): what the next render of a batch with an ACTIVE filter and no envelope
    program launches; rendered(frames): a render has run."""

    def __init__(self):
        self.queues, self.sweeps = 0, 0

    def set(self, program):
        left = [int(s["frames"]) - int(s["done"]) for s in program if int(s["flags"]) & wref.ACTIVE]
        if len(program) >= 2:
            self.queues = max(self.queues, 1 + sum(left[:-1]))
        self.sweeps = max(self.sweeps, sum(left))

    def kernel(self):
        return NEW if self.queues > 0 else "k_sweep_rows" if self.sweeps > 0 else "k_biquad_rows"

    def rendered(self, frames):
        if self.queues > 0 or self.sweeps > 0:
            self.sweeps = max(0, self.sweeps - frames)
        self.queues = max(0, self.queues - frames)


def set_filter_programs(b, case, horizons=None):
    for k in range(case.lanes):
        b.set_filter_programs(case.filter_programs[k], lane=k)
        for p in case.filter_programs[k]:
            if horizons:
                horizons.set(p)


def expect_filter_programs(b, want, label):
    bad = []
    for k in range(len(want)):
        got, current = b.get_filter_programs(lane=k), b.get_sweeps(lane=k)
        for i, p in enumerate(want[k]):
            if got[i].tobytes() != np.asarray(p, wref.DTYPE).tobytes() or current[i].tobytes() != p[0].tobytes():
                bad.append((k, i))
    assert not bad, f"{label}: the filter programs of (lane, instance) {bad[:6]} differ: got {b.get_filter_programs(instances=[bad[0][1]], lane=bad[0][0])}, want {want[bad[0][0]][bad[0][1]]}"


def set_up(b, case, records, programs=True, horizons=None):
    b.set_polyphony(case.lanes)
    programmed = any(len(p) > 1 for lane in case.programs for p in lane)
    for k in range(case.lanes):
        b.set_samplers(records[k], lane=k)
        if programmed:
            b.set_env_programs(case.programs[k], lane=k)
        else:
            b.set_envelopes(wcases.first_segments(case)[k], lane=k)
    set_filters(b, case.filters)
    if programs:
        set_filter_programs(b, case, horizons)
    return programmed


def run_calls(b, case, records, sizes, label, horizons=None, kernels=None, state=None, **kw):
    """One render per size, each against the restatement, with everything read back after every call.  The kernel's name: the one
    `horizons` foretells, or one of `kernels`.  state: (records, envelope programs, filters, filter programs) to go on from.  Returns
    (the outputs side by side, the state afterwards)."""
    r, p, f, fp = state or (records, case.programs, case.filters, case.filter_programs)
    outs = []
    for frames in sizes:
        want, r, p, f, fp = fref.render(r, p, case.resamplers, f, fp, {}, case.pcm, frames, case.channels)
        expected = (horizons.kernel(),) if horizons else kernels
        got = device_render(b, frames, **kw)
        if horizons:
            horizons.rendered(frames)
        assert b.last_render_kernel() in expected, f"{label}, {frames} frames: {b.last_render_kernel()}, not {expected}"
        expect_output(got, want, f"{label}, {frames} frames")
        expect_programs(b, r, p, f"{label}, after {frames} frames")
        expect_filters(b, f, f"{label}, after {frames} frames")
        expect_filter_programs(b, fp, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), (r, p, f, fp)


def same_programs(a, b):
    return all(np.asarray(x, wref.DTYPE).tobytes() == np.asarray(y, wref.DTYPE).tobytes() for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.parametrize("channels", sorted(fcases.SHAPES))
def test_every_render_size_and_the_split(channels):
    """5 to 9 instances of 1 to 3 lanes: renders of 1, 63, 64, 65 and 300 frames, each on a batch of its own, and the 300 frames once more
    as 1 + 63 + 64 + 65 + 107, then 800 frames more in which every program but the longest runs out: k_filter_program_rows while the
    batch's bound on the queues is positive, k_sweep_rows behind it, k_biquad_rows behind that.  Beside the programmed voices in the
    same launch: a plain sweep, filtered voices without a sweep, unfiltered voices under an envelope, idle voices."""
    case = fcases.build(channels)
    assets, records = placed(case)
    whole = None
    for frames in fcases.SIZES:
        with Batch(case.n, FORMAT[channels], 48000, 1) as b:
            h = Horizons()
            set_up(b, case, records, horizons=h)
            expect_filter_programs(b, case.filter_programs, "as set")
            whole, after = run_calls(b, case, records, (frames,), f"{channels} channels", h, offset=frames % 3)
            assert b.last_render_kernel() == NEW
    with Batch(case.n, FORMAT[channels], 48000, 1) as b:
        h = Horizons()
        set_up(b, case, records, horizons=h)
        parts, split = run_calls(b, case, records, fcases.SPLIT, f"{channels} channels, split", h, offset=channels % 3)
        assert same_bits(whole, parts)[0] and after[2].tobytes() == split[2].tobytes() and same_programs(after[3], split[3])
        _, late = run_calls(b, case, records, (400, 301, 64, 64), f"{channels} channels, behind the 300", h, state=split)
        assert b.last_render_kernel() == "k_biquad_rows" and all(len(late[3][k][i]) == 1 for k, i in case.programmed)
    assert np.abs(whole).max() > 0 and np.isfinite(whole).all()
    kinds = set(case.what.values())
    assert "one plain sweep, R = 150" in kinds and "idle" in kinds and (case.lanes == 1 or "unfiltered, under an envelope" in kinds)


@pytest.mark.parametrize("channels", [2, 7])
def test_programmed_filters_under_envelope_programs(channels):
    """The programmed voices' envelopes are programs of three segments that switch at frames 40 and 75, inside the renders:
    k_filter_program_env_rows, in one render of 300 frames and in the split."""
    case = fcases.build(channels, program=True)
    assets, records = placed(case)
    with Batch(case.n, FORMAT[channels], 48000, 1) as b, Batch(case.n, FORMAT[channels], 48000, 1) as twin:
        assert set_up(b, case, records) and set_up(twin, case, records)
        whole, after = run_calls(b, case, records, (300,), "envelope programs", kernels=(NEW_ENV,))
        parts, split = run_calls(twin, case, records, fcases.SPLIT[:2], "envelope programs, split", kernels=(NEW_ENV,), offset=1)
        rest, split = run_calls(twin, case, records, fcases.SPLIT[2:], "envelope programs, split", kernels=(NEW_ENV, NEW), state=split, offset=1)
    assert same_bits(whole, np.concatenate([parts, rest], axis=1))[0] and after[2].tobytes() == split[2].tobytes() and same_programs(after[3], split[3])
    assert all(len(after[1][k][i]) == 1 for k, i in case.programmed), "every programmed voice's envelope queue has run out"


def shortened(case):
    """The case with no program that outlasts 300 frames: the segments that would are cut to what is left of the 300."""
    for k, i in case.programmed:
        p, at = case.filter_programs[k][i], 0
        for j, s in enumerate(p):
            left = int(s["frames"]) - int(s["done"])
            room = max(1, 300 - at - (len(p) - 1 - j))
            if left > room:
                p[j] = wref.make(s["from"], s["to"], room)[0]
                left = room
            at += left
        case.sweeps[k][i] = p[0]
    return case


def test_after_completion_the_batch_is_a_plain_filtered_one():
    case = shortened(fcases.build(2))
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        h = Horizons()
        set_up(b, case, records, horizons=h)
        _, state = run_calls(b, case, records, (300, 2), "until every program is done", h)
        filters = np.stack([b.get_filters(lane=k) for k in range(case.lanes)])
        for k, i in case.programmed:
            (last,) = b.get_filter_programs(instances=[i], lane=k)[0:1]
            assert len(last) == 1 and not last[0]["flags"] & wref.ACTIVE and last[0]["done"] == last[0]["frames"], case.what[(k, i)]
            assert bref.coefficients(filters[k][i]).tobytes() == case.filter_programs[k][i][-1]["to"].tobytes(), "get_filters shows the last `to`"
        uploads = b.filter_program_uploads(), b.sweep_uploads()
        run_calls(b, case, records, (64, 65), "behind the programs", kernels=("k_biquad_rows",), state=state)
        assert (b.filter_program_uploads(), b.sweep_uploads()) == uploads


def test_upload_counters():
    case = fcases.build(2)
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        set_up(b, case, records, programs=False)
        assert b.filter_program_uploads() == 0
        none = [[[np.zeros(1, wref.DTYPE)[0]] for _ in range(case.n)] for _ in range(case.lanes)]
        _, state = run_calls(b, case, records, (10,), "before any program", kernels=("k_biquad_rows",), state=(records, case.programs, case.filters, none))
        assert b.filter_program_uploads() == 0 and b.sweep_uploads() == 0
        others = lambda: (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads(), b.filter_uploads(), b.program_uploads())
        before = others()
        # (the programs as built start on the coefficients the filters were set with, which the ten frames have not changed)
        set_filter_programs(b, case)
        assert b.filter_program_uploads() == 0 and b.sweep_uploads() == 0, "a set call uploads nothing by itself"
        _, state = run_calls(b, case, records, (20,), "the first render with programs", kernels=(NEW,), state=state[:3] + (case.filter_programs,))
        assert b.filter_program_uploads() == 1 and b.sweep_uploads() == 1 and others() == before, "all lanes' rows in one launch, and no other table's"
        _, state = run_calls(b, case, records, (20,), "the second", kernels=(NEW,), state=state)
        assert b.filter_program_uploads() == 1 and b.sweep_uploads() == 1 and others() == before


def test_a_plain_set_empties_the_queue():
    """A plain sweep set and a plain filter set each empty the voice's queue, and the emptied row goes to the device once."""
    case = fcases.build(6)
    assets, records = placed(case)
    (k, i), (k2, i2) = [v for v in case.programmed if case.shape[v] in (fcases.PROGRAMS[3], fcases.PROGRAMS[8])][:2]
    with Batch(case.n, FORMAT[6], 48000, 1) as b:
        set_up(b, case, records)
        _, (r, p, f, fp) = run_calls(b, case, records, (70,), "in mid-program", kernels=(NEW,))
        assert len(fp[k][i]) >= 2 and len(fp[k2][i2]) >= 2
        # a filter set
        row = bcases.filt(bcases.band_pass(0.07))
        b.set_filters(row, instances=[i], lane=k)
        f = f.copy()
        bcases.set_model(f, row, k, [i])
        fp[k][i] = [np.zeros(1, wref.DTYPE)[0]]
        # a sweep set
        sweep = wref.make(bref.coefficients(f[k2][i2]), bcases.low_pass(0.11), 90)
        b.set_sweeps(sweep, instances=[i2], lane=k2)
        fp[k2][i2] = [sweep[0]]
        expect_filter_programs(b, fp, "after the two sets")
        uploads = b.filter_program_uploads()
        _, state = run_calls(b, case, records, (70, 64), "behind the two sets", kernels=(NEW, "k_sweep_rows"), state=(r, p, f, fp))
        assert b.filter_program_uploads() == uploads + 1, "the emptied rows went to the device, in one launch"
        b.set_filters(row, instances=[i], lane=k)
        run_calls(b, case, records, (5,), "a filter set again", kernels=(NEW, "k_sweep_rows"), state=state)
        assert b.filter_program_uploads() == uploads + 1, "an empty queue is not uploaded again"


@pytest.mark.parametrize("channels", [1, 8])
def test_without_programs_the_batch_does_what_it_did(channels):
    """The same voices with their first segments alone, set through set_sweeps on one batch and as programs of one through
    set_filter_programs on its twin: the parent's kernels on both, the same bytes, no queue table."""
    case = fcases.build(channels)
    for k, i in case.programmed:
        case.filter_programs[k][i] = case.filter_programs[k][i][:1]
    assets, records = placed(case)
    with Batch(case.n, FORMAT[channels], 48000, 1) as b, Batch(case.n, FORMAT[channels], 48000, 1) as twin:
        set_up(b, case, records, programs=False)
        for k in range(case.lanes):
            b.set_sweeps(case.sweeps[k], lane=k)
        h = Horizons()
        set_up(twin, case, records, horizons=h)
        a, _ = run_calls(b, case, records, fcases.SPLIT, "set_sweeps", kernels=("k_sweep_rows",))
        c, _ = run_calls(twin, case, records, fcases.SPLIT, "programs of one", h)
        assert a.tobytes() == c.tobytes() and b.filter_program_uploads() == 0 and twin.filter_program_uploads() == 0


def test_one_lane_keeps_a_negative_zero():
    """K == 1: a programmed voice whose input and histories are -0.0f is stored as it is, -0.0f in its first frame and across a switch."""
    case = fcases.build(1)
    silence = np.zeros((8, 1), f32)
    case.pool = case.pool + [(sref.PCM_F32, 1, silence)]
    i = case.programmed[3][1]
    case.records[0][i] = rec(data=0, format=sref.PCM_F32, channels=1, frames=8, loop_start=0, loop_end=8, flags=sref.PLAYING | sref.LOOP, gain=0.0)[0]
    case.records[0][i]["gain"][0] = -1.0
    case.pcm[0][i], case.keys[0][i] = silence, 2
    low, mid, high = bcases.low_pass(0.01), bcases.low_pass(0.05), bcases.low_pass(0.2)
    case.filters[0][i] = bcases.filt(low, x=np.full((8, 2), -0.0, f32), y=np.stack([np.full(8, -0.0, f32), np.zeros(8, f32)], axis=-1))[0]
    case.filter_programs[0][i] = fref.chain([low, mid, high], [20, 100])
    case.sweeps[0][i] = case.filter_programs[0][i][0]
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_MONO, 48000, 1) as b:
        set_up(b, case, records)
        out, _ = run_calls(b, case, records, (65,), "one lane", kernels=(NEW,))
    assert out[i, 0, 0].view(np.uint32) == MINUS_ZERO, hex(int(out[i, 0, 0].view(np.uint32)))


def test_refusals():
    case = fcases.build(2)
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        set_up(b, case, records)
        good = wref.make((1, 0, 0, 0, 0), (0.5, 0.1, 0, -0.2, 0.1), 100)
        two = np.concatenate([good, good])
        for fields, why in ((dict(flags=5), "flags"), (dict(reserved=9), "reserved"), (dict(frames=0), "frames"), (dict(frames=(1 << 24) + 1), "frames"),
                            (dict(step=np.inf), "finite")):
            bad = two.copy()
            for name, v in fields.items():
                bad[name][1] = v
            with pytest.raises(BatchError, match=wref.MESSAGES[why].replace(".", r"\.")):
                b.set_filter_programs([bad], instances=[0])
        idle, started = two.copy(), two.copy()
        idle["flags"][1], started["done"][1] = 0, 3
        with pytest.raises(BatchError, match=r"A filter program's segment is not active\."):
            b.set_filter_programs([idle], instances=[0])
        with pytest.raises(BatchError, match=r"A queued filter sweep has already started\."):
            b.set_filter_programs([started], instances=[0])
        with pytest.raises(BatchError, match=r"Filter program length out of range\."):
            b.set_filter_programs([np.concatenate([good] * 9)], instances=[0])
        k, i = next(v for v, what in case.what.items() if what == "idle")
        with pytest.raises(BatchError, match="filter is not active"):
            b.set_filter_programs([two], instances=[i], lane=k)
        with pytest.raises(BatchError, match="Lane out of range"):
            b.set_filter_programs([two], instances=[0], lane=case.lanes)
        with pytest.raises(BatchError, match="listed twice as a filter program target"):
            b.set_filter_programs([two, two], instances=[0, 0])
        with pytest.raises(BatchError):
            b.set_filter_programs([two], instances=[case.n])
        expect_filter_programs(b, case.filter_programs, "nothing was changed")
        assert b.filter_program_uploads() == 0
        # programs built by the library's helpers
        nodes = np.concatenate([b.get_filters(instances=[0]), bcases.filt(bcases.low_pass(0.3)), bcases.filt(bcases.low_pass(0.1))])
        built = filter_program(nodes, [480, 20])
        assert built.tobytes() == np.asarray(fref.chain([bref.coefficients(n) for n in nodes], [480, 20]), wref.DTYPE).tobytes()
        b.set_filter_programs([built], instances=[0])
        assert b.get_filter_programs(instances=[0])[0].tobytes() == built.tobytes()
        log, freq = filter_sweep_log(desc.VF_LOW_PASS, 1.0, 0.01, 0.16, 1.0, 1000, 4)
        b.set_filter_programs([log], instances=[0])
        assert b.get_filter_programs(instances=[0])[0].tobytes() == log.tobytes() and len(freq) == 5


def test_polyphony_carries_the_queues():
    case = fcases.build(6)
    assets, records = placed(case)
    with Batch(case.n, FORMAT[6], 48000, 1) as b:
        h = Horizons()
        set_up(b, case, records, horizons=h)
        _, (r, p, f, fp) = run_calls(b, case, records, (30,), "two lanes", h)
        b.set_polyphony(3)
        expect_filter_programs(b, fp + [[[np.zeros(1, wref.DTYPE)[0]] for _ in range(case.n)]], "three lanes")
        with pytest.raises(BatchError, match="still in use"):
            b.set_polyphony(1)
        b.set_polyphony(2)
        run_calls(b, case, records, (70, 300), "two lanes again", h, state=(r, p, f, fp))


def test_api_array_filter_programs(tmp_path):
    """tests/cpp/api_array_filter_programs.cpp: ApiArray::program_voice_filter and get_voice_filter_program against the batch calls."""
    exe = str(tmp_path / "api_array_filter_programs")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_filter_programs.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
