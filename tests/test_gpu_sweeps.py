"""GPU: the voice filter sweeps (oalsfx_batch_set_sweeps and its lane form, and the renders while a sweep may be under way;
include/oalsfx_hip.h, "voice filter sweeps") against their restatement (tests/sweep_ref.py).  Every comparison is on the bit patterns
(NaNs by position) and on the records' bytes: outputs, the samplers, the envelopes or programs, the filters and the sweeps of every
voice, read back after every call; there is no tolerance anywhere.  tests/test_sweep_ref.py shows on these very voices that a running
sum, a fused product and coefficients held per tile would each fail the comparison.  No test provokes a device fault: every refusal is
decided on the host."""
import os
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import sampler_ref as sref
import sweep_cases as wcases
import sweep_ref as wref
import voice_ref as vref
from harness import ROOT, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch, BatchError, filter_sweep
from test_gpu_biquad import expect_filters, set_filters
from test_gpu_polyphony import place
from test_gpu_programs import expect_programs
from test_gpu_resample import FORMAT
from test_gpu_sampler import Assets, device_render, expect_output
from test_sampler_abi import rec

pytestmark = pytest.mark.gpu
f32 = np.float32
MINUS_ZERO = 0x80000000


def placed(case):
    """The case's assets on the device (alive as long as the object returned) and its records with their addresses."""
    assets = Assets(case.pool)
    records = case.records.copy()
    records["data"] = place(assets, case.keys)
    records["data"][(records["flags"] & sref.PLAYING) == 0] = 0
    return assets, records


def set_sweeps(b, sweeps):
    for k in range(sweeps.shape[0]):
        b.set_sweeps(sweeps[k], lane=k)


def get_sweeps(b):
    return np.stack([b.get_sweeps(lane=k) for k in range(b.polyphony)])


def expect_sweeps(b, want, label):
    got = get_sweeps(b)
    bad = [(k, i) for k in range(want.shape[0]) for i in range(want.shape[1]) if got[k][i].tobytes() != want[k][i].tobytes()]
    assert not bad, f"{label}: the sweeps of (lane, instance) {bad[:6]} differ: got {got[bad[0]]}, want {want[bad[0]]}"


def set_up(b, case, records, sweeps=True):
    b.set_polyphony(case.lanes)
    programmed = any(len(p) > 1 for lane in case.programs for p in lane)
    for k in range(case.lanes):
        b.set_samplers(records[k], lane=k)
        if programmed:
            b.set_env_programs(case.programs[k], lane=k)
        else:
            b.set_envelopes(wcases.first_segments(case)[k], lane=k)
    set_filters(b, case.filters)
    if sweeps:
        set_sweeps(b, case.sweeps)
    return programmed


def run_calls(b, case, records, sizes, label, kernel, state=None, **kw):
    """One render per size, each against the restatement, with everything read back after every call.  state: (records, programs,
    filters, sweeps) to go on from.  Returns (the outputs side by side, the state afterwards)."""
    r, p, f, s = state or (records, case.programs, case.filters, case.sweeps)
    outs = []
    for frames in sizes:
        # (while a queue holds a segment the render walks the queues; once none does the batch may go on doing so for a while)
        pending = any(len(q) > 1 for lane in p for q in lane)
        kernels = (kernel,) if pending or kernel != "k_sweep_program_rows" else (kernel, "k_sweep_rows")
        want, r, p, f, s = wref.render(r, p, case.resamplers, f, s, {}, case.pcm, frames, case.channels)
        got = device_render(b, frames, **kw)
        assert b.last_render_kernel() in kernels, f"{label}, {frames} frames: {b.last_render_kernel()}"
        expect_output(got, want, f"{label}, {frames} frames")
        expect_programs(b, r, p, f"{label}, after {frames} frames")
        expect_filters(b, f, f"{label}, after {frames} frames")
        expect_sweeps(b, s, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), (r, p, f, s)


@pytest.mark.parametrize("channels", sorted(wcases.SHAPES))
def test_every_render_size_and_the_split(channels):
    """5 to 9 instances of 1 to 3 lanes: renders of 1, 63, 64, 65 and 300 frames, each on a batch of its own, and the 300 frames once more
    as 1 + 63 + 64 + 65 + 107.  Sweeps of 1, 2, 64, 100, 128, 300 and 1000 frames, from their start and mid-way: they complete in
    mid-tile, on a tile boundary, on a render's last frame and inside a render with plain frames behind them, or not at all.  Beside the
    swept voices in the same launch: filtered voices without a sweep, unfiltered voices under an envelope, idle voices."""
    case = wcases.build(channels)
    assets, records = placed(case)
    whole = None
    for frames in wcases.SIZES:
        with Batch(case.n, FORMAT[channels], 48000, 1) as b:
            set_up(b, case, records)
            expect_sweeps(b, case.sweeps, "as set")
            whole, after = run_calls(b, case, records, (frames,), f"{channels} channels", "k_sweep_rows", offset=frames % 3)
    with Batch(case.n, FORMAT[channels], 48000, 1) as b:
        set_up(b, case, records)
        parts, split = run_calls(b, case, records, wcases.SPLIT, f"{channels} channels, split", "k_sweep_rows", offset=channels % 3)
    assert same_bits(whole, parts)[0] and after[2].tobytes() == split[2].tobytes() and after[3].tobytes() == split[3].tobytes()
    assert np.abs(whole).max() > 0 and np.isfinite(whole).all()
    kinds = set(case.what.values())
    assert "filtered, no sweep" in kinds and "idle" in kinds and (case.lanes == 1 or "unfiltered, under an envelope" in kinds)


@pytest.mark.parametrize("channels", [2, 7])
def test_swept_voices_under_envelope_programs(channels):
    """The swept voices' envelopes are programs of three segments that switch at frames 40 and 75, inside the renders:
    k_sweep_program_rows, in one render of 300 frames and in the split."""
    case = wcases.build(channels, program=True)
    assets, records = placed(case)
    with Batch(case.n, FORMAT[channels], 48000, 1) as b, Batch(case.n, FORMAT[channels], 48000, 1) as twin:
        assert set_up(b, case, records) and set_up(twin, case, records)
        whole, after = run_calls(b, case, records, (300,), "programs", "k_sweep_program_rows")
        parts, split = run_calls(twin, case, records, wcases.SPLIT, "programs, split", "k_sweep_program_rows", offset=1)
    assert same_bits(whole, parts)[0] and after[2].tobytes() == split[2].tobytes() and after[3].tobytes() == split[3].tobytes()
    assert all(len(after[1][k][i]) == 1 for k, i in case.swept), "every swept voice's queue has run out"


def shortened(case, longest=300):
    """The case with no sweep that outlasts `longest` frames."""
    for k, i in case.swept:
        s = case.sweeps[k][i]
        if int(s["frames"]) - int(s["done"]) > longest:
            case.sweeps[k][i] = wref.make(s["from"], s["to"], longest)[0]
    return case


def test_after_completion_the_batch_is_a_plain_filtered_one():
    case = shortened(wcases.build(2))
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        set_up(b, case, records)
        _, state = run_calls(b, case, records, (300,), "until every sweep is done", "k_sweep_rows")
        filters, sweeps = np.stack([b.get_filters(lane=k) for k in range(case.lanes)]), get_sweeps(b)
        for k, i in case.swept:
            assert bref.coefficients(filters[k][i]).tobytes() == case.sweeps[k][i]["to"].tobytes(), "get_filters shows `to`"
            assert not sweeps[k][i]["flags"] & wref.ACTIVE and sweeps[k][i]["done"] == sweeps[k][i]["frames"] == case.sweeps[k][i]["frames"]
        uploads = b.sweep_uploads()
        run_calls(b, case, records, (64, 65), "behind the sweeps", "k_biquad_rows", state=state)
        assert b.sweep_uploads() == uploads


def test_upload_counters():
    case = wcases.build(2)
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        set_up(b, case, records, sweeps=False)
        assert b.sweep_uploads() == 0
        plain = case.sweeps.copy()
        case.sweeps = np.zeros_like(plain)
        _, state = run_calls(b, case, records, (10,), "before any sweep", "k_biquad_rows")
        assert b.sweep_uploads() == 0
        others = lambda: (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads(), b.filter_uploads(), b.program_uploads())
        before = others()
        # (the sweeps as built ramp from the coefficients the filters were set with, which the ten frames have not changed)
        set_sweeps(b, plain)
        assert b.sweep_uploads() == 0, "a set call uploads nothing by itself"
        _, state = run_calls(b, case, records, (20,), "the first render with sweeps", "k_sweep_rows", state=state[:3] + (plain,))
        assert b.sweep_uploads() == 1 and others() == before, "all lanes' rows in one launch, and no other table's"
        _, state = run_calls(b, case, records, (20,), "the second", "k_sweep_rows", state=state)
        assert b.sweep_uploads() == 1 and others() == before
        # a plain filter set on a voice that never had a sweep uploads no sweep row
        k, i = next(v for v, what in case.what.items() if what == "filtered, no sweep")
        row = state[2][k][i:i + 1].copy()
        b.set_filters(row, instances=[i], lane=k)
        _, state = run_calls(b, case, records, (5,), "a filter set again", "k_sweep_rows", state=state)
        assert b.sweep_uploads() == 1 and b.filter_uploads() == before[3] + 1


def test_a_plain_filter_set_cancels_the_sweep():
    case = wcases.build(6)
    assets, records = placed(case)
    k, i = next(v for v in case.swept if case.sweeps[v]["frames"] == 1000 and case.sweeps[v]["done"] == 0)
    with Batch(case.n, FORMAT[6], 48000, 1) as b:
        set_up(b, case, records)
        _, (r, p, f, s) = run_calls(b, case, records, (70,), "in mid-sweep", "k_sweep_rows")
        assert s[k][i]["done"] == 70 and s[k][i]["flags"] & wref.ACTIVE
        row = bcases.filt(bcases.band_pass(0.07))
        b.set_filters(row, instances=[i], lane=k)
        f, s = f.copy(), s.copy()
        bcases.set_model(f, row, k, [i])
        s[k][i] = np.zeros(1, wref.DTYPE)[0]
        expect_sweeps(b, s, "after the filter set")
        uploads = b.sweep_uploads()
        run_calls(b, case, records, (70, 64), "behind the cancel", "k_sweep_rows", state=(r, p, f, s))
        assert b.sweep_uploads() == uploads + 1, "the cancelled row went to the device"
        assert b.get_sweeps(instances=[i], lane=k).tobytes() == bytes(wref.DTYPE.itemsize)


@pytest.mark.parametrize("channels", [1, 8])
def test_without_sweeps_the_batch_does_what_it_did(channels):
    """The same voices, no sweep set on one batch and all-zero sweep records set on its twin: k_biquad_rows on both, the same bytes, and
    those of the voice filters' restatement."""
    case = wcases.build(channels)
    case.sweeps = np.zeros_like(case.sweeps)
    case.swept = []
    assets, records = placed(case)
    with Batch(case.n, FORMAT[channels], 48000, 1) as b, Batch(case.n, FORMAT[channels], 48000, 1) as twin:
        set_up(b, case, records, sweeps=False)
        set_up(twin, case, records, sweeps=True)
        a, _ = run_calls(b, case, records, wcases.SPLIT, "no sweep", "k_biquad_rows")
        c, _ = run_calls(twin, case, records, wcases.SPLIT, "zero sweeps", "k_biquad_rows")
        assert a.tobytes() == c.tobytes() and b.sweep_uploads() == 0


def test_one_lane_keeps_a_negative_zero():
    """K == 1: a swept voice whose input and histories are -0.0f is stored as it is, -0.0f in its first frame."""
    case = wcases.build(1)
    silence = np.zeros((8, 1), f32)
    case.pool = case.pool + [(sref.PCM_F32, 1, silence)]
    i = case.swept[3][1]
    case.records[0][i] = rec(data=0, format=sref.PCM_F32, channels=1, frames=8, loop_start=0, loop_end=8, flags=sref.PLAYING | sref.LOOP, gain=0.0)[0]
    case.records[0][i]["gain"][0] = -1.0
    case.pcm[0][i], case.keys[0][i] = silence, 2
    low, high = bcases.low_pass(0.01), bcases.low_pass(0.2)
    case.filters[0][i] = bcases.filt(low, x=np.full((8, 2), -0.0, f32), y=np.stack([np.full(8, -0.0, f32), np.zeros(8, f32)], axis=-1))[0]
    case.sweeps[0][i] = wref.make(low, high, 100)[0]
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_MONO, 48000, 1) as b:
        set_up(b, case, records)
        out, _ = run_calls(b, case, records, (65,), "one lane", "k_sweep_rows")
    assert out[i, 0, 0].view(np.uint32) == MINUS_ZERO, hex(int(out[i, 0, 0].view(np.uint32)))


def test_refusals():
    case = wcases.build(2)
    assets, records = placed(case)
    with Batch(case.n, desc.FMT_STEREO, 48000, 1) as b:
        set_up(b, case, records)
        good = case.sweeps[0][:1].copy()
        for fields, why in ((dict(flags=5), "flags"), (dict(reserved=9), "reserved"), (dict(frames=0), "frames"), (dict(frames=(1 << 24) + 1), "frames"),
                            (dict(done=2), "done"), (dict(step=np.inf), "finite")):
            bad = good.copy()
            for name, v in fields.items():
                bad[name] = v
            with pytest.raises(BatchError, match=wref.MESSAGES[why].replace(".", r"\.")):
                b.set_sweeps(bad, instances=[0])
        k, i = next(v for v, what in case.what.items() if what == "idle")
        with pytest.raises(BatchError, match="filter is not active"):
            b.set_sweeps(good, instances=[i], lane=k)
        with pytest.raises(BatchError, match="Lane out of range"):
            b.set_sweeps(good, instances=[0], lane=case.lanes)
        with pytest.raises(BatchError, match="listed twice as a filter sweep target"):
            b.set_sweeps(np.concatenate([good, good]), instances=[0, 0])
        with pytest.raises(BatchError):
            b.set_sweeps(good, instances=[case.n])
        expect_sweeps(b, case.sweeps, "nothing was changed")
        # a sweep built by the library's helper from the filter as it stands
        built = filter_sweep(b.get_filters(instances=[0]), bcases.filt(bcases.low_pass(0.3)), 480)
        assert built.tobytes() == wref.make(bref.coefficients(case.filters[0][0]), bcases.low_pass(0.3), 480).tobytes()
        b.set_sweeps(built, instances=[0])
        assert b.get_sweeps(instances=[0]).tobytes() == built.tobytes()


def test_polyphony_carries_the_sweeps():
    case = wcases.build(6)
    assets, records = placed(case)
    with Batch(case.n, FORMAT[6], 48000, 1) as b:
        set_up(b, case, records)
        _, (r, p, f, s) = run_calls(b, case, records, (30,), "two lanes", "k_sweep_rows")
        b.set_polyphony(3)
        assert get_sweeps(b)[:2].tobytes() == s.tobytes() and get_sweeps(b)[2].tobytes() == bytes(case.n * wref.DTYPE.itemsize)
        with pytest.raises(BatchError, match="still in use"):
            b.set_polyphony(1)
        b.set_polyphony(2)
        run_calls(b, case, records, (70,), "two lanes again", "k_sweep_rows", state=(r, p, f, s))


def test_api_array_sweeps(tmp_path):
    """tests/cpp/api_array_sweeps.cpp: ApiArray::sweep_voice_filter and get_voice_filter_sweep against the batch calls."""
    exe = str(tmp_path / "api_array_sweeps")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_sweeps.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
