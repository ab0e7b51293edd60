"""GPU: the envelope programs (oalsfx_batch_set_env_programs and its lane form, and the renders while a voice's queue may hold a segment;
include/oalsfx_hip.h, "envelope programs") against their restatement (tests/program_ref.py).  Every comparison is on the bit patterns
(NaNs by position) and on the exact integers: outputs, both records and the queue of every voice, read back after every call; there is
no tolerance anywhere.  No test provokes a device fault: every refusal is decided on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import polyphony_cases as pcases
import program_cases as gcases
import program_ref as gref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from harness import ROOT, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import ENV_PROGRAM_MAX, ENVELOPE_DTYPE, Batch, BatchError, envelope_adsr
from test_gpu_biquad import expect_filters, set_filters
from test_gpu_polyphony import place
from test_gpu_resample import FORMAT, Guarded, set_tables
from test_gpu_sampler import Assets, device_render, expect_output, expect_records
from test_sampler_abi import rec
from test_voice_abi import env

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE


def _torch():
    import torch
    return torch


def set_programs(b, records, programs, resamplers):
    for k in range(records.shape[0]):
        b.set_samplers(records[k], lane=k)
        b.set_env_programs(programs[k], lane=k)
        b.set_resamplers(resamplers[k], lane=k)


def expect_programs(b, state, programs, label):
    """Both records and the queue of every voice, and get_envelopes beside get_env_programs."""
    for k in range(state.shape[0]):
        expect_records(b.get_samplers(lane=k), state[k], f"{label}, lane {k}")
        got, current = b.get_env_programs(lane=k), b.get_envelopes(lane=k)
        for i, want in enumerate(programs[k]):
            want = np.asarray(want, dtype=vref.DTYPE)
            assert len(got[i]) == len(want), f"{label}: (lane {k}, instance {i}) has {len(got[i])} segments, not {len(want)}"
            assert got[i].tobytes() == want.tobytes(), f"{label}: the program of (lane {k}, instance {i}) differs"
            assert current[i].tobytes() == want[0].tobytes(), f"{label}: get_envelopes of (lane {k}, instance {i}) is not the current segment"


def run_calls(b, records, programs, resamplers, filters, tables, pcm, sizes, label, **kw):
    """One render per size, each against the restatement, with everything read back after every call."""
    kernel = "k_program_rows" if filters is None else "k_program_biquad_rows"
    plain = ("k_fir_rows" if records.shape[0] == 1 else "k_mix_rows") if filters is None else "k_biquad_rows"
    state, p_state, f_state, outs = records, programs, filters, []
    for frames in sizes:
        p_state_before = p_state
        want, state, p_state, f_state = gref.render(state, p_state, resamplers, f_state, tables, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        # (while a queue holds a segment the render walks the queues; once none does the batch may go on doing so for a while)
        pending = any(len(p) > 1 for lane in p_state_before for p in lane)
        assert b.last_render_kernel() in ((kernel,) if pending else (kernel, plain))
        expect_output(got, want, f"{label}, {frames} frames")
        expect_programs(b, state, p_state, f"{label}, after {frames} frames")
        if filters is not None:
            expect_filters(b, f_state, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), state, p_state, f_state


def named(placed):
    names, records, programs, resamplers, pcm, which = gcases.named_programs(2)
    records = records.copy()
    records["data"] = place(placed, pcm)
    records["data"][(records["flags"] & sref.PLAYING) == 0] = 0
    return names, records, programs, resamplers, pcm, which


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("offset", [0, 1, 2])
def test_the_voices_the_contract_names(offset, filtered):
    """8 stereo instances of 4 lanes in calls of 1, 63, 64, 65, 256 and 7 frames, and in one call of their sum on a twin: boundaries at
    frames 1, 63, 64, 65 and 128, three inside one tile, one on a call's last frame, eight segments used up in one call, zero-length
    segments, a queued delay, a STOP in mid-program, a one-shot that ends inside a later segment, a loop shorter than the taps, and voices
    without a program beside them."""
    placed = Guarded()
    names, records, programs, resamplers, pcm, which = named(placed)
    filters = bcases.named_filters(names) if filtered else None
    tables = cases.tables()
    _torch().cuda.synchronize()
    with Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as b, Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as twin:
        for batch in (b, twin):
            set_tables(batch, tables)
            batch.set_polyphony(pcases.LANES)
            set_programs(batch, records, programs, resamplers)
            if filtered:
                set_filters(batch, filters)
        expect_programs(b, records, programs, "as set")
        parts, state, p_state, f_state = run_calls(b, records, programs, resamplers, filters, tables, pcm, gcases.CALLS, "the named voices", offset=offset)
        whole, state1, p1, f1 = run_calls(twin, records, programs, resamplers, filters, tables, pcm, (sum(gcases.CALLS),), "one call of the sum", offset=offset)
        assert same_bits(parts, whole)[0] and state.tobytes() == state1.tobytes()
        assert all(np.asarray(a).tobytes() == np.asarray(c).tobytes() for la, lc in zip(p_state, p1) for a, c in zip(la, lc))
        assert not filtered or f_state.tobytes() == f1.tobytes()
        assert not np.isnan(parts).any(), "a guard frame was read"
        k, i = which["STOP in mid-program"]
        assert not state[k][i]["flags"] & sref.PLAYING and len(p_state[k][i]) == 1 and p_state[k][i][0]["ramp_done"] == 10
        k, i = which["eight segments used up in one call"]
        assert len(p_state[k][i]) == 1
        k, i = which["a one-shot that ends inside a later segment"]
        assert not state[k][i]["flags"] & sref.PLAYING and len(p_state[k][i]) == 2


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("channels", [1, 4, 6, 7, 8])
def test_every_channel_count_with_random_programs(channels, filtered):
    """13 instances (a partial fourth workgroup) of 4 lanes: 52 random voices, half of them with a random program of 2 .. 8 segments; the
    destination 0, 1 or 2 floats off its allocation."""
    rng = np.random.default_rng(7000 + channels)
    calls = (70, 200, 3)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 13, 4, channels, True, calls=calls, asset_frames=(1, 500))
    programs = gcases.random_programs(rng, envelopes, channels)
    filters = bcases.random_filters(rng, 4, 13) if filtered else None
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(13, FORMAT[channels], 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(4)
        set_programs(b, records, programs, resamplers)
        if filtered:
            set_filters(b, filters)
        parts, _, after, _ = run_calls(b, records, programs, resamplers, filters, cases.tables(), pcm, calls, f"{channels} channels", offset=channels % 3)
        assert np.abs(parts).max() > 0
        assert sum(len(p) for lane in after for p in lane) < sum(len(p) for lane in programs for p in lane)


def test_a_twin_whose_renders_are_split_at_every_boundary():
    """One batch gets the programs and one render of 456 frames.  Its twin gets every voice's first segment, and its render is split at
    every boundary of every voice, with set_lane_envelopes of the segment that takes over between the renders.  Outputs and final records
    are byte-equal: no reference takes part."""
    placed = Guarded()
    names, records, programs, resamplers, pcm, which = named(placed)
    tables = cases.tables()
    frames = sum(gcases.CALLS)
    # at frame t the voice (k, i) takes segment j: the last one where several are taken at once
    events = {}
    for k in range(pcases.LANES):
        for i in range(pcases.INSTANCES):
            for j, t in enumerate(gref.boundaries(programs[k][i], frames)):
                events.setdefault(t, {})[(k, i)] = j + 1
    assert {1, 63, 64, 65, 128, 193}.issubset(events) and len(events) > 20
    _torch().cuda.synchronize()
    with Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as b, Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as twin:
        for batch in (b, twin):
            set_tables(batch, tables)
            batch.set_polyphony(pcases.LANES)
        set_programs(b, records, programs, resamplers)
        whole = device_render(b, frames)
        assert b.last_render_kernel() == "k_program_rows"
        for k in range(pcases.LANES):
            twin.set_samplers(records[k], lane=k)
            twin.set_envelopes(gcases.first_segments(programs)[k], lane=k)
            twin.set_resamplers(resamplers[k], lane=k)
        parts, t = [], 0
        for at in sorted(set(events) | {frames}):
            if at > t:
                parts.append(device_render(twin, at - t))
                assert twin.last_render_kernel() == "k_mix_rows"
                t = at
            for (k, i), j in events.get(at, {}).items():
                twin.set_envelopes(np.asarray(programs[k][i][j:j + 1], dtype=ENVELOPE_DTYPE), instances=[i], lane=k)
        assert same_bits(whole, np.concatenate(parts, axis=1))[0]
        for k in range(pcases.LANES):
            assert b.get_samplers(lane=k).tobytes() == twin.get_samplers(lane=k).tobytes()
            assert b.get_envelopes(lane=k).tobytes() == twin.get_envelopes(lane=k).tobytes()
            assert all(len(p) == 1 for p in twin.get_env_programs(lane=k))


def test_the_dispatch_follows_the_horizon_and_a_lone_negative_zero_stays_negative():
    torch = _torch()
    pcm = np.full((6, 1), -0.0, f32)
    asset = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    r = rec(data=asset.data_ptr(), format=sref.PCM_F32, frames=6, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=6, step=ONE)
    rng = np.random.default_rng(3)
    program = [gcases.segment(rng, 2, 10), gcases.segment(rng, 2, 20)]
    for e in program:
        for name in ("gain_from", "gain_step", "gain_to"):
            e[name] = np.abs(e[name]) + f32(0.25)
    program[0]["gain_step"] = program[1]["gain_step"] = 0
    with Batch(1, desc.FMT_STEREO, 48000, 1) as b, Batch(1, desc.FMT_STEREO, 48000, 1) as never:
        for batch in (b, never):
            batch.set_samplers(r)
        never.set_envelopes(np.asarray(program[:1], dtype=ENVELOPE_DTYPE))
        b.set_env_programs([program])
        assert b.program_uploads() == 0
        kernels = []
        for _ in range(4):
            got = device_render(b, 8)
            kernels.append(b.last_render_kernel())
            assert np.signbit(got).all() and (got == 0).all(), "a lone voice's -0.0f reaches the input as -0.0f"
        # the horizon: the 10 frames in front of the last segment and one more, less 8 per render
        assert kernels == ["k_program_rows", "k_program_rows", "k_voice_rows", "k_voice_rows"]
        assert b.program_uploads() == 1 and [len(p) for p in b.get_env_programs()] == [1]
        device_render(never, 8)
        assert never.last_render_kernel() == "k_voice_rows" and never.program_uploads() == 0
        # with a filter ACTIVE: the other family, and the old kernel again behind the horizon
        b.set_filters(bcases.filt(bcases.low_pass(0.2), flags=bref.ACTIVE | bref.LOAD))
        b.set_env_programs([program])
        device_render(b, 16)
        assert b.last_render_kernel() == "k_program_biquad_rows"
        device_render(b, 16)
        assert b.last_render_kernel() == "k_biquad_rows"
        # at two lanes the sum starts at +0.0f
        b.set_filters(bcases.filt(bcases.low_pass(0.2), flags=0))
        b.set_polyphony(2)
        b.set_env_programs([program])
        got = device_render(b, 8)
        assert b.last_render_kernel() == "k_program_rows" and not np.signbit(got).any()


def test_refusals_change_nothing_and_plain_sets_empty_the_queue():
    rng = np.random.default_rng(5)
    seg = lambda ramp, **kw: gcases.segment(rng, 2, ramp, **kw)
    good = [seg(10), seg(20, delay=3), seg(5)]
    with Batch(3, desc.FMT_STEREO, 48000, 1) as b:
        b.set_env_programs([good, [seg(7)]], instances=[2, 0])
        before = [p.tobytes() for p in b.get_env_programs()]
        assert [len(p) for p in b.get_env_programs()] == [1, 1, 3] and b.get_env_programs()[2].tobytes() == np.asarray(good, ENVELOPE_DTYPE).tobytes()

        def refused(message, programs, lengths=None, instances=(1,), lane=0, through_python=True):
            if through_python:
                with pytest.raises(BatchError, match=message):
                    b.set_env_programs(programs, instances=list(instances), lane=lane)
            # the library's own refusal, past the checks of the Python layer
            segments = np.zeros((len(programs), ENV_PROGRAM_MAX), ENVELOPE_DTYPE)
            for k, p in enumerate(programs):
                segments[k, :min(len(p), ENV_PROGRAM_MAX)] = np.asarray(p[:ENV_PROGRAM_MAX], ENVELOPE_DTYPE)
            lens = (C.c_int * len(programs))(*(lengths or [len(p) for p in programs]))
            idx = (C.c_int * len(instances))(*instances)
            assert not b._lib.oalsfx_batch_set_lane_env_programs(b._h, lane, idx, len(programs), lens, C.c_void_p(segments.ctypes.data))
            assert b._lib.oalsfx_batch_error(b._h).decode() == message.replace("\\", "")
            assert [p.tobytes() for p in b.get_env_programs()] == before

        inactive, gliding, unknown, beyond = seg(4, flags=0), seg(4), seg(4, flags=vref.ACTIVE | 8), seg(4)
        vref.glide(gliding, ONE, 2 * ONE, 10)
        beyond["ramp_done"] = 5
        refused("Envelope program length out of range\\.", [[seg(1)]], lengths=[0], through_python=False)
        refused("Envelope program length out of range\\.", [[seg(1)] * 8], lengths=[9], through_python=False)
        refused("A program's segment is not active\\.", [[seg(3), inactive]])
        refused("A program's segment glides\\.", [[gliding, seg(3)]])
        refused("Unknown envelope flags\\.", [[seg(3), seg(2), unknown]])
        refused("The envelope's ramp_done is beyond its ramp\\.", [[beyond]])
        refused("Lane out of range\\.", [good], lane=1, through_python=False)
        refused("An instance is listed twice as an envelope target\\.", [good, good], instances=(1, 1))
        refused("Instance range is out of bounds\\.", [good], instances=(3,), through_python=False)
        # a program of one is set_envelopes, GLIDE included; and a plain set empties a queue
        b.set_samplers(rec(data=0, flags=0, step=ONE), instances=[1])
        b.set_env_programs([[gliding]], instances=[1])
        assert b.get_envelopes(instances=[1]).tobytes() == np.asarray([gliding], ENVELOPE_DTYPE).tobytes()
        b.set_envelopes(np.asarray([seg(9)], ENVELOPE_DTYPE), instances=[2])
        assert [len(p) for p in b.get_env_programs()] == [1, 1, 1]
        # round trips through set_polyphony: kept lanes kept, new lanes empty
        b.set_env_programs([good], instances=[1])
        b.set_polyphony(3)
        b.set_env_programs([good[1:]], instances=[0], lane=2)
        assert [len(p) for p in b.get_env_programs()] == [1, 3, 1] and [len(p) for p in b.get_env_programs(lane=1)] == [1, 1, 1]
        assert b.get_env_programs(lane=2)[0].tobytes() == np.asarray(good[1:], ENVELOPE_DTYPE).tobytes()
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use\\."):
            b.set_polyphony(2)


def test_an_adsr_note_on_and_note_off():
    """envelope_adsr's first three segments as a program, the release set at a call boundary: the voice ends silent and stopped."""
    torch = _torch()
    pcm = np.linspace(-1, 1, 64, dtype=f32).reshape(-1, 1)
    asset = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    r = rec(data=asset.data_ptr(), format=sref.PCM_F32, frames=64, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=0, loop_end=64, step=ONE // 3)
    adsr = envelope_adsr([1.0, 0.5], [0.25, 0.125], 30, 50, 7, 40)
    with Batch(1, desc.FMT_STEREO, 48000, 1) as b:
        b.set_samplers(r)
        b.set_env_programs([adsr[:3]])
        state, programs = r.reshape(1, 1), [[list(adsr[:3])]]
        for frames in (64, 64):
            want, state, programs, _ = gref.render(state, programs, np.full((1, 1), ref.NONE), None, {}, [[pcm]], frames, 2)
            expect_output(device_render(b, frames), want, "note-on")
        assert [len(p) for p in b.get_env_programs()] == [1]
        b.set_envelopes(adsr[3:])
        got = device_render(b, 64)
        assert (got[0, 40:] == 0).all() and np.abs(got[0, :39]).max() > 0 and not b.get_samplers()[0]["flags"] & sref.PLAYING


def test_api_array_programs(tmp_path):
    """tests/cpp/api_array_programs.cpp: ApiArray::set_envelope_program / get_envelope_program against a twin array whose render is split."""
    exe = str(tmp_path / "api_array_programs")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_programs.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
