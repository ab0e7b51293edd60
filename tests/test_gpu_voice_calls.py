"""GPU: what the ten per-voice record calls (oalsfx_batch_set_lane_* / get_lane_* of samplers, envelopes, envelope programs, resamplers and
voice filters) and their ten lane-0 forms share, pinned where a change to the shared code could move it unseen: the order in which a call
that breaks two rules at once is refused, a program of one segment against a plain envelope set, a queue emptied by a plain set, and the
records across set_polyphony.  4 stereo instances of 2 lanes, renders of 65 frames.  Every comparison is exact.  No test provokes a device
fault: every refusal is decided on the host."""
import ctypes as C

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import program_cases as gcases
import resample_cases as cases
import sampler_ref as sref
import voice_ref as vref
from harness import same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import ENV_PROGRAM_MAX, ENVELOPE_DTYPE, FILTER_DTYPE, SAMPLER_DTYPE, Batch, BatchError
from test_gpu_resample import set_tables
from test_gpu_sampler import device_render
from test_sampler_abi import rec

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
N, LANES, FRAMES = 4, 2, 65
RANGE = "Instance range is out of bounds."
SEEDED = "Polyphony out of range."

# kind: (the arrays the call takes, the text for each one that is null in the order they are tested, the text for an instance listed twice)
KINDS = {
    "samplers": ((SAMPLER_DTYPE,), ("No sampler records.",), "An instance is listed twice as a sampler target."),
    "envelopes": ((ENVELOPE_DTYPE,), ("No envelope records.",), "An instance is listed twice as an envelope target."),
    "env_programs": ((C.c_int, ENVELOPE_DTYPE), ("No envelope program lengths.", "No envelope records."), "An instance is listed twice as an envelope target."),
    "resamplers": ((C.c_int,), ("No resampler indices.",), "An instance is listed twice as a resampler target."),
    "filters": ((FILTER_DTYPE,), ("No voice filter records.",), "An instance is listed twice as a voice filter target."),
}


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def batch():
    with Batch(N, desc.FMT_STEREO, 48000, 1) as b:
        b.set_polyphony(LANES)
        yield b


def arrays_of(kind, count):
    """Arrays a call of `kind` accepts for `count` voices (all-zero records, programs of one segment, no resampler), and their arguments."""
    kept, args = [], []
    for what in KINDS[kind][0]:
        if what is C.c_int:
            a = (C.c_int * max(count, 1))(*([1 if kind == "env_programs" else -1] * count))
            args.append(a)
        else:
            a = np.zeros(count * (ENV_PROGRAM_MAX if kind == "env_programs" else 1), what)
            args.append(C.c_void_p(a.ctypes.data))
        kept.append(a)
    return kept, args


def voice_call(b, kind, op, lane, instances, count, args):
    """The library's own entry point, past the checks of the Python layer: the lane form, or with lane None the lane-0 form."""
    name = f"oalsfx_batch_{op}_{'' if lane is None else 'lane_'}{kind}"
    idx = None if instances is None else (C.c_int * max(len(instances), 1))(*instances)
    head = (b._h,) if lane is None else (b._h, lane)
    return getattr(lib.load(), name)(*head, idx, count, *args)


def seed_error(b):
    """A refusal of another call, so that the text a voice call leaves is known to be its own."""
    assert lib.load().oalsfx_batch_set_polyphony(b._h, 0) == 0 and b.error == SEEDED


def refused(b, kind, op, lane, instances, args, text):
    seed_error(b)
    assert voice_call(b, kind, op, lane, instances, len(instances), args) == 0
    assert b.error == text, f"{op}_{kind}, lane {lane}, instances {instances}: refused with {b.error!r}, not {text!r}"


def snapshot(b, lanes=LANES):
    """Every getter's answer for the first `lanes` lanes, as bytes."""
    out = []
    for k in range(lanes):
        out += [b.get_samplers(lane=k).tobytes(), b.get_envelopes(lane=k).tobytes(), b.get_resamplers(lane=k).tobytes(), b.get_filters(lane=k).tobytes()]
        out += [p.tobytes() for p in b.get_env_programs(lane=k)]
    return out


@pytest.mark.parametrize("lane_form", [True, False], ids=["lane", "lane0"])
@pytest.mark.parametrize("op", ["set", "get"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_call_that_breaks_two_rules_is_refused_for_the_earlier_one(batch, kind, op, lane_form):
    b = batch
    before = snapshot(b)
    lane = 1 if lane_form else None
    nulls = [None] * len(KINDS[kind][0])
    null_texts, twice = KINDS[kind][1], KINDS[kind][2]
    kept, good = arrays_of(kind, 2)
    if lane_form:
        # lane out of range + instance out of range (and with it the null arrays)
        for bad_lane in (LANES, -1):
            refused(b, kind, op, bad_lane, [N], nulls, "Lane out of range.")
            refused(b, kind, op, bad_lane, [0, N], good, "Lane out of range.")
        # ... and in front of "nothing to do"
        seed_error(b)
        assert voice_call(b, kind, op, LANES, None, 0, nulls) == 0 and b.error == "Lane out of range."
    # instance out of range + null array
    refused(b, kind, op, lane, [N], nulls, RANGE)
    refused(b, kind, op, lane, [0, -1], nulls, RANGE)
    seed_error(b)
    assert voice_call(b, kind, op, lane, None, N + 1, nulls) == 0 and b.error == RANGE
    seed_error(b)
    assert voice_call(b, kind, op, lane, None, -1, nulls) == 0 and b.error == RANGE
    # null array + instance listed twice (a getter may list one twice: the null array alone); of two null arrays the first one's text
    for k, text in enumerate(null_texts):
        refused(b, kind, op, lane, [1, 1], good[:k] + nulls[k:], text)
        refused(b, kind, op, lane, [2, 1], good[:k] + nulls[k:], text)
    if op == "set":
        refused(b, kind, op, lane, [1, 1], good, twice)
    else:
        seed_error(b)
        assert voice_call(b, kind, op, lane, [1, 1], 2, good) == 1 and b.error == SEEDED
    # nothing to do: 1, and the error text stays whatever it was
    seed_error(b)
    assert voice_call(b, kind, op, lane, None, 0, nulls) == 1 and b.error == SEEDED
    assert voice_call(b, kind, op, lane, [], 0, nulls) == 1 and b.error == SEEDED
    assert snapshot(b) == before


def looping_asset():
    torch = _torch()
    pcm = np.linspace(-1, 1, 64, dtype=f32).reshape(-1, 1)
    asset = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    return asset


def samplers_for(asset, lane):
    r = np.concatenate([rec(data=asset.data_ptr(), format=sref.PCM_F32, frames=64, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=0, loop_end=64,
                            step=ONE + 100 * i + 7 * lane, position=(3 * i + lane) * ONE) for i in range(N)])
    r["gain"][:, :2] = [[0.5 + 0.1 * i, 0.75 - 0.1 * i] for i in range(N)]
    return r


def twins():
    b, twin = Batch(N, desc.FMT_STEREO, 48000, 1), Batch(N, desc.FMT_STEREO, 48000, 1)
    for batch in (b, twin):
        batch.set_polyphony(LANES)
    return b, twin


def expect_twins(b, twin, label):
    """One render on each, then everything the two forms of the call could leave different."""
    got, got_twin = device_render(b, FRAMES), device_render(twin, FRAMES)
    assert got.tobytes() == got_twin.tobytes() and same_bits(got, got_twin)[0], f"{label}: the renders differ"
    assert np.abs(got).max() > 0
    assert b.last_render_kernel() == twin.last_render_kernel() != ""
    for k in range(LANES):
        assert b.get_envelopes(lane=k).tobytes() == twin.get_envelopes(lane=k).tobytes(), f"{label}: envelopes of lane {k}"
        assert b.get_samplers(lane=k).tobytes() == twin.get_samplers(lane=k).tobytes(), f"{label}: samplers of lane {k}"
        mine, theirs = b.get_env_programs(lane=k), twin.get_env_programs(lane=k)
        assert [p.tobytes() for p in mine] == [p.tobytes() for p in theirs] and all(len(p) == 1 for p in mine), f"{label}: programs of lane {k}"
    assert b.envelope_uploads() == twin.envelope_uploads() and b.program_uploads() == twin.program_uploads()
    assert b.sampler_uploads() == twin.sampler_uploads()
    return got


def test_a_program_of_one_segment_is_a_plain_set():
    """Twin batches: one gets set_envelopes, the other set_env_programs with every length 1.  A plain ACTIVE ramp (ramps that end inside
    the render, on its last frame and behind it, one with a delay), then an ACTIVE | GLIDE envelope set behind a render that a glide took
    part in: the check of the new glide needs the step the first glide ended on, read back from the device."""
    asset = looping_asset()
    rng = np.random.default_rng(11)
    b, twin = twins()
    with b, twin:
        for k in range(LANES):
            ramps = np.asarray([gcases.segment(rng, 2, ramp, delay=delay) for ramp, delay in ((10, 0), (FRAMES, 0), (100, 0), (20, 30))], ENVELOPE_DTYPE)
            for batch in (b, twin):
                batch.set_samplers(samplers_for(asset, k), lane=k)
            b.set_envelopes(ramps, lane=k)
            twin.set_env_programs(ramps.reshape(N, 1), lane=k)
        expect_twins(b, twin, "ACTIVE ramps")
        assert b.last_render_kernel() == "k_mix_rows" and b.envelope_uploads() == 1 and b.program_uploads() == 0
        assert (b.get_envelopes()["ramp_done"] == [10, FRAMES, FRAMES, 20]).all()

        # lane 0 glides from its step to 2 * ONE in 40 frames: both batches alike, by the plain call, and nothing asks for the samplers
        # behind the render, so the host's steps stay the old ones, from which the second glide would leave the range
        steps = b.get_samplers()["step"].copy()
        first = np.asarray([vref.glide(gcases.segment(rng, 2, 50), int(steps[i]), 2 * ONE, 40) for i in range(N)], ENVELOPE_DTYPE)
        second = np.asarray([vref.glide(gcases.segment(rng, 2, 30), 2 * ONE, ONE // 2, 50) for i in range(N)], ENVELOPE_DTYPE)
        assert all(not lib.load().oalsfx_host_envelope_check(C.c_void_p(second[i:i + 1].ctypes.data), int(steps[i]), None) for i in range(N))
        for batch in (b, twin):
            batch.set_envelopes(first, lane=0)
        device_render(b, FRAMES)
        device_render(twin, FRAMES)
        b.set_envelopes(second, lane=0)
        twin.set_env_programs([[e] for e in second], lane=0)
        expect_twins(b, twin, "a glide set behind a glide")
        assert (b.get_envelopes()["glide_done"] == 50).all() and (b.get_samplers()["step"] == ONE // 2).all()


@pytest.mark.parametrize("rendered", [False, True])
def test_a_plain_set_empties_a_queue_in_both_forms(rendered):
    """A voice with a queue of two segments, before and after a render that left the queue in place; then a plain set: by set_envelopes on
    one batch, by a program of one on its twin."""
    asset = looping_asset()
    rng = np.random.default_rng(12)
    queued = [gcases.segment(rng, 2, 200), gcases.segment(rng, 2, 30), gcases.segment(rng, 2, 40)]
    plain = np.asarray([gcases.segment(rng, 2, 20)], ENVELOPE_DTYPE)
    b, twin = twins()
    with b, twin:
        for batch in (b, twin):
            for k in range(LANES):
                batch.set_samplers(samplers_for(asset, k), lane=k)
            batch.set_env_programs([queued], instances=[2], lane=1)
            assert [len(p) for p in batch.get_env_programs(lane=1)] == [1, 1, 3, 1]
            if rendered:
                device_render(batch, FRAMES)
                assert batch.last_render_kernel() == "k_program_rows" and batch.program_uploads() == 1
                assert [len(p) for p in batch.get_env_programs(lane=1)] == [1, 1, 3, 1]
        b.set_envelopes(plain, instances=[2], lane=1)
        twin.set_env_programs([plain], instances=[2], lane=1)
        for batch in (b, twin):
            assert [len(p) for p in batch.get_env_programs(lane=1)] == [1, 1, 1, 1]
            assert batch.get_env_programs(lane=1)[2].tobytes() == plain.tobytes()
        expect_twins(b, twin, "a queue emptied")
        # the emptied row went to the device in front of that render
        assert b.program_uploads() == (2 if rendered else 1)
        assert b.get_envelopes(instances=[2], lane=1)["ramp_done"][0] == 20


def test_the_records_of_kept_lanes_across_set_polyphony():
    """Every table filled in both lanes, a render, then a filter set with LOAD that is still pending: 2 -> 4 -> 2 lanes, every getter the
    same in lanes 0 and 1 after each step, and 2 -> 1 refused."""
    asset = looping_asset()
    rng = np.random.default_rng(13)
    with Batch(N, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, {t: coef for t, coef in cases.tables().items() if t < 2})
        b.set_polyphony(LANES)
        for k in range(LANES):
            b.set_samplers(samplers_for(asset, k), lane=k)
            b.set_envelopes(np.asarray([gcases.segment(rng, 2, 300 + i) for i in range(N)], ENVELOPE_DTYPE), lane=k)
            b.set_resamplers([(i + k) % 2 for i in range(N)], lane=k)
            filters = np.concatenate([bcases.filt(bcases.low_pass(0.05 + 0.02 * i + 0.01 * k), flags=bref.ACTIVE | bref.LOAD, x=rng.uniform(-1, 1, (8, 2)).astype(f32),
                                                  y=rng.uniform(-1, 1, (8, 2)).astype(f32)) for i in range(N)])
            b.set_filters(filters, lane=k)
        b.set_env_programs([[gcases.segment(rng, 2, 400), gcases.segment(rng, 2, 10)]], instances=[3], lane=1)
        device_render(b, FRAMES)
        assert b.last_render_kernel() == "k_program_biquad_rows"
        loaded = bcases.filt(bcases.band_pass(0.1), flags=bref.ACTIVE | bref.LOAD, x=np.full((8, 2), 0.25, f32), y=np.full((8, 2), -0.5, f32))
        b.set_filters(loaded, instances=[1], lane=1)
        uploads = b.filter_uploads()
        want = snapshot(b)
        got = b.get_filters(instances=[1], lane=1)
        assert got["flags"][0] == bref.ACTIVE and (got["x"] == 0.25).all() and (got["y"] == -0.5).all()
        assert len(b.get_env_programs(lane=1)[3]) == 2 and (b.get_envelopes()["ramp_done"] == FRAMES).all()

        b.set_polyphony(4)
        assert b.polyphony == 4 and snapshot(b) == want
        for k in (2, 3):
            assert not b.get_samplers(lane=k).tobytes().strip(b"\0") and not b.get_envelopes(lane=k).tobytes().strip(b"\0")
            assert (b.get_resamplers(lane=k) == -1).all() and not b.get_filters(lane=k).tobytes().strip(b"\0")
            assert all(len(p) == 1 for p in b.get_env_programs(lane=k))
        b.set_polyphony(2)
        assert b.polyphony == 2 and snapshot(b) == want
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use\\."):
            b.set_polyphony(1)
        assert b.polyphony == 2 and snapshot(b) == want
        # (the pending LOAD went to the device with the whole table, not by an upload of its own: the next render has none to make)
        device_render(b, FRAMES)
        assert b.filter_uploads() == uploads and b.last_render_kernel() == "k_program_biquad_rows"
        assert (b.get_envelopes(lane=1)["ramp_done"] == 2 * FRAMES).all()
