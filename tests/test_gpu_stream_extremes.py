"""GPU: the sampler streams at the ends of their 64-bit range -- the case families of tests/test_stream_extremes.py, which the frame-at-a-time
model (tests/stream_model.py) has vouched for -- against their restatement (tests/stream_ref.py): k_stream_rows with the storing sink
(one lane) and with the adding sink and its lane rotation (three lanes), k_stream_filter_rows, the chunks of a long asset against the
device's own k_sampler_rows, and an append between two renders that nothing waits for.  Every comparison is on the bit patterns (NaNs by
position) and on the exact bytes of the records: outputs, the current record and the ring of every voice, the taken counts and the
envelope programs, read back after every call; there is no tolerance anywhere.  Every asset lies between guard frames of NaN (fp32) or
full scale: a frame read outside a chunk shows.  No test provokes a device fault: every record passes the host's checks, and no wrong
form of anything runs here."""
import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import filter_program_cases as fcases
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import stream_cases as scases
import stream_ref as stref
import sweep_cases as wcases
import sweep_ref as wref
import test_stream_extremes as x
import voice_ref as vref
from oalsfxpp_amd import desc
from oalsfxpp_amd.api import Batch
from test_gpu_resample import FORMAT
from test_gpu_sampler import device_render, expect_output
from test_gpu_streams import GuardedPool, Pair

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE, PLAYING = sref.ONE, sref.PLAYING
FAMILIES = ["takes past 2^32", "an excess that skips entries", "an excess into a loop", "ends on the grid at large values",
            "under envelopes at their bounds", "fields a take must carry whole"]


def _torch():
    import torch
    return torch


def play(pair, case, appends, label, kernel):
    """The case's calls and SPLIT's on `pair`, everything compared after every call, the appends behind the calls they follow: the outputs
    side by side.  The first render walks the rings, through `kernel`."""
    pair.expect_state(f"{label}: as set")
    parts = []
    for c, frames in enumerate(case.calls + x.SPLIT):
        parts.append(pair.render(frames, f"{label}, call {c}", offset=c % 2))
        if c == 0:
            assert pair.b.last_render_kernel() == kernel, pair.b.last_render_kernel()
        for k, i, entries in appends.get(c, ()):
            pair.append(k, i, entries)
    out = np.concatenate(parts, axis=1)
    assert not np.isnan(out).any(), f"{label}: a guard frame was read"
    return out


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_in_one_lane(name):
    """k_stream_rows with the storing sink, stereo: every case of the family, a voice per instance; and on a twin batch one render of the
    calls' sum (a case with an append: of the calls in front of it, and of those behind it): the same bits and the same state."""
    family = x.cases_of(name, 2)
    placed = GuardedPool(family[0].pool)
    for case in family:
        n = len(case.names)
        calls = case.calls + x.SPLIT
        with Batch(n, desc.FMT_STEREO, 48000, 1) as b, Batch(n, desc.FMT_STEREO, 48000, 1) as twin:
            streams, assets, appends = case.placed(placed.bases)
            pair = Pair(b, streams, [case.programs], [case.resamplers], cases.tables(), assets)
            out = play(pair, case, appends, case.label, "k_stream_rows")
            streams, assets, appends = case.placed(placed.bases)
            other = Pair(twin, streams, [case.programs], [case.resamplers], cases.tables(), assets)
            upto = 1 + min(appends) if appends else len(calls)
            sums = [other.render(sum(calls[:upto]), f"{case.label}, in one render")]
            for k, i, entries in appends.get(upto - 1, ()):
                other.append(k, i, entries)
            if upto < len(calls):
                sums.append(other.render(sum(calls[upto:]), f"{case.label}, the rest in one render"))
            assert sref.same_floats(out, np.concatenate(sums, axis=1))[0], f"{case.label}: one render differs from the calls"
            assert (pair.taken == other.taken).all() and pair.taken.sum() >= n // 2


def in_three_lanes(case, channels, assets_at, seed):
    """The case's voices in lanes 0 and 2 of a batch whose instance count is no multiple of 4, an ordinary random voice of
    stream_cases.random_streams in every instance of lane 1: (n, streams [3][n], programs, resamplers, assets, appends, what to keep alive)."""
    voices = len(case.names)
    half = -(-voices // 2)
    n = max(half, 5)
    while n % 4 == 0:
        n += 1
    assert n % 4 != 0 and n >= half
    where = [(0, v) if v < half else (2, v - half) for v in range(voices)]
    own, assets, appends = case.placed(assets_at.bases)
    rng = np.random.default_rng(seed)
    middle, middle_programs, middle_resamplers, pool = scases.random_streams(rng, n, 1, channels, case.calls + x.SPLIT)
    middle_placed = GuardedPool(pool)
    middle, middle_assets = scases.resolve_streams(middle, pool, middle_placed.bases)
    assets.update(middle_assets)
    idle, none = np.zeros(1, sref.DTYPE), [np.zeros(1, vref.DTYPE)[0]]
    streams = [[idle.copy() for _ in range(n)], middle[0], [idle.copy() for _ in range(n)]]
    programs = [[list(none) for _ in range(n)], middle_programs[0], [list(none) for _ in range(n)]]
    resamplers = np.full((3, n), ref.NONE)
    resamplers[1] = middle_resamplers[0]
    for v, (k, i) in enumerate(where):
        streams[k][i], programs[k][i], resamplers[k][i] = own[0][v], case.programs[v], case.resamplers[v]
    appends = {c: [(where[i][0], where[i][1], e) for _, i, e in items] for c, items in appends.items()}
    return n, streams, programs, resamplers, assets, appends, middle_placed


@pytest.mark.parametrize("channels", [2, 6])
@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_in_three_lanes(name, channels):
    """k_stream_rows with the adding sink, whose lanes are rotated by t % 64 at every span: the family's voices in lanes 0 and 2, an
    ordinary random voice in lane 1, the instances no multiple of 4 (a partial last workgroup); stereo, and 6 channels wide with mono and
    wide assets."""
    family = x.cases_of(name, channels)
    placed = GuardedPool(family[0].pool)
    for c, case in enumerate(family):
        n, streams, programs, resamplers, assets, appends, keep = in_three_lanes(case, channels, placed, 7000 + 10 * channels + c)
        with Batch(n, FORMAT[channels], 48000, 1) as b:
            pair = Pair(b, streams, programs, resamplers, cases.tables(), assets)
            play(pair, case, appends, case.label + ", three lanes", "k_stream_rows")
            assert pair.taken[0].sum() + pair.taken[2].sum() >= len(case.names) // 2


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_under_the_filter_stage(name):
    """k_stream_filter_rows, stereo, one lane: every second voice has an ACTIVE filter with a filter program whose first switch falls on
    the frame of the voice's first take (a voice that takes nothing in its first frames: at frame 10); the filters and the filter programs
    are read back after every call."""
    family = x.cases_of(name, 2)
    placed = GuardedPool(family[0].pool)
    rng = np.random.default_rng(len(name))
    for case in family:
        n = len(case.names)
        first_takes = [next((sum((case.calls + x.SPLIT)[:c]) + r[4][i][0] for c, r in enumerate(x.restated(name, 2)[family.index(case)]) if r[4][i]), 0) for i in range(n)]
        filters = np.zeros((1, n), bref.DTYPE)
        filter_programs = [[[np.zeros(1, wref.DTYPE)[0]] for _ in range(n)]]
        for i in range(0, n, 2):
            filters[0][i] = bcases.filt(wcases.design(rng), x=rng.uniform(-1, 1, (8, 2)).astype(f32), y=rng.uniform(-1, 1, (8, 2)).astype(f32))[0]
            switch = first_takes[i] if first_takes[i] > 0 else 10
            filter_programs[0][i] = fcases.make_program(rng, bref.coefficients(filters[0][i]), ((switch, 0), (37, 0), (500, 0)), continuous=i % 4 == 0)
        assert any(0 < first_takes[i] for i in range(0, n, 2))
        with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
            streams, assets, appends = case.placed(placed.bases)
            pair = Pair(b, streams, [case.programs], [case.resamplers], cases.tables(), assets, filters=filters, filter_programs=filter_programs)
            play(pair, case, appends, case.label + ", filtered", "k_stream_filter_rows")
            assert pair.taken.sum() >= n // 2


def test_chunks_play_the_whole_long_assets_on_the_device():
    """The chunks property against the device itself at large values: the nearest-sample voices of "takes past 2^32" -- steps 1, 2^23 + 1,
    2^31 + 12345 and 2^32 - 1 among them, every start just below a cut beyond frame 2^20 -- as streams of chunks through k_stream_rows,
    and their twins as whole long assets through k_sampler_rows: the same bits, the same final positions in the asset, and taken the
    count of the chunks where the voice has finished."""
    case = x.case_named("takes past 2^32", "nearest and LINEAR", 2)
    placed = GuardedPool(case.pool)
    streams, assets, _ = case.placed(placed.bases)
    rows = [i for i, s in enumerate(case.streams) if not int(s[0]["flags"]) & sref.LINEAR and int(case.resamplers[i]) == ref.NONE]
    assert {1, *x.LARGE_STEPS} <= {int(case.streams[i][0]["step"]) for i in rows} and len(rows) >= 8
    chunks = [streams[0][i] for i in rows]
    whole = np.zeros(len(rows), sref.DTYPE)
    firsts = []
    for k, s in enumerate(chunks):
        key = int(case.streams[rows[k]][0]["data"]) >> 32
        whole[k] = s[0]
        whole[k]["frames"] = case.pool[key].shape[0]
        assert int(s[0]["data"]) == placed.bases[key] and int(s["frames"].sum()) == case.pool[key].shape[0]
        firsts.append(key)
    with Batch(len(rows), desc.FMT_STEREO, 48000, 1) as plain, Batch(len(rows), desc.FMT_STEREO, 48000, 1) as streamed:
        plain.set_samplers(whole)
        streamed.set_streams(chunks)
        for frames in case.calls + x.SPLIT:
            a, b = device_render(plain, frames), device_render(streamed, frames)
            assert plain.last_render_kernel() == "k_sampler_rows" and streamed.last_render_kernel() == "k_stream_rows"
            expect_output(b, a, f"{frames} frames: the chunks against the whole long assets")
            assert not np.isnan(a).any() and not np.isnan(b).any(), "a guard frame was read"
        ends, current = plain.get_samplers(), streamed.get_samplers()
        taken, queued = streamed.get_stream_state()
        for k, key in enumerate(firsts):
            width = case.pool[key].shape[1] * case.pool[key].dtype.itemsize
            first = (int(current[k]["data"]) - placed.bases[key]) // width
            assert first * ONE + int(current[k]["position"]) == int(ends[k]["position"]) and int(current[k]["flags"]) == int(ends[k]["flags"]), case.names[rows[k]]
        done = (ends["flags"] & PLAYING) == 0
        assert done.any() and not done.all()
        assert (taken[done] == np.asarray([len(s) - 1 for s in chunks])[done]).all() and not queued[done].any()


def test_an_append_between_renders_nothing_waits_for():
    """"an excess that skips entries", the case whose voice runs dry with an excess left over: the first render, the append and the
    second render are queued without a wait in between, then one state call; the appended entry starts at its own position on frame 0
    of the second render."""
    case = x.case_named(*x.REFILLED, 2)
    placed = GuardedPool(case.pool)
    streams, assets, appends = case.placed(placed.bases)
    torch = _torch()
    n = len(case.names)
    (c, items), = appends.items()
    assert c == 0
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        pair = Pair(b, streams, [case.programs], [case.resamplers], cases.tables(), assets)
        bufs = [torch.empty((n, frames, 2), dtype=torch.float32, device="cuda") for frames in case.calls[:2]]
        torch.cuda.synchronize()
        b.sample_device(case.calls[0], bufs[0].data_ptr())
        for k, i, entries in items:
            b.append_streams([entries], instances=[i], lane=k)
        b.sample_device(case.calls[1], bufs[1].data_ptr())
        state, taken = pair.streams, pair.taken
        wants = []
        for r, frames in enumerate(case.calls[:2]):
            want, state, taken, pair.programs = stref.render(state, taken, pair.programs, pair.resamplers, pair.tables, assets, frames, 2)
            wants.append(want)
            if r == 0:
                for k, i, entries in items:
                    state[k][i] = stref.append(state[k][i], entries)
        pair.streams, pair.taken = state, taken
        pair.expect_state("behind the two renders")         # (the state call: it waits for both)
        assert b.last_render_kernel() == "k_stream_rows"
        b.synchronize()
        for buf, want, frames in zip(bufs, wants, case.calls):
            expect_output(buf.cpu().numpy(), want, f"the render of {frames} frames")
        k, i, entries = items[0]
        assert pair.taken[k][i] == 3 and int(pair.streams[k][i][0]["position"]) == int(entries[0]["position"]) + case.calls[1] * int(entries[0]["step"])
        pair.render(case.calls[2], "a render behind the state call")
