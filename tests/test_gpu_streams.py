"""GPU: the sampler streams (oalsfx_batch_set_streams, _append_streams, _get_streams, _get_stream_state and their lane forms, and the
renders while a voice's ring may hold an entry; include/oalsfx_hip.h, "sampler streams") against their restatement
(tests/stream_ref.py).  Every comparison is on the bit patterns (NaNs by position) and on the exact bytes of the records: outputs, the
current record and the ring of every voice, the taken counts and the envelope programs, read back after every call; there is no
tolerance anywhere.  Every asset lies between guard frames of NaN (fp32) or full scale: a frame read outside a chunk shows.  No test
provokes a device fault: every refusal is decided on the host."""
import os
import subprocess

import numpy as np
import pytest

import biquad_ref as bref
import filter_program_cases as fcases
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import stream_cases as scases
import stream_ref as stref
import sweep_ref as wref
import voice_ref as vref
from harness import ROOT
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import STREAM_QUEUE, Batch, BatchError, stream_chunks
from test_gpu_biquad import expect_filters, set_filters
from test_gpu_filter_programs import expect_filter_programs
from test_gpu_resample import FORMAT, GUARD_FRAMES, set_tables
from test_gpu_sampler import device_render, expect_output
from test_voice_abi import env

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
PLAYING = sref.PLAYING


def _torch():
    import torch
    return torch


class GuardedPool:
    """The assets of a pool in device memory, each inside an allocation of its own between guard frames; bases[k] is asset k's address."""

    def __init__(self, pool):
        torch = _torch()
        self.kept, self.bases = [], []
        for pcm in pool:
            fill = np.nan if pcm.dtype == np.float32 else np.iinfo(pcm.dtype).max
            guard = np.full((GUARD_FRAMES, pcm.shape[1]), fill, pcm.dtype)
            whole = torch.from_numpy(np.concatenate([guard, pcm, guard])).cuda()
            self.kept.append(whole)
            self.bases.append(whole.data_ptr() + GUARD_FRAMES * pcm.shape[1] * pcm.dtype.itemsize)
        torch.cuda.synchronize()


def is_idle(stream):
    return len(stream) == 1 and not np.asarray(stream[0]).tobytes().strip(b"\0")


class Pair:
    """A batch and the restatement of its voices, given the same calls."""
    filters = filter_programs = None

    def __init__(self, b, streams, programs, resamplers, tables, assets, filters=None, filter_programs=None):
        self.b, self.tables, self.assets = b, tables, assets
        self.filters, self.filter_programs = filters, filter_programs
        self.lanes, self.n = len(streams), len(streams[0])
        self.streams, self.programs, self.resamplers = streams, programs, np.asarray(resamplers)
        self.taken = np.zeros((self.lanes, self.n), np.uint32)
        set_tables(b, tables)
        if self.lanes > 1:
            b.set_polyphony(self.lanes)
        for k in range(self.lanes):
            # (a voice nothing is set on stays in the state after creation: all zero)
            some = [i for i in range(self.n) if not is_idle(streams[k][i])]
            b.set_streams([streams[k][i] for i in some], instances=some, lane=k)
            b.set_env_programs(programs[k], lane=k)
            b.set_resamplers(self.resamplers[k], lane=k)
        if filters is not None:
            set_filters(b, filters)
            if filter_programs is not None:
                for k in range(self.lanes):
                    b.set_filter_programs(filter_programs[k], lane=k)

    def pending(self):
        return any(len(s) > 1 for lane in self.streams for s in lane)

    def render(self, frames, label, **kw):
        pending = self.pending()
        fp = self.filter_programs
        if self.filters is not None and fp is None:
            fp = [[[np.zeros(1, wref.DTYPE)[0]] for _ in lane] for lane in self.streams]
        want = stref.render(self.streams, self.taken, self.programs, self.resamplers, self.tables, self.assets, frames, self.b.channels, filters=self.filters,
                            filter_programs=fp)
        filtered = self.filters is not None and bool((self.filters["flags"] & bref.ACTIVE).any())
        if self.filters is not None:
            self.filters = want[4]
            if self.filter_programs is not None:
                self.filter_programs = want[5]
        want, self.streams, self.taken, self.programs = want[:4]
        got = device_render(self.b, frames, **kw)
        # (expect_state's state call has told the batch which rings are empty: it walks them exactly while one holds an entry)
        walks = "k_stream_filter_rows" if filtered else "k_stream_rows"
        assert (self.b.last_render_kernel() == walks) == pending and (pending or not self.b.last_render_kernel().startswith("k_stream")), \
            f"{label}: {self.b.last_render_kernel()} with rings {'' if pending else 'not '}pending"
        expect_output(got, want, f"{label}, {frames} frames")
        self.expect_state(f"{label}, after {frames} frames")
        return got

    def append(self, k, i, entries):
        self.b.append_streams([entries], instances=[i], lane=k)
        self.streams[k][i] = stref.append(self.streams[k][i], entries)
        assert self.streams[k][i] is not None

    def expect_state(self, label):
        for k in range(self.lanes):
            got, current = self.b.get_streams(lane=k), self.b.get_samplers(lane=k)
            taken, queued = self.b.get_stream_state(lane=k)
            for i, want in enumerate(self.streams[k]):
                want = np.asarray(want, dtype=sref.DTYPE)
                assert len(got[i]) == len(want), f"{label}: (lane {k}, instance {i}) has {len(got[i])} records, not {len(want)}"
                assert got[i].tobytes() == want.tobytes(), f"{label}: the stream of (lane {k}, instance {i}) differs: got {got[i]}, want {want}"
                assert current[i].tobytes() == want[0].tobytes(), f"{label}: get_samplers of (lane {k}, instance {i}) is not the current record"
                assert queued[i] == len(want) - 1, f"{label}: {queued[i]} entries wait at (lane {k}, instance {i}), not {len(want) - 1}"
            assert (taken == self.taken[k]).all(), f"{label}: taken in lane {k} is {taken}, not {self.taken[k]}"
            programs = self.b.get_env_programs(lane=k)
            for i, want in enumerate(self.programs[k]):
                assert programs[i].tobytes() == np.asarray(want, dtype=vref.DTYPE).tobytes(), f"{label}: the envelope program of (lane {k}, instance {i}) differs"
        if self.filters is not None:
            expect_filters(self.b, self.filters, label)
        if self.filter_programs is not None:
            expect_filter_programs(self.b, self.filter_programs, label)


def named_pair(b, channels=2):
    names, streams, programs, resamplers, pool, appends = scases.named_streams(channels)
    placed = GuardedPool(pool)
    streams, assets = scases.resolve_streams(streams, pool, placed.bases)
    appends = {c: [(k, i, scases.resolve(e, pool, placed.bases, assets)) for k, i, e in v] for c, v in appends.items()}
    return Pair(b, streams, programs, resamplers, cases.tables(), assets), appends, placed


@pytest.mark.parametrize("offset", [0, 1])
def test_the_voices_the_contract_names(offset):
    """6 stereo instances of 2 lanes in calls of 1, 63, 64, 65, 256, 7 and 200 frames: takes at frame 0 of a render, on and off the 64-frame
    tile boundaries, three inside one tile, on renders' last frames and at frame 512; chains through one-frame chunks; an intro and its
    loop; an idle voice started by an append and a dry one restarted by one; a gain ramp, a delay, a STOP fade, an envelope program whose
    switches fall in the tile of a take; LINEAR and both tap counts over the seams.  Then the same calls cut in two on a twin: the same
    bits and bytes."""
    with Batch(scases.INSTANCES, desc.FMT_STEREO, 48000, 1) as b, Batch(scases.INSTANCES, desc.FMT_STEREO, 48000, 1) as twin:
        pair, appends, placed = named_pair(b)
        other, appends2, placed2 = named_pair(twin)
        pair.expect_state("as set")
        parts, halves = [], []
        for c, frames in enumerate(scases.CALLS):
            parts.append(pair.render(frames, f"call {c}", offset=offset))
            for piece in ((frames // 2, frames - frames // 2) if frames > 1 else (1,)):
                halves.append(other.render(piece, f"call {c} in halves", offset=offset))
            for k, i, entries in appends.get(c, ()):
                pair.append(k, i, entries)
            for k, i, entries in appends2.get(c, ()):
                other.append(k, i, entries)
        out = np.concatenate(parts, axis=1)
        assert sref.same_floats(out, np.concatenate(halves, axis=1))[0]
        assert not np.isnan(out).any(), "a guard frame was read"
        assert pair.taken[0][0] == 7 and pair.taken[0][4] == 9 and pair.taken[0][5] == 3 and pair.taken[1][2] == 1


@pytest.mark.parametrize("channels", [1, 2, 6, 8])
def test_every_channel_count_with_random_streams(channels):
    """7 instances (a partial second workgroup) of 3 lanes: random voices of every PCM format, mono and wide, nearest, LINEAR and through
    4- and 8-tap tables, under random envelopes, most one-shots cut into 2 .. 8 random chunks, loops behind an intro; the destination 0 or
    1 float off its allocation."""
    rng = np.random.default_rng(9100 + channels)
    calls = (70, 200, 3, 330)
    streams, programs, resamplers, pool = scases.random_streams(rng, 7, 3, channels, calls)
    placed = GuardedPool(pool)
    streams, assets = scases.resolve_streams(streams, pool, placed.bases)
    assert sum(len(s) > 1 for lane in streams for s in lane) >= 8
    with Batch(7, FORMAT[channels], 48000, 1) as b:
        pair = Pair(b, streams, programs, resamplers, cases.tables(), assets)
        pair.expect_state("as set")
        for c, frames in enumerate(calls):
            out = pair.render(frames, f"{channels} channels, call {c}", offset=c % 2)
            assert not np.isnan(out).any(), "a guard frame was read"


def chunked_voices(rng, n, channels):
    """n random one-shots, nearest, as whole records and as streams of 2 .. 8 chunks (asset placeholders): (whole [n], streams, pool)."""
    pool, whole, streams = [], [], []
    for i in range(n):
        frames = int(rng.integers(2, 301))
        fmt, width = int(rng.integers(0, 3)), int(rng.choice([1, channels]))
        pool.append(cases.asset(rng, fmt, width, frames))
        pieces = int(rng.integers(2, min(8, frames) + 1))
        at = np.sort(rng.choice(np.arange(1, frames), pieces - 1, replace=False))
        if i % 3 == 0 and frames > pieces + 1:
            at = int(rng.integers(1, frames - pieces)) + np.arange(pieces - 1)      # one-frame chunks in a row
        lengths = np.diff(np.concatenate([[0], at, [frames]])).tolist()
        r = scases.whole(pool, i, fmt, step=int(rng.integers(1, 16384)), position=int(rng.integers(0, lengths[0] << 12)),
                         gain=rng.uniform(-1, 1, sref.MAX_CHANNELS).astype(f32))
        whole.append(r)
        streams.append(stref.chunks(r, lengths))
    return np.array(whole, dtype=sref.DTYPE), streams, pool


@pytest.mark.parametrize("channels", [2, 6])
def test_chunks_play_the_whole_asset_on_the_device(channels):
    """The chunks property against the device itself: 8 voices play whole assets through k_sampler_rows, their twins the same assets as
    streams of chunks through k_stream_rows, in the same launch shape and the same renders of 1 .. 700 frames: the same bits."""
    rng = np.random.default_rng(40 + channels)
    whole, streams, pool = chunked_voices(rng, 8, channels)
    placed = GuardedPool(pool)
    whole = scases.resolve(whole, pool, placed.bases, {})
    streams = [scases.resolve(s, pool, placed.bases, {}) for s in streams]
    with Batch(8, FORMAT[channels], 48000, 1) as plain, Batch(8, FORMAT[channels], 48000, 1) as streamed:
        plain.set_samplers(whole)
        streamed.set_streams(streams)
        for frames in (1, 64, 700, 333, 700, 700):
            a, b = device_render(plain, frames), device_render(streamed, frames)
            assert plain.last_render_kernel() == "k_sampler_rows" and streamed.last_render_kernel() == "k_stream_rows"
            expect_output(b, a, f"{frames} frames: the chunks against the whole assets")
        ends, current = plain.get_samplers(), streamed.get_samplers()
        done = (ends["flags"] & PLAYING) == 0
        assert done.any() and ((current["flags"] & PLAYING) == 0)[done].all()
        taken, queued = streamed.get_stream_state()
        assert (taken[done] == np.asarray([len(s) - 1 for s in streams])[done]).all() and not queued[done].any()


def one_voice(rng, frames=100, pieces=(25, 25, 25, 25), **fields):
    pool = [cases.asset(rng, sref.PCM_S16, 1, frames)]
    placed = GuardedPool(pool)
    assets = {}
    chunks = scases.resolve(scases.cut(pool, 0, sref.PCM_S16, list(pieces), **fields), pool, placed.bases, assets)
    return chunks, assets, placed


def test_the_batch_leaves_the_rings_kernel_only_behind_a_state_call():
    """last_render_kernel through a stream's life: the samplers' kernel before a stream is set; the rings' while the host cannot rule out
    a waiting entry, which it cannot by itself however long the batch is rendered; the samplers' again once a state call has shown the
    rings empty; the rings' again behind an append, which starts the dry voice at the next render's frame 0 (underrun and restart)."""
    rng = np.random.default_rng(3)
    chunks, assets, placed = one_voice(rng)
    none = [[[np.zeros(1, vref.DTYPE)[0]] for _ in range(5)]]
    with Batch(5, desc.FMT_STEREO, 48000, 1) as b:
        idle = [np.zeros(1, sref.DTYPE) for _ in range(5)]
        b.set_samplers(chunks[:1], instances=[2])
        device_render(b, 10)
        assert b.last_render_kernel() == "k_sampler_rows"
        pair = Pair.__new__(Pair)
        pair.b, pair.tables, pair.assets, pair.lanes, pair.n = b, {}, assets, 1, 5
        pair.resamplers, pair.programs, pair.taken = np.full((1, 5), ref.NONE), none, np.zeros((1, 5), np.uint32)
        pair.streams = [idle[:2] + [chunks.copy()] + idle[3:]]
        b.set_streams([chunks], instances=[2])
        pair.render(60, "the first takes")
        want, pair.streams, pair.taken, pair.programs = stref.render(pair.streams, pair.taken, pair.programs, pair.resamplers, {}, assets, 200, 2)
        expect_output(device_render(b, 200), want, "to the end and beyond")
        assert b.last_render_kernel() == "k_stream_rows"
        device_render(b, 50)
        assert b.last_render_kernel() == "k_stream_rows", "the host cannot know that the rings are empty"
        taken, queued = b.get_stream_state()
        assert taken.tolist() == [0, 0, 3, 0, 0] and not queued.any()
        device_render(b, 50)
        assert b.last_render_kernel() == "k_sampler_rows"
        pair.expect_state("dry")
        pair.append(0, 2, chunks[1:3])
        got = pair.render(30, "restarted")
        assert got[2, 0].any() and pair.taken[0][2] == 5
        # set_samplers empties the ring and zeroes taken: a plain set is a stream of one
        b.set_samplers(chunks[:1], instances=[2])
        pair.streams[0][2], pair.taken[0][2] = chunks[:1].copy(), 0
        pair.expect_state("behind a plain set")
        pair.render(40, "a plain voice again")
        assert b.last_render_kernel() == "k_sampler_rows"


def test_appends_against_the_device_count_and_the_full_ring():
    rng = np.random.default_rng(4)
    chunks, assets, placed = one_voice(rng, 90, (10,) * 9)
    with Batch(5, desc.FMT_MONO, 48000, 1) as b:
        b.set_polyphony(2)
        b.set_streams([chunks, chunks[:2]], instances=[1, 3], lane=1)            # a full ring, and one with room
        before = [s.copy() for s in b.get_streams(lane=1)]
        # truly full: refused whole, the voice with room untouched as well
        with pytest.raises(BatchError, match="The stream queue is full."):
            b.append_streams([chunks[:1], chunks[:1]], instances=[3, 1], lane=1)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(before, b.get_streams(lane=1)))
        assert b.get_stream_state(lane=1)[1].tolist() == [0, 8, 0, 1, 0]
        # the device takes three entries; the host still believes the ring full, reads the count back and finds room for exactly three
        device_render(b, 35)
        assert b.last_render_kernel() == "k_stream_rows"
        with pytest.raises(BatchError, match="The stream queue is full."):
            b.append_streams([chunks[:4]], instances=[1], lane=1)
        b.append_streams([chunks[:3]], instances=[1], lane=1)
        taken, queued = b.get_stream_state(lane=1)
        assert taken.tolist() == [0, 3, 0, 1, 0] and queued.tolist() == [0, 8, 0, 0, 0]
        got = b.get_streams(instances=[1], lane=1)[0]
        assert got[1:6].tobytes() == chunks[4:].tobytes() and got[6:].tobytes() == chunks[:3].tobytes()
        # the counters run on past the ring's length: 8 entries taken, 3 + 8 queued
        device_render(b, 200)
        taken, queued = b.get_stream_state(lane=1)
        assert taken.tolist() == [0, 11, 0, 1, 0] and not queued.any()
        # a dropped lane whose ring holds an entry is refused; an empty one goes
        b.append_streams([chunks[:1]], instances=[0], lane=1)
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use."):
            b.set_polyphony(1)
        device_render(b, 20)
        assert not b.get_stream_state(lane=1)[1].any() and not (b.get_samplers(lane=1)["flags"] & PLAYING).any()
        b.set_polyphony(1)
        b.set_polyphony(3)
        assert not b.get_stream_state(lane=2)[0].any()


def test_refusals_leave_the_streams_alone():
    rng = np.random.default_rng(6)
    chunks, assets, placed = one_voice(rng)
    with Batch(5, desc.FMT_STEREO, 48000, 1) as b:
        b.set_streams([chunks[:3]], instances=[4])
        before = b.get_streams()
        stopped = chunks[:3].copy()
        stopped["flags"][2] = 0
        glide = env(flags=vref.ACTIVE | vref.GLIDE)
        vref.glide(glide[0], ONE, 2 * ONE, 100)
        lp = np.zeros(1, desc_filter())
        lp["flags"], lp["b0"] = 1, 0.5
        outside = chunks[:2].copy()
        outside["frames"][1] = 2 ** 30       # (2 GiB: past the end of whatever allocation the chunk lies in)
        for call, message in ((lambda: b.set_streams([stopped], instances=[0]), "A queued sampler is not playing."),
                              (lambda: b.append_streams([stopped[2:]], instances=[4]), "A queued sampler is not playing."),
                              (lambda: b.set_streams([outside], instances=[0]), "does not lie inside one allocation"),
                              (lambda: b.set_streams([chunks[:2]], instances=[0], lane=1), "Lane out of range."),
                              (lambda: b.append_streams([chunks[:2]], instances=[0], lane=-1), "Lane out of range."),
                              (lambda: b.get_stream_state(lane=1), "Lane out of range."),
                              (lambda: b.set_envelopes(glide, instances=[4]), "The gliding voice streams.")):
            with pytest.raises(BatchError, match=message):
                call()
        b.set_envelopes(glide, instances=[1])
        with pytest.raises(BatchError, match="The streaming voice's envelope glides."):
            b.set_streams([chunks[:2]], instances=[1])
        with pytest.raises(BatchError, match="The streaming voice's envelope glides."):
            b.append_streams([chunks[:1]], instances=[1])
        b.set_streams([chunks[:1]], instances=[1])                                 # a stream of one may glide
        assert all(a.tobytes() == c.tobytes() for a, c in zip(before, b.get_streams()) if len(a) > 1)
        # a voice filter is taken while a voice streams, and a stream while a filter is ACTIVE: the render then has the filter stage
        b.set_filters(lp, instances=[0])
        device_render(b, 20)
        assert b.last_render_kernel() == "k_stream_filter_rows"
        b.append_streams([chunks[:1]], instances=[2])
        # once a state call has shown the ring empty, the voice may glide
        device_render(b, 300)
        assert b.last_render_kernel() == "k_stream_filter_rows"
        b.get_stream_state()
        b.set_envelopes(glide, instances=[4])
        device_render(b, 5)
        assert b.last_render_kernel() == "k_biquad_rows"


@pytest.mark.parametrize("kind", ["filters", "sweeps and filter programs", "with envelope programs"])
@pytest.mark.parametrize("channels", [2, 6])
def test_streams_under_filters_sweeps_and_filter_programs(channels, kind):
    """filter_program_cases' voices -- filtered without a sweep, swept, under filter programs whose switches fall inside the renders,
    unfiltered and idle ones beside them, in 2 or 3 lanes -- with most of them turned into streams of 2 .. 8 chunks: k_stream_filter_rows
    against the restatement, the filter stage over every voice's concatenated spans, the histories, the sweeps and their queues read back
    after every call.  "filters": no sweep is ever set, so the kernel gets no queue table of either kind."""
    case = fcases.build(channels, program=kind == "with envelope programs")
    rng = np.random.default_rng(600 + channels)
    pool = [p for _, _, p in case.pool]
    placed = GuardedPool(pool)
    streams, assets = scases.resolve_streams(scases.streams_of(rng, case.records, case.keys), pool, placed.bases)
    assert sum(len(s) > 1 for lane in streams for s in lane) >= 4
    with Batch(case.n, FORMAT[channels], 48000, 1) as b:
        pair = Pair(b, streams, case.programs, case.resamplers, {}, assets, filters=case.filters,
                    filter_programs=None if kind == "filters" else case.filter_programs)
        pair.expect_state("as set")
        for c, frames in enumerate((1, 63, 64, 65, 107, 300)):
            out = pair.render(frames, f"{channels} channels, {kind}, call {c}", offset=c % 2)
            assert not np.isnan(out).any(), "a guard frame was read"
        assert pair.taken.sum() >= 8


def test_api_array_streams(tmp_path):
    """tests/cpp/api_array_streams.cpp: ApiArray::set_stream, queue_sampler and stream_state against the batch calls, and
    oalsfx_host_stream_chunks' chunks against the whole asset."""
    exe = str(tmp_path / "api_array_streams")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_streams.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout


def desc_filter():
    from oalsfxpp_amd.api import FILTER_DTYPE
    return FILTER_DTYPE


def test_a_batch_without_streams_renders_the_parents_kernels():
    """Nothing of a batch on which no stream of two or more was set has changed: the ladder's kernels by name, and a stream of one is a
    plain sampler set."""
    rng = np.random.default_rng(8)
    chunks, assets, placed = one_voice(rng)
    ramp = env(flags=vref.ACTIVE)
    vref.ramp(ramp[0], [0.0, 0.0], [1.0, 1.0], 50)
    with Batch(6, desc.FMT_STEREO, 48000, 1) as b:
        b.set_streams([chunks[:1]], instances=[0])
        want, _ = sref.render_one(chunks[0], assets[stref.asset_key(chunks[0])], 20, 2)
        expect_output(device_render(b, 20)[0], want, "a stream of one")
        assert b.last_render_kernel() == "k_sampler_rows"
        b.set_envelopes(ramp, instances=[0])
        device_render(b, 5)
        assert b.last_render_kernel() == "k_voice_rows"
        set_tables(b, {0: ref.cubic(4)})
        b.set_resamplers([0], instances=[0])
        device_render(b, 5)
        assert b.last_render_kernel() == "k_fir_rows"
        b.set_polyphony(2)
        device_render(b, 5)
        assert b.last_render_kernel() == "k_mix_rows"
        assert not b.get_stream_state()[0].any() and not b.get_stream_state(lane=1)[1].any()
