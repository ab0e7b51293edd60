"""GPU: call sequences over the whole voice stack as it stands now -- the samplers with their streams, the envelopes with their programs,
the resamplers, the voice filters with their sweeps and filter programs, set_polyphony and the thirteen-rung launch ladder of
sampler_queue -- against the host model of tests/stream_stack_model.py, whose renders are stream_ref.render's.  Renders go to the batch's
stream and to a caller's, most of them not waited for; every output is compared on its bits (NaNs by position) at the next point that
waits, every read-back on its bytes, and the kernel launched and the seven upload counters after every render.  There is no tolerance
anywhere.  The assets lie between guard frames of NaN or full scale: a frame read outside an asset shows.  No test provokes a device
fault: every refusal is decided on the host before anything is queued, and stream_stack_model.check_bounds has walked every sequence.
tests/test_stream_stack_model.py checks the sequences themselves, and the kernels' host builds against the model, without a GPU."""
import re

import numpy as np
import pytest

import stream_stack_model as ssm
from downmix_ref import downmix
from harness import same_bits
from oalsfxpp_amd.api import Batch, BatchError
from test_gpu_resample import FORMAT, set_tables
from test_gpu_sampler import GUARD
from test_gpu_streams import GuardedPool

pytestmark = pytest.mark.gpu
f32 = np.float32
N_BUSES, THRESHOLD = 2, f32(1e-4)
COUNTERS = dict(samplers="sampler_uploads", envelopes="envelope_uploads", resamplers="resampler_uploads", filters="filter_uploads", programs="program_uploads",
                sweeps="sweep_uploads", filter_programs="filter_program_uploads")


def _torch():
    import torch
    return torch


def same_lists(got, want):
    return [len(g) for g in got] == [len(w) for w in want] and all(np.asarray(g).tobytes() == np.asarray(w, dtype=g.dtype).tobytes() for g, w in zip(got, want))


class Replay:
    """One batch that replays one script's calls, one call per step(); a twin batch serves only mix() for the plays.  The renders'
    buffers, with their guards of -7.5, are all made and filled before the first call: nothing here waits between two calls that the
    script does not make wait."""

    def __init__(self, script, fmt, side, name=""):
        torch = _torch()
        self.s, self.side, self.name = script, side, name
        self.n, self.ch = script.n, script.channels
        self.b, self.twin = Batch(self.n, fmt, 48000, 1), Batch(self.n, fmt, 48000, 1)
        self.bus, self.gain = np.arange(self.n) % N_BUSES, np.linspace(0.3, 1.0, self.n).astype(f32)
        self.b.set_routing(self.bus, self.gain)
        set_tables(self.b, script.tables)
        self.buffers = {k: torch.full((GUARD + op["offset"] + self.n * op["frames"] * self.ch + GUARD,), -7.5, dtype=torch.float32, device="cuda")
                        for k, op in enumerate(script.ops) if op["kind"] == "render"}
        torch.cuda.synchronize()
        self.base = self.counters()
        self.queued, self.at = [], 0

    def close(self):
        """(whatever is still queued has run before the batches, the buffers and the assets go)"""
        self.b.synchronize()
        self.side.synchronize()
        self.b.close()
        self.twin.close()

    def counters(self):
        return {table: getattr(self.b, name)() for table, name in COUNTERS.items()}

    def settle(self, label):
        torch = _torch()
        self.b.synchronize()
        self.side.synchronize()
        torch.cuda.synchronize()
        for k, what in self.queued:
            op = self.s.ops[k]
            host, first, count = self.buffers.pop(k).cpu().numpy(), GUARD + op["offset"], self.n * op["frames"] * self.ch
            assert (host[:first] == -7.5).all() and (host[first + count:] == -7.5).all(), f"{label}: {what} wrote outside its buffer"
            got = host[first:first + count].reshape(self.n, op["frames"], self.ch)
            assert not np.isnan(got).any(), f"{label}: {what} read a guard frame"
            bad = ssm.bits_differ(got, op["want"])
            assert not bad, f"{label}: {what} ({op['frames']} frames, {op['kernel']}) differs at (instance, frame, channel) {bad}"
        del self.queued[:]

    def rendered(self, op, label):
        assert self.b.last_render_kernel() == op["kernel"], f"{label}: {self.b.last_render_kernel()} launched, not {op['kernel']}"
        moved = {table: count - self.base[table] for table, count in self.counters().items()}
        assert moved == op["uploads"], f"{label}: the upload counters are {moved}, not {op['uploads']}"

    def step(self):
        k, op = self.at, self.s.ops[self.at]
        self.at += 1
        b, kind = self.b, op["kind"]
        label = f"{self.name}call {k} ({kind})"
        where = dict(instances=op.get("rows"))
        if op.get("lane_form"):
            where["lane"] = op["lane"]
        if kind in ssm.SETS or kind == "set_polyphony":
            if kind == "set_polyphony":
                call = lambda: b.set_polyphony(op["to"])
            elif kind in ("set_envelopes", "set_sweeps"):
                call = lambda: getattr(b, kind)(np.concatenate(op["data"]), **where)
            elif kind in ("set_env_programs", "set_filter_programs", "set_streams", "append_streams"):
                call = lambda: getattr(b, kind)(list(op["data"]), **where)
            else:
                call = lambda: getattr(b, kind)(op["data"], **where)
            if op["refused"]:
                with pytest.raises(BatchError, match=re.escape(op["refused"])):
                    call()
            else:
                call()
        elif kind == "render":
            b.sample_device(op["frames"], self.buffers[k].data_ptr() + 4 * (GUARD + op["offset"]), stream=self.side.cuda_stream if op["side"] else None)
            self.rendered(op, label)
            self.queued.append((k, f"the render of call {k}"))
            if op["wait"]:
                self.settle(label)
        elif kind == "play":
            got, _, _ = b.play_downmix_meter(op["frames"], N_BUSES, THRESHOLD)
            self.rendered(op, label)
            self.settle(label)
            ok, nbad = same_bits(got, downmix(self.twin.mix(op["want"]), self.bus, self.gain, N_BUSES))
            assert ok, f"{label}: {nbad} bus samples differ"
        else:
            got = getattr(b, kind)(**where)
            self.settle(label)
            self.compare(kind, got, op["want"], label)

    def compare(self, kind, got, want, label):
        if kind in ("get_streams", "get_env_programs", "get_filter_programs"):
            assert same_lists(got, want), f"{label}: got {[len(g) for g in got]} records, want {[len(w) for w in want]}, or their bytes differ"
        elif kind == "get_stream_state":
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), f"{label}: (taken, queued) is {got}, not {want}"
        elif kind == "get_resamplers":
            assert (got == want).all(), label
        else:
            want = np.asarray(want, dtype=got.dtype)
            assert not ssm.records_differ(got, want), f"{label}: the records differ at {ssm.records_differ(got, want)}"

    def finish(self):
        """All eight tables and the stream state of every lane read back against the model."""
        s, b = self.s, self.b
        self.settle(f"{self.name}at the end")
        assert self.at == len(s.ops) and b.polyphony == s.lanes
        every = range(s.n)
        for k in range(s.lanes):
            label = f"{self.name}at the end, lane {k}"
            self.compare("get_samplers", b.get_samplers(lane=k), s.rec[k], label + ": samplers")
            self.compare("get_streams", b.get_streams(lane=k), s.streams[k], label + ": streams")
            self.compare("get_stream_state", b.get_stream_state(lane=k), (s.taken[k], s.ring_queued[k] - s.taken[k]), label)
            self.compare("get_envelopes", b.get_envelopes(lane=k), np.array([s.prog[k][i][0] for i in every]), label + ": envelopes")
            self.compare("get_env_programs", b.get_env_programs(lane=k), [np.array(s.prog[k][i]) for i in every], label + ": envelope programs")
            self.compare("get_resamplers", b.get_resamplers(lane=k), s.res[k], label + ": resamplers")
            self.compare("get_filters", b.get_filters(lane=k), s.filt[k], label + ": filters")
            self.compare("get_sweeps", b.get_sweeps(lane=k), np.array([s.fprog[k][i][0] for i in every]), label + ": sweeps")
            self.compare("get_filter_programs", b.get_filter_programs(lane=k), [np.array(s.fprog[k][i]) for i in every], label + ": filter programs")
        assert {table: count - self.base[table] for table, count in self.counters().items()} == s.uploads, f"{self.name}at the end"


def script_on_the_device(seed, n, channels, lanes_max, pool=None, placed=None, **kw):
    pool = pool or ssm.pool_for(seed, channels)
    placed = placed or GuardedPool([pcm for _, _, pcm in pool])
    s = ssm.build(seed, n, channels, lanes_max, pool, placed.bases, **kw)
    s.placed = placed
    ssm.check_bounds(s.ops)
    return s


@pytest.mark.parametrize("channels, n, lanes_max, seed", ssm.SHAPES)
def test_call_sequences_follow_the_stream_stack_model(channels, n, lanes_max, seed):
    """Some 325 calls in a seeded order over all eight tables and the polyphony, every set and get call on subsets and on all instances
    and in both lane forms; renders of 1 to 300 frames on both streams, more than four in five not waited for, 0, 1 and 2 floats off
    their allocation; plays; read-backs of every table.  stream_stack_model.present() names the stretches every sequence holds; tests/test_stream_stack_model.py asserts that
    it does.  Stereo at 9 instances and up to 4 lanes (a partial third workgroup, 2- and 4-float stores), 5.1 at 5 and 3, 7.1 and 6.1
    at 4 and 2 (6.1: k_stream_rows<7, 1>, the variant at its register ceiling), mono at 3 instances, rendered at one lane (the store
    sink) but for the polyphony stretch and the ladder's k_mix_rows rung, which need a second."""
    torch = _torch()
    s = script_on_the_device(seed, n, channels, lanes_max)
    missing = [what for what, there in ssm.present(s.ops).items() if not there]
    assert not missing, missing
    replay = Replay(s, FORMAT[channels], torch.cuda.Stream())
    try:
        for _ in s.ops:
            replay.step()
        replay.finish()
    finally:
        replay.close()


def test_two_batches_interleaved_on_one_callers_stream():
    """Two batches replay two different sequences of some 55 calls, call by call in turn, their side renders on the same caller's
    stream and their records over the same pool of assets: each follows its own model.  State that had leaked into something the batches
    share would show."""
    torch = _torch()
    side = torch.cuda.Stream()
    pool = ssm.pool_for(41, 2)
    placed = GuardedPool([pcm for _, _, pcm in pool])
    scripts = [script_on_the_device(seed, 5, 2, 3, pool=pool, placed=placed, only=ssm.SHORT) for seed in (41, 42)]
    assert [op["kind"] for op in scripts[0].ops] != [op["kind"] for op in scripts[1].ops]
    replays = [Replay(s, FORMAT[2], side, name=f"batch {k}, ") for k, s in enumerate(scripts)]
    try:
        for k in range(max(len(s.ops) for s in scripts)):
            for r in replays:
                if r.at < len(r.s.ops):
                    r.step()
        for r in replays:
            r.finish()
    finally:
        for r in replays:
            r.close()
