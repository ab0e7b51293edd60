"""GPU: call sequences over the whole voice stack -- the five record tables behind one set/get path, the FIR tables, set_polyphony and the
seven-rung launch ladder of sampler_queue -- against the host model of tests/stack_model.py, whose renders are program_ref.render's.
Renders go to the batch's stream and to a caller's, most of them not waited for; every output is compared on its bits (NaNs by
position) at the next point that waits, every read-back on its bytes, and the kernel launched and the five upload counters after every
render.  There is no tolerance anywhere.  No test provokes a device fault: every refusal is decided on the host before anything is
queued.  tests/test_stack_model.py checks the sequences themselves, and the kernels' host build against the model, without a GPU."""
import re

import numpy as np
import pytest

import stack_model as sm
from downmix_ref import downmix
from harness import same_bits
from oalsfxpp_amd.api import Batch, BatchError
from test_gpu_biquad import expect_filters
from test_gpu_programs import expect_programs
from test_gpu_resample import FORMAT, set_tables
from test_gpu_sampler import GUARD, Assets, expect_output, expect_same_bytes
from test_gpu_voice import expect_envelope_bytes

pytestmark = pytest.mark.gpu
f32 = np.float32
N_BUSES, THRESHOLD = 2, f32(1e-4)
COUNTERS = dict(samplers="sampler_uploads", envelopes="envelope_uploads", resamplers="resampler_uploads", filters="filter_uploads", programs="program_uploads")


def _torch():
    import torch
    return torch


class Replay:
    """One batch that replays one script's calls, one call per step(); a twin batch serves only mix() for the plays.  The renders'
    buffers, with their guards of -7.5, are all made and filled before the first call: nothing here waits between two calls that the
    script does not make wait."""

    def __init__(self, script, fmt, side, name=""):
        torch = _torch()
        self.s, self.side, self.name = script, side, name
        self.n, self.ch = script.n, script.channels
        self.assets = script.assets
        self.b, self.twin = Batch(self.n, fmt, 48000, 1), Batch(self.n, fmt, 48000, 1)
        self.bus, self.gain = np.arange(self.n) % N_BUSES, np.linspace(0.3, 1.0, self.n).astype(f32)
        self.b.set_routing(self.bus, self.gain)
        set_tables(self.b, script.initial_tables)
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
            expect_output(host[first:first + count].reshape(self.n, op["frames"], self.ch), op["want"], f"{label}: {what}")
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
        if kind in sm.SETS or kind in ("set_fir_table", "set_polyphony"):
            if kind == "set_fir_table":
                call = lambda: b.set_fir_table(op["table"], op["data"])
            elif kind == "set_polyphony":
                call = lambda: b.set_polyphony(op["to"])
            elif kind == "set_envelopes":
                call = lambda: b.set_envelopes(np.concatenate(op["data"]), **where)
            elif kind == "set_env_programs":
                call = lambda: b.set_env_programs(list(op["data"]), **where)
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
            want = op["want"]
            if kind == "get_samplers":
                expect_same_bytes(got, want, label)
            elif kind == "get_envelopes":
                expect_envelope_bytes(got, want, label)
            elif kind == "get_filters":
                assert got.dtype == want.dtype and not sm.records_differ(got, want), f"{label}: the filters differ at {sm.records_differ(got, want)}"
            elif kind == "get_resamplers":
                assert (got == want).all(), label
            else:
                assert [len(p) for p in got] == [len(p) for p in want], f"{label}: the programs' lengths"
                assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), f"{label}: the programs differ"

    def finish(self):
        """All five tables read back against the model."""
        s, b = self.s, self.b
        label = f"{self.name}at the end"
        self.settle(label)
        assert self.at == len(s.ops) and b.polyphony == s.lanes
        expect_programs(b, s.rec, s.prog, label)
        expect_filters(b, s.filt, label)
        for k in range(s.lanes):
            expect_same_bytes(b.get_samplers(lane=k), s.rec[k], f"{label}, lane {k}")
            assert (b.get_resamplers(lane=k) == s.res[k]).all(), f"{label}: the resamplers of lane {k}"
        assert {table: count - self.base[table] for table, count in self.counters().items()} == s.uploads, label


def script_on_the_device(seed, n, channels, lanes_max, **kw):
    pool = sm.pool_for(seed, channels)
    assets = Assets(pool)
    initial = dict(sm.cases.tables())
    s = sm.build(seed, n, channels, lanes_max, pool, [assets.address(k) for k in range(len(pool))], **kw)
    s.assets, s.initial_tables = assets, initial
    return s


@pytest.mark.parametrize("channels, n, lanes_max, seed", sm.SHAPES)
def test_call_sequences_follow_the_stack_model(channels, n, lanes_max, seed):
    """Some 130 calls in a seeded order over samplers, envelopes, programs, resamplers, filters, FIR tables and the polyphony, on subsets
    and on all instances, in both lane forms; renders of 1 to 300 frames on both streams, most not waited for, 0, 1 and 2 floats off
    their allocation; plays; read-backs of every table.  stack_model.present() names the sixteen stretches every sequence holds;
    tests/test_stack_model.py asserts that it does.  Stereo at 9 instances and up to 4 lanes (a partial third workgroup, 2- and 4-float
    stores), 5.1 at 5 and 3 (the 2-float and the scalar path), 7.1 and 6.1 at 4 and 2 (the filtered program kernel at its register
    ceiling)."""
    torch = _torch()
    s = script_on_the_device(seed, n, channels, lanes_max)
    missing = [what for what, there in sm.present(s.ops).items() if not there]
    assert not missing, missing
    replay = Replay(s, FORMAT[channels], torch.cuda.Stream())
    try:
        for _ in s.ops:
            replay.step()
        replay.finish()
    finally:
        replay.close()


def test_two_batches_interleaved_on_one_callers_stream():
    """Two batches replay two different sequences of some thirty calls, call by call in turn, their side renders on the same caller's
    stream: each follows its own model.  State that had leaked into something the batches share would show."""
    torch = _torch()
    side = torch.cuda.Stream()
    scripts = [script_on_the_device(seed, 5, 2, 3, only=sm.SHORT) for seed in (21, 22)]
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
