"""GPU parity of the multi-buffer entry point (oalsfx_batch_mix_device_multi): K queued device buffers of one size go through
as few launches as the batch's instances allow, and the result is bit-identical to K consecutive mix_device calls -- outputs, effect
state and delay lines, against the CPU oracle.  Every buffer is an allocation of its own, with inputs of its own (seeded noise), and
the buffers are handed in out of address order: a pass that read the wrong buffer, or assumed a stride between them, fails.

Where the one-launch path cannot be taken (a changed instance, two slots, a send filter, a ragged size, buffers that overlap) the call
falls back to one ordinary call per buffer; the debug counter (oalsfx_batch_multi_counts) tells the two apart."""
import ctypes as C
import math

import numpy as np
import pytest

from harness import ShadowArmy, make_effect, preset_effect, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch, Group

pytestmark = pytest.mark.gpu

E = make_effect
MAX_CHUNK = 2048


def _torch():
    import torch
    return torch


class Run:
    """A batch, an oracle for every followed instance, and device buffers that live until the run is checked."""

    def __init__(self, n, fmt, effect_count=1, setup=None, follow=None, seed=0, rate=48000):
        self.b = Batch(n, fmt, rate, effect_count)
        if setup is None:
            self.b.set_effect(0, E(desc.EAX_REVERB))
        else:
            setup(self.b)
        self.b.apply_changes()
        self.army = ShadowArmy(self.b, follow)
        self.rng = np.random.default_rng(seed)
        self.pending = []   # (device output, oracle output of the followed instances, label), in call order
        self.keep = []      # device buffers of calls not checked yet

    def inputs(self, frames, count):
        return [self.rng.uniform(-1.0, 1.0, size=(self.b.n, frames, self.b.channels)).astype(np.float32) for _ in range(count)]

    def buffers(self, xs):
        """Device copies of `xs` and as many outputs: separate allocations (with gaps between them), handed out in descending address
        order -- buffer k is never at a fixed stride from buffer k - 1."""
        torch = _torch()
        allocs = []
        for x in xs:
            allocs.append(torch.empty(x.shape, dtype=torch.float32, device="cuda"))
            allocs.append(torch.empty(x.shape, dtype=torch.float32, device="cuda"))
            self.keep.append(torch.empty(64 * 1024 + 17, dtype=torch.float32, device="cuda"))
        allocs.sort(key=lambda t: -t.data_ptr())
        srcs, dsts = allocs[0::2], allocs[1::2]
        for x, s in zip(xs, srcs):
            s.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        self.keep += allocs
        return srcs, dsts

    def expect(self, xs, dsts, label):
        for k, (x, d) in enumerate(zip(xs, dsts)):
            self.pending.append((d, self.army.mix(x), f"{label} buffer {k}"))

    def single(self, frames, label="single"):
        (x,) = self.inputs(frames, 1)
        (s,), (d,) = self.buffers([x])
        self.b.mix_device(frames, s.data_ptr(), d.data_ptr())
        self.expect([x], [d], label)

    def multi(self, frames, k, stream=None, label="multi"):
        xs = self.inputs(frames, k)
        srcs, dsts = self.buffers(xs)
        self.b.mix_device_multi(frames, [s.data_ptr() for s in srcs], [d.data_ptr() for d in dsts], stream=stream)
        self.expect(xs, dsts, label)

    def check(self, state_sample=(0,)):
        torch = _torch()
        self.b.synchronize()
        torch.cuda.synchronize()
        for d, ref, label in self.pending:
            y = d.cpu().numpy()
            bad = self.army.differing(y, ref)
            assert not bad, f"{label}: instances differ (instance, samples): {bad[:8]}"
        self.pending, self.keep = [], []
        for i in state_sample:
            s = self.army.shadows[self.army.instances.index(i)]
            d = s.compare_state()
            assert not d, f"instance {i}: " + "; ".join(d[:4])

    def warm_up(self, frames, calls=3):
        """Ordinary calls until the device has proven every instance steady (what the one-launch path needs)."""
        for _ in range(6):
            for _ in range(calls):
                self.single(frames, "warm-up")
            self.check()
            if self.b.plan(0)[1] == self.b.n:
                return
        raise AssertionError(f"not every instance proven steady after the warm-up: plan {self.b.plan(0)}")

    def close(self):
        self.b.close()


@pytest.mark.parametrize("n", [72, 4096])
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
@pytest.mark.parametrize("frames", [64, 256])
def test_one_pass_parity(n, fmt, frames):
    """Each dst_k bit-identical to the oracle's call k; state and rings of sampled instances too; the counter shows the passes (K = 11
    at 256 frames crosses a pass boundary: 8 + 3)."""
    r = Run(n, fmt, seed=n + frames + fmt)
    try:
        r.warm_up(frames)
        for k in (2, 8, 11):
            before = r.b.multi_counts()
            r.multi(frames, k, label=f"K={k}")
            after = r.b.multi_counts()
            assert after[0] - before[0] == k, (before, after)
            assert after[1] - before[1] == math.ceil(k * frames / MAX_CHUNK), (before, after)
            assert r.b.last_reverb_kernel.startswith("k_reverb_steady_multi<"), r.b.last_reverb_kernel
            r.check(state_sample=(0, n // 2 + 1, n - 1))
    finally:
        r.close()


def test_presets_every_kind_and_off_grid_positions():
    """Preset i % 113 on instance i covers the three proven kinds (plain, close taps, short taps / modulated).  After one call of an odd
    size the write positions are off the 128-byte line grid: the pass then takes the plain kind's line-aligned build (CR == 2)."""
    n = 4096
    r = Run(n, desc.FMT_STEREO, setup=lambda b: b.set_effect(0, [preset_effect(i % 113) for i in range(n)]), seed=5)
    try:
        r.warm_up(256)
        before = r.b.multi_counts()
        r.multi(256, 8, label="presets")
        assert r.b.multi_counts()[1] == before[1] + 1
        assert r.b.last_reverb_kernel == "k_reverb_steady_multi<2, 0>", r.b.last_reverb_kernel
        r.check(state_sample=(0, 1, 2, 57, 112, 4095))
        r.single(100, "odd size")
        r.check()
        r.warm_up(256, calls=1)
        before = r.b.multi_counts()
        r.multi(256, 8, label="off grid")
        assert r.b.multi_counts()[1] == before[1] + 1
        assert r.b.last_reverb_kernel == "k_reverb_steady_multi<2, 2>", r.b.last_reverb_kernel
        r.check(state_sample=(0, 1, 2, 57, 112, 4095))
    finally:
        r.close()


def test_presets_with_the_calls_blocks_shorter_than_the_pass_blocks():
    """The presets again (all three proven kinds: plain, close taps, short taps / modulated), now with buffers shorter than the reverb's
    256-frame blocks: a pass's blocks then end where no call's does, which the modulator's index, the hot record and the carried filter
    histories of every build must not notice.  64-frame buffers where every preset's gains rest for one-tile blocks, else 128."""
    n = 4096
    taken = []
    for frames in (64, 128):
        r = Run(n, desc.FMT_STEREO, setup=lambda b: b.set_effect(0, [preset_effect(i % 113) for i in range(n)]), seed=7 + frames)
        try:
            r.warm_up(frames)
            k = MAX_CHUNK // frames
            before = r.b.multi_counts()
            r.multi(frames, k, label=f"presets {k} x {frames}")
            r.multi(frames, k, label=f"presets {k} x {frames}")
            after = r.b.multi_counts()
            if after != before:
                assert after == (before[0] + 2 * k, before[1] + 2), (frames, before, after)
                assert r.b.last_reverb_kernel.startswith("k_reverb_steady_multi<2,"), r.b.last_reverb_kernel
                taken.append(frames)
            r.check(state_sample=(0, 1, 2, 3, 57, 112, 4095))
        finally:
            r.close()
    assert taken, "neither 64- nor 128-frame buffers of the presets took the one-launch path"


@pytest.mark.parametrize("frames", [2112, 4096])
def test_buffers_longer_than_a_chunk_fall_back(frames):
    """A pass is one chunk of at most 2048 frames: buffers longer than that go one call each (chunked like any call), the counter stays
    put, and outputs, state and delay lines are those of the single calls -- for the calls after them too."""
    r = Run(72, desc.FMT_STEREO, seed=frames)
    try:
        r.warm_up(frames)
        before = r.b.multi_counts()
        r.multi(frames, 1, label="one long buffer")
        r.multi(frames, 2, label="two long buffers")
        r.check(state_sample=(0, 35, 71))
        assert r.b.multi_counts() == before, (before, r.b.multi_counts())
        r.warm_up(256, calls=1)
        r.multi(256, 8, label="after the long buffers")
        assert r.b.multi_counts() == (before[0] + 8, before[1] + 1), (before, r.b.multi_counts())
        r.check(state_sample=(0, 35, 71))
    finally:
        r.close()


def _two_slots(b):
    b.set_effect(0, E(desc.EAX_REVERB))
    b.set_effect(1, E(desc.CHORUS))


@pytest.mark.parametrize("case", ["property_change", "two_slots", "send_filter", "ragged", "dst0_is_src1"])
def test_fallbacks_stay_exact(case):
    n = 72
    r = Run(n, desc.FMT_STEREO, effect_count=2 if case == "two_slots" else 1, setup=_two_slots if case == "two_slots" else None, seed=11)
    torch = _torch()
    try:
        frames = 480 if case == "ragged" else 256
        for _ in range(3):
            r.single(frames, "warm-up")
        r.check()
        if case in ("property_change", "send_filter", "dst0_is_src1"):
            r.warm_up(frames)
            before = r.b.multi_counts()
            r.multi(frames, 4, label="one pass")
            assert r.b.multi_counts()[1] == before[1] + 1
            r.check()
        before = r.b.multi_counts()
        if case == "property_change":
            r.b.set_effect(0, E(desc.EAX_REVERB, decay_time=2.5), first=3, count=1)
            r.b.apply_changes()
        if case == "send_filter":
            r.b.set_send_props(0, 1.0, 0.5, 1.0, first=5, count=1)
            r.b.apply_changes()
            # every instance proven again, the filter on: the send filter alone keeps the call off the one-launch path
            r.warm_up(frames)
            before = r.b.multi_counts()
        if case == "dst0_is_src1":
            # buffer 1 reads what buffer 0 wrote: K sequential calls see it, one pass could not
            xs = r.inputs(frames, 2)
            srcs, dsts = r.buffers(xs)
            r.b.mix_device_multi(frames, [srcs[0].data_ptr(), dsts[0].data_ptr()], [dsts[0].data_ptr(), dsts[1].data_ptr()])
            r.b.synchronize()
            y0 = dsts[0].cpu().numpy()
            ref0 = r.army.mix(xs[0])
            ref1 = r.army.mix(y0)
            assert not r.army.differing(y0, ref0)
            assert not r.army.differing(dsts[1].cpu().numpy(), ref1)
            r.pending, r.keep = [], []
        else:
            r.multi(frames, 4, label=case)
            assert r.b.multi_counts() == before, (case, before, r.b.multi_counts())
            r.multi(frames, 3, label=case)
            r.check(state_sample=(0, 3, 5))
        if case != "property_change":
            # (a changed instance is proven again once its cross-fade is through and the device has said so: the calls of the fallback
            # get it there, and a later multi call may take the one-launch path again)
            assert r.b.multi_counts() == before, (case, before, r.b.multi_counts())
        torch.cuda.synchronize()
    finally:
        r.close()


def test_explicit_stream_takes_the_one_pass_path_in_stream_order():
    torch = _torch()
    r = Run(72, desc.FMT_STEREO, seed=17)
    try:
        r.warm_up(256)
        s = torch.cuda.Stream()
        before = r.b.multi_counts()
        r.multi(256, 8, stream=s.cuda_stream, label="stream")
        r.multi(256, 11, stream=s.cuda_stream, label="stream")
        assert r.b.multi_counts() == (before[0] + 19, before[1] + 3)
        s.synchronize()
        r.check(state_sample=(0, 71))
    finally:
        r.close()


@pytest.mark.parametrize("n", [72, 4096])
def test_single_and_multi_calls_alternate_in_one_run(n):
    """mix_device and mix_device_multi alternating without a wait in between (one chained run on the batch's stream)."""
    r = Run(n, desc.FMT_STEREO, follow=None if n <= 128 else range(0, n, 7), seed=23)
    try:
        r.warm_up(256)
        before = r.b.multi_counts()
        for j in range(6):
            r.single(256, f"single {j}")
            r.multi(256, 3 + j, label=f"multi {j}")
        assert r.b.multi_counts()[0] == before[0] + sum(3 + j for j in range(6))
        r.check(state_sample=(0, n - 1 - (n - 1) % 7))
    finally:
        r.close()


def test_group_of_two_shards_matches_one_batch():
    group_matches_one_batch(72, 256, 8)


def group_matches_one_batch(n, frames, k):
    """A Group of two shards on one device, fed mix_device_multi, against one Batch fed the same buffers one mix_device call each."""
    torch = _torch()
    g = Group(n, [0, 0], desc.FMT_STEREO)
    one = Batch(n, desc.FMT_STEREO)
    try:
        for x in (g, one):
            x.set_effect(0, E(desc.EAX_REVERB))
            x.apply_changes()
        rng = np.random.default_rng(29)
        for call in range(8):
            xs = [rng.uniform(-1.0, 1.0, size=(n, frames, 2)).astype(np.float32) for _ in range(k)]
            dx = [torch.from_numpy(x).cuda() for x in xs]
            dy_one = [torch.empty_like(d) for d in dx]
            parts = [[(d[first:first + count].clone(), torch.empty((count, frames, 2), dtype=torch.float32, device="cuda")) for d in dx]
                     for (_, first, count) in g.shards]
            torch.cuda.synchronize()
            for kk in range(k):
                one.mix_device(frames, dx[kk].data_ptr(), dy_one[kk].data_ptr())
            g.mix_device_multi(frames, [[p[0].data_ptr() for p in shard] for shard in parts], [[p[1].data_ptr() for p in shard] for shard in parts])
            one.synchronize()
            g.synchronize()
            torch.cuda.synchronize()
            for kk in range(k):
                got = torch.cat([parts[d][kk][1] for d in range(len(parts))]).cpu().numpy()
                ok, nbad = same_bits(got, dy_one[kk].cpu().numpy())
                assert ok, f"call {call} buffer {kk}: {nbad} samples differ"
        # the shards' batches took the one-launch path once their instances were proven
        so = lib.load()
        for d in range(len(g.shards)):
            bufs, passes = C.c_longlong(0), C.c_longlong(0)
            assert so.oalsfx_batch_multi_counts(so.oalsfx_group_batch(g._h, d), C.byref(bufs), C.byref(passes))
            assert bufs.value > 0 and passes.value > 0, (d, bufs.value, passes.value)
    finally:
        g.close()
        one.close()
