"""GPU parity of calls that join a queued launch: a chained launch that sits behind a gate of its own takes the plain
mix_device calls that arrive before the gate lets it go, as further buffers of its table.  Whatever joins, every buffer's output, then
effect state and delay lines, must be bit-identical to the same calls made one by one -- against the CPU oracle.

When the gate closes depends on the device, so the test hook (Batch.join_hold) makes the groupings deterministic: a joinable launch is
queued only once it has k buffers or something closes it.  oalsfx_batch_join_counts then says exactly what happened.  One test runs
without the hook and must be right whatever joined."""
import math
import os

import numpy as np
import pytest

from harness import ShadowArmy, make_effect, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch

pytestmark = pytest.mark.gpu

E = make_effect
MAX_CHUNK = 2048
CHAIN_ALWAYS = 0x8000   # OALSFX_DEBUG_FLAGS: chained launches for short calls of small batches too (the 64-frame cases)


def _torch():
    import torch
    return torch


@pytest.fixture(autouse=True)
def chain_short_calls():
    so = lib.load()
    base = int(os.environ.get("OALSFX_DEBUG_FLAGS", "0"), 0)
    so.oalsfx_debug_set_flags(base | CHAIN_ALWAYS)
    yield
    so.oalsfx_debug_set_flags(base)


class Run:
    """A batch, an oracle for every followed instance, and device buffers that live until the run is checked."""

    def __init__(self, n, fmt, follow=None, seed=0):
        self.b = Batch(n, fmt, 48000, 1)
        self.b.set_effect(0, E(desc.EAX_REVERB))
        self.b.apply_changes()
        self.army = ShadowArmy(self.b, follow)
        self.rng = np.random.default_rng(seed)
        self.queue = []     # (input, device output, label, compare?) of calls the oracle has not followed yet, in call order
        self.pending = []   # (device output, oracle output of the followed instances, label)
        self.keep = []

    def input(self, frames):
        return self.rng.uniform(-1.0, 1.0, size=(self.b.n, frames, self.b.channels)).astype(np.float32)

    def device(self, x):
        torch = _torch()
        t = torch.from_numpy(x).cuda()
        self.keep.append(t)
        return t

    def out(self, frames):
        torch = _torch()
        t = torch.empty((self.b.n, frames, self.b.channels), dtype=torch.float32, device="cuda")
        self.keep.append(t)
        return t

    def call(self, frames, x=None, src=None, dst=None, label="call", expect=True):
        """One plain mix_device call on the batch's own stream.  (The input is complete on the device before the call is made: a joined
        call may be consumed before calls queued earlier have finished.)  The oracle follows in `check`, in call order: it reads the
        batch's descriptors back, which would end the run."""
        torch = _torch()
        if x is None:
            x = self.input(frames)
        if src is None:
            src = self.device(x)
            torch.cuda.synchronize()
        if dst is None:
            dst = self.out(frames)
        self.b.mix_device(frames, src.data_ptr(), dst.data_ptr())
        self.queue.append((x, dst, label, expect))
        return dst

    def calls(self, frames, count, label="call"):
        """`count` calls back to back: the inputs are on the device first, nothing between two calls that would slow the host down."""
        torch = _torch()
        xs = [self.input(frames) for _ in range(count)]
        srcs = [self.device(x) for x in xs]
        dsts = [self.out(frames) for _ in range(count)]
        torch.cuda.synchronize()
        for k, (x, s, d) in enumerate(zip(xs, srcs, dsts)):
            self.b.mix_device(frames, s.data_ptr(), d.data_ptr())
            self.queue.append((x, d, f"{label} {k}", True))

    def oracle(self):
        """The oracle's turn for every call made so far; returns its outputs for them."""
        refs = []
        for x, d, label, expect in self.queue:
            refs.append(self.army.mix(x))
            if expect:
                self.pending.append((d, refs[-1], label))
        self.queue = []
        return refs

    def check(self, state_sample=(0,)):
        torch = _torch()
        self.b.synchronize()
        torch.cuda.synchronize()
        refs = self.oracle()
        for d, ref, label in self.pending:
            bad = self.army.differing(d.cpu().numpy(), ref)
            assert not bad, f"{label}: instances differ (instance, samples): {bad[:8]}"
        self.pending, self.keep = [], []
        for i in state_sample:
            s = self.army.shadows[self.army.instances.index(i)]
            d = s.compare_state()
            assert not d, f"instance {i}: " + "; ".join(d[:4])
        return refs

    def warm_up(self, frames, calls=3):
        """Ordinary calls until the device has proven every instance steady (what a joinable launch needs)."""
        for _ in range(6):
            for _ in range(calls):
                self.call(frames, label="warm-up")
            self.check()
            if self.b.plan(0)[1] == self.b.n:
                return
        raise AssertionError(f"not every instance proven steady after the warm-up: plan {self.b.plan(0)}")

    def close(self):
        self.b.close()


def grouped(calls, k):
    """(joined calls, joinable launches) of `calls` back-to-back calls after a synchronize, held to groups of k: the run's first two
    launches take nobody (the first has no gate, the second is not worth a table), every launch after them is joinable and takes k - 1
    (the last what is left)."""
    launches = math.ceil((calls - 2) / k)
    return (calls - 2) - launches, launches


def delta(r, before):
    after = r.b.join_counts()
    return after[0] - before[0], after[1] - before[1]


@pytest.mark.parametrize("n", [6, 70])
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
@pytest.mark.parametrize("frames,k", [(256, 2), (256, 3), (256, 8), (64, 32)])
def test_groupings_with_distinct_outputs(n, fmt, frames, k):
    r = Run(n, fmt, seed=n + frames + k + fmt)
    try:
        r.warm_up(frames)
        r.b.join_hold(k)
        before = r.b.join_counts()
        calls = 2 + 2 * k + 1   # the run's first two, two full launches, one that the synchronize closes at a single buffer
        r.calls(frames, calls, label=f"{k} x {frames}")
        assert r.b.last_reverb_kernel.startswith("k_reverb_steady_joined<"), r.b.last_reverb_kernel
        r.check(state_sample=(0, n // 2 + 1, n - 1))
        assert delta(r, before) == grouped(calls, k), (before, r.b.join_counts())
        assert r.b.multi_counts() == (0, 0)
    finally:
        r.close()


@pytest.mark.parametrize("n,fmt", [(6, desc.FMT_STEREO), (70, desc.FMT_MONO), (70, desc.FMT_STEREO)])
def test_one_output_buffer_and_eight_inputs_in_turn(n, fmt):
    """What bench.py does: eight inputs used in turn, every call into the same output buffer.  The buffer holds the last call's output,
    and state and delay lines say that every call before it happened, in order."""
    torch = _torch()
    r = Run(n, fmt, seed=n + fmt)
    try:
        r.warm_up(256)
        xs = [r.input(256) for _ in range(8)]
        srcs = [r.device(x) for x in xs]
        dst = r.out(256)
        torch.cuda.synchronize()
        r.b.join_hold(8)
        before = r.b.join_counts()
        calls = 21
        for j in range(calls):
            r.call(256, x=xs[j % 8], src=srcs[j % 8], dst=dst, label="the last call's output", expect=j == calls - 1)
        r.check(state_sample=(0, n - 1))
        assert delta(r, before) == grouped(calls, 8), (before, r.b.join_counts())
    finally:
        r.close()


def test_eight_inputs_in_turn_distinct_outputs():
    r = Run(70, desc.FMT_STEREO, seed=31)
    torch = _torch()
    try:
        r.warm_up(256)
        xs = [r.input(256) for _ in range(8)]
        srcs = [r.device(x) for x in xs]
        torch.cuda.synchronize()
        r.b.join_hold(3)
        before = r.b.join_counts()
        for j in range(17):
            r.call(256, x=xs[j % 8], src=srcs[j % 8], label=f"call {j}")
        r.check(state_sample=(0, 35, 69))
        assert delta(r, before) == grouped(17, 3)
    finally:
        r.close()


def test_the_ninth_call_starts_a_new_launch():
    """A table holds OALSFX_MAX_CHUNK frames: the launch is full with eight 256-frame buffers, whatever the hook asks for."""
    r = Run(70, desc.FMT_STEREO, seed=41)
    try:
        r.warm_up(256)
        r.b.join_hold(12)
        before = r.b.join_counts()
        r.calls(256, 2 + 9)
        # the run's first two; a launch of eight; the ninth call in a launch of its own
        assert delta(r, before) == (7, 2), (before, r.b.join_counts())
        r.check(state_sample=(0, 69))
    finally:
        r.close()


def test_a_property_change_between_two_calls():
    """A launch that brings an upload is closed at birth (the upload kernel is its gate), and while the changed instance is not proven
    again no launch is joinable.  Once it is, calls join again."""
    r = Run(70, desc.FMT_STEREO, seed=43)
    try:
        r.warm_up(256)
        r.b.join_hold(3)
        before = r.b.join_counts()
        r.calls(256, 4)          # the run's first two, a launch of two so far (held)
        r.oracle()               # (the oracle reads the batch's descriptors as they are now; the read-back closes the held launch)
        assert delta(r, before) == (1, 1), (before, r.b.join_counts())
        r.b.set_effect(0, E(desc.EAX_REVERB, decay_time=2.5), first=3, count=1)
        r.b.apply_changes()
        # The first call brings the upload.  The second and third find the changed instance not proven -- or proven again by a read-back
        # that has just come in, and then bring the rebuilt lists, an upload again: none of their launches is joinable, none of them joins.
        r.calls(256, 2)
        assert delta(r, before) == (1, 1), (before, r.b.join_counts())
        r.check(state_sample=(0, 3, 69))
        r.b.join_hold(0)
        r.warm_up(256)
        r.b.join_hold(3)
        before = r.b.join_counts()
        r.calls(256, 7)
        assert delta(r, before) == grouped(7, 3), (before, r.b.join_counts())
        r.check(state_sample=(0, 3, 69))
    finally:
        r.close()


def test_instances_not_yet_proven_do_not_join():
    """A fresh batch: its second call is a chained launch behind a gate of its own, but nothing is proven yet, so it takes nobody.  (When
    the device's word that the instances have settled is looked at depends on timing: from the third call on a launch may be joinable,
    but only with every instance proven.)"""
    r = Run(70, desc.FMT_STEREO, seed=47)
    try:
        r.b.join_hold(3)
        r.calls(256, 2)
        assert r.b.join_counts() == (0, 0)
        r.calls(256, 4)
        if r.b.join_counts()[1] > 0:
            assert r.b.plan(0)[1] == r.b.n, r.b.plan(0)
        r.check(state_sample=(0, 69))
    finally:
        r.close()


def test_an_output_that_partially_overlaps_an_earlier_one():
    """Call k + 1 writes where call k wrote, half a buffer further on: it must not join (one instance's frames would land where another
    wavefront writes another's), and memory ends as the two calls in order leave it."""
    torch = _torch()
    n, frames = 70, 256
    r = Run(n, desc.FMT_STEREO, seed=53)
    try:
        r.warm_up(frames)
        floats = n * frames * 2
        big = torch.zeros(floats + floats // 2, dtype=torch.float32, device="cuda")
        d1, d2 = big[:floats], big[floats // 2:]
        r.b.join_hold(4)
        before = r.b.join_counts()
        r.call(frames, label="the run's first")
        r.call(frames, label="the run's second")
        x1, x2 = r.input(frames), r.input(frames)
        r.call(frames, x=x1, dst=d1, expect=False)   # joinable, held
        r.call(frames, x=x2, dst=d2, expect=False)   # overlaps: no join
        assert delta(r, before)[0] == 0, (before, r.b.join_counts())
        *_, ref1, ref2 = r.check(state_sample=(0, 69))
        got = big.cpu().numpy()
        assert list(r.army.instances) == list(range(n))
        want = np.concatenate([ref1.reshape(-1)[:floats // 2], ref2.reshape(-1)])
        ok, nbad = same_bits(got, want)
        assert ok, f"{nbad} samples differ from the two calls in order"
    finally:
        r.close()


def test_an_input_that_is_an_earlier_output_of_the_run():
    torch = _torch()
    r = Run(70, desc.FMT_STEREO, seed=59)
    try:
        r.warm_up(256)
        r.b.join_hold(4)
        before = r.b.join_counts()
        r.call(256, label="the run's first")
        r.call(256, label="the run's second")
        x = r.input(256)
        s = r.device(x)
        torch.cuda.synchronize()
        d1, d2 = r.out(256), r.out(256)
        r.b.mix_device(256, s.data_ptr(), d1.data_ptr())    # joinable, held
        r.b.mix_device(256, d1.data_ptr(), d2.data_ptr())   # reads what the call before writes: stream order, no join
        assert delta(r, before) == (0, 1), (before, r.b.join_counts())
        r.b.synchronize()
        r.oracle()
        y1 = d1.cpu().numpy()
        ref1 = r.army.mix(x)
        ref2 = r.army.mix(y1)
        assert not r.army.differing(y1, ref1)
        assert not r.army.differing(d2.cpu().numpy(), ref2)
        r.check(state_sample=(0, 69))
    finally:
        r.close()


def test_a_call_of_another_size_does_not_join():
    r = Run(70, desc.FMT_STEREO, seed=61)
    try:
        r.warm_up(256)
        r.warm_up(128, calls=1)
        r.b.join_hold(4)
        before = r.b.join_counts()
        r.calls(256, 4)          # the run's first two, a launch of two so far
        r.calls(128, 1)          # closes it; a launch of its own
        r.calls(256, 2)          # another size again: a launch of its own, and one call that joins it
        j, l = delta(r, before)
        assert j == 2 and l >= 2, (before, r.b.join_counts())
        r.check(state_sample=(0, 69))
    finally:
        r.close()


def test_a_read_back_in_mid_run():
    r = Run(70, desc.FMT_STEREO, seed=67)
    try:
        r.warm_up(256)
        r.b.join_hold(4)
        before = r.b.join_counts()
        r.calls(256, 4)                  # the run's first two, a launch of two so far (held)
        r.b.read_slot(5, 0)              # ends the run: the held launch goes out with its two buffers
        assert delta(r, before) == (1, 1)
        r.calls(256, 7)                  # a new run: its first two, then a launch of four and one of one
        assert delta(r, before) == (1 + 3, 1 + 2), (before, r.b.join_counts())
        r.check(state_sample=(0, 5, 69))
    finally:
        r.close()


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_write_positions_off_the_line_grid(fmt):
    """After one 37-frame call every ring store begins and ends inside a cache line: the joinable launch takes the plain kind's
    line-aligned build (CR == 2) too."""
    r = Run(70, fmt, seed=71 + fmt)
    try:
        r.warm_up(256)
        r.call(37, label="37 frames")
        r.check()
        r.warm_up(256, calls=1)
        r.b.join_hold(3)
        before = r.b.join_counts()
        r.calls(256, 8)
        assert r.b.last_reverb_kernel == f"k_reverb_steady_joined<{r.b.channels}, 2>", r.b.last_reverb_kernel
        assert delta(r, before) == grouped(8, 3)
        r.check(state_sample=(0, 35, 69))
    finally:
        r.close()


def test_the_flag_that_switches_joining_off():
    so = lib.load()
    base = int(os.environ.get("OALSFX_DEBUG_FLAGS", "0"), 0) | CHAIN_ALWAYS
    r = Run(70, desc.FMT_STEREO, seed=73)
    try:
        r.warm_up(256)
        so.oalsfx_debug_set_flags(base | 0x1000)
        r.b.join_hold(3)
        chained = r.b.chained_calls
        before = r.b.join_counts()   # (the warm-up's calls may have joined)
        r.calls(256, 7)
        assert delta(r, before) == (0, 0)
        assert r.b.chained_calls - chained == 7     # (chained launches as ever)
        r.check(state_sample=(0, 69))
    finally:
        so.oalsfx_debug_set_flags(base)
        r.close()


def test_late_joins_without_the_hook():
    """No hook: what joins is up to the device and the host's pace.  1024 instances, 24 calls back to back, every 37th instance against
    the oracle: right whatever joined.  The counts are recorded, not asserted."""
    n = 1024
    r = Run(n, desc.FMT_STEREO, follow=range(0, n, 37), seed=79)
    try:
        r.warm_up(256)
        before = r.b.join_counts()
        r.calls(256, 24)
        r.check(state_sample=(0, 37 * 27))
        j, l = delta(r, before)
        print(f"late joins: {j} of 24 calls joined {l} joinable launches")
        assert 0 <= j <= 22 and j + l <= 22
    finally:
        r.close()
