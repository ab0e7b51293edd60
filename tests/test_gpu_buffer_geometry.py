"""The caller's buffer geometry on the device paths, bit-exact against the CPU oracle (outputs; effect state and delay lines of sampled
instances).

1. Multi-buffer passes (oalsfx_batch_mix_device_multi) at every shape the path accepts: buffer sizes that are not powers of two, so that a
   reverb block (256 frames) spans two buffers and a pass's last block is shorter than any call's; counts of buffers that split into
   uneven passes or fill the 32-entry buffer table; sampling rates other than 48 kHz; write positions off the cache-line grid; gains that
   are only nearly at rest; a group of two shards.
2. Buffers laid out the way callers lay them out -- slices of one tensor, one source for every call, in place -- and a property test of
   the overlap decision (one pass, or one call per buffer) over random layouts carved from one allocation.
3. Buffers at offsets into larger allocations, every channel count: a chained launch writes the caller's frames with 64-bit stores, so an
   output that is not 8-byte aligned must go in stream order (batch.cpp: chain_eligible); the bytes around it stay untouched."""
import math

import numpy as np
import pytest

from harness import preset_effect, same_bits
from oalsfxpp_amd import desc
from test_gpu_multi_buffer import E, MAX_CHUNK, Run, _torch, group_matches_one_batch

pytestmark = pytest.mark.gpu

# every multiple of 64 that is not a power of two below 2048, and the powers of two not yet tested; the count of buffers for each makes
# the passes split unevenly where it can (192 x 11: 10 + 1; 448 x 9: 4 + 4 + 1; 2048 x 3: 1 + 1 + 1)
COUNTS = {128: 17, 192: 11, 320: 7, 448: 9, 576: 4, 960: 3, 1024: 3, 1088: 2, 2048: 3}


def sample(n):
    """Instances a large batch is followed at: the first, a stride, and the last workgroup (four instances; the remainder where n % 4)."""
    return sorted(set([0, 1] + list(range(0, n, 97)) + list(range(4 * ((n - 1) // 4), n))))


def passes(frames, k):
    return math.ceil(k / (MAX_CHUNK // frames))


def multi_taking_the_pass(r, frames, k, label):
    """r.multi, asserting that the buffers went through ceil(k / (2048 / frames)) one-launch passes."""
    before = r.b.multi_counts()
    r.multi(frames, k, label=label)
    after = r.b.multi_counts()
    assert after == (before[0] + k, before[1] + passes(frames, k)), (label, before, after)
    assert r.b.last_reverb_kernel.startswith("k_reverb_steady_multi<"), r.b.last_reverb_kernel


def presets(n):
    return lambda b: b.set_effect(0, [preset_effect(i % 113) for i in range(n)])


# ---- 1. passes at every shape the path accepts ----

@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
@pytest.mark.parametrize("frames", sorted(COUNTS))
def test_passes_at_every_buffer_size(frames, fmt):
    """Default EAX reverb: an uneven split, then passes filled to the chunk.  Where frames is not a power of two, blocks span buffers."""
    r = Run(72, fmt, seed=frames * 8 + fmt)
    try:
        r.warm_up(frames)
        for k in (COUNTS[frames], MAX_CHUNK // frames):
            multi_taking_the_pass(r, frames, k, f"{k} x {frames}")
            r.check(state_sample=(0, 37, 71))
    finally:
        r.close()


def test_presets_at_odd_buffer_sizes():
    """Preset i % 113 (all three proven kinds) at buffer sizes whose blocks span buffers; the presets whose gains do not rest for the
    shorter blocks keep a size off the one-launch path, so some size, not every one, must take it."""
    n = 4096
    taken = []
    for frames in (192, 448):
        k = COUNTS[frames]
        r = Run(n, desc.FMT_STEREO, setup=presets(n), follow=sorted(set(sample(n) + [2, 57, 112])), seed=frames)
        try:
            r.warm_up(frames)
            before = r.b.multi_counts()
            r.multi(frames, k, label=f"presets {k} x {frames}")
            r.multi(frames, k, label=f"presets {k} x {frames}")
            after = r.b.multi_counts()
            if after != before:
                assert after == (before[0] + 2 * k, before[1] + 2 * passes(frames, k)), (frames, before, after)
                assert r.b.last_reverb_kernel.startswith("k_reverb_steady_multi<2,"), r.b.last_reverb_kernel
                taken.append(frames)
            r.check(state_sample=(0, 1, 2, 57, 112, n - 1))
        finally:
            r.close()
    assert taken, "neither 192- nor 448-frame buffers of the presets took the one-launch path"


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_the_buffer_table_filled_and_overrun_at_64_frames(fmt):
    """32 buffers of 64 frames fill the table of one pass exactly; 31, 33 and 65 end one short, one over and one over two full passes."""
    r = Run(72, fmt, seed=64 + fmt)
    try:
        r.warm_up(64)
        for k in (31, 32, 33, 65):
            multi_taking_the_pass(r, 64, k, f"{k} x 64")
            r.check(state_sample=(0, 36, 71))
    finally:
        r.close()


RATE_SIZES = {8000: 320, 22050: 576, 44100: 960, 96000: 192}


@pytest.mark.parametrize("rate", sorted(RATE_SIZES))
def test_default_reverb_at_other_rates(rate):
    """Exact whether or not a pass is taken; at 44.1 and 96 kHz (as at 48) the default EAX reverb takes it."""
    frames = RATE_SIZES[rate]
    k = COUNTS[frames]
    r = Run(72, desc.FMT_STEREO, seed=rate, rate=rate)
    try:
        for _ in range(3):
            r.single(frames, "warm-up")
        r.check()
        if rate in (44100, 96000):
            r.warm_up(frames)
            multi_taking_the_pass(r, frames, k, f"{rate} Hz")
        else:
            r.multi(frames, k, label=f"{rate} Hz")
        r.multi(frames, k, label=f"{rate} Hz")
        r.check(state_sample=(0, 35, 71))
    finally:
        r.close()


def test_presets_at_other_rates():
    """Every preset twice over (226 instances: the last workgroup holds two) at 8, 22.05, 44.1 and 96 kHz; exact whichever way each call
    goes, and some rate takes the pass."""
    n = 226
    taken = []
    for rate, frames in sorted(RATE_SIZES.items()):
        k = COUNTS[frames]
        r = Run(n, desc.FMT_STEREO, setup=presets(n), seed=rate + 1, rate=rate)
        try:
            for _ in range(3):
                r.single(frames, "warm-up")
            r.check()
            before = r.b.multi_counts()
            r.multi(frames, k, label=f"presets {rate} Hz")
            r.multi(frames, k, label=f"presets {rate} Hz")
            after = r.b.multi_counts()
            if after != before:
                taken.append(rate)
            r.check(state_sample=(0, 1, 2, 57, 112, n - 2, n - 1))
        finally:
            r.close()
    assert taken, "no rate's presets took the one-launch path"


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_off_grid_write_positions_with_blocks_across_buffers(fmt):
    """One 100-frame call puts the write positions off the 128-byte line grid: the passes then take the line-aligned build (CR == 2), with
    blocks that span buffers."""
    r = Run(72, fmt, seed=100 + fmt)
    try:
        r.warm_up(256)
        r.single(100, "odd size")
        r.check()
        r.warm_up(192, calls=1)
        for frames in (192, 448, 320):
            multi_taking_the_pass(r, frames, COUNTS[frames], f"off grid {COUNTS[frames]} x {frames}")
            assert r.b.last_reverb_kernel == f"k_reverb_steady_multi<{r.b.channels}, 2>", r.b.last_reverb_kernel
            r.check(state_sample=(0, 35, 71))
    finally:
        r.close()


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_gains_only_nearly_at_rest_through_passes(fmt):
    """The instances of test_gpu_proven.py's test_output_gains_that_never_reach_their_target (targets a few millionths from current
    gains that stay put for whole-tile blocks), through passes of 192-frame buffers: where a block boundary could still change a result."""
    tiny = [1e-6, 4e-6, 8e-6, 1.2e-5, 2e-5, 5e-5, 2e-4, 1e-3]
    groups = [[E(desc.EAX_REVERB, reflections_gain=g, late_reverb_gain=(g if k % 2 else 1.0)) for k, g in enumerate(tiny)],
              [E(desc.EAX_REVERB if k % 2 else desc.REVERB, reflections_gain=0.3, late_reverb_gain=g) for k, g in enumerate(tiny)]]
    taken = 0
    for j, effects in enumerate(groups):
        r = Run(len(effects), fmt, setup=lambda b, e=effects: b.set_effect(0, e), seed=j + fmt)
        try:
            r.warm_up(192)
            before = r.b.multi_counts()
            for _ in range(2):
                r.multi(192, 11, label=f"group {j}")
            taken += r.b.multi_counts()[1] - before[1]
            r.check(state_sample=range(len(effects)))
        finally:
            r.close()
    assert taken > 0, "no pass taken"


def test_group_of_two_shards_at_192_frames():
    group_matches_one_batch(72, 192, 11)


# ---- 2. buffer layouts and the overlap decision ----

def _layout_call(r, frames, srcs, dsts, expect_pass, label):
    k = len(srcs)
    before = r.b.multi_counts()
    r.b.mix_device_multi(frames, [s.data_ptr() for s in srcs], [d.data_ptr() for d in dsts])
    after = r.b.multi_counts()
    if expect_pass:
        assert after == (before[0] + k, before[1] + passes(frames, k)), (label, before, after)
        assert r.b.last_reverb_kernel.startswith("k_reverb_steady_multi<"), r.b.last_reverb_kernel
    else:
        assert after == before, (label, before, after)


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_buffers_sliced_from_one_tensor(fmt):
    """Contiguous buffers at a fixed stride, one source for every call, and in place: each one pass, equal to K calls in order."""
    torch = _torch()
    frames, k = 192, 11
    r = Run(72, fmt, seed=7 + fmt)
    try:
        r.warm_up(frames)
        xs = r.inputs(frames, k)
        src = torch.from_numpy(np.stack(xs)).cuda()
        dst = torch.empty_like(src)
        r.keep += [src, dst]
        _layout_call(r, frames, list(src), list(dst), True, "contiguous")
        r.expect(xs, list(dst), "contiguous")
        r.check(state_sample=(0, 71))

        (x,) = r.inputs(frames, 1)
        one = torch.from_numpy(x).cuda()
        dst = torch.empty((k,) + x.shape, dtype=torch.float32, device="cuda")
        r.keep += [one, dst]
        _layout_call(r, frames, [one] * k, list(dst), True, "one source")
        r.expect([x] * k, list(dst), "one source")
        r.check(state_sample=(0, 71))

        xs = r.inputs(frames, k)
        buf = torch.from_numpy(np.stack(xs)).cuda()
        r.keep.append(buf)
        _layout_call(r, frames, list(buf), list(buf), True, "in place")
        r.expect(xs, list(buf), "in place")
        r.check(state_sample=(0, 35, 71))
    finally:
        r.close()


def _overlap(a, b, size):
    return a < b + size and b < a + size


def _random_layout(rng, k, size, align):
    """2k ranges of `size` bytes at `align`-aligned offsets: packed one after another (touching exactly, or a few words apart), then --
    some of them -- moved onto another range (a source shared by two calls, a call in place, an output written twice) or partly over one
    (a call in place among them).
    A call's own source and output are the same range or apart (what a single call allows).  Returns (sources, outputs, bytes spanned)."""
    while True:
        placed, lo = [], 0
        for _ in range(2 * k):
            placed.append(lo)
            lo += size + int(rng.integers(0, 4)) * int(rng.integers(0, 3)) * align
        order = rng.permutation(2 * k)
        srcs = [placed[i] for i in order[:k]]
        dsts = [placed[i] for i in order[k:]]
        for _ in range(int(rng.integers(0, 4))):
            how, i, j = int(rng.integers(6)), int(rng.integers(k)), int(rng.integers(k))
            shift = int(rng.integers(1, size // align)) * align * (1 if rng.integers(2) else -1)
            near = min(max((srcs + dsts)[int(rng.integers(2 * k))] + shift, 0), lo)
            if how == 0:
                srcs[i] = srcs[j]                   # one source for two calls (apart)
            elif how == 1:
                srcs[i] = dsts[i]                   # in place (apart)
            elif how == 2:
                dsts[i] = dsts[j]                   # two calls write the same output
            elif how == 3:
                dsts[i] = near                      # an output partly over another range
            elif how == 4:
                srcs[i] = near                      # a source partly over another range
            elif i != j:
                # a call in place, and another call's source starting below it and reaching into it: at the in-place call's output
                # the sweep's last source is that call's own (the case for keeping the last two ranges of each kind)
                srcs[i] = dsts[i]
                srcs[j] = max(dsts[i] - abs(shift), 0)
        if all(s == d or not _overlap(s, d, size) for s, d in zip(srcs, dsts)):
            return srcs, dsts, lo + size


def _apart(srcs, dsts, size):
    """Brute force: no output of call i overlaps a source or an output of another call j."""
    k = len(srcs)
    return not any(_overlap(dsts[i], x, size) for i in range(k) for j in range(k) if j != i for x in (srcs[j], dsts[j]))


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_overlap_decision_on_random_layouts(fmt):
    """100 random layouts per format carved from one allocation (4-byte offsets, 8-byte for stereo): one pass exactly when the brute-force
    check finds the buffers apart, and always the K calls in order -- every byte of the allocation as the oracle's calls leave it (where
    two calls write the same bytes, the later one's)."""
    torch = _torch()
    n, frames = 8, 64
    r = Run(n, fmt, seed=3 + fmt)
    rng = np.random.default_rng(1000 + fmt)
    floats = n * frames * r.b.channels
    size, align = floats * 4, 4 * r.b.channels
    decided = {True: 0, False: 0}
    try:
        r.warm_up(frames)
        for layout in range(100):
            k = int(rng.integers(2, 8))
            srcs, dsts, space = _random_layout(rng, k, size, align)
            mem = rng.uniform(-1.0, 1.0, size=space // 4).astype(np.float32)
            dev = torch.from_numpy(mem).cuda()
            torch.cuda.synchronize()
            apart = _apart(srcs, dsts, size)
            decided[apart] += 1
            base = dev.data_ptr()
            before = r.b.multi_counts()
            r.b.mix_device_multi(frames, [base + s for s in srcs], [base + d for d in dsts])
            after = r.b.multi_counts()
            want = (before[0] + k, before[1] + 1) if apart else before
            assert after == want, (layout, srcs, dsts, before, after)
            for s, d in zip(srcs, dsts):
                x = mem[s // 4: s // 4 + floats].reshape(n, frames, r.b.channels).copy()
                mem[d // 4: d // 4 + floats] = r.army.mix(x).reshape(-1)
            r.b.synchronize()
            ok, nbad = same_bits(dev.cpu().numpy(), mem)
            assert ok, f"layout {layout} (apart: {apart}, sources {srcs}, outputs {dsts}, {size} bytes each): {nbad} floats differ"
        r.check(state_sample=(0, n - 1))
    finally:
        r.close()
    assert decided[True] >= 20 and decided[False] >= 20, decided


def test_outputs_of_one_multi_call_are_the_sources_of_the_next():
    """A -> B, B -> A, A -> B in one run on the batch's stream: each call's sources are the outputs of the call before (a feedback loop
    through the caller's buffers), which a chained launch must not read before they are written."""
    torch = _torch()
    n, frames, k = 72, 256, 8
    r = Run(n, desc.FMT_STEREO, seed=41)
    try:
        r.warm_up(frames)
        xs = r.inputs(frames, k)
        a, b = r.buffers(xs)
        chained = r.b.chained_calls
        r.b.mix_device_multi(frames, [s.data_ptr() for s in a], [d.data_ptr() for d in b])
        refs = [r.army.mix(x) for x in xs]
        assert r.b.chained_calls == chained + 1, "the first pass was expected to be a chained launch"
        outs = []
        for j, (src, dst) in enumerate(((b, a), (a, b))):
            r.b.mix_device_multi(frames, [s.data_ptr() for s in src], [d.data_ptr() for d in dst])
            refs = [r.army.mix(y) for y in refs]
            outs.append([ref.copy() for ref in refs])
        r.b.synchronize()
        torch.cuda.synchronize()
        for kk in range(k):
            assert not r.army.differing(b[kk].cpu().numpy(), outs[1][kk]), f"third call, buffer {kk}"
            assert not r.army.differing(a[kk].cpu().numpy(), outs[0][kk]), f"second call, buffer {kk}"
        r.pending, r.keep = [], []
        r.check(state_sample=(0, 35, 71))
    finally:
        r.close()


# ---- 3. offsets into larger allocations ----

GUARD = 64                  # floats of guard before and after the buffer
SENTINEL = 0x5A5AA5A5


def _at_offset(torch, floats, offset):
    """An allocation (int32, filled with SENTINEL) and the float view of `floats` floats at byte offset GUARD * 4 + `offset` into it."""
    assert offset % 4 == 0
    whole = torch.full((floats + 2 * GUARD + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    at = GUARD + offset // 4
    return whole, whole.view(torch.float32)[at: at + floats], at


def _guards_intact(whole, at, floats):
    w = whole.cpu().numpy().view(np.uint32)
    outside = np.concatenate([w[:at], w[at + floats:]])
    return int((outside != SENTINEL).sum())


OFFSET_CASES = [(desc.FMT_MONO, 4), (desc.FMT_QUAD, 4), (desc.FMT_5POINT1, 4), (desc.FMT_6POINT1, 4), (desc.FMT_7POINT1, 4),
                (desc.FMT_STEREO, 8)]


@pytest.mark.parametrize("fmt,offset", OFFSET_CASES + [(f, 0) for f, _ in OFFSET_CASES])
def test_buffers_at_an_offset_into_a_larger_allocation(fmt, offset):
    """mix_device and mix_device_multi with source and output at `offset` bytes past a 256-byte boundary: 4 for mono and more than two
    channels (allowed; not 8-byte aligned, so in stream order), 8 for stereo (8-byte aligned, not 16 or 128), 0 the aligned control.
    Outputs exact, the bytes around each output untouched; chained launches only where the output is 8-byte aligned."""
    torch = _torch()
    n, frames = 4096, 256
    r = Run(n, fmt, follow=sample(n), seed=fmt * 16 + offset)
    floats = n * frames * r.b.channels
    try:
        r.warm_up(frames)
        chained = r.b.chained_calls
        outputs = []
        for call in range(5):
            k = 1 if call < 3 else 3
            xs = r.inputs(frames, k)
            srcs, dsts = [], []
            for x in xs:
                s_whole, s, _ = _at_offset(torch, floats, offset)
                s.copy_(torch.from_numpy(x.reshape(-1)))
                d_whole, d, at = _at_offset(torch, floats, offset)
                assert d.data_ptr() % 8 == offset % 8 and (offset == 0 or d.data_ptr() % 16 != 0)
                r.keep += [s_whole, d_whole]
                srcs.append(s)
                dsts.append(d)
                outputs.append((d_whole, at))
            torch.cuda.synchronize()
            if k == 1:
                r.b.mix_device(frames, srcs[0].data_ptr(), dsts[0].data_ptr())
            else:
                r.b.mix_device_multi(frames, [s.data_ptr() for s in srcs], [d.data_ptr() for d in dsts])
            r.expect(xs, [d.view(n, frames, r.b.channels) for d in dsts], f"call {call} at +{offset}")
        r.check(state_sample=(0, 97, n - 1))
        for j, (whole, at) in enumerate(outputs):
            bad = _guards_intact(whole, at, floats)
            assert not bad, f"output {j}: {bad} guard words around it overwritten"
        if offset % 8:
            assert r.b.chained_calls == chained, "an output that is not 8-byte aligned went into a chained launch"
        else:
            assert r.b.chained_calls > chained, "the aligned shape did not chain: the test would not see the guard"
    finally:
        r.close()
