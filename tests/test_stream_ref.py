"""CPU: the sampler streams' restatement (tests/stream_ref.py) against the properties the contract states (include/oalsfx_hip.h, "sampler
streams"), so that what the device is held against is itself held against something: a stream of chunks plays the whole asset's bits;
every split of the frames gives one result; a render equals the hand-made split with a plain sampler set at each take; an intro and its
loop; a ring that runs dry and is refilled.  And four wrong forms a device could take -- the overshoot dropped, the take a frame late,
the take moved to the 64-frame tile boundary, the take moved to the render boundary (the best a caller can do without streams) -- each
fail on the committed cases; where one coincides with the right form, the coincidence is asserted as a stated blind spot."""
import numpy as np
import pytest

import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import stream_cases as scases
import stream_ref as stref
import voice_ref as vref
from test_voice_abi import env

f32 = np.float32
ONE = sref.ONE
NONE_ENV = [env()[0]]
WHOLE = "whole"      # the key of a chunked asset's whole PCM in random_chunked's table


def play(stream, assets, sizes, channels, program=NONE_ENV, coef=None, wrong=None, taken=0):
    """The renders of `sizes` frames one after the other: (outputs joined, the stream afterwards, taken, the program afterwards, the
    frames of the takes counted from the first render's start)."""
    outs, takes, t0 = [], [], 0
    for frames in sizes:
        out, stream, taken, program, at = stref.render_voice(stream, taken, program, coef, assets, frames, channels, wrong)
        outs.append(out)
        takes += [t0 + t for t in at]
        t0 += frames
    return np.concatenate(outs), stream, taken, program, takes


def random_chunked(rng, channels=2):
    """A random asset of 50 .. 400 frames as one record and as 2 .. 8 chunks, at a random step of 1 .. 16383 and a random start inside the
    first chunk: (whole record, chunk records, assets)."""
    frames = int(rng.integers(50, 401))
    fmt = int(rng.integers(0, 3))
    width = int(rng.choice([1, channels]))
    pool = [cases.asset(rng, fmt, width, frames)]
    pieces = int(rng.integers(2, 9))
    at = np.sort(rng.choice(np.arange(1, frames), pieces - 1, replace=False))
    if rng.random() < 0.4:
        at = int(rng.integers(1, frames - pieces)) + np.arange(pieces - 1)       # chunks of one frame in a row
    lengths = np.diff(np.concatenate([[0], at, [frames]])).tolist()
    record = scases.whole(pool, 0, fmt, step=int(rng.integers(1, 16384)), position=int(rng.integers(0, lengths[0] << 12)),
                          gain=rng.uniform(-1, 1, sref.MAX_CHANNELS).astype(f32))
    assets = {}
    bases = scases.fake_bases(pool)
    # (the whole record and the first chunk share an address: the table holds the chunks, the whole asset is WHOLE)
    whole = scases.resolve([record], pool, bases, {})[0]
    chunks = scases.resolve(stref.chunks(record, lengths), pool, bases, assets)
    assets[WHOLE] = pool[0]
    return whole, chunks, assets


def random_sizes(rng, total):
    sizes = []
    while sum(sizes) < total:
        sizes.append(int(rng.integers(1, 701)))
    return sizes


def test_chunks_play_the_whole_asset():
    """300 random cases, renders of 1 .. 700 frames until the asset has ended at any step: outputs, the final position and PLAYING are
    sampler_ref's for the whole asset.  Steps above a chunk's length (chunks shorter than one step) are among them, and asserted to be."""
    rng = np.random.default_rng(20)
    skipped = 0
    for case in range(300):
        record, chunks, assets = random_chunked(rng)
        total = (int(record["frames"]) << 12) // int(record["step"]) + 5
        sizes = random_sizes(rng, min(total, 3000))
        want, state = [], record
        for frames in sizes:
            out, state = sref.render_one(state, assets[WHOLE], frames, 2)
            want.append(out)
        got, stream, taken, _, takes = play(chunks, assets, sizes, 2)
        assert sref.same_floats(got, np.concatenate(want))[0], f"case {case}: the chunks do not play the whole asset's bits"
        skipped += len(takes) != len(set(takes))
        if not int(state["flags"]) & sref.PLAYING:
            assert taken == len(chunks) - 1 and len(stream) == 1 and not int(stream[0]["flags"]) & sref.PLAYING
            assert int(stream[0]["position"]) == int(stream[0]["frames"]) << 12
    assert skipped > 20, "no case chained through a chunk shorter than a step"


def named(channels=2):
    names, streams, programs, resamplers, pool, appends = scases.named_streams(channels)
    bases = scases.fake_bases(pool)
    streams, assets = scases.resolve_streams(streams, pool, bases)
    appends = {c: [(k, i, scases.resolve(e, pool, bases, assets)) for k, i, e in v] for c, v in appends.items()}
    return names, streams, programs, resamplers, assets, appends


def run_named(sizes_between, wrong=None):
    """The named voices through renders that add up to stream_cases.CALLS' ends, `sizes_between[c]` the split of call c, the appends behind
    the calls they follow: (out [n][total][2], streams, taken, programs)."""
    names, streams, programs, resamplers, assets, appends = named()
    taken = np.zeros((scases.LANES, scases.INSTANCES), np.uint32)
    tables = cases.tables()
    outs = []
    for c, sizes in enumerate(sizes_between):
        assert sum(sizes) == scases.CALLS[c]
        for frames in sizes:
            out, streams, taken, programs = stref.render(streams, taken, programs, resamplers, tables, assets, frames, 2, wrong)
            outs.append(out)
        for k, i, entries in appends.get(c, ()):
            streams[k][i] = stref.append(streams[k][i], entries)
            assert streams[k][i] is not None
    return np.concatenate(outs, axis=1), streams, taken, programs


def same_state(a, b):
    return (all(x.tobytes() == y.tobytes() for la, lb in zip(a[1], b[1]) for x, y in zip(la, lb)) and a[2].tobytes() == b[2].tobytes() and
            all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for la, lb in zip(a[3], b[3]) for x, y in zip(la, lb)))


def test_every_split_gives_one_result():
    """The named voices: the committed calls, every call in one-frame renders, and random splits, the appends at the same frames: outputs,
    records, taken counts, rings and envelope programs agree."""
    whole = run_named([(c,) for c in scases.CALLS])
    assert sref.same_floats(whole[0], run_named([(1,) * c for c in scases.CALLS])[0])[0]
    rng = np.random.default_rng(3)
    for _ in range(3):
        split = []
        for c in scases.CALLS:
            at = np.sort(rng.choice(np.arange(1, c), min(c - 1, int(rng.integers(0, 4))), replace=False)) if c > 1 else []
            split.append(tuple(np.diff(np.concatenate([[0], at, [c]])).astype(int).tolist()))
        other = run_named(split)
        assert sref.same_floats(whole[0], other[0])[0] and same_state(whole, other)


def test_what_the_named_voices_do():
    names, streams, programs, resamplers, assets, appends = named()
    out, after, taken, p_after = run_named([(c,) for c in scases.CALLS])
    # takes at 64, 128, 129, 130, 131, 168 and 512
    _, _, _, _, takes = play(streams[0][0], assets, (sum(scases.CALLS),), 2)
    assert takes == [64, 128, 129, 130, 131, 168, 512] and taken[0][0] == 7
    # the loop holds the entry behind it
    assert len(after[0][3]) == 2 and int(after[0][3][0]["flags"]) & sref.LOOP and taken[0][3] == 1
    # the chain went dry inside the first calls and was restarted by the append behind call 4; the idle voice was started by an append
    assert taken[0][4] == 9 and taken[0][5] == 3
    silent, idle, none, _, _ = play(streams[0][5], assets, (1,), 2)
    sound, _, one, _, at = play(stref.append(idle, appends[0][0][2]), assets, (63,), 2)
    assert not silent.any() and none == 0 and sound[0].any() and at[0] == 0 and one >= 1, "the idle voice starts with the first frame behind its append"
    # the STOP fade stopped the voice in its second chunk, the third is held
    assert taken[1][2] == 1 and len(after[1][2]) == 2 and not int(after[1][2][0]["flags"]) & sref.PLAYING
    # the envelope program ran through while the chunks were taken
    assert len(p_after[1][3]) == 1 and taken[1][3] == 2


def test_a_render_is_the_hand_made_split():
    """Voices without an envelope: the render cut at the takes, each span a plain sampler render, the next entry set by hand at its
    position plus the excess P + s * step - E of the span in front of it; chains resolved by hand as well."""
    rng = np.random.default_rng(77)
    for case in range(60):
        record, chunks, assets = random_chunked(rng)
        if case % 3 == 0:
            chunks["flags"] |= sref.LINEAR
        if case % 5 == 0:
            chunks["position"][1:] = rng.integers(0, ONE, len(chunks) - 1)       # queued positions other than 0
        frames = min((int(record["frames"]) << 12) // int(record["step"]) + 5, 2500)
        got, stream, taken, _, takes = play(chunks, assets, (frames,), 2)
        current, ring, t, pieces, over = chunks[0].copy(), list(chunks[1:]), 0, [], 0
        for at in sorted(set(takes)) + [frames]:
            span = at - t
            if span:
                excess = int(current["position"]) + span * int(current["step"]) - stref.end_of(current)
                out, current = sref.render_one(current, assets.get(stref.asset_key(current)), span, 2)
                pieces.append(out)
                over, t = max(excess, 0), at
            while ring and stref.at_end(current) and takes.count(at) > 0:
                takes.remove(at)
                current = ring.pop(0).copy()
                start = int(current["position"]) + over
                over = max(start - stref.end_of(current), 0)
                current["position"] = min(start, stref.end_of(current))
                if start >= stref.end_of(current):
                    current["flags"] = int(current["flags"]) & ~sref.PLAYING
        assert sref.same_floats(got, np.concatenate(pieces))[0], f"case {case}"
        assert stream[0].tobytes() == current.tobytes() and len(stream) == 1 + len(ring)


def test_the_ring_runs_dry_and_is_refilled():
    rng = np.random.default_rng(5)
    record, chunks, assets = random_chunked(rng)
    chunks["step"] = ONE
    chunks[0]["position"] = 0
    total = int(record["frames"])
    out, stream, taken, _, _ = play(chunks, assets, (total + 40,), 2)
    assert taken == len(chunks) - 1 and len(stream) == 1 and stref.at_end(stream[0]) and not out[total:].any()
    # appended to the dry voice: it starts at the next render's frame 0, with no excess carried over the gap
    again = stref.append(stream, chunks[:2])
    out2, stream, taken, _, takes = play(again, assets, (10,), 2, taken=taken)
    first, _ = sref.render_one(chunks[0], assets[stref.asset_key(chunks[0])], 10, 2)
    assert takes[0] == 0 and sref.same_floats(out2[:min(10, int(chunks[0]["frames"]))], first[:min(10, int(chunks[0]["frames"]))])[0]
    assert taken == len(chunks) and stref.append(np.zeros(1 + stref.QUEUE, sref.DTYPE), chunks[:1]) is None


@pytest.mark.parametrize("wrong", ["dropped", "late", "tile", "render"])
def test_a_wrong_form_fails_on_the_committed_cases(wrong):
    right = run_named([(c,) for c in scases.CALLS])
    other = run_named([(c,) for c in scases.CALLS], wrong)
    differ = [i for i in range(scases.INSTANCES) if not sref.same_floats(right[0][i], other[0][i])[0]]
    assert differ, f"the wrong form '{wrong}' gives the named voices' outputs"
    # the stated blind spots
    names, streams, programs, resamplers, assets, appends = named()
    total = sum(scases.CALLS)
    if wrong == "dropped":
        # step 4096 from an integer position: every excess is 0, nothing to drop
        a, b = play(streams[0][0], assets, (total,), 2), play(streams[0][0], assets, (total,), 2, wrong=wrong)
        assert sref.same_floats(a[0], b[0])[0] and a[1].tobytes() == b[1].tobytes()
        a, b = play(streams[0][1], assets, (total,), 2), play(streams[0][1], assets, (total,), 2, wrong=wrong)
        assert not sref.same_floats(a[0], b[0])[0]
    if wrong == "tile":
        # takes that fall on 64-frame boundaries coincide: the first two chunks of the first voice
        two = streams[0][0][:3]
        a, b = play(two, assets, (150,), 2), play(two, assets, (150,), 2, wrong=wrong)
        assert a[4] == [64, 128] and sref.same_floats(a[0], b[0])[0]
    if wrong == "render":
        # a take on a render's last frame coincides: the first chunk ends with the second committed call
        two = streams[0][0][:2]
        a, b = play(two, assets, (1, 63, 20), 2), play(two, assets, (1, 63, 20), 2, wrong=wrong)
        assert sref.same_floats(a[0], b[0])[0]
