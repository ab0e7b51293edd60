"""CPU: the samplers' records at the ends of their 64-bit range -- positions past 2^32, steps up to 2^32 - 1, one-shots that end on the
last frame of a tile, loops of one frame and of a whole long asset, record fields the render must leave alone -- as case families that
tests/test_gpu_sampler.py plays on the device.  Here: an independent scalar model (tests/sampler_model.py) agrees with the restatement
(tests/sampler_ref.py) on every family, bit for bit; every family reaches what it claims to reach; and deliberately wrong restatements
are caught by the family aimed at them -- no GPU needed."""
import ast
import functools
import os

import numpy as np
import pytest

import sampler_model as model
import sampler_ref as ref
from test_sampler_abi import random_records, rec

f32 = np.float32
ONE = ref.ONE
H = 1 << 20                     # the frame whose position is 2^32
N = H + 5000                    # frames of a long asset
TWO32 = 1 << 32
SPLIT = [1, 63, 512, 513]       # the calls that follow a case's own, continuing it
TILE = {1: 512, 2: 512, 4: 256, 6: 256, 7: 256, 8: 256}        # frames of one pass of a wavefront (Ahead<C> of sampler.hip, times 64)
ENDING_FRAMES = [255, 256, 257, 511, 512, 513, 1024, 1025]
ADDRESS_OFFSETS = [1, 3, 5]     # elements between an allocation's start and the asset in it: the GPU test places the assets so
LARGE_STEPS = [(1 << 23) + 1, (1 << 31) + 12345, (1 << 32) - 1]
IDLE_GAINS = np.asarray([0x7FC12345, 0x80000000, 0x00000123, 0x7F800000], np.uint32)     # a NaN with a payload, -0.0, a denormal, Inf
PLAY, LOOP, LIN = ref.PLAYING, ref.LOOP, ref.LINEAR


@functools.lru_cache(maxsize=None)
def long_assets():
    """The three long assets, made once: 16-bit stereo, 8-bit mono and fp32 mono of N frames; and the 16-bit one read as a mono asset of
    2 N frames, which is the same memory."""
    rng = np.random.default_rng(2032)
    s16 = rng.integers(-32768, 32768, (N, 2)).astype(np.int16)
    u8 = rng.integers(0, 256, (N, 1)).astype(np.uint8)
    fp = rng.standard_normal((N, 1)).astype(f32)
    s16[-1], u8[-1], fp[-1] = (12345, -23456), 200, 0.75           # the last frame is not silence: a neighbour read past it shows
    return {"s16 stereo": (ref.PCM_S16, s16), "s16 mono": (ref.PCM_S16, s16.reshape(-1, 1)), "u8": (ref.PCM_U8, u8), "f32": (ref.PCM_F32, fp)}


def long_pool(channels):
    """[(format, PCM)]: the long assets a batch of `channels` channels can play."""
    a = long_assets()
    return [a["s16 stereo" if channels == 2 else "s16 mono"], a["u8"], a["f32"]]


@functools.lru_cache(maxsize=None)
def small_assets(channels):
    """Small assets: 16-bit of the batch's width, 16-bit stereo, 8-bit mono and fp32 of 8 channels."""
    rng = np.random.default_rng(77 + channels)
    return {"s16 wide": (ref.PCM_S16, rng.integers(-32768, 32768, (5000, channels)).astype(np.int16)),
            "s16 stereo": (ref.PCM_S16, rng.integers(-32768, 32768, (900, 2)).astype(np.int16)),
            "u8": (ref.PCM_U8, rng.integers(0, 256, (901, 1)).astype(np.uint8)),
            "f32 x8": (ref.PCM_F32, rng.standard_normal((333, 8)).astype(f32))}


def collect(channels, seed, entries):
    """entries: [((format, PCM), fields)] -> (records, assets); gains are random, `data` is left to whoever places the assets."""
    rng = np.random.default_rng(seed)
    records, assets = [], []
    for (fmt, pcm), fields in entries:
        r = rec(format=fmt, frames=pcm.shape[0], channels=pcm.shape[1], data=0, **fields)
        r["gain"][0, :] = 0
        r["gain"][0, :channels] = rng.uniform(-1.0, 1.0, channels).astype(f32)
        assert pcm.shape[1] in (1, channels)
        limit = int(r["loop_end"][0] if r["flags"][0] & LOOP else r["frames"][0]) * ONE
        assert int(r["position"][0]) < limit and (not r["flags"][0] & LOOP or r["loop_start"][0] < r["loop_end"][0] <= r["frames"][0])
        records.append(r)
        assets.append(pcm)
    return np.concatenate(records), assets


# ---- the families: each a plain function of the batch's channel count that returns (records, assets) ----
def high_positions(channels):
    entries = []
    for asset in long_pool(channels):
        n = asset[1].shape[0]
        for lin in (0, LIN):
            entries += [
                (asset, dict(flags=PLAY | lin, position=(H - 100) * ONE, step=ONE)),                   # crosses 2^32 at frame 100: inside the first tile
                (asset, dict(flags=PLAY | lin, position=(H - 600) * ONE + 4001, step=ONE + 37)),        # ... inside a later tile, fractions moving
                (asset, dict(flags=PLAY | lin, position=(H + 50) * ONE + 77, step=ONE - 3)),            # starts above 2^32
                (asset, dict(flags=PLAY | LOOP | lin, loop_start=H - 300, loop_end=n, position=(H - 200) * ONE + 9, step=3 * ONE + 5)),  # a loop across 2^32
                (asset, dict(flags=PLAY | LOOP | lin, loop_start=H + 10, loop_end=H + 1000, position=(H + 900) * ONE, step=ONE + 1))]   # ... and above it
        # a one-shot whose last frames lie at frames - 1 with fraction 4095: it interpolates into silence and finishes
        entries += [(asset, dict(flags=PLAY | LIN, position=(n - 1) * ONE + 4000, step=1)),
                    (asset, dict(flags=PLAY | LIN, position=(n - 5) * ONE + 4095, step=ONE))]
    return collect(channels, 1, entries)


def large_steps(channels):
    entries = []
    for a, asset in enumerate(long_pool(channels)):
        n = asset[1].shape[0]
        for s, step in enumerate(LARGE_STEPS):
            lin = LIN if (a + s) % 2 else 0
            entries += [
                (asset, dict(flags=PLAY | lin, position=(n - 3000) * ONE + 11, step=step)),                                                 # finishes in its first frames
                (asset, dict(flags=PLAY | LOOP | LIN - lin, loop_start=H + 7, loop_end=H + 8, position=(H + 7) * ONE + 123, step=step)),    # a 1-frame loop
                (asset, dict(flags=PLAY | LOOP | lin, loop_start=n - 3, loop_end=n, position=(n - 3) * ONE + 5, step=step)),          # a 3-frame loop
                (asset, dict(flags=PLAY | LOOP | LIN - lin, loop_start=0, loop_end=n, position=(H // 3) * ONE + 1000 * s, step=step))]  # the whole asset
    return collect(channels, 2, entries)


def loop_extremes(channels):
    entries = []
    for asset in long_pool(channels):
        n = asset[1].shape[0]
        entries += [
            (asset, dict(flags=PLAY | LOOP | LIN, loop_start=n - 1, loop_end=n, position=(n - 1) * ONE + 4095, step=1)),          # one frame, the asset's last
            # 2^20 frames in front of loop_start, entered at frame 300 or so: in mid-tile
            (asset, dict(flags=PLAY | LOOP | LIN, loop_start=H, loop_end=H + 777, position=17, step=H * ONE // 300)),
            (asset, dict(flags=PLAY | LOOP, loop_start=H, loop_end=n, position=(H - 1000) * ONE + 5, step=3 * ONE + 1)),
            (asset, dict(flags=PLAY | LOOP | LIN, loop_start=100, loop_end=3100, position=2900 * ONE, step=ONE + 1)),               # longer than 512 steps
            (asset, dict(flags=PLAY | LOOP | LIN, loop_start=H + 1, loop_end=H + 3, position=(H + 2) * ONE + 4000, step=4097)),     # 2 frames at 4097
            (asset, dict(flags=PLAY | LOOP, loop_start=0, loop_end=n, position=(n - 200) * ONE, step=ONE))]                          # ends with the asset
    return collect(channels, 3, entries)


ENDING_STEPS = [ONE, ONE + 5, 777, 3 * ONE + 1]


def exact_endings(channels, frames):
    """One-shots that a call of `frames` frames takes to their end E exactly, to E - 1, and whose last frame lies at E - 1: three records
    in a row per asset."""
    entries = []
    for a, asset in enumerate(long_pool(channels) + [small_assets(channels)["s16 wide"]]):
        end, step = asset[1].shape[0] * ONE, ENDING_STEPS[(a + frames) % 4]
        lin = LIN if (a + frames) % 2 else 0
        for position in (end - frames * step, end - 1 - frames * step, end - 1 - (frames - 1) * step):
            entries.append((asset, dict(flags=PLAY | lin, position=position, step=step)))
    return collect(channels, 4 + frames, entries)


def addresses(channels):
    """The records whose assets the GPU test places ADDRESS_OFFSETS elements into an allocation; the family itself names no address."""
    small = small_assets(channels)
    entries = []
    for name in ("s16 stereo", "u8", "f32 x8"):
        fmt, pcm = small[name]
        if pcm.shape[1] != channels:
            pcm = pcm[:, :1].copy() if name == "f32 x8" else pcm.reshape(-1, 1)
        n = pcm.shape[0]
        for lin in (0, LIN):
            entries += [((fmt, pcm), dict(flags=PLAY | lin, position=3 * ONE + 100, step=ONE + 9)),
                        ((fmt, pcm), dict(flags=PLAY | LOOP | lin, loop_start=1, loop_end=n, position=(n - 40) * ONE, step=2 * ONE - 7))]
    return collect(channels, 5, entries)


def idle_fields(channels):
    """Random records whose gains beyond the batch's channels hold a NaN with a payload, -0.0, a denormal and Inf (on the one-shots
    loop_start and loop_end are random 32-bit values already): none of it is the render's to read or change."""
    records, assets, _, _ = random_records(np.random.default_rng(6 + channels), 40, channels, assets_per_format=1, cycle=True)
    idle = ref.MAX_CHANNELS - channels
    records["gain"].view(np.uint32)[:, channels:] = np.resize(IDLE_GAINS, (len(records), idle)) if idle else 0
    return records, assets


# name -> [(label, builder(channels) -> (records, assets), the case's own frame counts)]
FAMILIES = {
    "high positions": [("", high_positions, [700])],
    "large steps": [("", large_steps, [600])],
    "loop extremes": [("", loop_extremes, [1300])],
    "exact endings": [(f"F {F}", functools.partial(exact_endings, frames=F), [F]) for F in ENDING_FRAMES],
    "addresses": [("", addresses, [300])],
    "idle fields": [("", idle_fields, [64, 256, 441])],
}


def cases(name, channels):
    for label, builder, sizes in FAMILIES[name]:
        records, assets = builder(channels)
        yield f"{name} {label}".strip() + f", {channels} channels", records, assets, sizes


def same_records(a, b):
    """Whole records on their 80 bytes; a NaN gain must be the same NaN."""
    return a.dtype == b.dtype == ref.DTYPE and a.tobytes() == b.tobytes()


# ---- model against restatement ----
def agree(label, records, assets, sizes, channels):
    state, parts = records, []
    for frames in sizes:
        want, after = ref.render(state, assets, frames, channels)
        got, got_after = model.render(state, assets, frames, channels)
        ok, nbad = ref.same_floats(got, want)
        assert ok, f"{label}, {frames} frames: model and restatement differ in {nbad} samples"
        assert same_records(got_after, after), f"{label}, {frames} frames: records differ at {np.nonzero(got_after != after)[0][:8].tolist()}"
        parts.append(want)
        state = after
    # ... and the restatement's one call of as many frames gives what its calls gave
    whole, after = ref.render(records, assets, sum(sizes), channels)
    assert ref.same_floats(whole, np.concatenate(parts, axis=1))[0] and same_records(after, state), f"{label}: one call differs from the split"
    return state


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_model_and_restatement_agree(name, channels):
    """The case's own call, then the calls of SPLIT continuing it: outputs on their bits (NaNs by position) and the records on their 80
    bytes after every call."""
    for label, records, assets, sizes in cases(name, channels):
        agree(label, records, assets, sizes + SPLIT, channels)


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_model_and_restatement_agree_on_the_random_records(channels):
    records, assets, _, _ = random_records(np.random.default_rng(40 + channels), 150, channels)
    after = agree(f"random records, {channels} channels", records, assets, [441, 1, 258], channels)
    finished = (after["flags"] & PLAY) == 0
    assert finished.any() and not finished.all()


def test_the_model_computes_the_values_worked_out_by_hand():
    """(tests/test_sampler_abi.py holds the restatement against the same values.)"""
    asset = np.asarray([16384, -16384, 8192, 32767], np.int16).reshape(-1, 1)
    out, after = model.render_one(rec(frames=4, step=3 * ONE // 4, flags=PLAY | LIN)[0], asset, 8, 1)
    last = f32(32767.0 / 32768.0)
    want = [0.5, 0.5 + (-1.0 * 0.75), -0.5 + (0.75 * 0.5), 0.25 + float((last - f32(0.25)) * f32(0.25)), float(last), float(last + (f32(0.0) - last) * f32(0.75)), 0.0, 0.0]
    assert ref.same_bits(out[:, 0], np.asarray(want, f32)) and after["position"] == 4 * ONE and after["flags"] == LIN
    ramp = np.arange(10.0, dtype=f32).reshape(-1, 1)
    out, after = model.render_one(rec(format=ref.PCM_F32, frames=10, loop_start=4, loop_end=7, flags=PLAY | LOOP, position=3 * ONE, step=7 * ONE)[0], ramp, 5, 1)
    assert out[:, 0].tolist() == [3, 4, 5, 6, 4] and after["position"] == (4 + 34 % 3) * ONE


# ---- the cases reach what they claim ----
def first_call(name, channels):
    (label, records, assets, sizes), = list(cases(name, channels))
    return records, assets, sizes[0], ref.render(records, assets, sizes[0], channels)[1]


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_high_positions_cross_2_to_the_32(channels):
    records, assets, frames, after = first_call("high positions", channels)
    crossed = (records["position"] >> np.uint64(32) == 0) & (after["position"] >> np.uint64(32) != 0)
    above = records["position"] >> np.uint64(32) != 0
    for fmt in (ref.PCM_U8, ref.PCM_S16, ref.PCM_F32):
        assert (crossed & (records["format"] == fmt)).any() and (above & (records["format"] == fmt)).any(), fmt
    # playing frames on both sides of 2^32 inside one tile of 512 frames, and of 256
    for tile in (256, 512):
        straddling = 0
        for r in records[(records["flags"] & LOOP) == 0]:
            q = [int(r["position"]) + f * int(r["step"]) for f in range(frames)]
            assert q[-1] < int(r["frames"]) * ONE or r["position"] >> np.uint64(12) >= r["frames"] - 5
            straddling += any(q[t] < TWO32 <= q[min(t + tile, frames) - 1] < int(r["frames"]) * ONE for t in range(0, frames, tile))
        assert straddling >= 3, (tile, straddling)
    # the one-shots at frames - 1, fraction 4095: the last playing frame interpolates into silence, then the voice has finished
    ends = records[(records["position"] >> np.uint64(12)) >= records["frames"] - 5]
    assert len(ends) == 6 and (ends["flags"] == PLAY | LIN).all()
    for r in ends:
        q = [int(r["position"]) + f * int(r["step"]) for f in range(frames)]
        assert int(r["frames"]) * ONE - 1 in q
    finished = after[(records["position"] >> np.uint64(12)) >= records["frames"] - 5]
    assert (finished["flags"] == LIN).all() and (finished["position"] == finished["frames"].astype(np.uint64) * ONE).all()


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_large_steps_pass_every_loop_more_than_twice(channels):
    """A lane's offset in_tile * step (in_tile <= 255 in the shorter tile) is at least two loop lengths for some record of every loop
    length: the remainder is taken, one subtraction is not enough.  Every step takes a tile's advance, step * 512, past 32 bits.  The
    one-shots finish in the first call."""
    records, assets, frames, after = first_call("large steps", channels)
    loops = records[(records["flags"] & LOOP) != 0]
    lengths = (loops["loop_end"] - loops["loop_start"]).astype(np.int64)
    assert set(lengths.tolist()) == {1, 3} | {a.shape[0] for a in assets}
    for length in set(lengths.tolist()):
        assert any(255 * int(r["step"]) >= 2 * length * ONE for r in loops[lengths == length]), length
    assert set(records["step"].tolist()) == set(LARGE_STEPS) and all(512 * s >= TWO32 for s in LARGE_STEPS)      # a tile's advance is past 32 bits
    one_shots = (records["flags"] & LOOP) == 0
    assert one_shots.sum() == 9 and (after["flags"][one_shots] & PLAY == 0).all() and (after["flags"][~one_shots] & PLAY != 0).all()


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_loop_extremes_are_what_they_say(channels):
    records, assets, frames, after = first_call("loop extremes", channels)
    length = (records["loop_end"] - records["loop_start"]).astype(np.int64)
    steps_round = length * ONE // np.maximum(records["step"].astype(np.int64), 1)
    one_frame = (length == 1) & (records["loop_end"] == records["frames"]) & (records["step"] == 1) & ((records["position"] & np.uint64(4095)) == 4095)
    assert one_frame.sum() == 3
    assert ((records["loop_end"] == records["frames"]) & (length > 4000)).sum() >= 3           # a loop that ends with a long asset
    lead_in = (records["loop_start"] >= H) & (records["position"] < np.uint64(64))
    assert lead_in.sum() == 3
    for r in records[lead_in]:                                                                  # ... entered in mid-tile, of either length
        entry = -(-(int(r["loop_start"]) * ONE - int(r["position"])) // int(r["step"]))
        assert 0 < entry < frames and 16 < entry % 256 < 240 and 16 < entry % 512 < 496, entry
    assert (steps_round > 512).any() and ((length == 2) & (records["step"] == 4097)).sum() == 3
    assert (after["flags"] == records["flags"]).all()


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_exact_endings_finish_on_the_frame(channels):
    """Of the pair that a call of F frames takes to E and to E - 1, the first has finished and the second plays on, for every F; the
    third record's last frame lay at E - 1 and it has finished.  The F of the list sit on and beside both tile lengths."""
    assert {TILE[channels] - 1, TILE[channels], TILE[channels] + 1} <= set(ENDING_FRAMES)
    seen = []
    for label, records, assets, (frames,) in cases("exact endings", channels):
        _, after = ref.render(records, assets, frames, channels)
        _, after_model = model.render(records[:3], assets[:3], frames, channels)
        assert same_records(after_model, after[:3])
        for k in range(0, len(records), 3):
            p, step, end = [int(x) for x in records["position"][k:k + 3]], int(records["step"][k]), int(records["frames"][k]) * ONE
            assert (p[0] + frames * step, p[1] + frames * step, p[2] + (frames - 1) * step) == (end, end - 1, end - 1), label
            assert [int(f) & PLAY for f in after["flags"][k:k + 3]] == [0, PLAY, 0], label
            assert after["position"][k:k + 3].tolist() == [end, end - 1, end], label
        seen.append(frames)
    assert seen == ENDING_FRAMES


def test_idle_fields_hold_what_the_render_must_not_touch():
    for channels in (1, 2, 4, 7):
        records, assets = idle_fields(channels)
        bits = records["gain"].view(np.uint32)[:, channels:]
        assert set(bits.reshape(-1).tolist()) == set(IDLE_GAINS.tolist()) and np.isnan(records["gain"][:, channels:]).any()
        one_shots = records[(records["flags"] & LOOP) == 0]
        assert len(one_shots) and (one_shots["loop_end"].astype(np.int64) > one_shots["frames"]).any()
        state = records
        for frames in (64, 256, 441):
            _, state = ref.render(state, assets, frames, channels)
        changed = [name for name in ref.DTYPE.names if state[name].tobytes() != records[name].tobytes()]
        assert changed == ["position", "flags"]


def test_address_offsets_misalign_every_format():
    """Placed 1, 3 or 5 elements into an aligned allocation, the 16-bit stereo asset lies at 2 mod 4 bytes, the 8-bit one at an odd
    address and the fp32 8-channel one at 4 mod 16."""
    for offset in ADDRESS_OFFSETS:
        assert offset * 2 % 4 == 2 and offset % 2 == 1 and offset * 4 % 16 in (4, 12)
    records, assets = addresses(8)
    assert {(int(r["format"]), int(r["channels"])) for r in records} == {(ref.PCM_S16, 1), (ref.PCM_U8, 1), (ref.PCM_F32, 8)}
    records, assets = addresses(2)
    assert {(int(r["format"]), int(r["channels"])) for r in records} == {(ref.PCM_S16, 2), (ref.PCM_U8, 1), (ref.PCM_F32, 1)}


def test_the_device_tests_play_every_family():
    """tests/test_gpu_sampler.py names every family of this file in its parametrisation: one taken out there shows here."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sampler.py")).read()
    listed = text[text.index("EXTREME_FAMILIES = ["):]
    listed = listed[:listed.index("]")]
    assert sorted(ast.literal_eval(listed.split("=", 1)[1] + "]")) == sorted(FAMILIES)


# ---- controls: restatements with one thing wrong ----
def wrong_render_one(record, asset, frames, channels, wrong):
    """sampler_ref.render_one with one mistake a kernel could make (`wrong` None: none)."""
    u64 = np.uint64
    out = np.zeros((frames, channels), dtype=f32)
    after = record.copy()
    flags = int(record["flags"])
    if not flags & PLAY:
        return out, after
    n, k, p, step = int(record["frames"]), int(record["channels"]), int(record["position"]), int(record["step"])
    first, last = int(record["loop_start"]), int(record["loop_end"])
    end, l0, l1 = n << 12, first << 12, last << 12

    def wrap(q):
        q = np.asarray(q, dtype=u64)
        if not flags & LOOP:
            return q
        past = q >= u64(l1)
        if wrong == "one subtraction":
            return np.where(past, q - u64(l1 - l0), q)
        return np.where(past, u64(l0) + (np.where(past, q, u64(l1)) - u64(l0)) % u64(l1 - l0), q)

    f = np.arange(frames, dtype=u64)
    if wrong == "32 bits":
        q = wrap((u64(p) + f * u64(step)) & u64(0xFFFFFFFF))
    elif wrong == "lane offset in 32 bits":            # the tile's base exact, a lane's in_tile * step kept in 32 bits
        t0 = f // u64(512) * u64(512)
        q = wrap(wrap(u64(p) + t0 * u64(step)) + (((f - t0) * u64(step)) & u64(0xFFFFFFFF)))
    else:
        q = wrap(u64(p) + f * u64(step))
    live = np.ones(frames, dtype=bool) if flags & LOOP else q < u64(end)
    padded = np.concatenate([ref.to_float(asset), np.zeros((1, k), f32)])         # (a wrong index reads silence, not another array)
    i = np.minimum(np.where(live, q >> u64(12), u64(0)), u64(n)).astype(np.int64)
    a = padded[i]
    if flags & LIN:
        j = np.minimum(i + 1, n)
        if flags & LOOP and wrong != "neighbour not wrapped":
            j = np.where(j == last, first, j)
        mu = (q & u64(4095)).astype(f32) * f32(1.0 / ONE)
        v = ref.lerp(a, padded[j], mu[:, None])
    else:
        v = a
    if k == 1:
        v = np.repeat(v, channels, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(live[:, None], v * record["gain"][:channels][None, :], f32(0.0)).astype(f32)
    final = p + frames * step
    if wrong == "32 bits":
        final &= 0xFFFFFFFF
    if wrong != "final position not wrapped":
        final = int(wrap(u64(final)))
    if not flags & LOOP and (final > end if wrong == "finishes at >" else final >= end):
        final = end
        after["flags"] = flags & ~PLAY
    after["position"] = final
    return out, after


def caught(wrong, records, assets, sizes, channels):
    """Whether the wrong restatement differs from the true one in any call, each call started from the true state."""
    state = records
    for frames in sizes:
        want, after = ref.render(state, assets, frames, channels)
        for r in range(len(state)):
            out, rec_after = wrong_render_one(state[r], assets[r], frames, channels, wrong)
            if not ref.same_floats(out, want[r])[0] or rec_after.tobytes() != after[r].tobytes():
                return True
        state = after
    return False


def caught_by_family(wrong, name, channels=2):
    return any(caught(wrong, records, assets, sizes + SPLIT, channels) for _, records, assets, sizes in cases(name, channels))


@functools.lru_cache(maxsize=None)
def old_set():
    """The records the device tests played before this file: random_records as tests/test_sampler_abi.py draws them for its split law."""
    rng = np.random.default_rng(20)
    return [(channels,) + random_records(rng, 1000 if channels == 2 else 100, channels)[:2] for channels in (1, 2, 6)]


def caught_by_the_old_set(wrong):
    return any(caught(wrong, records, assets, [441, 256, 1, 1802], channels) for channels, records, assets in old_set())


# wrong -> (the family aimed at it, whether the old random set catches it too)
CONTROLS = {
    "32 bits": ("high positions", False),
    "one subtraction": ("large steps", True),
    "neighbour not wrapped": ("loop extremes", True),
    "final position not wrapped": ("loop extremes", True),
    "finishes at >": ("exact endings", False),
    "lane offset in 32 bits": ("large steps", False),
}


def test_the_wrong_restatement_without_a_mistake_is_the_restatement():
    assert not caught_by_the_old_set(None)
    for name in FAMILIES:
        assert not caught_by_family(None, name), name


@pytest.mark.parametrize("wrong", list(CONTROLS))
def test_a_wrong_restatement_is_caught_by_its_family(wrong):
    """Position arithmetic truncated to 32 bits before the wrap; the wrap as one subtraction of the loop length; the neighbour not taken
    back to loop_start at loop_end; the final position without the wrap; a one-shot that finishes at > instead of >=; and, sixth, a
    lane's offset in_tile * step kept in 32 bits beside an exact 64-bit base.  Each differs from the restatement on the family aimed at
    it.

    On the old random set -- assets of at most 700 frames, steps of at most 8 frames --, the two 32-bit mistakes pass unseen, and so
    does the finish at > (no record of it lands on E exactly): those gaps were real.  The other three of the first four do not: the old set's loops are as short as one frame and its calls as long as 2500
    frames, so a position passes a loop many times over, a neighbour at loop_end is read with a fraction, and a final position lies past
    loop_end without its wrap.  The issue that asked for these cases took the remainder, the neighbour and the final wrap for reached
    "only by luck"; they were reached all along, and the families for them add the extremes (loops of 1 frame against steps of 2^32 - 1,
    loop_end == frames on a long asset), not the first coverage.  The controls stay, with what the old set does to each asserted."""
    family, old = CONTROLS[wrong]
    assert caught_by_family(wrong, family), f"{family} does not show '{wrong}'"
    assert caught_by_the_old_set(wrong) == old, f"the old random set {'misses' if old else 'catches'} '{wrong}'"
