"""CPU: the voice envelopes at their bounds -- the samplers' extreme records under the voice kernel, glides of 2^20 frames whose fine step
ends at 2^36 - 1 and at 0, ramps of 2^24 frames, delays, fades and glides that end on and beside a tile's edge, one-shots that land on
their end to the fine unit -- as case families that tests/test_gpu_voice.py plays on the device.  Here: an independent frame-at-a-time
model (tests/voice_model.py) agrees with the restatement (tests/voice_ref.py) on every family, bit for bit and on both records' bytes;
every family reaches what it claims to reach; and deliberately wrong restatements are caught by the family aimed at them -- no GPU
needed."""
import ast
import functools
import os

import numpy as np
import pytest

import sampler_ref as sref
import test_sampler_extremes as sx
import voice_model as model
import voice_ref as ref
from test_sampler_abi import rec
from test_sampler_extremes import ENDING_FRAMES, SPLIT, TILE, N, H, collect, long_assets, long_pool, small_assets
from test_voice_abi import GLIDING, env, library_check

f32 = np.float32
ONE = sref.ONE
PLAY, LOOP, LIN = sref.PLAYING, sref.LOOP, sref.LINEAR
ACTIVE, STOP, GLIDE = ref.ACTIVE, ref.STOP, ref.GLIDE
FINE = ref.FINE_BITS
TOP_STEP = (1 << 20) - 1                    # the largest step a glide may start from or end on
NAN_BITS = 0x7FC12345                       # a NaN with a payload


def paired(channels, seed, rows):
    """rows: [((format, PCM), the sampler's fields, envelope [1])] -> (records, envelopes, assets)."""
    records, assets = collect(channels, seed, [(asset, fields) for asset, fields, _ in rows])
    return records, np.concatenate([e for _, _, e in rows]), assets


def gliding(step, step_to, frames, done=0, **kw):
    """An active envelope whose glide oalsfx_host_envelope_glide would set up for a sampler at `step`, `done` frames of it behind it."""
    e = env(**dict(kw, flags=GLIDING | kw.get("flags", 0)))
    ref.glide(e[0], step, step_to, frames)
    e["glide_done"] = done
    return e


def ramped(gain_from, gain_to, frames, done=0, channels=8, **kw):
    e = env(**kw)
    ref.ramp(e[0], np.resize(np.asarray(gain_from, f32), channels), np.resize(np.asarray(gain_to, f32), channels), frames)
    e["ramp_done"] = done
    return e


# ---- 1. the samplers' families under the voice kernel ----
def noise_envelopes(rng, records):
    """Envelopes that are not ACTIVE with noise in every field the check lets noise into: they come back byte for byte."""
    n = len(records)
    e = rng.integers(0, 2 ** 32, (n, ref.DTYPE.itemsize // 4), dtype=np.uint64).astype(np.uint32).view(ref.DTYPE).reshape(-1).copy()
    e["reserved"] = 0
    e["ramp_frames"] %= np.uint32(ref.MAX_RAMP + 1)
    e["ramp_done"] %= e["ramp_frames"] + np.uint32(1)
    e["sub"] &= np.uint32(0xFFFF)
    e["gain_to"].view(np.uint32)[:, -1] = NAN_BITS
    glide_fits = records["step"] < ref.MAX_STEP
    e["flags"] = np.where(glide_fits, np.resize([STOP, STOP | GLIDE, 0, GLIDE], n), np.resize([STOP, 0], n)).astype(np.uint32)
    with_glide = (e["flags"] & GLIDE) != 0
    e["glide_frames"][with_glide] %= np.uint32(ref.MAX_GLIDE + 1)
    e["glide_done"][with_glide] %= e["glide_frames"][with_glide] + np.uint32(1)
    e["step_to"][with_glide] &= np.uint32(ref.MAX_STEP - 1)
    e["glide_slope"][with_glide] = 0
    return e


def under_the_voice_kernel(channels, name, index):
    """Every record of one case of tests/test_sampler_extremes.py three times over: rows 3 k with an all-zero envelope, rows 3 k + 1 with
    one that is not ACTIVE and full of noise, rows 3 k + 2 with an ACTIVE one that changes nothing (R = 0, gain_to = 1, no delay, sub 0;
    gain_from and gain_step are not to be read)."""
    label, builder, sizes = sx.FAMILIES[name][index]
    records, assets = builder(channels)
    rng = np.random.default_rng(900 + index)
    envelopes = np.zeros(3 * len(records), ref.DTYPE)
    envelopes[1::3] = noise_envelopes(rng, records)
    envelopes[2::3] = env(gain_from=-7.0, gain_step=3.0)[0]
    return np.repeat(records, 3), envelopes, [a for a in assets for _ in range(3)]


# ---- 2. glide bounds ----
ODD_GLIDE = 3 * 5 * 7 * 13 * 19 * 37        # 959595 frames: (2^36 - 1) / 959595 = 71613, so a glide from 0 can end on S_G = 2^36 - 1
BEHIND = 1500                               # frames of a long glide still to come when the case starts


def glide_bounds(channels):
    pool = long_pool(channels)
    u8 = long_assets()["u8"]
    small = small_assets(channels)
    whole = lambda asset, lin, **kw: dict(flags=PLAY | LOOP | lin, loop_start=0, loop_end=asset[1].shape[0], **kw)
    top = env(flags=GLIDING, glide_frames=ODD_GLIDE, glide_done=ODD_GLIDE - BEHIND, glide_slope=((1 << 36) - 1) // ODD_GLIDE, step_to=TOP_STEP, sub=40000)
    rows = [
        # S_G = 2^36 - 1, the largest there is; g * slope is near 2^36 from the first frame on
        (pool[0], whole(pool[0], LIN, step=0, position=5 * ONE + 7), top), (pool[2], whole(pool[2], 0, step=0, position=(H + 9) * ONE), top),
        # 2^20 frames at the largest slope a glide of that length can have: S_G = 2^36 - 2^20
        (pool[1], whole(pool[1], LIN, step=0, position=123), env(flags=GLIDING, glide_frames=1 << 20, glide_done=(1 << 20) - BEHIND, glide_slope=(1 << 16) - 1, step_to=TOP_STEP)),
        (pool[1], whole(pool[1], 0, step=0, position=123), env(flags=GLIDING, glide_frames=1 << 20, glide_done=(1 << 20) - BEHIND + 700, glide_slope=(1 << 16) - 1, step_to=TOP_STEP)),
        # S_G = 0 exactly: 255 frames a frame down to a hold over 2^20 frames
        (pool[0], whole(pool[0], LIN, step=255 * ONE, position=77 * ONE), gliding(255 * ONE, 0, 1 << 20, done=(1 << 20) - BEHIND, sub=1)),
        (pool[2], whole(pool[2], LIN, step=255 * ONE, position=(N - 1) * ONE), gliding(255 * ONE, 0, 1 << 20, done=(1 << 20) - BEHIND - 300))]
    assert int(rows[4][2]["glide_slope"][0]) * (1 << 20) == -((255 * ONE) << 16)
    # slopes the helper saturates at +-(2^31 - 1): S_G is not step_to << 16
    for k, G in enumerate((1, 3, 16)):
        rows += [(pool[k % 3], whole(pool[k % 3], LIN if k % 2 else 0, step=0, position=(H - 5 + k) * ONE), gliding(0, TOP_STEP, G)),
                 (pool[(k + 1) % 3], whole(pool[(k + 1) % 3], 0 if k % 2 else LIN, step=TOP_STEP, position=k * ONE + 11), gliding(TOP_STEP, 0, G, sub=65535))]
        assert abs(int(rows[-1][2]["glide_slope"][0])) == int(rows[-2][2]["glide_slope"][0]) == 2 ** 31 - 1
    wide = small["s16 wide"]
    looped = dict(flags=PLAY | LOOP | LIN, loop_start=100, loop_end=4900)
    rows += [
        (wide, dict(looped, step=ONE), gliding(ONE, 2 * ONE, 1)), (wide, dict(looped, step=ONE), gliding(ONE, 3 * ONE, 0)),        # G = 1; G = 0 with GLIDE
        (wide, dict(looped, step=ONE, flags=LOOP | LIN), gliding(ONE, 5 * ONE, 0, delay=3000)),                                       # ... on a sampler that does not play
        (wide, dict(looped, step=2 * ONE + 1), gliding(2 * ONE + 1, 0, 700, sub=9)),                                                  # down to 0, then holds
        # from the last position of the longest asset here, the fine position all ones: a one-shot, and a loop that ends with the asset
        (u8, dict(flags=PLAY | LIN, step=ONE, position=N * ONE - 1), gliding(ONE, 2 * ONE, 1000, sub=65535)),
        (u8, whole(u8, LIN, step=ONE, position=N * ONE - 1), gliding(ONE, TOP_STEP, 1000, sub=65535)),
        # loops of one frame and of three under steps of many frames: every lane takes the remainder
        (u8, dict(flags=PLAY | LOOP | LIN, loop_start=H + 7, loop_end=H + 8, step=TOP_STEP, position=(H + 7) * ONE + 123), gliding(TOP_STEP, 5, 1700, sub=65535)),
        (pool[0], dict(flags=PLAY | LOOP, loop_start=H + 7, loop_end=H + 8, step=9 * ONE + 1, position=(H + 7) * ONE), gliding(9 * ONE + 1, TOP_STEP, 900)),
        (u8, dict(flags=PLAY | LOOP | LIN, loop_start=N - 3, loop_end=N, step=3 * ONE + 5, position=(N - 3) * ONE + 5), gliding(3 * ONE + 5, TOP_STEP, 1800, sub=77)),
        (pool[2], dict(flags=PLAY | LOOP, loop_start=N - 3, loop_end=N, step=TOP_STEP, position=(N - 1) * ONE + 4095), gliding(TOP_STEP, 7 * ONE, 2100, done=50))]
    return paired(channels, 21, rows)


LONG_CALL = 70000


def one_long_render(channels):
    """One row, one render of 70 000 frames under a glide longer than that: glide indices and pair counts inside a render far past 2^16
    and 2^32."""
    u8 = small_assets(channels)["u8"]
    return paired(channels, 22, [(u8, dict(flags=PLAY | LOOP | LIN, loop_start=1, loop_end=901, step=ONE, position=5 * ONE), gliding(ONE, 3 * ONE + 77, 100000, sub=5))])


# ---- 3. ramp bounds ----
def ramp_bounds(channels):
    small = small_assets(channels)
    wide, u8 = small["s16 wide"], small["u8"]
    looped = dict(flags=PLAY | LOOP | LIN, loop_start=0, loop_end=5000, step=ONE + 3, position=17)
    mono = dict(flags=PLAY | LOOP, loop_start=3, loop_end=901, step=ONE - 5, position=4 * ONE)
    R = ref.MAX_RAMP
    specials = env(ramp_frames=300, gain_from=1.0)
    specials["gain_step"][0, :] = np.resize(np.asarray([np.inf, 1e-42, -0.0, -np.inf], f32), 8)
    payload = env(ramp_frames=50, ramp_done=20)
    payload["gain_to"].view(np.uint32)[0, :] = NAN_BITS
    payload["gain_from"].view(np.uint32)[0, :] = 0xFFC00001
    rows = [
        (wide, looped, ramped([1.0, 0.5], [0.0, -0.25], R, done=R - 300)),                   # (float)n exact only because of the bound; ends in mid-call
        (u8, mono, ramped([0.0], [1.0, 0.7], R, done=R - 300, flags=ACTIVE | STOP)),          # ... and stops the voice there
        (wide, looped, ramped([1.0, 0.5], [0.0, -0.25], R)), (u8, mono, ramped([-1.0], [1.0], R, delay=100)),
        (wide, looped, ramped([0.5], [-0.5], 1)), (u8, mono, ramped([0.5], [-0.5], 1, flags=ACTIVE | STOP, delay=64)),
        (wide, looped, ramped([9.0], [0.5, 0.25], 100, done=100)), (wide, looped, ramped([9.0], [0.5], 100, done=100, flags=ACTIVE | STOP)),
        (u8, mono, ramped([9.0], [0.5], R, done=R, flags=ACTIVE | STOP, delay=5)), (u8, mono, ramped([9.0], [0.5, 2.0], R, done=R)),
        (wide, looped, specials), (u8, mono, specials),
        (wide, looped, env(ramp_frames=600, gain_from=1e38, gain_step=1e36, gain_to=0.5)),    # overflows to Inf at n = 241 or so
        (u8, mono, env(ramp_frames=600, ramp_done=100, gain_from=-1e38, gain_step=-1e36, gain_to=-0.0)),
        (wide, dict(looped, flags=LOOP | LIN), payload), (u8, mono, payload)]
    return paired(channels, 23, rows)


# ---- 4. delay, STOP and a glide's end against the grid ----
def edges(channels):
    T = TILE[channels]
    return [1, 63, 64, 65, T - 1, T, T + 1]


def grid_calls(channels):
    T = TILE[channels]
    return [T - 1, T, T + 1, 2 * T + 65]


@functools.lru_cache(maxsize=None)
def short_assets(channels):
    rng = np.random.default_rng(400 + channels)
    return {"wide": (sref.PCM_S16, rng.integers(-32768, 32768, (40, channels)).astype(np.int16)),
            "mono": (sref.PCM_F32, rng.standard_normal((47, 1)).astype(f32))}


def against_the_grid(channels, frames):
    """For every edge x: a delay that ends at output frame x, a fade with STOP that completes there, a glide that ends there; on loops and
    on one-shots of 40 and 47 frames, which end before most of the fades do.  Then D == frames, D == frames - 1 and the longest delay."""
    small, short = small_assets(channels), short_assets(channels)
    wide, u8 = small["s16 wide"], small["u8"]
    loops = [(wide, dict(flags=PLAY | LOOP | LIN, loop_start=10, loop_end=4000, step=ONE + 9, position=11 * ONE)),
             (u8, dict(flags=PLAY | LOOP, loop_start=0, loop_end=901, step=2 * ONE - 1, position=900 * ONE))]
    shots = [(short["wide"], dict(flags=PLAY | LIN, step=ONE - 7, position=5)), (short["mono"], dict(flags=PLAY, step=ONE, position=ONE + 1))]
    rows = []
    for k, x in enumerate(edges(channels)):
        for one_shot in (0, 1):
            asset, fields = (shots if one_shot else loops)[k % 2]
            step = fields["step"]
            D = (0, x // 2, x - 1)[(k + one_shot) % 3]
            rows += [(asset, fields, ramped([0.2, -0.3], [1.0, 0.6], 900, delay=x)),
                     (asset, fields, ramped([1.0, 0.8], [0.0], x - D + 5, done=5, delay=D, flags=ACTIVE | STOP)),
                     (asset, fields, gliding(step, step + ONE // 2 + x, x - D + 7, done=7, delay=D, ramp_frames=30, gain_from=0.5, gain_step=0.01, gain_to=0.8))]
    asset, fields = loops[0]
    rows += [(asset, fields, ramped([0.2], [1.0], 300, delay=frames)), (asset, fields, ramped([0.2], [1.0], 300, delay=frames - 1)),
             (asset, fields, gliding(ONE + 9, 2 * ONE, 100, delay=2 ** 32 - 1, flags=STOP)),
             # ten frames of delay, a one-shot that ends some 40 frames on, a fade that completes at frame 70: three stretches of zeros
             (shots[0][0], shots[0][1], ramped([1.0, 0.8], [0.0], 60, delay=10, flags=ACTIVE | STOP))]
    return paired(channels, 24 + frames, rows)


# ---- 5. exact endings with a fine position ----
LANDINGS = (0, -1, 1)               # fine units between where the call takes PHI and E


def fine_endings(channels, frames):
    """One-shots that a call of `frames` frames takes to E exactly, one fine unit short of it and one past it: under a glide that ends
    inside the call or goes on behind it, and at a constant step (where landing beside E takes a sub that is not 0), with and without a
    delay.  The ramp is longer than every call: its counter goes on."""
    rows = []
    for a, asset in enumerate(long_pool(channels) + [small_assets(channels)["s16 wide"]]):
        E = asset[1].shape[0] << FINE
        step = sx.ENDING_STEPS[(a + frames) % 4]
        lin = LIN if (a + frames) % 2 else 0
        D = 3 if a % 2 else 0
        for with_glide in (1, 0):
            G = (frames + 300, max(frames // 2, 1))[a // 2 % 2]
            e = gliding(step, step + ONE // 2 + 1, G, done=a, delay=D) if with_glide else env(delay=D)
            ref.ramp(e[0], np.resize(np.asarray([0.25, -0.5], f32), 8), np.resize(np.asarray([1.0], f32), 8), 5000)
            e["ramp_done"] = 10 * a
            env_glide = (int(e["glide_frames"][0]), int(e["glide_slope"][0]), int(e["step_to"][0])) if with_glide else None
            moved = sum(ref.fine_step(step, env_glide, a + j) for j in range(frames - D))
            for landing in LANDINGS:
                phi0 = E + landing - moved
                this = e.copy()
                this["sub"] = phi0 & 0xFFFF
                rows.append((asset, dict(flags=PLAY | lin, step=step, position=phi0 >> 16), this))
    return paired(channels, 25 + frames, rows)


# name -> [(label, builder(channels) -> (records, envelopes, assets), the case's own frame counts: a list, or a function of the channels)]
FAMILIES = {
    "samplers under the voice kernel": [(f"{name} {label}".strip(), functools.partial(under_the_voice_kernel, name=name, index=k), sizes)
                                        for name in sx.FAMILIES for k, (label, _, sizes) in enumerate(sx.FAMILIES[name])],
    "glide bounds": [("", glide_bounds, [2000]), ("one long render", one_long_render, [LONG_CALL])],
    "ramp bounds": [("", ramp_bounds, [700])],
    "against the grid": [(f"call {k}", lambda channels, k=k: against_the_grid(channels, grid_calls(channels)[k]), lambda channels, k=k: [grid_calls(channels)[k]])
                         for k in range(4)],
    "fine endings": [(f"F {F}", functools.partial(fine_endings, frames=F), [F]) for F in ENDING_FRAMES],
}


def cases(name, channels):
    for label, builder, sizes in FAMILIES[name]:
        records, envelopes, assets = builder(channels)
        yield f"{name}, {label}".rstrip(", ") + f", {channels} channels", records, envelopes, assets, sizes(channels) if callable(sizes) else list(sizes)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- model against restatement ----
@functools.lru_cache(maxsize=None)
def traced(name, channels):
    """Every case of a family through agree(), its own call and then the calls of SPLIT continuing it, once for all the tests that look at
    it: [(label, records, envelopes, assets, the case's own sizes, all the calls, the model's traces of every call, agree()'s states)]."""
    found = []
    for label, records, envelopes, assets, sizes in cases(name, channels):
        traces = []
        states = agree(label, records, envelopes, assets, sizes + SPLIT, channels, traces)
        found.append((label, records, envelopes, assets, sizes, sizes + SPLIT, traces, states))
    return found


def agree(label, records, envelopes, assets, sizes, channels, traces=None):
    """Call after call, both from the restatement's state: outputs on their bits (NaNs by position), both records on their bytes; then
    the restatement's one render of the sum against its calls.  The model is the same over any split by construction, so the two
    together are the header's "any split" law held against an independent witness.  traces: receives the model's trace of every call.  Returns
    [(the records, the envelopes) after every call]."""
    state, env_state, parts, states = records, envelopes, [], []
    for frames in sizes:
        want, after, env_after = ref.render(state, env_state, assets, frames, channels)
        seen = [] if traces is not None else None
        got, got_after, got_env = model.render(state, env_state, assets, frames, channels, seen)
        ok, nbad = sref.same_floats(got, want)
        assert ok, f"{label}, {frames} frames: model and restatement differ in {nbad} samples"
        bad = [r for r in range(len(state)) if got_after[r].tobytes() != after[r].tobytes() or got_env[r].tobytes() != env_after[r].tobytes()]
        assert not bad, f"{label}, {frames} frames: records differ at {bad[:8]}"
        if traces is not None:
            traces.append(seen)
        parts.append(want)
        state, env_state = after, env_after
        states.append((after, env_after))
    whole, after, env_after = ref.render(records, envelopes, assets, sum(sizes), channels)
    assert sref.same_floats(whole, np.concatenate(parts, axis=1))[0] and same_bytes(after, state) and same_bytes(env_after, env_state), f"{label}: one render differs from the split"
    return states


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_model_and_restatement_agree(name, channels):
    """The case's own call, then the calls of SPLIT continuing it."""
    assert len(traced(name, channels)) == len(FAMILIES[name])


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_model_and_restatement_agree_on_the_random_pairs(channels):
    records, envelopes, assets, _, _ = ref.random_pairs(np.random.default_rng(50 + channels), 64, channels)
    after, env_after = agree(f"random pairs, {channels} channels", records, envelopes, assets, list(ref.CALLS), channels)[-1]
    finished = (after["flags"] & PLAY) == 0
    assert finished.any() and not finished.all() and (env_after["sub"] != 0).any()


def test_the_model_computes_the_values_worked_out_by_hand():
    """(tests/test_voice_abi.py holds the restatement against the same three.)"""
    asset = np.asarray([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], f32).reshape(-1, 1)
    r = rec(format=sref.PCM_F32, frames=8, gain=0.5)
    # two frames of delay, four of the fade (1, 0.75, 0.5, 0.25 on v * gain = 0.5, 1, 2, 4), then the voice has stopped
    e = env(flags=ACTIVE | STOP, delay=2, ramp_frames=4, gain_from=1.0, gain_step=-0.25, gain_to=99.0)
    out, after, e_after = model.render_one(r[0], e[0], asset, 8, 1)
    assert out[:, 0].tolist() == [0.0, 0.0, 0.5, 0.75, 1.0, 1.0, 0.0, 0.0] and not out[6:].view(np.uint32).any()
    assert after["position"] == 4 * ONE and after["flags"] == 0 and (e_after["delay"], e_after["ramp_done"], e_after["sub"]) == (0, 4, 0)
    # from a step of 1 to a step of 2 over four frames: fine steps 1, 1.25, 1.5, 1.75, then 2
    count = np.arange(64.0, dtype=f32).reshape(-1, 1)
    r = rec(format=sref.PCM_F32, frames=64, flags=PLAY | LIN)
    out, after, e_after = model.render_one(r[0], gliding(ONE, 2 * ONE, 4)[0], count, 7, 1)
    assert out[:, 0].tolist() == [0.0, 1.0, 2.25, 3.75, 5.5, 7.5, 9.5]
    assert after["position"] == int(11.5 * ONE) and after["step"] == 2 * ONE and (e_after["glide_done"], e_after["sub"]) == (4, 0)
    # a slope of one fine unit moves the 12-bit position only after 362 frames: 362 * 361 / 2 < 65536 <= 363 * 362 / 2
    e = env(flags=GLIDING, glide_frames=1000, glide_slope=1, step_to=0)
    out, after, e_after = model.render_one(rec(format=sref.PCM_F32, frames=64, step=0, flags=PLAY | LIN)[0], e[0], count, 364, 1)
    assert not out[:363].any() and out[363, 0] == f32(1.0 / ONE)
    assert after["position"] == 1 and e_after["sub"] == 364 * 363 // 2 - 65536 and after["step"] == 0 and e_after["glide_done"] == 364


def test_every_envelope_passes_both_checks():
    for name in FAMILIES:
        for channels in (1, 2, 4, 8):
            for label, records, envelopes, assets, sizes in cases(name, channels):
                for r in range(len(records)):
                    step = int(records["step"][r])
                    assert ref.check(envelopes[r], step) is None and library_check(envelopes[r:r + 1], step) == (1, ""), (label, r)


# ---- the cases reach what they claim ----
def first_calls(name, channels):
    """traced() with the records and envelopes as the case's own call leaves them."""
    return [(label, records, envelopes, assets, sizes, traces) + states[0] for label, records, envelopes, assets, sizes, calls, traces, states in traced(name, channels)]


@pytest.mark.parametrize("channels", [1, 4])
def test_the_samplers_families_are_all_there_three_ways(channels):
    """Rows with an all-zero envelope, with a noisy one that is not ACTIVE and with an ACTIVE one that changes nothing, for every record of
    the six families; the first two get the samplers' bits and records and keep their envelope's bytes; of the third, positions cross
    2^32 << 16."""
    seen, crossed = set(), 0
    for label, records, envelopes, assets, sizes, traces, after, env_after in first_calls("samplers under the voice kernel", channels):
        seen.add(label.split(",")[1].split(" F ")[0].strip())
        active = (envelopes["flags"] & ACTIVE) != 0
        assert not any(envelopes[0::3].tobytes()) and not active[1::3].any() and any(envelopes[1::3].tobytes()) and active[2::3].all()
        assert np.isnan(envelopes["gain_to"][1::3]).any()
        assert (envelopes["ramp_frames"][2::3] == 0).all() and (envelopes["gain_to"][2::3] == 1).all() and not (envelopes["delay"][2::3] | envelopes["sub"][2::3]).any()
        assert same_bytes(env_after[~active], envelopes[~active])
        want, want_after = sref.render(records, assets, sizes[0], channels)
        got, got_after, _ = ref.render(records, envelopes, assets, sizes[0], channels)
        assert sref.same_bits(got[~active], want[~active]) and same_bytes(got_after[~active], want_after[~active])
        assert sref.same_floats(got[active], want[active])[0] and same_bytes(got_after[active], want_after[active])       # (x * 1.0f is x)
        crossed += sum(1 for r in range(2, len(records), 3) if int(records["position"][r]) << 16 < 1 << 48 <= traces[0][r]["phi"])
    assert seen == set(sx.FAMILIES), seen
    assert crossed >= 6, crossed


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_glide_bounds_reach_the_bounds(channels):
    found = first_calls("glide bounds", channels)
    label, records, envelopes, assets, sizes, traces, after, env_after = found[0]
    trace = traces[0]
    assert max(t["g_slope"] for t in trace) > 1 << 32
    assert max(t["S"] for t in trace) >= (1 << 36) - (1 << 16)
    G, done, slope = (envelopes[k].astype(np.int64) for k in ("glide_frames", "glide_done", "glide_slope"))
    S_G = (records["step"].astype(np.int64) << 16) + G * slope
    assert (1 << 36) - 1 in S_G and 0 in S_G[G == 1 << 20] and (S_G >= 0).all() and (S_G < 1 << 36).all()
    long_glides = G >= ODD_GLIDE
    assert long_glides.sum() == 6 and ((G - done)[long_glides] < sizes[0]).all() and (env_after["glide_done"][long_glides] == G[long_glides]).all()     # they end in mid-call
    assert (slope == 2 ** 31 - 1).sum() == 3 and (slope == 1 - 2 ** 31).sum() == 3
    assert (S_G[np.abs(slope) == 2 ** 31 - 1] != envelopes["step_to"][np.abs(slope) == 2 ** 31 - 1].astype(np.int64) << 16).all()
    assert {0, 1} <= set(G.tolist()) and (after["step"][G <= 1] == envelopes["step_to"][G <= 1]).all()
    holds = (envelopes["step_to"] == 0) & ((records["flags"] & PLAY) != 0)
    assert holds.sum() >= 5 and (after["step"][holds] == 0).all()
    last = (records["position"] == N * ONE - 1) & (envelopes["sub"] == 65535)
    assert last.sum() == 2 and (after["flags"][last] & PLAY).tolist() == [0, PLAY] and after["position"][last][0] == N * ONE
    # loops of one and three frames: from the second lane on, a tile's offsets lie two loop lengths and more past the loop's end
    length = (records["loop_end"].astype(np.int64) - records["loop_start"]) * ((records["flags"] & LOOP) != 0)
    for tiny in (1, 3):
        assert ((length == tiny) & (np.maximum(records["step"], envelopes["step_to"]) >= 2 * tiny * ONE)).sum() == 2
    idle = (records["flags"] & PLAY) == 0
    assert idle.sum() == 1 and (after["step"][idle] == envelopes["step_to"][idle]).all() and (after["position"][idle] == records["position"][idle]).all()
    # the one long render: a glide longer than the call, indices past 2^16 and a pair count past 2^32 inside it
    label, records, envelopes, assets, sizes, traces, after, env_after = found[1]
    assert len(records) == 1 and sizes == [LONG_CALL] and envelopes["glide_frames"][0] > LONG_CALL and env_after["glide_done"][0] == LONG_CALL
    assert LONG_CALL > 1 << 16 and LONG_CALL * (LONG_CALL - 1) > 1 << 32 and records["format"][0] == sref.PCM_U8 and records["channels"][0] == 1


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_ramp_bounds_reach_the_bounds(channels):
    (label, records, envelopes, assets, sizes, traces, after, env_after), = first_calls("ramp bounds", channels)
    R, done = envelopes["ramp_frames"].astype(np.int64), envelopes["ramp_done"].astype(np.int64)
    stop = (envelopes["flags"] & STOP) != 0
    out, _, _ = ref.render(records, envelopes, assets, sizes[0], channels)
    top = R == ref.MAX_RAMP
    assert int(f32(2 ** 24 - 1)) == 2 ** 24 - 1 and int(f32(2 ** 24 + 1)) != 2 ** 24 + 1
    assert (top & (done == R - 300)).sum() == 2 and (env_after["ramp_done"][top & (done == R - 300)] == R[top & (done == R - 300)]).all()      # ends in mid-call
    assert (top & (done == 0)).sum() == 2 and (R == 1).sum() == 2
    for with_stop in (False, True):
        assert ((done == R) & (R > 1) & (stop == with_stop)).sum() == 2
    at_once = (done == R) & stop
    assert not out[at_once].view(np.uint32).any() and not (after["flags"][at_once] & PLAY).any() and (after["position"][at_once] == records["position"][at_once]).all()
    steps = envelopes["gain_step"][:, :channels]
    assert np.isinf(steps).any() and (steps.view(np.uint32) == 0x80000000).any() == (channels > 2) and ((steps != 0) & (np.abs(steps) < np.finfo(f32).tiny)).any() == (channels > 1)
    overflowing = np.abs(envelopes["gain_from"][:, 0]) == f32(1e38)
    assert overflowing.sum() == 2
    for r in np.nonzero(overflowing)[0]:
        infinite = np.isinf(out[r]).all(axis=1)
        assert not infinite[0] and infinite.any() and not infinite[-1]                      # Inf from mid-ramp to the ramp's end
    payload = envelopes["gain_to"].view(np.uint32)[:, 0] == NAN_BITS
    assert payload.sum() == 2 and (records["flags"][payload] & PLAY).tolist() == [0, PLAY]
    assert (env_after["gain_to"].view(np.uint32)[payload] == NAN_BITS).all() and (env_after["gain_from"].view(np.uint32)[payload] == 0xFFC00001).all()
    assert not out[payload][0].view(np.uint32).any() and np.isnan(out[payload][1][40:]).all()


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_the_grid_cases_put_every_end_on_every_edge(channels):
    T = TILE[channels]
    assert grid_calls(channels) == [T - 1, T, T + 1, 2 * T + 65]
    for (label, records, envelopes, assets, sizes, traces, after, env_after), frames in zip(first_calls("against the grid", channels), grid_calls(channels)):
        assert sizes == [frames]
        trace = traces[0]
        delay = envelopes["delay"].astype(np.int64)
        stop, glides = (envelopes["flags"] & STOP) != 0, (envelopes["flags"] & GLIDE) != 0
        one_shot = (records["flags"] & LOOP) == 0
        fade_end = delay + envelopes["ramp_frames"] - envelopes["ramp_done"]
        glide_end = delay + envelopes["glide_frames"] - envelopes["glide_done"]
        for x in edges(channels):
            for shot in (False, True):
                rows = np.nonzero((delay == x) & ~stop & ~glides & (one_shot == shot) & (envelopes["ramp_frames"] == 900))[0]
                assert len(rows) == 1 and (x >= frames or trace[rows[0]]["kinds"][x - 1:x + 1] in ("dp", "de")), (label, x, "a delay")
                rows = np.nonzero((fade_end == x) & stop & ~glides & (one_shot == shot))[0]
                assert len(rows) == 1 and (x >= frames or trace[rows[0]]["kinds"][x - 1:x + 1] in ("ps", "es")), (label, x, "a STOP")
                rows = np.nonzero((glide_end == x) & glides & ~stop & (one_shot == shot))[0]
                assert len(rows) == 1, (label, x, "a glide's end")
                r = rows[0]
                assert env_after["glide_done"][r] == min(envelopes["glide_frames"][r], envelopes["glide_done"][r] + max(frames - delay[r], 0))
                assert (env_after["glide_done"][r] == envelopes["glide_frames"][r]) == (x <= frames)
        special = envelopes["ramp_frames"] == 300
        assert (special & (delay == frames)).sum() == 1 and (special & (delay == frames - 1)).sum() == 1 and (delay == 2 ** 32 - 1).sum() == 1
        assert env_after["delay"][delay == 2 ** 32 - 1] == 2 ** 32 - 1 - frames
        # delay, a one-shot's end and a completed STOP in one call, all three with frames in them
        three = [r for r in range(len(records)) if "d" in trace[r]["kinds"] and "pe" in trace[r]["kinds"] and "es" in trace[r]["kinds"]]
        assert three and all(one_shot[r] and stop[r] for r in three), label


@pytest.mark.parametrize("channels", [1, 2, 4, 8])
def test_fine_endings_land_where_they_say(channels):
    """Of each three rows the call takes the first to E exactly, the second one fine unit short of it and the third one past it, under a
    glide and without.  The first and third have finished with position E and sub 0, the second plays on at E - 1 and 65535 fine units
    and finishes in the next call; the ramp's counter goes on through every later call."""
    assert {TILE[channels] - 1, TILE[channels], TILE[channels] + 1} <= set(ENDING_FRAMES)
    seen = []
    for label, records, envelopes, assets, sizes, calls, traces, states in traced("fine endings", channels):
        frames, (after, env_after) = calls[0], states[-1]
        E = records["frames"].astype(np.uint64) << np.uint64(12)
        landed = [traces[0][r]["landed"] - (int(records["frames"][r]) << FINE) for r in range(len(records))]
        assert landed == list(LANDINGS) * (len(records) // 3), label
        first, env_first = states[0]
        assert (first["flags"] & PLAY).tolist() == [0, PLAY, 0] * (len(records) // 3)
        assert (first["position"] == np.where((first["flags"] & PLAY) != 0, E - np.uint64(1), E)).all()
        assert (env_first["sub"] == np.where((first["flags"] & PLAY) != 0, 65535, 0)).all()
        assert ((envelopes["flags"] & GLIDE) != 0).sum() == len(records) // 2 and (envelopes["sub"] != 0).sum() > len(records) // 2
        steady = envelopes["sub"][(envelopes["flags"] & GLIDE) == 0]                          # without a glide, beside E means a sub that is not 0
        assert not steady[0::3].any() and (steady[1::3] == 65535).all() and (steady[2::3] == 1).all()
        assert (after["position"] == E).all() and not (env_after["sub"] != 0).any() and not (after["flags"] & PLAY).any()
        assert (env_after["ramp_done"] == envelopes["ramp_done"] + sum(calls) - envelopes["delay"]).all()
        seen.append(frames)
    assert seen == ENDING_FRAMES


def test_the_device_tests_play_every_family():
    """tests/test_gpu_voice.py names every family of this file in its parametrisation: one taken out there shows here."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_voice.py")).read()
    listed = text[text.index("EXTREME_FAMILIES = ["):]
    listed = listed[:listed.index("]")]
    assert sorted(ast.literal_eval(listed.split("=", 1)[1] + "]")) == sorted(FAMILIES)


# ---- controls: restatements with one thing wrong ----
u64 = np.uint64
M64 = (1 << 64) - 1


def wrong_render_one(record, e, asset, frames, channels, wrong):
    """voice_ref.render_one with one mistake a kernel or its launcher could make (`wrong` None: none).  Positions in 64-bit modular
    arithmetic, as a kernel has them; a wrong index reads silence, not another array."""
    eflags = int(e["flags"])
    if not eflags & ACTIVE:
        out, after = sref.render_one(record, asset, frames, channels)
        return out, after, e.copy()
    out = np.zeros((frames, channels), dtype=f32)
    after, env_after = record.copy(), e.copy()
    flags, step = int(record["flags"]), int(record["step"])
    delay, R, n0 = int(e["delay"]), int(e["ramp_frames"]), int(e["ramp_done"])
    D = min(delay, frames)
    shown = frames - D
    advanced = min(shown, R - n0) if eflags & STOP else shown
    glides = bool(eflags & GLIDE)
    G, g0, slope, step_to = (int(e["glide_frames"]), int(e["glide_done"]), int(e["glide_slope"]), int(e["step_to"])) if glides else (0, 0, 0, step)
    env_after["delay"], env_after["ramp_done"] = delay - D, min(R, n0 + shown)
    if flags & PLAY and advanced > 0:
        n, k = int(record["frames"]), int(record["channels"])
        first, last = int(record["loop_start"]), int(record["loop_end"])
        E, L0, L1 = u64(n << FINE), u64(first << FINE), u64(last << FINE)
        loop = bool(flags & LOOP)
        phi0 = u64((int(record["position"]) << 16) | int(e["sub"]))
        bend = g0 * slope
        if wrong == "g * slope in 32 bits":
            bend = (bend + 2 ** 31) % 2 ** 32 - 2 ** 31
        sg0 = u64(((step << 16) + bend) & M64)
        sto = u64(((step << 16) + G * slope) & M64) if wrong == "S_G from the slope" and glides else u64(step_to << 16)
        left = u64(max(G - g0, 0))

        def offsets(t):
            m = np.minimum(t, left)
            pairs = m * (m - u64(1))
            if wrong == "pairs in 32 bits over a call":
                pairs = pairs & u64(0xFFFFFFFF)
            return m * sg0 + (pairs >> u64(1)) * u64(slope & M64) + (t - m) * sto

        def wrap(q):
            if not loop:
                return q
            past = q >= L1
            return np.where(past, L0 + (np.where(past, q, L1) - L0) % (L1 - L0), q)

        t = np.arange(advanced, dtype=u64)
        if wrong == "one subtraction in a lane":           # the tile's base exact, a lane past the loop's end taken back by one loop length
            t0 = t // u64(512) * u64(512)
            phi = wrap(phi0 + offsets(t0)) + (offsets(t) - offsets(t0))
            if loop:
                phi = np.where(phi >= L1, phi - (L1 - L0), phi)
        else:
            phi = wrap(phi0 + offsets(t))
        live = np.ones(advanced, dtype=bool) if loop else phi < E
        q = phi >> u64(16)
        padded = np.concatenate([sref.to_float(asset), np.zeros((1, k), f32)])
        i = np.minimum(np.where(live, q >> u64(12), u64(0)), u64(n)).astype(np.int64)
        a = padded[i]
        if flags & LIN:
            j = np.minimum(i + 1, n)
            if loop:
                j = np.where(j == last, first, j)
            mu = (q & u64(4095)).astype(np.int64).astype(f32) * f32(1.0 / ONE)
            v = sref.lerp(a, padded[j], mu[:, None])
        else:
            v = a
        if k == 1:
            v = np.repeat(v, channels, axis=1)
        factors = ref.factors(e, n0 + (D if wrong == "ramp index without the delay" else 0) + np.arange(advanced, dtype=np.int64), channels)
        with np.errstate(invalid="ignore", over="ignore"):
            o = (v * record["gain"][:channels][None, :]).astype(f32)
            out[D:D + advanced] = np.where(live[:, None], o * factors, f32(0.0))
        moved = shown if wrong == "advanced over F' under STOP" else advanced
        end = int(wrap(phi0 + offsets(np.asarray([moved], dtype=u64)))[0])
        sub = end & 0xFFFF
        if not loop and end >= int(E):
            end = int(E)
            flags &= ~PLAY
            if wrong != "sub kept at a one-shot's end":
                sub = 0
        after["position"], env_after["sub"] = end >> 16, sub
    if glides:
        env_after["glide_done"] = min(G, g0 + advanced)
        if env_after["glide_done"] == G:
            after["step"] = step_to
    if eflags & STOP and env_after["ramp_done"] == R:
        flags &= ~PLAY
    after["flags"] = flags
    return out, after, env_after


def true_calls(records, envelopes, assets, sizes, channels):
    """[(the state a call starts from, its envelopes, frames, what the restatement makes of it)]"""
    state, env_state, calls = records, envelopes, []
    for frames in sizes:
        result = ref.render(state, env_state, assets, frames, channels)
        calls.append((state, env_state, frames, result))
        state, env_state = result[1], result[2]
    return calls


def caught(wrong, calls, assets, channels):
    """Whether the wrong restatement differs from the true one in any call, each call started from the true state."""
    for state, env_state, frames, (want, after, env_after) in calls:
        for r in range(len(state)):
            out, rec_after, e_after = wrong_render_one(state[r], env_state[r], assets[r], frames, channels, wrong)
            if not sref.same_floats(out, want[r])[0] or rec_after.tobytes() != after[r].tobytes() or e_after.tobytes() != env_after[r].tobytes():
                return True
    return False


@functools.lru_cache(maxsize=None)
def family_calls(name, channels=2):
    return [(assets, true_calls(records, envelopes, assets, sizes + SPLIT, channels)) for _, records, envelopes, assets, sizes in cases(name, channels)]


def caught_by_family(wrong, name, channels=2):
    return any(caught(wrong, calls, assets, channels) for assets, calls in family_calls(name, channels))


@functools.lru_cache(maxsize=None)
def old_set():
    """What the device tests played before this file: the pairs tests/test_voice_abi.py draws for its split law (seed 21, the restatement's
    four calls), and the rows tests/test_gpu_voice.py names one by one in its three calls."""
    from test_gpu_voice import required_rows
    rng = np.random.default_rng(21)
    sets = []
    for channels in (2, 1, 6):
        records, envelopes, assets, _, _ = ref.random_pairs(rng, 300 if channels == 2 else 96, channels)
        sets.append((channels, assets, true_calls(records, envelopes, assets, list(ref.CALLS), channels)))
    _, records, envelopes, assets = required_rows(lambda pcm: 0x10000)
    sets.append((2, assets, true_calls(records, envelopes, assets, [256, 256, 1024], 2)))
    return sets


def caught_by_the_old_set(wrong):
    return any(caught(wrong, calls, assets, channels) for channels, assets, calls in old_set())


# wrong -> the family aimed at it
CONTROLS = {
    "g * slope in 32 bits": "glide bounds",
    "pairs in 32 bits over a call": "glide bounds",
    "ramp index without the delay": "against the grid",
    "advanced over F' under STOP": "against the grid",
    "sub kept at a one-shot's end": "fine endings",
    "one subtraction in a lane": "glide bounds",
    "S_G from the slope": "glide bounds",
}


def test_the_wrong_restatement_without_a_mistake_is_the_restatement():
    assert not caught_by_the_old_set(None)
    for name in FAMILIES:
        assert not caught_by_family(None, name), name


@pytest.mark.parametrize("wrong", list(CONTROLS))
def test_a_wrong_restatement_is_caught_by_its_family(wrong):
    """g * glide_slope wrapped to 32 bits; the pair count m (m - 1) / 2 with its product in 32 bits over a whole call, where the kernel
    forms it per tile; the ramp index counted from the output frame and not from the frame behind the delay; the sampler moved over F'
    and not F'' frames under STOP (outputs right, position and sub wrong); sub left as it fell when a one-shot reaches E; a lane past
    the loop's end taken back by one loop length beside an exact base; S_g behind the glide taken as S_G from the slope and not as
    step_to << 16.  Each differs from the restatement on the family aimed at it.

    Found, not assumed, on the old set (492 random pairs of seed 21 over 441 + 256 + 1 + 1802 frames, and the 35 rows
    tests/test_gpu_voice.py names, over 256 + 256 + 1024): it catches six of the seven already.  Its glides go down to G = 1 from steps
    of up to 8 frames, so g * slope passes 2^31 and the helper's truncated slopes make S_G differ from step_to << 16; its loops are as
    short as one frame; its delays sit in front of ramps, its fades complete in mid-call, and its gliding one-shots end between fine
    units.  Only the pair count passes it unseen: no call of the old set has 65 537 frames of one glide in it.  So of these mistakes the
    families add one first catch; for the others they add the bounds (S_G at 2^36 - 1 and at 0, glides of 2^20 frames, slopes at
    +-(2^31 - 1), every edge of both tiles), not the first coverage.  What the old set does with a control is printed, not asserted."""
    assert caught_by_family(wrong, CONTROLS[wrong]), f"{CONTROLS[wrong]} does not show '{wrong}'"
    print(f"the old set {'catches' if caught_by_the_old_set(wrong) else 'misses'} '{wrong}'")
