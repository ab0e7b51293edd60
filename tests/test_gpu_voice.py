"""GPU: the voice envelopes (oalsfx_batch_set_envelopes, _get_envelopes, and the renders of _sample_device and _play_downmix_meter with an
envelope active; include/oalsfx_hip.h, "voice envelopes") against their restatement (tests/voice_ref.py).  Every comparison is on the bit
patterns (NaNs by position) and on the exact integers, outputs and both records; there is no tolerance anywhere.  No test provokes a
device fault: every refusal is decided on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meter_ref
import sampler_ref as sref
import voice_ref as ref
from downmix_ref import downmix
from harness import ROOT, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import ENVELOPE_DTYPE, METER_DTYPE, SAMPLER_DTYPE, Batch, BatchError
from test_gpu_sampler import Assets, Placed, device_render, expect_output, expect_records, expect_same_bytes
from test_sampler_abi import rec
from test_voice_abi import GLIDING, env

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
CALLS = (441, 256, 1, 63)


def _torch():
    import torch
    return torch


def expect_envelopes(got, want, label):
    for field in ENVELOPE_DTYPE.names:
        a, w = got[field], want[field]
        same = sref.same_floats(a, w)[0] if field.startswith("gain_") else bool((a == w).all())
        assert same, f"{label}: envelope field {field} differs at instances {np.nonzero((a != w).reshape(len(got), -1).any(axis=1))[0][:8].tolist()}"


def run_calls(b, records, envelopes, pcm, sizes, label, **kw):
    """set_samplers and set_envelopes, then one render per size, each against the restatement, with both records read back after every
    call.  Returns (the outputs side by side, the records, the envelopes)."""
    b.set_samplers(records)
    b.set_envelopes(envelopes)
    expect_envelopes(b.get_envelopes(), envelopes, f"{label}: as set")
    state, env_state, outs = records, envelopes, []
    for frames in sizes:
        want, state, env_state = ref.render(state, env_state, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        expect_output(got, want, f"{label}, {frames} frames")
        expect_records(b.get_samplers(), state, f"{label}, after {frames} frames")
        expect_envelopes(b.get_envelopes(), env_state, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), state, env_state


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_6POINT1, desc.FMT_7POINT1])
def test_seventy_voices_in_four_renders_and_in_one(fmt, offset):
    """70 instances -- a partial last workgroup --, every PCM format x mono / wide asset x nearest / linear x looped / one-shot taken in
    turn, the envelopes' kinds of voice_ref.random_pairs taken in turn beside them; renders of 441, 256, 1 and 63 frames, then the same
    records again in one render of 761: the same outputs and the same final records.  The destination 0, 1 and 2 floats off its
    allocation: every store width runs."""
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(1000 * fmt + offset)
    records, envelopes, pcm, keys, pool = ref.random_pairs(rng, 70, ch, calls=CALLS, assets_per_format=1, cycle=True, asset_frames=(1, 3000))
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    combos = {(int(r["format"]), int(r["channels"]) == 1, int(r["flags"]) & (sref.LOOP | sref.LINEAR)) for r in records}
    assert len(combos) == 3 * (1 if ch == 1 else 2) * 4, combos
    with Batch(70, fmt, 48000, 1) as b:
        parts, after, env_after = run_calls(b, records, envelopes, pcm, CALLS, f"format {fmt}, offset {offset}", offset=offset)
        assert b.last_render_kernel() == "k_voice_rows"
        whole, after_whole, env_whole = run_calls(b, records, envelopes, pcm, [sum(CALLS)], f"format {fmt}, offset {offset}, one render", offset=offset)
        assert same_bits(parts, whole)[0], "four renders and one differ"
        expect_records(after, after_whole, "four renders and one")
        expect_envelopes(env_after, env_whole, "four renders and one")
        assert np.abs(whole).max() > 0 and (after_whole["step"] != records["step"]).any() and (env_whole["sub"] != 0).any()


def required_rows(assets_at):
    """The rows the contract names one by one, for stereo calls of 256, 256 and 1024 frames (a tile is 512 frames): [(what, sampler record,
    envelope, PCM)]."""
    rng = np.random.default_rng(77)
    noise = rng.standard_normal((3000, 1)).astype(f32)
    short = rng.standard_normal((150, 2)).astype(f32)
    special = np.asarray([1.0, np.inf, 2.0, -0.0, np.nan, 1e-39, 3e38, -3e38, 0.5, -np.inf], f32).reshape(-1, 1)
    looped = dict(format=sref.PCM_F32, frames=3000, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=100, loop_end=2900, step=ONE + 17)
    one_shot = dict(format=sref.PCM_F32, frames=150, channels=2, flags=sref.PLAYING | sref.LINEAR, step=ONE - 100)
    tiny_loop = dict(format=sref.PCM_F32, frames=3000, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=7, loop_end=10, position=8 * ONE, step=3 * ONE + 5)

    def fade(frames, stop=True, **kw):
        e = env(flags=ref.ACTIVE | (ref.STOP if stop else 0))
        ref.ramp(e[0], [1.0, 0.5], [0.0, -0.25], frames)
        for k, v in kw.items():
            e[k] = v
        return e

    def gliding(step, step_to, frames, **kw):
        e = env(flags=GLIDING, **kw)
        ref.glide(e[0], step, step_to, frames)
        return e

    rows = [("delay 0", looped, env(), noise), ("delay < F", looped, env(delay=100), noise), ("delay == F", looped, env(delay=256), noise),
            ("a delay that spans two calls", looped, env(delay=300), noise), ("a delay longer than every call", looped, env(delay=5000), noise),
            ("R = 0", looped, fade(0, stop=False), noise), ("R = 1", looped, fade(1, stop=False), noise),
            ("R ends in mid-tile", looped, fade(200, stop=False), noise), ("R spans calls", looped, fade(400, stop=False), noise),
            ("R ends in the second tile of the third call", looped, fade(512 + 512 + 388, stop=False), noise),
            ("STOP completes at frame 0", looped, fade(0), noise), ("STOP with R = 0 behind a delay", looped, fade(0, delay=256), noise),
            ("STOP completes in mid-call", looped, fade(100), noise), ("STOP completes on a call's last frame", looped, fade(256), noise),
            ("STOP completes on the last frame of the second call, under way", looped, fade(600, ramp_done=88), noise),
            ("a one-shot ends before its ramp", one_shot, fade(1000, stop=False), short), ("a one-shot ends before its STOP", one_shot, fade(1000), short),
            ("a negative factor past a one-shot's end", one_shot, env(gain_to=-1.0), short),
            ("a negative ramp past a one-shot's end", one_shot, env(ramp_frames=2000, gain_from=-1.0, gain_step=-0.001), short),
            ("a glide up", looped, gliding(ONE + 17, 2 * ONE, 1000), noise), ("a glide down", looped, gliding(ONE + 17, ONE // 3, 1000), noise),
            ("a glide that ends in mid-tile", looped, gliding(ONE + 17, 3 * ONE, 200), noise),
            ("a glide down to a hold, delayed, under a fade", looped, gliding(ONE + 17, 0, 700, delay=40, ramp_frames=900, gain_step=-0.001, gain_to=0.1), noise),
            ("a glide over a loop shorter than one tile's advance", tiny_loop, gliding(3 * ONE + 5, 40 * ONE, 900, sub=65535), noise),
            ("a glide down over a three-frame loop", tiny_loop, gliding(3 * ONE + 5, 1, 300), noise),
            ("a glide on a one-shot that ends under it", one_shot, gliding(ONE - 100, 5 * ONE, 400), short),
            ("a sub without a glide", looped, env(sub=40000), noise), ("no envelope", looped, env(flags=0, delay=9, sub=3, gain_to=0.0), noise),
            ("no envelope, one-shot", one_shot, env(flags=ref.STOP | ref.GLIDE, ramp_frames=5), short), ("no envelope at all", tiny_loop, np.zeros(1, ref.DTYPE), noise),
            ("an envelope on a sampler that does not play", dict(looped, flags=sref.LOOP), gliding(ONE + 17, 77, 300, delay=10, ramp_frames=400), noise),
            ("NaN and Inf samples under a ramp", dict(format=sref.PCM_F32, frames=10, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_end=10, step=ONE // 3),
             fade(700, stop=False), special),
            ("denormal factors", looped, env(ramp_frames=600, gain_from=1e-39, gain_step=1e-42, gain_to=1e-45), noise),
            ("denormal products", dict(looped, gain=1e-30), env(ramp_frames=300, gain_from=1e-9, gain_step=-1e-12, gain_to=np.inf), noise),
            ("a NaN factor", looped, env(ramp_frames=300, gain_from=np.nan, gain_to=np.nan), noise)]
    records = np.concatenate([rec(**fields) for _, fields, _, _ in rows])
    records["gain"][:, :2] *= np.asarray([0.75, -0.5], f32)
    envelopes = np.concatenate([e for _, _, e, _ in rows])
    pcm = [p for _, _, _, p in rows]
    for r, p in enumerate(pcm):
        records["data"][r] = assets_at(p)
        assert ref.check(envelopes[r], int(records["step"][r])) is None, rows[r][0]
    return [what for what, _, _, _ in rows], records, envelopes, pcm


def test_the_rows_the_contract_names():
    torch = _torch()
    kept = {}

    def assets_at(pcm):
        if id(pcm) not in kept:
            kept[id(pcm)] = torch.from_numpy(pcm).cuda()
        return kept[id(pcm)].data_ptr()

    names, records, envelopes, pcm = required_rows(assets_at)
    torch.cuda.synchronize()
    sizes = [256, 256, 1024]
    with Batch(len(records), desc.FMT_STEREO, 48000, 1) as b, Batch(len(records), desc.FMT_STEREO, 48000, 1) as plain:
        state, env_state = records, envelopes
        b.set_samplers(records)
        b.set_envelopes(envelopes)
        plain.set_samplers(records)              # no envelope is ever set here: k_sampler_rows renders it
        idle = [r for r, name in enumerate(names) if name.startswith("no envelope")]
        for k, frames in enumerate(sizes):
            want, state, env_state = ref.render(state, env_state, pcm, frames, 2)
            got = device_render(b, frames)
            bad = [names[r] for r in range(len(names)) if not sref.same_floats(got[r], want[r])[0]]
            assert not bad, f"call {k}: the outputs of {bad} differ"
            now, env_now = b.get_samplers(), b.get_envelopes()
            bad = [names[r] for r in range(len(names)) if now[r].tobytes() != state[r].tobytes() or not ref.same_envelopes(env_now[r:r + 1], env_state[r:r + 1])]
            assert not bad, f"call {k}: the records of {bad} differ"
            # rows without an envelope, beside rows with one: k_sampler_rows' bits
            theirs = device_render(plain, frames)
            assert b.last_render_kernel() == "k_voice_rows" and plain.last_render_kernel() == "k_sampler_rows"
            assert same_bits(got[idle], theirs[idle])[0] and plain.get_samplers()[idle].tobytes() == now[idle].tobytes()
            if k == 0:
                row = dict(zip(names, range(len(names))))
                assert not got[row["delay == F"]].view(np.uint32).any() and not got[row["STOP completes at frame 0"]].view(np.uint32).any()
                assert not now["flags"][row["STOP completes at frame 0"]] & sref.PLAYING and not now["flags"][row["STOP completes on a call's last frame"]] & sref.PLAYING
                assert not now["flags"][row["STOP with R = 0 behind a delay"]] & sref.PLAYING        # ramp_done == R after the render
                assert now["flags"][row["STOP completes in mid-call"]] & sref.PLAYING == 0 and now["position"][row["STOP completes in mid-call"]] != records["position"][row["STOP completes in mid-call"]]
                tail = got[row["a negative factor past a one-shot's end"]][200:]
                assert not tail.view(np.uint32).any(), "-0.0f past a one-shot's end"
                assert np.isnan(got[row["NaN and Inf samples under a ramp"]]).any() and np.isinf(got[row["NaN and Inf samples under a ramp"]]).any()
                quiet = got[row["denormal factors"]]
                assert (quiet != 0).any() and np.abs(quiet).max() < np.finfo(f32).tiny


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("fmt", [desc.FMT_5POINT1, desc.FMT_7POINT1])
def test_nine_rows_around_the_tile_boundary(fmt, offset):
    """Where k_voice_rows' tile is 256 frames (5.1 and 7.1; k_fir_rows' is 192 at 7.1): nine rows -- three workgroups, the last with one
    row --, calls of 255, 256, 257 and 513 frames that continue one another, the destination 0, 1 and 2 floats off its allocation (every
    store width).  Outputs on their bits and both records after every call against the restatement; the row without an envelope against
    the samplers' restatement too; and the same nine rows on a second batch whose tenth instance names a table, so that k_fir_rows
    renders them: the same bits and records."""
    import resample_ref as rref
    torch = _torch()
    ch = desc.FORMAT_CHANNELS[fmt]
    sizes = [255, 256, 257, 513]
    rng = np.random.default_rng(500 + fmt)
    noise = rng.standard_normal((3000, 1)).astype(f32)
    wide = rng.integers(-32768, 32768, (1024, ch)).astype(np.int16)
    looped = dict(format=sref.PCM_F32, frames=3000, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=100, loop_end=2900, step=ONE + 17)
    one_shot = dict(format=sref.PCM_S16, channels=ch, frames=1024, flags=sref.PLAYING | sref.LINEAR, step=ONE)     # frame 1024 is frame 256 of the fourth call

    def ramped(frames, flags=ref.ACTIVE, **kw):
        e = env(flags=flags, **kw)
        ref.ramp(e[0], np.linspace(1.0, 0.5, ch), np.linspace(0.0, -0.25, ch), frames)
        return e

    gliding = env(flags=GLIDING)
    ref.glide(gliding[0], ONE + 17, 3 * ONE, 900)                                                              # ends at frame 132 of the fourth call
    rows = [("a delay of 63", looped, ramped(300, delay=63), noise), ("a delay of 64", looped, ramped(300, delay=64), noise),
            ("a delay of 65", looped, ramped(300, delay=65), noise),
            ("a ramp that ends on the fourth call's tile boundary", looped, ramped(768 + 256), noise),
            ("a ramp that ends one frame past it", looped, ramped(768 + 257), noise),
            ("a glide that ends in mid-tile", looped, gliding, noise),
            ("a STOP that completes in mid-call", looped, ramped(400, ref.ACTIVE | ref.STOP), noise),
            ("a one-shot that ends on a tile boundary", one_shot, env(), wide),
            ("no envelope", looped, env(flags=0, delay=9, sub=3, gain_to=0.0), noise)]
    names = [what for what, _, _, _ in rows]
    row = dict(zip(names, range(len(names))))
    records = np.concatenate([rec(**fields) for _, fields, _, _ in rows])
    records["gain"][:, :ch] *= np.linspace(0.75, -0.5, ch, dtype=f32)
    envelopes = np.concatenate([e for _, _, e, _ in rows])
    pcm = [p for _, _, _, p in rows]
    kept = {id(p): torch.from_numpy(p).cuda() for p in (noise, wide)}
    records["data"] = [kept[id(p)].data_ptr() for p in pcm]
    torch.cuda.synchronize()
    for r in range(9):
        assert ref.check(envelopes[r], int(records["step"][r])) is None, names[r]
    with Batch(9, fmt, 48000, 1) as b, Batch(10, fmt, 48000, 1) as tabled:
        b.set_samplers(records)
        b.set_envelopes(envelopes)
        tabled.set_fir_table(0, rref.cubic(12))
        tabled.set_samplers(np.concatenate([records, records[:1]]))
        tabled.set_envelopes(np.concatenate([envelopes, envelopes[:1]]))
        tabled.set_resamplers(np.asarray([rref.NONE] * 9 + [0]))
        state, env_state, alone_state = records, envelopes, records[8:]
        for k, frames in enumerate(sizes):
            label = f"format {fmt}, offset {offset}, call {k}"
            want, state, env_state = ref.render(state, env_state, pcm, frames, ch)
            got, theirs = device_render(b, frames, offset=offset), device_render(tabled, frames, offset=offset)
            assert b.last_render_kernel() == "k_voice_rows" and tabled.last_render_kernel() == "k_fir_rows"
            bad = [names[r] for r in range(9) if not sref.same_floats(got[r], want[r])[0]]
            assert not bad, f"{label}: the outputs of {bad} differ"
            now, env_now = b.get_samplers(), b.get_envelopes()
            expect_records(now, state, label)
            expect_envelopes(env_now, env_state, label)
            assert same_bits(got, theirs[:9])[0], f"{label}: k_fir_rows' rows without a table differ"
            assert tabled.get_samplers()[:9].tobytes() == now.tobytes() and tabled.get_envelopes()[:9].tobytes() == env_now.tobytes(), label
            alone, alone_state = sref.render(alone_state, pcm[8:], frames, ch)
            assert same_bits(got[8:], alone)[0], f"{label}: the row without an envelope has not the samplers' bits"
            expect_records(now[8:], alone_state, label + ", the row without an envelope")
            playing = (now["flags"] & sref.PLAYING) != 0
            assert playing[row["a STOP that completes in mid-call"]] == (k < 1) and playing[row["a one-shot that ends on a tile boundary"]] == (k < 3), label
            assert (now["step"][row["a glide that ends in mid-tile"]] == 3 * ONE) == (k == 3), label
            assert np.abs(got[[r for r in range(9) if playing[r]]]).max() > 0
        assert env_now["ramp_done"][row["a ramp that ends one frame past it"]] == 768 + 257 and env_now["delay"][:3].tolist() == [0, 0, 0]


def test_the_launch_follows_the_active_envelopes():
    """No envelope active: k_sampler_rows, and nothing of the envelopes goes to the device but what was set.  One ACTIVE envelope:
    k_voice_rows.  Cleared again: k_sampler_rows."""
    rng = np.random.default_rng(3)
    records, envelopes, pcm, keys, pool = ref.random_pairs(rng, 20, 2)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    with Batch(20, desc.FMT_STEREO, 48000, 1) as b:
        assert b.last_render_kernel() == "" and not b.get_envelopes().view(np.uint8).any()
        b.set_samplers(records)
        want, state = sref.render(records, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "before any envelope")
        assert b.last_render_kernel() == "k_sampler_rows" and b.envelope_uploads() == 0
        inactive = envelopes.copy()
        inactive["flags"] &= ~np.uint32(ref.ACTIVE)
        b.set_envelopes(inactive)
        want, state = sref.render(state, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "envelopes that are not ACTIVE")
        assert b.last_render_kernel() == "k_sampler_rows" and b.envelope_uploads() == 1
        expect_envelopes(b.get_envelopes(), inactive, "envelopes that are not ACTIVE")
        one = env(delay=30, ramp_frames=50, gain_from=0.0, gain_step=0.02)
        b.set_envelopes(one, instances=[4])
        env_state = inactive.copy()
        env_state[4] = one[0]
        want, state, env_state = ref.render(state, env_state, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "one ACTIVE envelope")
        assert b.last_render_kernel() == "k_voice_rows" and b.envelope_uploads() == 2
        device_render(b, 7)
        _, state, env_state = ref.render(state, env_state, pcm, 7, 2)
        assert b.envelope_uploads() == 2, "a render after which nothing was set put envelopes on the device"
        expect_envelopes(b.get_envelopes(), env_state, "after two renders")
        cleared = env_state[4:5].copy()
        cleared["flags"] = 0
        b.set_envelopes(cleared, instances=[4])
        env_state[4] = cleared[0]
        want, state = sref.render(state, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "the envelope cleared")
        assert b.last_render_kernel() == "k_sampler_rows" and b.envelope_uploads() == 3
        expect_records(b.get_samplers(), state, "the envelope cleared")
        expect_envelopes(b.get_envelopes(), env_state, "the envelope cleared")


def test_refusals_leave_the_envelopes_alone():
    so = lib.load()
    rng = np.random.default_rng(8)
    records, envelopes, pcm, keys, pool = ref.random_pairs(rng, 8, 2)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    records["step"][2], records["step"][3] = 2 ** 20, ONE
    envelopes[2], envelopes[3] = env()[0], env()[0]
    with Batch(8, desc.FMT_STEREO, 48000, 1) as b:
        b.set_samplers(records)
        b.set_envelopes(envelopes)
        uploads = b.envelope_uploads()

        def refused(message, e, instances=(1,)):
            idx = (C.c_int * len(instances))(*instances)
            arr = np.concatenate([e] * len(instances))
            assert not so.oalsfx_batch_set_envelopes(b._h, idx, len(instances), C.c_void_p(arr.ctypes.data)) and message in b.error, (message, b.error)

        refused("Unknown envelope flags", env(flags=9))
        refused("reserved", env(reserved=[0, 1, 0]))
        refused("ramp is longer", env(ramp_frames=2 ** 24 + 1))
        refused("ramp_done", env(ramp_frames=3, ramp_done=4))
        refused("sub is beyond", env(sub=65536))
        refused("glide is longer", env(flags=GLIDING, glide_frames=2 ** 20 + 1))
        refused("glide_done", env(flags=GLIDING, glide_frames=3, glide_done=4))
        refused("step_to", env(flags=GLIDING, step_to=2 ** 20))
        refused("gliding sampler's step", env(flags=GLIDING, step_to=ONE), instances=(2,))
        refused("leaves the range", env(flags=GLIDING, glide_frames=100, glide_slope=-((ONE << 16) // 100) - 1), instances=(3,))
        refused("Instance range", env(), instances=(8,))
        refused("Instance range", env(), instances=(-1,))
        refused("listed twice", env(), instances=(1, 2, 1))
        arr = np.concatenate([env(), env(sub=65536), env()])           # one bad record: none is taken
        assert not so.oalsfx_batch_set_envelopes(b._h, (C.c_int * 3)(5, 6, 7), 3, C.c_void_p(arr.ctypes.data)) and "sub is beyond" in b.error
        with pytest.raises(BatchError, match="leaves the range"):
            b.set_envelopes(env(flags=GLIDING, glide_frames=2 ** 20, glide_slope=2 ** 16, step_to=ONE), instances=[3])
        # a sampler whose envelope glides keeps a step the glide has room for
        gl = env(flags=GLIDING)
        ref.glide(gl[0], ONE, 2 * ONE, 1000)
        b.set_envelopes(gl, instances=[3])
        envelopes[3] = gl[0]
        for step, message in ((2 ** 20, "gliding sampler's step"), (2 ** 20 - 1, "leaves the range")):
            bad = records[3:4].copy()
            bad["step"] = step
            with pytest.raises(BatchError, match=message):
                b.set_samplers(bad, instances=[3])
        # more than 2^24 frames while an envelope is active (decided before the destination is looked at)
        assert not so.oalsfx_batch_sample_device(b._h, 2 ** 24 + 1, C.c_void_p(0), None) and "2^24 frames" in b.error, b.error
        bus = np.zeros(4, f32)
        assert not so.oalsfx_batch_play_downmix_meter(b._h, 2 ** 24 + 1, 1, bus.ctypes.data_as(C.POINTER(C.c_float)), 0.5, 0, None, None) and "2^24 frames" in b.error
        assert b.envelope_uploads() == uploads
        expect_records(b.get_samplers(), records, "the samplers after the refusals")
        expect_envelopes(b.get_envelopes(), envelopes, "the envelopes after the refusals")
        want, state, env_state = ref.render(records, envelopes, pcm, 300, 2)
        expect_output(device_render(b, 300), want, "after the refusals")
        expect_records(b.get_samplers(), state, "after the refusals")
        expect_envelopes(b.get_envelopes(), env_state, "after the refusals")


def test_fade_out_and_steal_through_play_downmix_meter():
    """64 voices into 4 buses, calls of 256 frames with carried meters.  Eight voices are faded out with STOP: their meters' quiet_run
    counts on from the frame the fade completes, get_samplers sees them not PLAYING, and they are started again on another asset after a
    delay with a fade-in.  The voices' outputs are those of a twin batch fed the restatement's render; buses and meters are downmix_ref's
    and meter_ref's over them."""
    n, n_buses, frames = 64, 4, 256
    threshold = f32(1e-4)
    rng = np.random.default_rng(64)
    records, _, pcm, keys, pool = ref.random_pairs(rng, n, 2, asset_frames=(2000, 6000), max_step=2 * ONE)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    records["flags"] |= np.uint32(sref.PLAYING | sref.LOOP)
    records["loop_start"], records["loop_end"] = 0, records["frames"]
    records["position"] %= records["frames"].astype(np.uint64) * np.uint64(ONE)
    records["gain"][:, :2] = rng.uniform(0.3, 0.9, (n, 2))
    pcm = list(pcm)
    envelopes = np.zeros(n, ref.DTYPE)
    stolen = list(range(3, 64, 8))
    bus, gain = rng.integers(0, n_buses, n), rng.uniform(0.2, 1, n).astype(f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b, Batch(n, desc.FMT_STEREO, 48000, 1) as twin:
        b.set_routing(bus, gain)
        b.set_samplers(records)
        state, env_state = records, envelopes
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        kernels = []
        for k in range(7):
            if k == 1:          # fade the eight out over 300 frames: the fade completes 44 frames into the call after this one
                fades = np.zeros(len(stolen), ref.DTYPE)
                for e in fades:
                    e["flags"] = ref.ACTIVE | ref.STOP
                    ref.ramp(e, [1.0, 1.0], [0.0, 0.0], 300)
                b.set_envelopes(fades, instances=stolen)
                env_state = env_state.copy()
                env_state[stolen] = fades
            if k == 4:          # they are free: start them on another asset, 100 frames from now, fading in over 200
                now = b.get_samplers(stolen)
                assert not (now["flags"] & sref.PLAYING).any() and (vm["quiet_run"][stolen] >= 256 - 44 + 256).all(), vm["quiet_run"][stolen]
                fresh, starts = state[stolen].copy(), np.zeros(len(stolen), ref.DTYPE)
                for j, v in enumerate(stolen):
                    other = (keys[v] + 1) % len(pool)
                    fmt, width, data = pool[other]
                    fresh[j] = rec(format=fmt, channels=width, frames=data.shape[0], step=ONE + 5 * j, flags=sref.PLAYING | sref.LINEAR, data=assets.address(other))[0]
                    fresh[j]["gain"][:2] = (0.5, 0.4)
                    pcm[v] = data
                    starts[j]["flags"], starts[j]["delay"] = ref.ACTIVE, 100
                    ref.ramp(starts[j], [0.0, 0.0], [1.0, 0.8], 200)
                b.set_samplers(fresh, instances=stolen)
                b.set_envelopes(starts, instances=stolen)
                state, env_state = state.copy(), env_state.copy()
                state[stolen], env_state[stolen] = fresh, starts
            x, state, env_state = ref.render(state, env_state, pcm, frames, 2)
            y = twin.mix(x)
            want_buses = downmix(y, bus, gain, n_buses)
            want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
            kernels.append(b.last_render_kernel())
            ok, nbad = same_bits(got, want_buses)
            assert ok, f"call {k}: {nbad} bus samples differ"
            assert meter_ref.same_records(vm, want_v) and meter_ref.same_records(bm, want_b), f"call {k}: the meters' records"
            expect_records(b.get_samplers(), state, f"call {k}")
            expect_envelopes(b.get_envelopes(), env_state, f"call {k}")
        assert kernels == ["k_sampler_rows"] + ["k_voice_rows"] * 6
        assert (vm["quiet_run"][stolen] < 256).all() and (state["flags"][stolen] & sref.PLAYING).all() and (env_state["ramp_done"][stolen] == 200).all()


def test_api_array_envelopes(tmp_path):
    """tests/cpp/api_array_envelopes.cpp: ApiArray::set_envelope / get_envelope, one round trip through a render."""
    exe = str(tmp_path / "api_array_envelopes")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_envelopes.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout


# ---- the pairs of tests/test_voice_extremes.py: the envelopes at their bounds, the samplers' extremes under this kernel, the tile grid ----
EXTREME_FAMILIES = ["samplers under the voice kernel", "glide bounds", "ramp bounds", "against the grid", "fine endings"]
EXTREME_FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_7POINT1]     # both tile lengths, the three store widths


def expect_envelope_bytes(got, want, label):
    """Whole envelopes on their 144 bytes: the render writes no gain, so a NaN in one comes back as the NaN it was."""
    expect_envelopes(got, want, label)
    rows = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not rows, f"{label}: envelopes differ in their bytes at instances {rows[:8]}"


def run_calls_on_bytes(b, records, envelopes, pcm, sizes, label):
    """run_calls with both records compared on their bytes after every call."""
    b.set_samplers(records)
    b.set_envelopes(envelopes)
    expect_envelope_bytes(b.get_envelopes(), envelopes, f"{label}: as set")
    state, env_state, outs = records, envelopes, []
    for frames in sizes:
        want, state, env_state = ref.render(state, env_state, pcm, frames, b.channels)
        got = device_render(b, frames)
        expect_output(got, want, f"{label}, {frames} frames")
        expect_same_bytes(b.get_samplers(), state, f"{label}, after {frames} frames")
        expect_envelope_bytes(b.get_envelopes(), env_state, f"{label}, after {frames} frames")
        assert b.last_render_kernel() == "k_voice_rows"
        outs.append(got)
    return np.concatenate(outs, axis=1), state, env_state


@pytest.mark.parametrize("fmt", EXTREME_FORMATS)
@pytest.mark.parametrize("family", EXTREME_FAMILIES)
def test_extreme_envelopes(family, fmt):
    """Every case of the family: its own call, then calls of 1, 63, 512 and 513 frames that continue it, against the restatement (which
    the frame-at-a-time model has vouched for on these very pairs): outputs on their bits, both records on their bytes after every
    call.  Then the same pairs again in one render of the calls' sum: the same bits and the same records."""
    import test_voice_extremes as extremes
    ch = desc.FORMAT_CHANNELS[fmt]
    placed = Placed()
    for label, records, envelopes, pcm, sizes in extremes.cases(family, ch):
        records = placed.fill_in(records, pcm)
        with Batch(len(records), fmt, 48000, 1) as b:
            parts, after, env_after = run_calls_on_bytes(b, records, envelopes, pcm, sizes + extremes.SPLIT, label)
            whole, after_whole, env_whole = run_calls_on_bytes(b, records, envelopes, pcm, [sum(sizes + extremes.SPLIT)], f"{label}, one render")
            assert same_bits(parts, whole)[0], f"{label}: the calls and one render of their sum differ"
            assert after.tobytes() == after_whole.tobytes() and env_after.tobytes() == env_whole.tobytes(), f"{label}: the records after the calls and after one render"


# ---- call sequences against a host model ----
class Script:
    """A seeded sequence of calls with what each must give, worked out on the host: two record arrays that set_samplers and
    set_envelopes overwrite and voice_ref.render advances, the rows set since the last render (one upload in front of the next), and
    voice_ref.check for what is refused.  Every refusal is the host's; nothing here is out of the device's bounds."""

    def __init__(self, seed, n, channels, pool, addresses):
        self.rng = np.random.default_rng(seed)
        self.n, self.channels, self.pool, self.addresses = n, channels, pool, addresses
        self.rec, self.env, self.pcm = np.zeros(n, sref.DTYPE), np.zeros(n, ref.DTYPE), [None] * n
        self.step_before = self.rec["step"].copy()          # the steps in front of the last render
        self.ops, self.dirty, self.uploads = [], set(), 0

    def rows(self, most=6):
        return sorted(self.rng.choice(self.n, size=int(self.rng.integers(1, min(most, self.n) + 1)), replace=False).tolist())

    def fresh(self, step=None, key=None):
        """A looped record on one of the pool's assets, with the asset."""
        rng = self.rng
        key = int(rng.integers(len(self.pool))) if key is None else key
        fmt, width, data = self.pool[key]
        frames = data.shape[0]
        r = rec(format=fmt, channels=width, frames=frames, flags=sref.PLAYING | sref.LOOP | (sref.LINEAR if rng.random() < 0.5 else 0), loop_start=0, loop_end=frames,
                step=int(rng.integers(0, 3 * ONE)) if step is None else step, position=int(rng.integers(0, frames * ONE)), data=self.addresses[key])
        r["gain"][0, :self.channels] = rng.uniform(-1, 1, self.channels)
        return r, data

    def envelope(self, row):
        """An envelope of a kind drawn: a fade out with STOP, a delayed fade in, a glide from the row's step as the model has it, none."""
        rng, ch = self.rng, self.channels
        kind = int(rng.integers(4))
        if kind == 3:
            return np.zeros(1, ref.DTYPE)
        e = env(flags=ref.ACTIVE | (ref.STOP if kind == 0 else 0), delay=int(rng.integers(0, 500)) if kind == 1 else 0)
        ref.ramp(e[0], rng.uniform(0.5, 1, ch) * (kind == 0), rng.uniform(0.5, 1, ch) * (kind != 0), int(rng.integers(0, 600)))
        if kind == 2:
            ref.glide(e[0], int(self.rec["step"][row]), int(rng.integers(0, 4 * ONE)), int(rng.integers(0, 800)))
        return e

    def refusal(self, envelopes, steps):
        for e, step in zip(envelopes, steps):
            what = ref.check(e, int(step))
            if what:
                return what
        return None

    def set_samplers(self, rows, records, pcm):
        rows = list(range(self.n)) if rows is None else rows
        gliding = [(self.env[r], records["step"][k]) for k, r in enumerate(rows) if int(self.env["flags"][r]) & ref.GLIDE]
        refused = self.refusal([e for e, _ in gliding], [s for _, s in gliding])
        e = self.env[rows]
        mid_glide = bool((((e["flags"] & GLIDING) == GLIDING) & (e["glide_done"] > 0) & (e["glide_done"] < e["glide_frames"]) & (records["step"] != self.rec["step"][rows])).any())
        self.ops.append(dict(kind="set_samplers", rows=rows, data=records.copy(), refused=refused, mid_glide=mid_glide and not refused))
        if not refused:
            self.rec[rows] = records
            for r, p in zip(rows, pcm):
                self.pcm[r] = p

    def set_envelopes(self, rows, envelopes, from_last_get=None):
        rows = list(range(self.n)) if rows is None else rows
        refused = self.refusal(envelopes, self.rec["step"][rows])
        self.ops.append(dict(kind="set_envelopes", rows=rows, data=envelopes.copy(), refused=refused, from_last_get=from_last_get,
                             steps_before=self.step_before[rows].copy(), steps_now=self.rec["step"][rows].copy()))
        if not refused:
            self.env[rows] = envelopes
            self.dirty |= set(rows)
        return refused

    def render(self, frames, side=False, wait=True, play=False):
        self.step_before = self.rec["step"].copy()
        kernel = "k_voice_rows" if (self.env["flags"] & ref.ACTIVE).any() else "k_sampler_rows"
        uploaded = len(self.dirty)
        self.uploads += 1 if self.dirty else 0
        self.dirty = set()
        want, self.rec, self.env = ref.render(self.rec, self.env, self.pcm, frames, self.channels)
        self.ops.append(dict(kind="play" if play else "render", frames=frames, side=side, wait=wait or play, want=want, kernel=kernel, uploads=self.uploads, uploaded=uploaded))

    def get(self, what, rows=None):
        rows = list(range(self.n)) if rows is None else rows
        self.ops.append(dict(kind="get_" + what, rows=rows, want=(self.rec if what == "samplers" else self.env)[rows].copy()))

    def filler(self, count):
        rng = self.rng
        for _ in range(count):
            kind = int(rng.integers(7))
            if kind == 0:
                rows = self.rows()
                new = [self.fresh() for _ in rows]
                self.set_samplers(rows, np.concatenate([r for r, _ in new]), [p for _, p in new])
            elif kind == 1:
                rows = self.rows()
                self.set_envelopes(rows, np.concatenate([self.envelope(r) for r in rows]))
            elif kind in (2, 3):
                self.render(int(rng.integers(1, 701)), side=kind == 3, wait=bool(rng.integers(2)))
            elif kind == 4:
                self.get("samplers", self.rows(self.n) if rng.integers(2) else None)
            elif kind == 5:
                self.get("envelopes", self.rows(self.n) if rng.integers(2) else None)
            else:
                self.render(int(rng.integers(1, 701)), play=True)


GLIDE_TO = 200 * ONE            # where the glides of the steps' scenarios end: far enough from a step of ONE that a second glide fits one of them only


def a_glide_that_completes(s, row):
    """The row on a fresh looped record at a step of ONE under a glide of 100 frames up to GLIDE_TO, then 300 frames queued without a wait:
    the device has the new step, the host's copy of the record the old one."""
    r, p = s.fresh(step=ONE, key=0)
    s.set_envelopes([row], np.zeros(1, ref.DTYPE))          # (an old glide would hold the row's step where it has room: clear it first)
    s.set_samplers([row], r, [p])
    assert not s.ops[-1]["refused"]
    e = env(flags=GLIDING)
    ref.glide(e[0], ONE, GLIDE_TO, 100)
    assert s.set_envelopes([row], e) is None
    s.render(300, wait=False)
    assert s.rec["step"][row] == GLIDE_TO and s.step_before[row] == ONE


def scenarios(s):
    """The stretches every sequence holds whatever its seed, in an order the seed chooses (the upload of every row comes before the
    sets of every row that clear and restore ACTIVE: it must be the first of its size)."""
    rng, n = s.rng, s.n

    def twice():
        a, b = (int(x) for x in rng.choice(n, 2, replace=False))
        s.set_envelopes([a], s.envelope(a))
        s.set_envelopes([b, a], np.concatenate([s.envelope(b), env(delay=7, ramp_frames=90, gain_from=0.0, gain_step=0.01)]))
        s.render(int(rng.integers(100, 400)))

    def get_between():
        rows = s.rows(3)
        s.set_envelopes(rows, np.concatenate([s.envelope(r) for r in rows]))
        s.get("envelopes")
        s.render(int(rng.integers(1, 300)))

    def set_behind_a_render():
        s.render(int(rng.integers(200, 700)), side=True, wait=False)
        rows = s.rows(2)
        s.set_envelopes(rows, np.concatenate([env(delay=3, ramp_frames=50, gain_from=1.0, gain_step=-0.01, gain_to=0.5) for _ in rows]))
        s.get("envelopes")
        s.get("samplers")

    def glide_for_the_new_step():
        row = int(rng.integers(n))
        a_glide_that_completes(s, row)
        down = env(flags=GLIDING, glide_frames=100, glide_slope=-(((150 * ONE) << 16) // 100), step_to=50 * ONE)
        assert ref.check(down[0], ONE) == "leaves the range" and s.set_envelopes([row], down) is None
        s.render(150)
        s.get("samplers", [row])

    def glide_for_the_old_step():
        row = int(rng.integers(n))
        a_glide_that_completes(s, row)
        up = env(flags=GLIDING, glide_frames=100, glide_slope=((100 * ONE) << 16) // 100, step_to=101 * ONE)
        assert ref.check(up[0], ONE) is None and s.set_envelopes([row], up) == "leaves the range"
        s.get("envelopes")
        s.get("samplers")
        s.render(60)

    def a_step_in_mid_glide():
        row = int(rng.integers(n))
        r, p = s.fresh(step=ONE, key=1)
        s.set_envelopes([row], np.zeros(1, ref.DTYPE))
        s.set_samplers([row], r, [p])
        assert not s.ops[-1]["refused"]
        e = env(flags=GLIDING, sub=12345)
        ref.glide(e[0], ONE, 2 * ONE, 2000)
        s.set_envelopes([row], e)
        s.render(300)
        faster = s.rec[row:row + 1].copy()
        faster["step"] = 3 * ONE
        s.set_samplers([row], faster, [p])
        assert s.ops[-1]["mid_glide"]
        s.render(200, wait=False)
        s.get("envelopes", [row])
        s.get("samplers", [row])

    def three_then_all():
        s.render(64, wait=False)                            # (whatever was set before goes up here)
        rows = sorted(int(x) for x in rng.choice(n, 3, replace=False))
        s.set_envelopes(rows, np.concatenate([s.envelope(r) for r in rows]))
        s.render(int(rng.integers(100, 700)), wait=False)
        every = np.concatenate([s.envelope(r) for r in range(n)])
        every[0] = env(ramp_frames=3000, gain_from=0.1, gain_step=0.0002)[0]            # (one ACTIVE at the least)
        assert s.set_envelopes(None, every) is None
        s.render(int(rng.integers(100, 700)), side=True, wait=False)
        s.get("envelopes")

    def active_cleared_and_set_again():
        s.get("envelopes")
        was = s.env.copy()
        stale = np.asarray([ref.check(s.env[r], int(s.rec["step"][r])) is not None for r in range(n)])      # a completed glide no longer fits its sampler's new step
        was["flags"][stale] &= ~np.uint32(ref.GLIDE)
        cleared = was.copy()
        cleared["flags"] &= ~np.uint32(ref.ACTIVE)
        assert (was["flags"] & ref.ACTIVE).any() and s.set_envelopes(None, cleared, from_last_get="clear") is None
        s.render(int(rng.integers(100, 400)))
        s.get("envelopes")
        assert s.set_envelopes(None, was, from_last_get="restore") is None
        s.render(int(rng.integers(100, 400)), wait=False)
        s.get("envelopes")
        s.get("samplers")

    first = [twice, get_between, set_behind_a_render, glide_for_the_new_step, glide_for_the_old_step, a_step_in_mid_glide, three_then_all]
    order = [first[k] for k in rng.permutation(len(first))]
    order.insert(int(rng.integers(order.index(three_then_all) + 1, len(order) + 1)), active_cleared_and_set_again)
    return order


def present(ops, n):
    """What the sequence holds, looked up in the calls themselves: {what: whether it is there}."""
    kinds = [op["kind"] for op in ops]
    renders = [k for k, kind in enumerate(kinds) if kind in ("render", "play")]
    waits = lambda op: op["kind"].startswith("get_") or op["kind"] == "play" or (op["kind"] == "render" and op["wait"])
    taken = lambda op, kind="set_envelopes": op["kind"] == kind and not op["refused"]
    with_glide = lambda op: bool((op["data"]["flags"] & ref.GLIDE).any())
    found = dict.fromkeys(["one instance set twice in front of a render", "get_envelopes between a set and the render", "a set behind an unsynchronised render, then a read-back",
                           "a glide that only the new step allows", "a glide that only the old step allows", "a sampler set in mid-glide",
                           "ACTIVE cleared everywhere and set again", "three records, then all, and no wait"], False)
    for k, op in enumerate(ops):
        behind = next((j for j in renders if j > k), None)         # the render in front of which this call's records go up
        since = max((j for j in renders if j < k), default=-1)
        if taken(op) and behind is not None:
            for j in range(since + 1, k):
                if taken(ops[j]) and set(ops[j]["rows"]) & set(op["rows"]) and ops[behind]["uploads"] == (ops[since]["uploads"] if since >= 0 else 0) + 1:
                    found["one instance set twice in front of a render"] = True
            if any(kinds[j] == "get_envelopes" and set(op["rows"]) < set(ops[j]["rows"]) for j in range(k + 1, behind)):
                found["get_envelopes between a set and the render"] = True
        if taken(op) and since >= 0 and not ops[since]["wait"] and not any(waits(ops[j]) for j in range(since + 1, k)):
            if any(kinds[j] == "get_envelopes" and set(op["rows"]) < set(ops[j]["rows"]) for j in range(k + 1, behind or len(ops))):
                found["a set behind an unsynchronised render, then a read-back"] = True
        if op["kind"] == "set_envelopes" and with_glide(op) and since == k - 1 and not ops[since]["wait"] and len(op["rows"]) == 1:
            e, old, new = op["data"][0], int(op["steps_before"][0]), int(op["steps_now"][0])
            if old != new and ref.check(e, old) == "leaves the range" and ref.check(e, new) is None and not op["refused"]:
                found["a glide that only the new step allows"] = True
            if old != new and ref.check(e, old) is None and op["refused"] == "leaves the range":
                found["a glide that only the old step allows"] = True
        if taken(op, "set_samplers") and op["mid_glide"]:
            found["a sampler set in mid-glide"] = True
        if taken(op) and op["from_last_get"] == "restore" and behind is not None and ops[behind]["kernel"] == "k_voice_rows":
            cleared = next(j for j in range(k - 1, -1, -1) if ops[j]["kind"] == "set_envelopes" and ops[j]["from_last_get"] == "clear")
            between = [j for j in renders if cleared < j < k]
            if between and all(ops[j]["kernel"] == "k_sampler_rows" for j in between) and any(ops[j]["kernel"] == "k_voice_rows" for j in renders if j < cleared):
                found["ACTIVE cleared everywhere and set again"] = True
    uploads = [j for j in renders if ops[j]["uploaded"]]
    whole = next((i for i, j in enumerate(uploads) if ops[j]["uploaded"] == n), None)
    if whole and ops[uploads[whole - 1]]["uploaded"] == 3 and all(ops[j]["uploaded"] <= 32 for j in uploads[:whole]):
        found["three records, then all, and no wait"] = not any(waits(ops[j]) for j in range(uploads[whole - 1], uploads[whole]))
    return found


@pytest.mark.parametrize("fmt, n, seed", [(desc.FMT_STEREO, 70, 7), (desc.FMT_QUAD, 9, 8)])
def test_call_sequences_follow_the_model(fmt, n, seed):
    """Some sixty calls in a seeded order -- set_samplers and set_envelopes on subsets, renders of 1 to 700 frames on the batch's stream and
    on a caller's, waited for or not, get_samplers, get_envelopes, play_downmix_meter -- against Script's host model: every render's
    output, every read-back, the kernel each render launched and the number of uploads.  Eight stretches are in every sequence, which
    present() looks up in the calls generated: see its keys."""
    torch = _torch()
    ch = desc.FORMAT_CHANNELS[fmt]
    _, _, _, _, pool = ref.random_pairs(np.random.default_rng(seed), 1, ch, assets_per_format=1, asset_frames=(300, 3000))
    pool = [entry for entry in pool if entry[0] == sref.PCM_F32] + [entry for entry in pool if entry[0] != sref.PCM_F32]
    assets = Assets(pool)
    s = Script(seed, n, ch, pool, [assets.address(k) for k in range(len(pool))])
    start = [s.fresh() for _ in range(n)]
    s.set_samplers(None, np.concatenate([r for r, _ in start]), [p for _, p in start])
    for block in scenarios(s):
        s.filler(int(s.rng.integers(2, 5)))
        block()
    s.filler(3)
    s.get("envelopes")
    s.get("samplers")
    missing = [what for what, there in present(s.ops, n).items() if not there]
    assert not missing and 50 <= len(s.ops) <= 90, (missing, len(s.ops))
    assert {op["kind"] for op in s.ops} == {"set_samplers", "set_envelopes", "render", "play", "get_samplers", "get_envelopes"}
    assert any(op["kind"] == "render" and op["side"] for op in s.ops)

    n_buses, threshold = 2, f32(1e-4)
    bus, gain = np.arange(n) % n_buses, np.linspace(0.3, 1.0, n).astype(f32)
    side = torch.cuda.Stream()
    with Batch(n, fmt, 48000, 1) as b, Batch(n, fmt, 48000, 1) as twin:
        b.set_routing(bus, gain)
        base = b.envelope_uploads()
        queued, last_get = [], None

        def settle(label):
            b.synchronize()
            side.synchronize()
            torch.cuda.synchronize()
            for buf, want, what in queued:
                expect_output(buf.cpu().numpy(), want, f"{label}: {what}")
            del queued[:]

        for k, op in enumerate(s.ops):
            label = f"call {k} ({op['kind']})"
            if op["kind"] in ("set_samplers", "set_envelopes"):
                data = op["data"]
                if op["kind"] == "set_envelopes" and op["from_last_get"]:
                    data = last_get.copy()                  # the counters as the device had them: only the flags are the caller's
                    data["flags"] = op["data"]["flags"]
                    assert data.tobytes() == op["data"].tobytes(), label
                call = b.set_samplers if op["kind"] == "set_samplers" else b.set_envelopes
                if op["refused"]:
                    with pytest.raises(BatchError, match=op["refused"]):
                        call(data, instances=op["rows"])
                else:
                    call(data, instances=op["rows"])
            elif op["kind"] == "render":
                buf = torch.empty((n, op["frames"], ch), dtype=torch.float32, device="cuda")
                b.sample_device(op["frames"], buf.data_ptr(), stream=side.cuda_stream if op["side"] else None)
                queued.append((buf, op["want"], f"the render of call {k}"))
                assert b.last_render_kernel() == op["kernel"] and b.envelope_uploads() - base == op["uploads"], label
                if op["wait"]:
                    settle(label)
            elif op["kind"] == "play":
                got, _, _ = b.play_downmix_meter(op["frames"], n_buses, threshold)
                assert b.last_render_kernel() == op["kernel"] and b.envelope_uploads() - base == op["uploads"], label
                settle(label)
                ok, nbad = same_bits(got, downmix(twin.mix(op["want"]), bus, gain, n_buses))
                assert ok, f"{label}: {nbad} bus samples differ"
            elif op["kind"] == "get_samplers":
                got = b.get_samplers(op["rows"])
                settle(label)
                expect_same_bytes(got, op["want"], label)
            else:
                got = b.get_envelopes(op["rows"])
                settle(label)
                expect_envelope_bytes(got, op["want"], label)
                if len(op["rows"]) == n:
                    last_get = got
        assert b.envelope_uploads() - base == s.uploads
