"""GPU: the voice filters (oalsfx_batch_set_filters and its lane forms, and the renders of _sample_device and _play_downmix_meter while
any voice's filter is ACTIVE; include/oalsfx_hip.h, "voice filters") against their restatement (tests/biquad_ref.py).  Every comparison
is on the bit patterns (NaNs by position) and on the exact integers: outputs and the four records of every voice; there is no tolerance
anywhere.  No test provokes a device fault: every refusal is decided on the host."""
import os
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import meter_ref
import polyphony_cases as pcases
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from downmix_ref import downmix
from harness import ROOT, ShadowArmy, make_effect, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, Batch, BatchError
from test_gpu_polyphony import expect_voices, place, set_voices
from test_gpu_resample import FORMAT, Guarded, set_tables
from test_gpu_sampler import Assets, device_render, expect_output
from test_sampler_abi import rec

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
CALLS = (1, 2, 63, 64, 65, 256, 7)


def _torch():
    import torch
    return torch


def set_filters(b, filters, load=True):
    for k in range(filters.shape[0]):
        rows = filters[k].copy()
        if load:
            rows["flags"] |= bref.LOAD
        b.set_filters(rows, lane=k)


def get_filters(b):
    return np.stack([b.get_filters(lane=k) for k in range(b.polyphony)])


def expect_filters(b, want, label):
    got = get_filters(b)
    for name in bref.DTYPE.names:
        a, w = got[name], want[name]
        same = bool((a == w).all()) if a.dtype.kind == "u" else same_bits(np.ascontiguousarray(a), np.ascontiguousarray(w))[0]
        assert same, f"{label}: field {name} of the filters differs at (lane, instance) {np.argwhere((a.view(np.uint32) != w.view(np.uint32)).reshape(a.shape[0], a.shape[1], -1).any(axis=2))[:6].tolist()}"


def run_calls(b, records, envelopes, resamplers, filters, tables, pcm, sizes, label, kernel="k_biquad_rows", **kw):
    """One render per size, each against the restatement, with all four records of every voice read back after every call.  Returns (the
    outputs side by side, the records, the envelopes, the filters)."""
    state, env_state, f_state, outs = records, envelopes, filters, []
    for frames in sizes:
        want, state, env_state, f_state = bref.render(state, env_state, resamplers, f_state, tables, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        assert b.last_render_kernel() == kernel
        expect_output(got, want, f"{label}, {frames} frames")
        expect_voices(b, state, env_state, resamplers, f"{label}, after {frames} frames")
        expect_filters(b, f_state, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), state, env_state, f_state


def named(placed):
    names, records, envelopes, resamplers, pcm = pcases.named_voices(2)
    records = records.copy()
    records["data"] = place(placed, pcm)
    records["data"][(records["flags"] & sref.PLAYING) == 0] = 0
    return names, records, envelopes, resamplers, pcm, bcases.named_filters(names)


def test_the_voices_the_contract_names():
    """polyphony_cases.named_voices under biquad_cases.named_filters: 8 stereo instances of 4 lanes in calls of 1, 2, 63, 64, 65, 256 and
    7 frames, and in one call of their sum on a twin; then, between three more calls, a coefficient change without LOAD (the histories
    carry), a LOAD of zeros (they do not), and a LOAD followed by a set without it before any render."""
    placed = Guarded()
    names, records, envelopes, resamplers, pcm, filters = named(placed)
    tables = cases.tables()
    where = {names[k][i]: (k, i) for k in range(pcases.LANES) for i in range(pcases.INSTANCES)}
    _torch().cuda.synchronize()
    with Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as b, Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as twin:
        for batch in (b, twin):
            set_tables(batch, tables)
            batch.set_polyphony(pcases.LANES)
            set_voices(batch, records, envelopes, resamplers)
            set_filters(batch, filters)
        expect_filters(b, filters, "as set: LOAD is not shown")
        parts, state, env_state, f_state = run_calls(b, records, envelopes, resamplers, filters, tables, pcm, CALLS, "the named voices")
        whole, state1, env1, f1 = run_calls(twin, records, envelopes, resamplers, filters, tables, pcm, (sum(CALLS),), "one call of the sum")
        assert same_bits(parts, whole)[0] and state.tobytes() == state1.tobytes() and env_state.tobytes() == env1.tobytes() and f_state.tobytes() == f1.tobytes()
        # the idle instance rings out of the loaded histories and nothing else
        assert np.abs(parts[5, :300]).min() > 0 and not (state["flags"][:, 5] & sref.PLAYING).any()
        alone, _ = bref.filter_one(filters[1][5], np.zeros((sum(CALLS), 2), f32), 2)
        assert same_bits(parts[5], alone + f32(0.0))[0]
        # the one-shot has ended, and its filter has run on over the silence behind it
        k, i = where["a one-shot that ends in mid-call"]
        assert not state[k][i]["flags"] & sref.PLAYING and (f_state[k][i]["x"][:2] == 0).all()
        assert not np.isnan(parts).any(), "a guard frame was read"
        assert f_state[2][6].tobytes() == filters[2][6].tobytes(), "a record that is not ACTIVE is not touched"
        # a coefficient change on a sounding voice: the histories carry
        before = b.filter_uploads()
        at = where["plain u8"]
        change = bcases.filt(bcases.low_pass(0.3, 0.7), x=np.full((8, 2), 9.0, f32))
        b.set_filters(change, instances=[at[1]], lane=at[0])
        bcases.set_model(f_state, change, at[0], [at[1]])
        assert (f_state[at]["x"][:2] != 9).all()
        expect_filters(b, f_state, "a set without LOAD keeps the device's histories")
        _, state, env_state, f_state = run_calls(b, state, env_state, resamplers, f_state, tables, pcm, (65,), "new coefficients, old histories")
        # LOAD of zeros: they do not
        at = where["plain fp32"]
        clean = bcases.filt(bcases.low_pass(0.05), flags=bref.ACTIVE | bref.LOAD)
        b.set_filters(clean, instances=[at[1]], lane=at[0])
        bcases.set_model(f_state, clean, at[0], [at[1]])
        assert (f_state[at]["y"] == 0).all() and f_state[at]["flags"] == bref.ACTIVE
        _, state, env_state, f_state = run_calls(b, state, env_state, resamplers, f_state, tables, pcm, (65,), "LOAD of zeros")
        # LOAD, then a set without it before any render: the pending histories and the new coefficients
        at = where["nearest samples, no table"]
        loaded = bcases.filt(bcases.low_pass(0.1), flags=bref.ACTIVE | bref.LOAD, x=np.full((8, 2), 0.25, f32), y=np.full((8, 2), -0.125, f32))
        again = bcases.filt(bcases.band_pass(0.2), x=np.full((8, 2), 7.0, f32))
        for r in (loaded, again):
            b.set_filters(r, instances=[at[1]], lane=at[0])
            bcases.set_model(f_state, r, at[0], [at[1]])
        assert (f_state[at]["x"] == 0.25).all() and f_state[at]["b1"] == 0
        expect_filters(b, f_state, "LOAD, then a set without it")
        run_calls(b, state, env_state, resamplers, f_state, tables, pcm, (65,), "LOAD, then a set without it")
        assert b.filter_uploads() == before + 3


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_every_channel_count_and_store_width_at_three_lanes(channels, offset):
    """9 instances (a partial third workgroup) of 3 lanes, random voices, six in ten of them filtered with random histories in all eight
    channels; the destination 0, 1 and 2 floats off its allocation.  Histories of channels at and above the channel count come back as
    they were set."""
    rng = np.random.default_rng(5000 + 10 * channels + offset)
    calls = (70, 200, 3)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 9, 3, channels, True, calls=calls, asset_frames=(1, 500))
    filters = bcases.random_filters(rng, 3, 9)
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(9, FORMAT[channels], 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(3)
        set_voices(b, records, envelopes, resamplers)
        set_filters(b, filters)
        parts, _, _, after = run_calls(b, records, envelopes, resamplers, filters, cases.tables(), pcm, calls, f"{channels} channels, offset {offset}", offset=offset)
        assert np.abs(parts).max() > 0
        assert after["x"][:, :, channels:].tobytes() == filters["x"][:, :, channels:].tobytes() and after["y"][:, :, channels:].tobytes() == filters["y"][:, :, channels:].tobytes()
        active = (filters["flags"] & bref.ACTIVE) != 0
        assert (after["y"][active][:, :channels] != filters["y"][active][:, :channels]).any()


def test_one_lane_filtered_and_unfiltered_instances_side_by_side():
    """K = 1: the unfiltered instances have k_fir_rows' bits of a twin batch; the filtered ones the restatement's."""
    rng = np.random.default_rng(11)
    calls = (100, 29, 64)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 10, 1, 2, True, calls=calls, asset_frames=(1, 400))
    filters = bcases.random_filters(rng, 1, 10, share=0.0)
    filters["flags"][0, ::3] = bref.ACTIVE
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    tables = cases.tables()
    with Batch(10, desc.FMT_STEREO, 48000, 1) as b, Batch(10, desc.FMT_STEREO, 48000, 1) as twin:
        for batch in (b, twin):
            set_tables(batch, tables)
            set_voices(batch, records, envelopes, resamplers)
        set_filters(b, filters)
        parts, _, _, _ = run_calls(b, records, envelopes, resamplers, filters, tables, pcm, calls, "one lane")
        theirs = np.concatenate([device_render(twin, frames) for frames in calls], axis=1)
        assert twin.last_render_kernel() == "k_fir_rows"
        plain = np.arange(10) % 3 != 0
        assert same_bits(parts[plain], theirs[plain])[0] and np.abs(parts[plain]).max() > 0
        assert not same_bits(parts[~plain], theirs[~plain])[0]
        assert b.get_samplers().tobytes() == twin.get_samplers().tobytes() and b.get_envelopes().tobytes() == twin.get_envelopes().tobytes()


def test_a_lone_negative_zero_stays_negative_at_one_lane():
    """The stated order turns most -0.0f inputs into +0.0f by itself ((-0) + (0 * x1) is +0 unless the product is -0 as well), an identity
    filter (b0 = 1, the rest 0) included, which runs here on a voice whose asset holds -0.0f.  So a y_f that IS -0.0f is made from
    silence: b0 = -1, the other coefficients -0.0f, output histories of -0.0f: every product is then -0 where it is added and +0 where it
    is subtracted, and every y_f is -0.0f.  At one lane it is stored as it is; at two it reaches the input as +0.0f."""
    torch = _torch()
    pcm = np.asarray([[-0.0], [0.5], [-0.0], [-0.25], [-0.0], [-0.0]], f32)
    asset = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    r = rec(data=asset.data_ptr(), format=sref.PCM_F32, frames=6, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=6, step=ONE)
    alone, _, _ = ref.render(r, np.zeros(1, vref.DTYPE), [ref.NONE], {}, [pcm], 70, 2)
    identity = bcases.filt(bcases.IDENTITY, flags=bref.ACTIVE | bref.LOAD)
    through, _ = bref.filter_one(identity[0], alone[0], 2)
    assert (through == alone[0]).all()
    minus = bcases.filt((-1.0, -0.0, -0.0, -0.0, -0.0), flags=bref.ACTIVE | bref.LOAD, y=np.full((8, 2), -0.0, f32))
    silent = np.zeros(1, sref.DTYPE)
    silent["channels"] = 1
    want, after = bref.filter_one(minus[0], np.zeros((70, 2), f32), 2)
    assert (want.view(np.uint32) == 0x80000000).all() and (after["y"][:2].view(np.uint32) == 0x80000000).all()
    with Batch(2, desc.FMT_STEREO, 48000, 1) as one, Batch(2, desc.FMT_STEREO, 48000, 1) as two:
        two.set_polyphony(2)
        for b in (one, two):
            b.set_samplers(np.concatenate([r, silent]))
            b.set_filters(np.concatenate([identity, minus]))
        got_one, got_two = device_render(one, 70), device_render(two, 70)
        assert one.last_render_kernel() == two.last_render_kernel() == "k_biquad_rows"
        assert same_bits(got_one[0], through)[0] and same_bits(got_two[0], through + f32(0.0))[0], "the identity filter"
        assert (got_one[1].view(np.uint32) == 0x80000000).all(), "-0.0f at one lane"
        assert (got_two[1].view(np.uint32) == 0).all(), "+0.0f at two lanes"
        assert (one.get_filters()["y"][1, :2].view(np.uint32) == 0x80000000).all() and one.get_filters().tobytes() == two.get_filters().tobytes()


@pytest.mark.parametrize("through", ["all sixteen", "lane 9 alone"])
def test_sixteen_lanes_on_five_instances(through):
    rng = np.random.default_rng(160 + len(through))
    calls = (100, 29, 7)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 5, 16, 2, True, calls=calls, asset_frames=(1, 400))
    filters = bcases.random_filters(rng, 16, 5, share=1.0)
    if through != "all sixteen":
        filters["flags"] = 0
        filters["flags"][9] = bref.ACTIVE
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(5, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(16)
        set_voices(b, records, envelopes, resamplers)
        set_filters(b, filters)
        parts, _, _, _ = run_calls(b, records, envelopes, resamplers, filters, cases.tables(), pcm, calls, through)
        assert np.abs(parts).max() > 0


def test_a_ring_out_of_6000_frames_is_not_flushed():
    """An idle voice's filter rings out of its histories in calls of 256 frames: the restatement's output is denormal for thousands of
    frames and never reaches zero, so a device that flushed denormals would differ."""
    filters = np.zeros((2, 3), bref.DTYPE)
    filters[1][1] = bcases.filt(bcases.low_pass(0.05, 0.2), x=np.full((8, 2), 0.5, f32), y=np.full((8, 2), 0.25, f32))[0]
    want, _ = bref.filter_one(filters[1][1], np.zeros((6000, 2), f32), 2)
    tiny = (want != 0) & (np.abs(want) < np.finfo(f32).tiny)
    assert tiny.sum() > 2 * 2000 and (want[-1] != 0).all()
    records, envelopes, resamplers = np.zeros((2, 3), sref.DTYPE), np.zeros((2, 3), vref.DTYPE), np.full((2, 3), ref.NONE)
    records["channels"] = 1
    with Batch(3, desc.FMT_STEREO, 48000, 1) as b:
        b.set_polyphony(2)
        set_filters(b, filters)
        state, outs = filters, []
        for frames in [256] * 23 + [112]:
            expected, _, _, state = bref.render(records, envelopes, resamplers, state, {}, [[None] * 3] * 2, frames, 2)
            got = device_render(b, frames)
            expect_output(got, expected, "ringing out")
            outs.append(got)
        expect_filters(b, state, "after 6000 frames")
        out = np.concatenate(outs, axis=1)
        assert same_bits(out[1], want + f32(0.0))[0] and (out[[0, 2]].view(np.uint32) == 0).all()


def test_inf_and_nan_in_one_lane_stay_in_their_instance_and_in_that_voices_histories():
    torch = _torch()
    rng = np.random.default_rng(6)
    special = np.tile(np.asarray([1.0, np.inf, 2.0, -0.0, np.nan, 1e-39, 3e38, -3e38, 0.5, -np.inf, 0.25, 0.75], f32).reshape(-1, 1), (1, 2))
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 6, 3, 2, False, calls=(50, 50, 50), asset_frames=(20, 200))
    filters = bcases.random_filters(rng, 3, 6, share=1.0)
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    held = torch.from_numpy(special).cuda()
    torch.cuda.synchronize()
    records[1][2] = rec(data=held.data_ptr(), format=sref.PCM_F32, channels=2, frames=12, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=0, loop_end=12, step=ONE // 3)[0]
    records["gain"][1][2][:2] = (0.5, -2.0)
    pcm[1][2] = special
    resamplers[1][2] = ref.NONE
    tables = cases.tables()
    with Batch(6, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(3)
        set_voices(b, records, envelopes, resamplers)
        set_filters(b, filters)
        out, _, _, after = run_calls(b, records, envelopes, resamplers, filters, tables, pcm, (150,), "Inf and NaN in lane 1 of instance 2")
    assert np.isnan(out[2]).any() and not np.isnan(np.delete(out, 2, axis=0)).any() and np.abs(np.delete(out, 2, axis=0)).max() > 0
    finite = np.isfinite(after["y"][:, :, :2]).all(axis=(2, 3))
    assert not finite[1][2] and finite.sum() == finite.size - 1


def test_the_launch_follows_the_active_filters():
    rng = np.random.default_rng(8)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 10, 4, 2, True, calls=(40, 40, 40, 40), asset_frames=(50, 300))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    tables = cases.tables()
    filters = np.zeros((4, 10), bref.DTYPE)
    with Batch(10, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(4)
        set_voices(b, records, envelopes, resamplers)
        _, state, env_state, _ = run_calls(b, records, envelopes, resamplers, filters, tables, pcm, (40,), "no filter", kernel="k_mix_rows")
        assert b.filter_uploads() == 0
        for k, at in ((0, [1, 5]), (2, [0, 9, 3]), (3, list(range(10)))):
            rows = bcases.random_filters(rng, 1, len(at), share=1.0)[0]
            rows["flags"] |= bref.LOAD
            b.set_filters(rows, instances=at, lane=k)
            bcases.set_model(filters, rows, k, at)
        assert b.filter_uploads() == 0, "nothing goes to the device before a render"
        _, state, env_state, filters = run_calls(b, state, env_state, resamplers, filters, tables, pcm, (40,), "rows set in lanes 0, 2 and 3")
        assert b.filter_uploads() == 1, "one launch for the rows of every lane"
        _, state, env_state, filters = run_calls(b, state, env_state, resamplers, filters, tables, pcm, (40,), "a second render")
        assert b.filter_uploads() == 1, "a render after which nothing was set put records on the device"
        # the last ACTIVE bit cleared: the former kernel again, in the same batch
        for k in range(4):
            rows = filters[k].copy()
            rows["flags"] = 0
            b.set_filters(rows, lane=k)
            bcases.set_model(filters, rows, k, range(10))
        run_calls(b, state, env_state, resamplers, filters, tables, pcm, (40,), "no ACTIVE filter left", kernel="k_mix_rows")
        with pytest.raises(BatchError, match="Lane out of range."):
            b.set_filters(filters[0], lane=4)
        with pytest.raises(BatchError, match="Lane out of range."):
            b.get_filters(lane=-1)


def test_set_polyphony_carries_the_filters_in_the_middle_of_a_sound():
    rng = np.random.default_rng(24)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 6, 4, 2, True, calls=(50, 50, 50), asset_frames=(100, 300))
    filters = bcases.random_filters(rng, 4, 6, share=1.0)
    records[2:], envelopes[2:], resamplers[2:], filters[2:] = np.zeros(1, sref.DTYPE), np.zeros(1, vref.DTYPE), ref.NONE, np.zeros(1, bref.DTYPE)
    records["channels"][2:] = 1
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    records["data"][2:] = 0
    tables = cases.tables()
    with Batch(6, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(2)
        set_voices(b, records[:2], envelopes[:2], resamplers[:2])
        set_filters(b, filters[:2])
        _, state, env_state, f_state = run_calls(b, records[:2], envelopes[:2], resamplers[:2], filters[:2], tables, pcm[:2], (50,), "two lanes")
        # (a row set since the render and not yet on the device is carried as well)
        change = bcases.filt(bcases.low_pass(0.25))
        b.set_filters(change, instances=[3], lane=1)
        bcases.set_model(f_state, change, 1, [3])
        uploads = b.filter_uploads()
        b.set_polyphony(4)
        assert b.polyphony == 4 and b.filter_uploads() == uploads
        wide = lambda a: np.concatenate([a, np.zeros((2, 6), a.dtype)])
        state, env_state, f_state = wide(state), wide(env_state), wide(f_state)
        expect_filters(b, f_state, "behind set_polyphony")
        _, state, env_state, f_state = run_calls(b, state, env_state, resamplers, f_state, tables, pcm, (50,), "four lanes")
        # a dropped lane with an ACTIVE filter is in use
        b.set_filters(bcases.filt(bcases.low_pass(0.1)), instances=[4], lane=3)
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use."):
            b.set_polyphony(3)
        assert b.polyphony == 4
        b.set_filters(bcases.filt(flags=0), instances=[4], lane=3)
        b.set_polyphony(2)
        assert b.polyphony == 2
        run_calls(b, state[:2], env_state[:2], resamplers[:2], f_state[:2], tables, pcm[:2], (50,), "two lanes again")


def test_play_downmix_meter_with_two_filtered_lanes_in_four():
    """16 instances of 4 lanes, two of them filtered per instance, under an EAX reverb with its defaults, into 2 buses, calls of 256
    frames with carried meters: the inputs are the restatement's, the outputs the oracle's, buses and meters downmix_ref's and
    meter_ref's over them."""
    n, lanes, n_buses, frames = 16, 4, 2, 256
    threshold = f32(1e-4)
    rng = np.random.default_rng(166)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, n, lanes, 2, True, calls=(frames,) * 3, asset_frames=(500, 3000), max_step=3 * ONE)
    filters = bcases.random_filters(rng, lanes, n, share=1.0, histories=False)
    for i in range(n):
        filters["flags"][rng.permutation(lanes)[:2], i] = 0
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    resamplers = np.where(np.isin(resamplers, (cases.TINY, cases.TINY + 1)), 0, resamplers)
    tables = cases.tables()
    bus, gain = rng.integers(0, n_buses, n), rng.uniform(0.2, 1, n).astype(f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect(0, make_effect(desc.EAX_REVERB))
        b.apply_changes()
        army = ShadowArmy(b)
        b.set_routing(bus, gain)
        set_tables(b, tables)
        b.set_polyphony(lanes)
        set_voices(b, records, envelopes, resamplers)
        set_filters(b, filters)
        state, env_state, f_state = records, envelopes, filters
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        for k in range(3):
            x, state, env_state, f_state = bref.render(state, env_state, resamplers, f_state, tables, pcm, frames, 2)
            y = army.mix(x)
            want_buses = downmix(y, bus, gain, n_buses)
            want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
            assert b.last_render_kernel() == "k_biquad_rows"
            ok, nbad = same_bits(got, want_buses)
            assert ok, f"call {k}: {nbad} bus samples differ"
            assert meter_ref.same_records(vm, want_v) and meter_ref.same_records(bm, want_b), f"call {k}: the meters' records"
            expect_voices(b, state, env_state, resamplers, f"call {k}")
            expect_filters(b, f_state, f"call {k}")
        assert np.abs(got).max() > 0


def test_api_array_biquad(tmp_path):
    """tests/cpp/api_array_biquad.cpp: ApiArray::set_voice_filter and get_voice_filter, one round trip through a render."""
    exe = str(tmp_path / "api_array_biquad")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_biquad.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
