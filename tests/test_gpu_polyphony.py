"""GPU: polyphony (oalsfx_batch_set_polyphony, the lane forms of the record calls, and the renders of _sample_device and
_play_downmix_meter while the batch has two lanes or more; include/oalsfx_hip.h, "polyphony") against its restatement
(tests/polyphony_ref.py).  Every comparison is on the bit patterns (NaNs by position) and on the exact integers, outputs and the 3 * K
records of every instance; there is no tolerance anywhere.  No test provokes a device fault: every refusal is decided on the host, and
the assets of the named voices lie inside larger allocations, so that a read outside an asset would show as a wrong value and not as a
fault.  The shapes are the smallest at which the kernel can still go wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meter_ref
import polyphony_cases as pcases
import polyphony_ref as pref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from downmix_ref import downmix
from harness import ROOT, ShadowArmy, make_effect, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, Batch, BatchError
from test_gpu_resample import FORMAT, Guarded, set_tables
from test_gpu_sampler import Assets, device_render, expect_output, expect_records
from test_gpu_voice import expect_envelopes
from test_sampler_abi import rec
from test_voice_abi import env

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
CALLS = pcases.CALLS


def place(assets, keys):
    """The device addresses of the voices' assets [lanes][n] (Assets: by pool key; Guarded: by the PCM itself)."""
    return np.asarray([[assets.address(k) for k in lane] for lane in keys], np.uint64)


def set_voices(b, records, envelopes, resamplers):
    for k in range(records.shape[0]):
        b.set_samplers(records[k], lane=k)
        b.set_envelopes(envelopes[k], lane=k)
        b.set_resamplers(resamplers[k], lane=k)


def get_voices(b):
    lanes = range(b.polyphony)
    return np.stack([b.get_samplers(lane=k) for k in lanes]), np.stack([b.get_envelopes(lane=k) for k in lanes]), np.stack([b.get_resamplers(lane=k) for k in lanes])


def expect_voices(b, state, env_state, resamplers, label):
    got, got_env, got_res = get_voices(b)
    for k in range(state.shape[0]):
        expect_records(got[k], state[k], f"{label}, lane {k}")
        expect_envelopes(got_env[k], env_state[k], f"{label}, lane {k}")
    assert (got_res == resamplers).all(), label


def run_calls(b, records, envelopes, resamplers, tables, pcm, sizes, label, set_them=True, **kw):
    """The voices set lane by lane, then one render per size, each against the restatement, with every lane's records read back after
    every call.  Returns (the outputs side by side, the records, the envelopes)."""
    if set_them:
        set_voices(b, records, envelopes, resamplers)
    state, env_state, outs = records, envelopes, []
    for frames in sizes:
        want, state, env_state = pref.render(state, env_state, resamplers, tables, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        assert b.last_render_kernel() == "k_mix_rows"
        expect_output(got, want, f"{label}, {frames} frames")
        expect_voices(b, state, env_state, resamplers, f"{label}, after {frames} frames")
        outs.append(got)
    return np.concatenate(outs, axis=1), state, env_state


def test_the_voices_the_contract_names():
    """polyphony_cases.named_voices: 8 stereo instances of 4 lanes -- idle voices, delays of 0, 1, 63, 64, 65 and 130 frames and one longer
    than the calls, a STOP that ends in mid-call, one-shots that end, a loop shorter than the taps, no table, 4 and 8 taps, mono and wide
    assets of every format -- in calls of 1, 63, 64, 65, 256 and 7 frames."""
    names, records, envelopes, resamplers, pcm = pcases.named_voices(2)
    tables = cases.tables()
    placed = Guarded()
    records = records.copy()
    records["data"] = place(placed, pcm)
    records["data"][(records["flags"] & sref.PLAYING) == 0] = 0
    _torch().cuda.synchronize()
    with Batch(pcases.INSTANCES, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(pcases.LANES)
        assert b.polyphony == pcases.LANES
        parts, after, env_after = run_calls(b, records, envelopes, resamplers, tables, pcm, CALLS, "the named voices")
    where = {names[k][i]: (k, i) for k in range(pcases.LANES) for i in range(pcases.INSTANCES)}
    assert (parts[5].view(np.uint32) == 0).all(), "an instance whose lanes are all idle is +0.0f"
    assert np.abs(parts[3]).max() > 0 and not np.isnan(parts).any(), "a guard frame was read"
    for name in ("a STOP ramp that ends in mid-call", "a one-shot that ends in mid-call", "delay 70 and a STOP of 200"):
        assert not after[where[name]]["flags"] & sref.PLAYING, name
    assert env_after[where["a delay longer than the calls"]]["delay"] == 1000 - sum(CALLS)


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_every_channel_count_and_store_width_at_three_lanes(channels, offset):
    """9 instances (a partial third workgroup) of 3 lanes, random voices; the destination 0, 1 and 2 floats off its allocation: 4, 1 and
    2 floats per access where the channel count allows them."""
    rng = np.random.default_rng(3000 + 10 * channels + offset)
    calls = (70, 200, 3)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 9, 3, channels, True, calls=calls, asset_frames=(1, 500))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(9, FORMAT[channels], 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(3)
        parts, _, _ = run_calls(b, records, envelopes, resamplers, cases.tables(), pcm, calls, f"{channels} channels, offset {offset}", offset=offset)
        assert np.abs(parts).max() > 0


@pytest.mark.parametrize("playing", ["lanes 0 and 15", "all sixteen"])
def test_sixteen_lanes_on_five_instances(playing):
    rng = np.random.default_rng(16 + len(playing))
    calls = (100, 29, 7)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 5, 16, 2, True, calls=calls, asset_frames=(1, 400))
    if playing != "all sixteen":
        records[1:15] = np.zeros(1, sref.DTYPE)
        records["channels"][1:15] = 1
        envelopes[1:15] = np.zeros(1, vref.DTYPE)
        resamplers[1:15] = ref.NONE
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(5, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(16)
        parts, _, _ = run_calls(b, records, envelopes, resamplers, cases.tables(), pcm, calls, playing)
        assert np.abs(parts).max() > 0


def test_one_call_of_300_frames_and_five_calls_on_a_twin():
    rng = np.random.default_rng(300)
    split = (1, 63, 64, 65, 107)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 12, 4, 2, True, calls=split, asset_frames=(1, 200))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    tables = cases.tables()
    with Batch(12, desc.FMT_STEREO, 48000, 1) as b, Batch(12, desc.FMT_STEREO, 48000, 1) as twin:
        for batch in (b, twin):
            set_tables(batch, tables)
            batch.set_polyphony(4)
            set_voices(batch, records, envelopes, resamplers)
        whole = device_render(b, 300)
        parts = np.concatenate([device_render(twin, frames) for frames in split], axis=1)
        assert sum(split) == 300 and same_bits(whole, parts)[0]
        for got, theirs in zip(get_voices(b), get_voices(twin)):
            assert got.tobytes() == theirs.tobytes()
        want, state, env_state = pref.render(records, envelopes, resamplers, tables, pcm, 300, 2)
        expect_output(whole, want, "one call of 300")
        expect_voices(b, state, env_state, resamplers, "one call of 300")
        assert np.abs(whole).max() > 0


def test_a_lone_negative_zero_is_negative_at_one_lane_and_positive_at_two():
    torch = _torch()
    pcm = np.asarray([[-0.0], [0.5], [-0.0], [-0.25], [-0.0], [-0.0]], f32)
    asset = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    r = rec(data=asset.data_ptr(), format=sref.PCM_F32, frames=6, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=6, step=ONE)
    none = np.zeros(1, vref.DTYPE)
    alone, _, _ = ref.render(r, none, [ref.NONE], {}, [pcm], 70, 2)
    minus = int((alone.view(np.uint32) == 0x80000000).sum())
    assert minus >= 2 * 40 and (alone != 0).any()
    with Batch(1, desc.FMT_STEREO, 48000, 1) as one, Batch(1, desc.FMT_STEREO, 48000, 1) as two:
        two.set_polyphony(2)
        for b in (one, two):
            b.set_samplers(r)
        got_one, got_two = device_render(one, 70), device_render(two, 70)
        assert one.last_render_kernel() == "k_sampler_rows" and two.last_render_kernel() == "k_mix_rows"
        expect_output(got_one, alone, "one lane")
        assert same_bits(got_one, alone)[0] and (got_one.view(np.uint32) == 0x80000000).sum() == minus, "-0.0f at one lane"
        assert not (got_two.view(np.uint32) == 0x80000000).any(), "+0.0f at two lanes"
        assert (got_two == got_one).all() and same_bits(got_two, got_one + f32(0.0))[0], "everything else is the same"
        assert one.get_samplers().tobytes() == two.get_samplers().tobytes() == two.get_samplers(lane=0).tobytes()


def test_inf_and_nan_in_one_lane_stay_in_their_instance():
    torch = _torch()
    rng = np.random.default_rng(6)
    special = np.tile(np.asarray([1.0, np.inf, 2.0, -0.0, np.nan, 1e-39, 3e38, -3e38, 0.5, -np.inf, 0.25, 0.75], f32).reshape(-1, 1), (1, 2))
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 6, 3, 2, False, calls=(50, 50, 50), asset_frames=(20, 200))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    held = torch.from_numpy(special).cuda()
    torch.cuda.synchronize()
    records[1][2] = rec(data=held.data_ptr(), format=sref.PCM_F32, channels=2, frames=12, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=0, loop_end=12, step=ONE // 3)[0]
    records["gain"][1][2][:2] = (0.5, -2.0)
    pcm[1][2] = special
    resamplers[1][2] = cases.FINE
    tables = cases.tables()
    with Batch(6, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(3)
        out, _, _ = run_calls(b, records, envelopes, resamplers, tables, pcm, (150,), "Inf and NaN in lane 1 of instance 2")
    assert np.isnan(out[2]).any() and not np.isnan(out[2]).all()
    assert not np.isnan(np.delete(out, 2, axis=0)).any() and np.abs(np.delete(out, 2, axis=0)).max() > 0


def test_life_cycle_of_the_lanes():
    rng = np.random.default_rng(77)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 6, 4, 2, True, calls=(50, 50, 50), asset_frames=(100, 300))
    records["flags"] |= sref.LOOP | sref.PLAYING
    records["loop_start"], records["loop_end"] = 0, records["frames"]
    records["position"] %= records["frames"].astype(np.uint64) << np.uint64(12)
    envelopes[:] = np.zeros(1, vref.DTYPE)
    resamplers[1:] = ref.NONE
    resamplers[0] = np.where(np.arange(6) % 2, ref.NONE, cases.FINE)
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    tables = cases.tables()
    with Batch(6, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        assert b.polyphony == 1
        with pytest.raises(BatchError, match="Lane out of range."):
            b.set_samplers(records[1], lane=1)
        with pytest.raises(BatchError, match="Lane out of range."):
            b.get_envelopes(lane=-1)
        for lanes in (0, 17):
            assert not lib.load().oalsfx_batch_set_polyphony(b._h, lanes) and "Polyphony out of range." in b.error
        # one lane: the kernels follow today's rules
        b.set_samplers(records[0])
        want, state = sref.render(records[0], pcm[0], 50, 2)
        expect_output(device_render(b, 50), want, "one lane, no table")
        assert b.last_render_kernel() == "k_sampler_rows"
        b.set_resamplers(resamplers[0])
        want, state, _ = ref.render(state, envelopes[0], resamplers[0], tables, pcm[0], 50, 2)
        expect_output(device_render(b, 50), want, "one lane, tables")
        assert b.last_render_kernel() == "k_fir_rows"
        # four lanes in mid-asset: lane 0 goes on from where it is, the new lanes are in the state after creation
        before = (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads())
        b.set_polyphony(4)
        b.set_polyphony(4)
        assert b.polyphony == 4 and (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads()) == before
        expect_records(b.get_samplers(lane=0), state, "lane 0 behind set_polyphony")
        for k in (1, 2, 3):
            assert not b.get_samplers(lane=k).tobytes().strip(b"\0") and not b.get_envelopes(lane=k).tobytes().strip(b"\0") and (b.get_resamplers(lane=k) == ref.NONE).all()
        want, state, _ = ref.render(state, envelopes[0], resamplers[0], tables, pcm[0], 50, 2)
        got = device_render(b, 50)
        assert b.last_render_kernel() == "k_mix_rows" and (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads()) == before
        expect_output(got, want + f32(0.0), "lane 0 alone under four lanes")
        expect_records(b.get_samplers(lane=0), state, "lane 0 alone under four lanes")
        # refusals of the lane calls
        with pytest.raises(BatchError, match="Lane out of range."):
            b.set_resamplers(resamplers[1], lane=4)
        with pytest.raises(BatchError, match="listed twice"):
            b.set_samplers(records[2][:2], instances=[1, 1], lane=2)
        idx, two = (C.c_int * 2)(1, 1), np.ascontiguousarray(records[2][:2])
        assert not lib.load().oalsfx_batch_set_lane_samplers(b._h, 2, idx, 2, C.c_void_p(two.ctypes.data)) and "An instance is listed twice as a sampler target." in b.error
        # a dropped lane in use: a PLAYING sampler, an ACTIVE envelope, a table index -- each alone
        idle = np.zeros(1, sref.DTYPE)
        idle["channels"] = 1
        b.set_samplers(records[3][4:5], instances=[4], lane=3)
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use."):
            b.set_polyphony(3)
        b.set_polyphony(4)
        assert b.polyphony == 4
        b.set_samplers(idle, instances=[4], lane=3)
        b.set_envelopes(env(delay=3), instances=[2], lane=2)
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use."):
            b.set_polyphony(2)
        b.set_polyphony(3)                          # lane 3 is free by now
        assert b.polyphony == 3
        b.set_envelopes(np.zeros(1, vref.DTYPE), instances=[2], lane=2)
        b.set_resamplers([cases.FINE + 1], instances=[0], lane=1)
        with pytest.raises(BatchError, match="A lane that would be dropped is still in use."):
            b.set_polyphony(1)
        with pytest.raises(BatchError, match="The FIR table is still named by an instance."):
            b.set_fir_table(cases.FINE + 1, None)
        assert b.polyphony == 3
        b.set_resamplers([ref.NONE], instances=[0], lane=1)
        # a voice in lane 1 that has played to its end no longer holds the lane
        shot = rec(data=int(records[1][0]["data"]), format=int(records[1][0]["format"]), channels=int(records[1][0]["channels"]), frames=int(records[1][0]["frames"]),
                   position=(int(records[1][0]["frames"]) - 1) << 12, step=ONE)
        b.set_samplers(shot, instances=[0], lane=1)
        with pytest.raises(BatchError, match="still in use"):
            b.set_polyphony(1)
        device_render(b, 8)
        state = b.get_samplers(lane=0)
        b.set_polyphony(1)
        assert b.polyphony == 1
        expect_records(b.get_samplers(), state, "lane 0 behind the return to one lane")
        # back at one lane the old kernels' names return
        want, state, _ = ref.render(state, envelopes[0], resamplers[0], tables, pcm[0], 50, 2)
        expect_output(device_render(b, 50), want, "one lane again")
        assert b.last_render_kernel() == "k_fir_rows"
        b.set_resamplers(np.full(6, ref.NONE))
        device_render(b, 3)
        assert b.last_render_kernel() == "k_sampler_rows"


def test_rows_of_any_lane_go_up_in_one_launch_per_table():
    rng = np.random.default_rng(8)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 10, 4, 2, True, calls=(40, 40, 40), asset_frames=(50, 300))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    tables = cases.tables()
    with Batch(10, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, tables)
        b.set_polyphony(4)
        counts = lambda: (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads())
        before = counts()
        held, held_env, held_res = np.zeros((4, 10), sref.DTYPE), np.zeros((4, 10), vref.DTYPE), np.full((4, 10), ref.NONE)
        assets_held = [[None] * 10 for _ in range(4)]
        for k, at in ((0, [1, 5]), (2, [0, 9, 3]), (3, list(range(10)))):
            b.set_samplers(records[k][at], instances=at, lane=k)
            b.set_envelopes(envelopes[k][at], instances=at, lane=k)
            b.set_resamplers(np.where(resamplers[k][at] == ref.NONE, cases.FINE, resamplers[k][at]), instances=at, lane=k)
            held[k][at], held_env[k][at], held_res[k][at] = records[k][at], envelopes[k][at], np.where(resamplers[k][at] == ref.NONE, cases.FINE, resamplers[k][at])
            for i in at:
                assets_held[k][i] = pcm[k][i]
        assert counts() == before, "nothing goes to the device before a render"
        want, state, env_state = pref.render(held, held_env, held_res, tables, assets_held, 40, 2)
        expect_output(device_render(b, 40), want, "rows set in lanes 0, 2 and 3")
        assert counts() == tuple(c + 1 for c in before), "one launch per table for the rows of every lane"
        want, state, env_state = pref.render(state, env_state, held_res, tables, assets_held, 40, 2)
        expect_output(device_render(b, 40), want, "a second render")
        assert counts() == tuple(c + 1 for c in before), "a render after which nothing was set put records on the device"
        expect_voices(b, state, env_state, held_res, "behind both renders")


def test_play_downmix_meter_with_four_lanes():
    """16 instances of 4 lanes under an EAX reverb with its defaults, into 2 buses, calls of 256 frames with carried meters: the
    instances' inputs are the restatement's sums, their outputs the oracle's, buses and meters downmix_ref's and meter_ref's over them."""
    n, lanes, n_buses, frames = 16, 4, 2, 256
    threshold = f32(1e-4)
    rng = np.random.default_rng(165)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, n, lanes, 2, True, calls=(frames,) * 3, asset_frames=(500, 3000), max_step=3 * ONE)
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    resamplers = np.where(np.isin(resamplers, (cases.TINY, cases.TINY + 1)), 0, resamplers)        # (audible voices for the meters)
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
        state, env_state = records, envelopes
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        for k in range(3):
            x, state, env_state = pref.render(state, env_state, resamplers, tables, pcm, frames, 2)
            y = army.mix(x)
            want_buses = downmix(y, bus, gain, n_buses)
            want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
            assert b.last_render_kernel() == "k_mix_rows"
            ok, nbad = same_bits(got, want_buses)
            assert ok, f"call {k}: {nbad} bus samples differ"
            assert meter_ref.same_records(vm, want_v) and meter_ref.same_records(bm, want_b), f"call {k}: the meters' records"
            expect_voices(b, state, env_state, resamplers, f"call {k}")
        assert np.abs(got).max() > 0


def test_64_instances_of_four_lanes_in_three_calls():
    rng = np.random.default_rng(64)
    calls = (256, 33, 128)
    records, envelopes, resamplers, pcm, keys, pool = pcases.random_voices(rng, 64, 4, 2, True, calls=calls, asset_frames=(1, 2000))
    assets = Assets(pool)
    records = records.copy()
    records["data"] = place(assets, keys)
    with Batch(64, desc.FMT_STEREO, 48000, 1) as b:
        set_tables(b, cases.tables())
        b.set_polyphony(4)
        parts, _, env_after = run_calls(b, records, envelopes, resamplers, cases.tables(), pcm, calls, "64 instances")
        assert np.abs(parts).max() > 0 and (env_after["sub"] != 0).any()


def test_api_array_polyphony(tmp_path):
    """tests/cpp/api_array_polyphony.cpp: ApiArray::set_polyphony and the (index, lane) overloads, one round trip through a render."""
    exe = str(tmp_path / "api_array_polyphony")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_polyphony.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
