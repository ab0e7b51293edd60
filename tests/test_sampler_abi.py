"""CPU checks of the samplers: the C ABI declares and exports them, the record is 80 bytes with the same offsets in C, ctypes and NumPy,
the constants are one value everywhere, the header states the arithmetic, the Python mirror refuses bad arguments before the library is
reached, the NumPy restatement computes what the header states (values worked out by hand, the split law, and orders other than the
stated one show), and the kernels keep nothing in scratch memory -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sampler_ref as ref
from oalsfxpp_amd import api, desc, lib
from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_set_samplers", "oalsfx_batch_get_samplers", "oalsfx_batch_sample_device", "oalsfx_batch_play_downmix_meter")
FIELDS = ("data", "position", "frames", "loop_start", "loop_end", "step", "format", "channels", "flags", "reserved", "gain")
OFFSETS = [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48]
f32 = np.float32
ONE = ref.ONE


def test_header_declares_and_the_mirror_binds_the_sampler_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in lib.SIGNATURES, name
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert re.search(r"\blong long oalsfx_debug_sampler_uploads\(", debug) and "oalsfx_debug_sampler_uploads" in lib.SIGNATURES
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert "A group (oalsfx_group_*) offers no samplers" in flat and "oalsfx_group_batch" in flat     # the group's limit is stated
    assert "oalsfx_batch_reset, _snapshot and _restore neither touch nor carry them" in flat         # ... and what the samplers are not
    assert "keeps one alive until" in flat                                                           # ... and who owns the assets
    for method in ("set_samplers", "get_samplers", "sample_device", "play_downmix_meter"):
        assert callable(getattr(api.Batch, method))


def test_the_library_exports_the_sampler_calls():
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + ("oalsfx_debug_sampler_uploads",):
        assert hasattr(so, name), name


def test_the_array_header_declares_the_sampler_methods():
    header = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool set_sampler\(int index, const oalsfx_sampler& sampler\);", header)
    assert re.search(r"bool get_sampler\(int index, oalsfx_sampler& sampler\);", header)
    assert re.search(r"bool play_to_buses_metered\(int sample_count, int bus_count, float\* dst_buses, float threshold, bool carry,\s+"
                     r"oalsfx_meter\* voice_meters, oalsfx_meter\* bus_meters\);", header)


def test_the_record_is_80_bytes_with_the_same_offsets_everywhere():
    src = r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "oalsfx_hip.h"
    #define O(f) offsetof(oalsfx_sampler, f)
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(oalsfx_sampler), O(data), O(position), O(frames), O(loop_start),
               O(loop_end), O(step), O(format), O(channels), O(flags), O(reserved), O(gain), _Alignof(oalsfx_sampler));
        printf("%d %d %d %d %d %d %d\n", OALSFX_SAMPLER_FRAC_BITS, OALSFX_PCM_U8, OALSFX_PCM_S16, OALSFX_PCM_F32, OALSFX_SAMPLER_PLAYING,
               OALSFX_SAMPLER_LOOP, OALSFX_SAMPLER_LINEAR);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 80 == C.sizeof(desc.Sampler) == api.SAMPLER_DTYPE.itemsize == ref.DTYPE.itemsize
    assert got[1:12] == OFFSETS and got[12] == 8
    assert [getattr(desc.Sampler, f).offset for f in FIELDS] == OFFSETS
    for dtype in (api.SAMPLER_DTYPE, ref.DTYPE):
        assert dtype.names == FIELDS and [dtype.fields[f][1] for f in FIELDS] == OFFSETS
    # the constants are one value everywhere
    assert got[13] == desc.SAMPLER_FRAC_BITS == api.SAMPLER_FRAC_BITS == ref.FRAC_BITS == 12
    assert got[14:17] == [desc.PCM_U8, desc.PCM_S16, desc.PCM_F32] == [ref.PCM_U8, ref.PCM_S16, ref.PCM_F32]
    assert got[17:20] == [desc.SAMPLER_PLAYING, desc.SAMPLER_LOOP, desc.SAMPLER_LINEAR] == [ref.PLAYING, ref.LOOP, ref.LINEAR] == [1, 2, 4]
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "sampler.hip")).read()
    assert "kFrac = OALSFX_SAMPLER_FRAC_BITS" in kernel


def test_the_header_states_the_arithmetic():
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read())
    for phrase in ("a + ((b - a) * mu)", "L0 + (q - L0) mod (L1 - L0)", "/ 32768.0F", "/ 128.0F", "q_f = wrap(P + f * step)",
                   "mu = (float)m * (1.0F / 4096.0F)", "position = wrap(P + F * step)", "out[f][c] = v_k * gain[c]",
                   "wrap(wrap(x) + y) == wrap(x + y)"):
        assert phrase in header, phrase


# ---- the Python mirror refuses before the library is reached ----
def _unopened(n=8, channels=2):
    """A Batch whose handle was never created: a check that let a call through would fail on the missing library, not with BatchError."""
    b = api.Batch.__new__(api.Batch)
    b.n = n
    b.channels = channels
    b._h = None
    b._lib = None
    return b


def rec(**fields):
    """One record: a playing one-shot S16 mono asset of 100 frames at its own rate with unit gains, unless told otherwise."""
    r = np.zeros(1, ref.DTYPE)
    base = dict(data=0x10000, position=0, frames=100, step=ONE, format=ref.PCM_S16, channels=1, flags=ref.PLAYING, gain=1.0)
    base.update(fields)
    for k, v in base.items():
        r[k] = v
    return r


@pytest.mark.parametrize("fields, what", [
    (dict(flags=8 | ref.PLAYING), "Unknown sampler flags"), (dict(flags=0x80000000), "Unknown sampler flags"),
    (dict(format=3), "Unknown sampler format"), (dict(format=0xFFFFFFFF, flags=0), "Unknown sampler format"),
    (dict(reserved=1), "reserved"), (dict(reserved=7, flags=0), "reserved"),
    (dict(channels=0), "channel count"), (dict(channels=4), "channel count"), (dict(channels=3, flags=0), "channel count"),
    (dict(data=0), "no data"), (dict(frames=0), "frame count"), (dict(frames=2 ** 31), "frame count"),
    (dict(data=0x10001), "not aligned"), (dict(data=0x10002, format=ref.PCM_F32), "not aligned"),
    (dict(flags=ref.PLAYING | ref.LOOP, loop_start=10, loop_end=10), "loop region"),
    (dict(flags=ref.PLAYING | ref.LOOP, loop_start=11, loop_end=10), "loop region"),
    (dict(flags=ref.PLAYING | ref.LOOP, loop_start=0, loop_end=101), "loop region"),
    (dict(position=100 * ONE), "past its end"), (dict(position=2 ** 63), "past its end"),
    (dict(flags=ref.PLAYING | ref.LOOP, loop_start=10, loop_end=50, position=50 * ONE), "past its end")])
def test_set_samplers_checks_its_records(fields, what):
    with pytest.raises(api.BatchError, match=what):
        _unopened().set_samplers(rec(**fields))
    with pytest.raises(api.BatchError, match=what):
        _unopened().set_samplers(np.concatenate([rec(), rec(**fields), rec()]), instances=[5, 1, 2])


def test_set_samplers_checks_its_instances_and_arrays():
    b = _unopened()
    for instances in ([8], [-1], [0, 9]):
        with pytest.raises(api.BatchError, match="out of bounds"):
            b.set_samplers(np.concatenate([rec()] * len(instances)), instances=instances)
    with pytest.raises(api.BatchError, match="out of bounds"):
        b.set_samplers(np.concatenate([rec()] * 9))
    with pytest.raises(api.BatchError, match="listed twice"):
        b.set_samplers(np.concatenate([rec()] * 3), instances=[1, 2, 1])
    with pytest.raises(api.BatchError, match="3 instances but 2 samplers"):
        b.set_samplers(np.concatenate([rec()] * 2), instances=[1, 2, 3])
    for bad in (np.zeros(2, api.METER_DTYPE), np.zeros((1, 2), ref.DTYPE), np.zeros(4, ref.DTYPE)[::2]):
        with pytest.raises(api.BatchError, match="the sampler array"):
            b.set_samplers(bad, instances=[0, 1])
    with pytest.raises(api.BatchError, match="sequence of desc.Sampler"):
        b.set_samplers([1.5, 2.5], instances=[0, 1])
    with pytest.raises(api.BatchError, match="out of bounds"):
        b.get_samplers([8])


@pytest.mark.parametrize("kwargs, what", [
    (dict(frames=-1), "Frame count is negative"), (dict(frames=2 ** 31), "Frame count is out of range"), (dict(dst_ptr=0), "No destination samples"),
    (dict(dst_ptr=0x1002), "4-byte aligned")])
def test_sample_device_checks_its_arguments(kwargs, what):
    args = dict(frames=16, dst_ptr=0x1000)
    args.update(kwargs)
    with pytest.raises(api.BatchError, match=what):
        _unopened().sample_device(**args)


def test_play_downmix_meter_checks_its_arguments():
    b = _unopened()
    with pytest.raises(api.BatchError, match="Bus count"):
        b.play_downmix_meter(16, 0, 0.0)
    with pytest.raises(api.BatchError, match="Frame count is negative"):
        b.play_downmix_meter(-1, 1, 0.0)
    for threshold in (-0.5, float("nan"), "loud"):
        with pytest.raises(api.BatchError, match="threshold"):
            b.play_downmix_meter(16, 1, threshold)
    with pytest.raises(api.BatchError, match="Unknown meter flags"):
        b.play_downmix_meter(16, 1, 0.0, carry=4)
    for meters in (np.zeros(7, api.METER_DTYPE), np.zeros(16, api.METER_DTYPE)[::2], [0] * 8):
        with pytest.raises(api.BatchError, match="the meter array"):
            b.play_downmix_meter(16, 1, 0.0, voice_meters=meters)
    with pytest.raises(api.BatchError, match="the meter array"):
        b.play_downmix_meter(16, 3, 0.0, bus_meters=np.zeros(2, api.METER_DTYPE))
    for dst in (np.zeros((2, 16, 2), f32), np.zeros((1, 16, 2), np.float64), np.zeros((1, 15, 2), f32)):
        with pytest.raises(api.BatchError, match="the bus array is"):
            b.play_downmix_meter(16, 1, 0.0, dst=dst)


# ---- the restatement against values worked out by hand ----
def _bits(value):
    return np.asarray(value, dtype=f32).tobytes()


def _mono(values, dtype):
    return np.asarray(values, dtype=dtype).reshape(-1, 1)


def _play(record, asset, frames, channels=1):
    out, after = ref.render_one(record[0], asset, frames, channels)
    return out, after


def test_the_conversions_of_u8_and_s16():
    out, _ = _play(rec(format=ref.PCM_U8, frames=3), _mono([0, 128, 255], np.uint8), 3)
    assert out[:, 0].tolist() == [-1.0, 0.0, 127.0 / 128.0] and _bits(out[1, 0]) == _bits(0.0)
    out, _ = _play(rec(frames=3), _mono([-32768, 32767, 1], np.int16), 3)
    assert out[:, 0].tolist() == [-1.0, 32767.0 / 32768.0, 2.0 ** -15]
    out, _ = _play(rec(format=ref.PCM_F32, frames=2), _mono([0.1, -3.5], f32), 2)
    assert ref.same_bits(out[:, 0], np.asarray([0.1, -3.5], f32))


def test_a_one_shot_interpolates_into_silence_and_finishes():
    # four frames at a step of three quarters: positions 0, 0.75, 1.5, 2.25, 3.0, 3.75 | 4.5 is past the end
    asset = _mono([16384, -16384, 8192, 32767], np.int16)      # 0.5, -0.5, 0.25, 32767 / 32768
    r = rec(frames=4, step=3 * ONE // 4, flags=ref.PLAYING | ref.LINEAR)
    out, after = _play(r, asset, 8)
    last = f32(32767.0 / 32768.0)
    want = [0.5, 0.5 + (-1.0 * 0.75), -0.5 + (0.75 * 0.5), 0.25 + float((last - f32(0.25)) * f32(0.25)), float(last),
            float(last + (f32(0.0) - last) * f32(0.75)), 0.0, 0.0]
    assert ref.same_bits(out[:, 0], np.asarray(want, f32))
    assert _bits(out[6, 0]) == _bits(0.0) and _bits(out[7, 0]) == _bits(0.0)
    # the finished record: position == E, PLAYING cleared, nothing else touched
    assert after["position"] == 4 * ONE and after["flags"] == ref.LINEAR
    for field in FIELDS:
        if field not in ("position", "flags"):
            assert ref.same_bits(after[field], r[0][field]), field
    # a finished record renders silence and stays as it is
    out2, after2 = ref.render_one(after, asset, 5, 1)
    assert not out2.view(np.uint32).any() and after2.tobytes() == after.tobytes()
    # exactly at the end after the call: frames 0 .. 3 played, nothing past the end, finished all the same
    out, after = _play(rec(frames=4), asset, 4)
    assert ref.same_bits(out[:, 0], ref.to_float(asset)[:, 0]) and after["position"] == 4 * ONE and after["flags"] == 0
    out, after = _play(rec(frames=4), asset, 3)
    assert after["position"] == 3 * ONE and after["flags"] == ref.PLAYING


def test_a_step_of_zero_holds():
    asset = _mono([0.0, 1.0, 3.0], f32)
    r = rec(format=ref.PCM_F32, frames=3, step=0, position=ONE + ONE // 2, flags=ref.PLAYING | ref.LINEAR)
    out, after = _play(r, asset, 5)
    assert out[:, 0].tolist() == [2.0] * 5 and after.tobytes() == r[0].tobytes()
    out, _ = _play(rec(format=ref.PCM_F32, frames=3, step=0, position=ONE + ONE // 2), asset, 5)
    assert out[:, 0].tolist() == [1.0] * 5          # without LINEAR the fraction is not looked at


def test_loops():
    asset = _mono(np.arange(10.0), f32)
    loop = dict(format=ref.PCM_F32, frames=10, loop_start=4, loop_end=7)
    # a start in front of loop_start plays into the loop
    out, after = _play(rec(flags=ref.PLAYING | ref.LOOP, position=2 * ONE, **loop), asset, 9)
    assert out[:, 0].tolist() == [2, 3, 4, 5, 6, 4, 5, 6, 4] and after["position"] == 5 * ONE and after["flags"] == ref.PLAYING | ref.LOOP
    # a step longer than the loop wraps as often as it must: 3 + 7k -> 3, then 4 + (10 - 4) % 3 = 4, 4 + 13 % 3 = 5, 4 + 20 % 3 = 6, 4 + 27 % 3 = 4
    out, after = _play(rec(flags=ref.PLAYING | ref.LOOP, position=3 * ONE, step=7 * ONE, **loop), asset, 5)
    assert out[:, 0].tolist() == [3, 4, 5, 6, 4] and after["position"] == (4 + 34 % 3) * ONE
    # j == loop_end reads loop_start: at 6.5 the neighbour of frame 6 is frame 4
    out, _ = _play(rec(flags=ref.PLAYING | ref.LOOP | ref.LINEAR, position=6 * ONE + ONE // 2, step=0, **loop), asset, 1)
    assert out[0, 0] == 6.0 + (4.0 - 6.0) * 0.5
    # ... and the loop may end with the asset: no read past it
    out, _ = _play(rec(flags=ref.PLAYING | ref.LOOP | ref.LINEAR, position=9 * ONE + ONE // 4, format=ref.PCM_F32, frames=10, loop_start=0, loop_end=10),
                   asset, 2)
    assert out[:, 0].tolist() == [9.0 + (0.0 - 9.0) * 0.25, 0.25]
    # fractions survive the wrap: 6.75 + 0.5 = 7.25 -> 4.25
    out, after = _play(rec(flags=ref.PLAYING | ref.LOOP | ref.LINEAR, position=6 * ONE + 3 * ONE // 4, step=ONE // 2, **loop), asset, 2)
    assert out[:, 0].tolist() == [6.0 + (4.0 - 6.0) * 0.75, 4.25] and after["position"] == 4 * ONE + 3 * ONE // 4


def test_non_finite_values_and_gains():
    asset = _mono([1.0, np.inf, 2.0], f32)
    # an Inf neighbour at m == 0: 1 + ((inf - 1) * 0) is NaN, the expression is evaluated as written
    out, _ = _play(rec(format=ref.PCM_F32, frames=3, flags=ref.PLAYING | ref.LINEAR), asset, 3)
    assert np.isnan(out[0, 0]) and np.isnan(out[1, 0]) and out[2, 0] == 2.0
    out, _ = _play(rec(format=ref.PCM_F32, frames=3), asset, 3)
    assert out[:, 0].tolist() == [1.0, np.inf, 2.0]                  # without LINEAR the neighbour is not looked at
    # a NaN gain; a gain of 0 on an Inf
    r = rec(format=ref.PCM_F32, frames=3, channels=1)
    r["gain"][0, :2] = [np.nan, 0.0]
    out, _ = _play(r, asset, 4, channels=2)
    assert np.isnan(out[:3, 0]).all() and out[0, 1] == 0.0 and np.isnan(out[1, 1])
    assert not out[3].view(np.uint32).any()                           # past the end: +0.0f whatever the gain
    # a stopped record is +0.0f whatever its gains
    r["flags"] = 0
    out, after = _play(r, asset, 4, channels=2)
    assert not out.view(np.uint32).any() and after.tobytes() == r[0].tobytes()


def test_negative_zero_and_denormals():
    asset = _mono([-0.0, -0.0, 1e-39, 0.0], f32)
    out, _ = _play(rec(format=ref.PCM_F32, frames=4), asset, 2)
    assert _bits(out[0, 0]) == _bits(-0.0)                            # -0 * 1 is -0
    out, _ = _play(rec(format=ref.PCM_F32, frames=4, flags=ref.PLAYING | ref.LINEAR), asset, 1)
    assert _bits(out[0, 0]) == _bits(0.0)                             # -0 + ((-0 - -0) * 0) = -0 + +0 = +0
    out, _ = _play(rec(format=ref.PCM_F32, frames=4, gain=-1.0), asset, 1)
    assert _bits(out[0, 0]) == _bits(0.0)
    # a denormal sample times a gain that keeps it denormal: nothing is flushed
    denormal = f32(1e-39)
    out, _ = _play(rec(format=ref.PCM_F32, frames=4, position=2 * ONE, gain=0.5), asset, 1)
    assert out[0, 0] == f32(denormal * f32(0.5)) != 0 and abs(out[0, 0]) < np.finfo(f32).tiny
    out, _ = _play(rec(format=ref.PCM_F32, frames=4, position=2 * ONE + ONE // 2, flags=ref.PLAYING | ref.LINEAR), asset, 1)
    assert out[0, 0] == f32(denormal + f32(f32(0.0) - denormal) * f32(0.5)) != 0


def test_a_mono_asset_is_panned_and_a_wide_one_goes_channel_by_channel():
    r = rec(format=ref.PCM_F32, frames=2)
    r["gain"][0, :2] = [0.25, 0.5]
    out, _ = _play(r, _mono([2.0, 4.0], f32), 2, channels=2)
    assert out.tolist() == [[0.5, 1.0], [1.0, 2.0]]
    r["channels"] = 2
    out, _ = _play(r, np.asarray([[2.0, 8.0], [4.0, 16.0]], f32), 2, channels=2)
    assert out.tolist() == [[0.5, 4.0], [1.0, 8.0]]


# ---- the split law ----
def random_records(rng, count, channels, assets_per_format=4, max_step=8 * ONE, asset_frames=(1, 700), cycle=False):
    """`count` seeded random playing records over a few random assets of every format, mono and `channels` wide: (records, the asset of
    every record, its number in the pool, the pool as [(format, asset channels, PCM)]).  `data` is left 0: a GPU test fills in where it
    put the asset.  cycle: asset, LINEAR and LOOP are taken in turn instead of drawn, so that few records cover every combination."""
    pool = []
    for fmt in (ref.PCM_U8, ref.PCM_S16, ref.PCM_F32):
        for k in sorted({1, channels}):
            for _ in range(assets_per_format):
                n = int(rng.integers(asset_frames[0], asset_frames[1] + 1))
                if fmt == ref.PCM_F32:
                    pcm = rng.standard_normal((n, k)).astype(f32)
                else:
                    info = np.iinfo(ref.PCM_DTYPE[fmt])
                    pcm = rng.integers(info.min, info.max + 1, (n, k)).astype(ref.PCM_DTYPE[fmt])
                pool.append((fmt, k, pcm))
    records = np.zeros(count, ref.DTYPE)
    assets, keys = [], []
    for r in range(count):
        key = r % len(pool) if cycle else int(rng.integers(len(pool)))
        fmt, k, pcm = pool[key]
        n = pcm.shape[0]
        linear, loop = ((r // len(pool)) % 2, (r // (2 * len(pool))) % 2) if cycle else (rng.random() < 0.5, rng.random() < 0.5)
        flags = ref.PLAYING | (ref.LINEAR if linear else 0)
        records[r]["frames"], records[r]["format"], records[r]["channels"] = n, fmt, k
        limit = n
        if loop:
            flags |= ref.LOOP
            start = int(rng.integers(0, n))
            records[r]["loop_start"], records[r]["loop_end"] = start, int(rng.integers(start + 1, n + 1))
            limit = int(records[r]["loop_end"])
        else:
            records[r]["loop_start"], records[r]["loop_end"] = rng.integers(0, 2 ** 32, 2)    # read only with LOOP
        records[r]["flags"] = flags
        records[r]["position"] = int(rng.integers(0, limit * ONE))
        records[r]["step"] = (0, ONE, int(rng.integers(0, max_step + 1)), int(rng.integers(ONE - 64, ONE + 65)))[int(rng.integers(4))]
        records[r]["gain"][:channels] = rng.uniform(-1.0, 1.0, channels).astype(f32)
        assets.append(pcm)
        keys.append(key)
    return records, assets, keys, pool


def test_any_split_of_a_call_gives_the_same_outputs_and_records():
    rng = np.random.default_rng(20)
    seen = set()
    for channels in (1, 2, 6):
        count = 1000 if channels == 2 else 100
        records, assets, _, _ = random_records(rng, count, channels)
        whole, after_whole = ref.render(records, assets, 2500, channels)
        parts, state = [], records
        for frames in (441, 256, 1, 1802):
            out, state = ref.render(state, assets, frames, channels)
            parts.append(out)
        assert ref.same_bits(np.concatenate(parts, axis=1), whole)
        assert ref.same_bits(state, after_whole)
        seen |= {(int(r["format"]), int(r["flags"]), int(r["channels"]) == 1) for r in records}
        finished = (after_whole["flags"] & ref.PLAYING) == 0
        assert finished.any() and not finished.all()
        assert (after_whole["position"][finished] == after_whole["frames"][finished].astype(np.uint64) * ONE).all()
    assert len(seen) == 3 * 4 * 2        # every format, looped and not, linear and not, mono and wide


# ---- the order is observable ----
def _stated_and_other_ways(a, b, m, gain):
    mu = m.astype(f32) * f32(1.0 / ONE)
    with np.errstate(invalid="ignore", over="ignore"):
        stated = ref.lerp(a, b, mu) * gain
        weights = (a * (f32(1.0) - mu) + b * mu) * gain
        fused = ((b - a).astype(np.float64) * mu.astype(np.float64) + a.astype(np.float64)).astype(f32) * gain     # (b - a) rounded, then one fma
        gain_first = ref.lerp(a * gain, b * gain, mu)
    return stated, {"a * (1 - mu) + b * mu": weights, "fma(b - a, mu, a)": fused, "gain before the interpolation": gain_first}


@pytest.mark.parametrize("fmt", [ref.PCM_S16, ref.PCM_F32])
def test_the_order_is_observable(fmt):
    """2^20 random pairs of neighbouring samples, m uniform in 0 .. 4095, gains uniform in 0.2 .. 1: three other ways of computing the value
    each differ from the stated one in more than 5 % of the outputs, so a kernel that computes another way cannot pass the GPU tests by
    luck.  (The fused form: the product and the sum in float64, rounded once.)"""
    rng = np.random.default_rng(7)
    count = 1 << 20
    if fmt == ref.PCM_S16:
        a, b = (ref.to_float(rng.integers(-32768, 32768, count).astype(np.int16)) for _ in range(2))
    else:
        a, b = (rng.standard_normal(count).astype(f32) for _ in range(2))
    m = rng.integers(0, ONE, count)
    gain = rng.uniform(0.2, 1.0, count).astype(f32)
    stated, others = _stated_and_other_ways(a, b, m, gain)
    shares = {name: float((other.view(np.uint32) != stated.view(np.uint32)).mean()) for name, other in others.items()}
    print(fmt, shares)
    for name, share in shares.items():
        assert share > 0.05, (name, shares)
    # ... and the restatement's render computes the stated one
    asset = np.stack([a[:1000], b[:1000]]).T.reshape(-1, 1).copy()     # a0 b0 a1 b1 ...
    for k in range(0, 1000, 97):
        r = rec(format=ref.PCM_F32, frames=2000, position=2 * k * ONE + int(m[k]), step=0, flags=ref.PLAYING | ref.LINEAR, gain=gain[k])
        assert _bits(ref.render_one(r[0], asset, 1, 1)[0][0, 0]) == _bits(stated[k])


def test_the_sampler_kernels_are_built_and_keep_nothing_in_scratch():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_sampler_")}
    # channels x floats per store: mono 1; stereo 1, 2; quad 1, 2, 4; 5.1 1, 2; 6.1 1; 7.1 1, 2, 4; and the kernel that puts set records in place
    assert sorted(ks) == sorted([f"k_sampler_rows<{c}, {v}>" for c, vs in ((1, (1,)), (2, (1, 2)), (4, (1, 2, 4)), (6, (1, 2)), (7, (1,)), (8, (1, 2, 4)))
                                 for v in vs] + ["k_sampler_upload"]), sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
