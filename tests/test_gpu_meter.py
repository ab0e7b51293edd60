"""GPU: the level meters (oalsfx_batch_meter_device, oalsfx_batch_mix_downmix_meter, the group and ApiArray forms; include/oalsfx_hip.h,
"level meters") against their NumPy restatement (tests/meter_ref.py).  Every comparison is on the bit patterns (NaNs by position) and on
the exact integers; there is no tolerance anywhere.  No test provokes a device fault: every refusal is decided on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meter_ref
from downmix_ref import downmix, same_bits
from harness import ROOT, preset_effect
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, Batch, BatchError, Group

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_5POINT1_REAR, desc.FMT_6POINT1, desc.FMT_7POINT1]
FRAMES = [1, 37, 64, 65, 256, 441, 2048, 5000]
RECORD = METER_DTYPE.itemsize
GARBAGE = 0xAB


def _torch():
    import torch
    return torch


def device_meter(b, x, threshold, carry=False, old=None, stream=None, offset=0):
    """x: host [rows][frames][channels]; `offset`: floats by which the source is shifted from its allocation; old: the records at the
    destination before the call (None: garbage).  Returns the records after the call; the records' neighbours must be untouched."""
    torch = _torch()
    rows, frames = x.shape[0], x.shape[1]
    src = torch.empty(x.size + offset, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(-1)
    host = np.full((rows + 2) * RECORD, GARBAGE, dtype=np.uint8)
    if old is not None:
        host[RECORD:-RECORD] = np.ascontiguousarray(old).view(np.uint8)
    dst = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    b.meter_device(rows, frames, src.data_ptr() + 4 * offset, dst.data_ptr() + RECORD, threshold, carry=carry, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:RECORD] == GARBAGE).all() and (host[-RECORD:] == GARBAGE).all(), "the meter wrote outside its records"
    return host[RECORD:-RECORD].view(METER_DTYPE).copy()


def expect(got, want, label):
    assert meter_ref.same_records(got, want), f"{label}: first difference (row, field, got, want) {meter_ref.first_difference(got, want)}"


def check(b, x, threshold, label, **kw):
    got = device_meter(b, x, threshold, **kw)
    expect(got, meter_ref.meter(x, threshold, kw.get("old") if kw.get("carry") else None), label)
    return got


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_rows_and_frames(fmt):
    ch = desc.FORMAT_CHANNELS[fmt]
    r = np.random.default_rng(fmt)
    with Batch(4, fmt, 48000, 1) as b:      # (the rows of a meter call are free: they need not be the batch's instances)
        for rows in (1, 3, 64):
            for frames in FRAMES:
                x = r.standard_normal((rows, frames, ch)).astype(f32)
                got = check(b, x, 2.0, f"format {fmt}, {rows} rows, {frames} frames")
                assert (got["frames"] == frames).all() and (got["peak"][:, ch:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("fmt, frames", [(f, 256) for f in FORMATS] + [(desc.FMT_STEREO, 441), (desc.FMT_STEREO, 2048), (desc.FMT_MONO, 5000),
                                                                      (desc.FMT_QUAD, 65), (desc.FMT_7POINT1, 1), (desc.FMT_6POINT1, 37)])
def test_4096_rows(fmt, frames):
    ch = desc.FORMAT_CHANNELS[fmt]
    x = np.random.default_rng(1000 * fmt + frames).standard_normal((4096, frames, ch)).astype(f32)
    with Batch(4, fmt, 48000, 1) as b:
        check(b, x, 1.5, f"4096 rows, format {fmt}, {frames} frames")


@pytest.mark.parametrize("fmt", FORMATS)
def test_buffers_at_odd_float_offsets(fmt):
    """Sources 4, 8, 12, 16, ... bytes off the allocation: every load width is taken, and the records are the same whatever it is."""
    ch = desc.FORMAT_CHANNELS[fmt]
    x = np.random.default_rng(50 + fmt).standard_normal((70, 300, ch)).astype(f32)
    with Batch(4, fmt, 48000, 1) as b:
        aligned = check(b, x, 1.0, "aligned")
        for offset in (1, 2, 3, 4, 5, 6):
            shifted = check(b, x, 1.0, f"format {fmt}, offset {offset}", offset=offset)
            assert shifted.tobytes() == aligned.tobytes() or meter_ref.same_records(shifted, aligned)


def test_special_values_at_known_places():
    frames, ch = 200, 2
    r = np.random.default_rng(3)
    x = (r.standard_normal((12, frames, ch)) * 0.1).astype(f32)
    x[0, 5, 1] = np.nan                 # ignored by the peak, counted, loud, and the channel's sum is NaN
    x[1, 199, 0] = np.inf               # the last frame
    x[2, 64, 1] = -np.inf               # lane 0's second frame
    x[3, :, :] = f32(1e-41)             # a row of denormals: the peak keeps them, their squares underflow
    x[4, :, :] = f32(-0.0)
    x[5, :, :] = f32(2.0 ** -70)        # squares that are denormal themselves
    x[6, 0, 0], x[6, 63, 1], x[6, 128, 0] = np.nan, np.inf, -np.nan
    x[7, :, 0] = np.nan                 # a channel of NaNs only: its peak stays +0.0f
    x[8, 100:, :] = 0.0
    x[8, 150, 1] = f32(1e-45)           # the smallest denormal is loud at a threshold of 0
    x[9, :, :] = f32(3e38)              # squares overflow to +Inf; the elements are finite
    x[10, 7, 0], x[10, 7, 1] = np.inf, -np.inf
    with Batch(4, desc.FMT_STEREO, 48000, 1) as b:
        for threshold in (0.0, 0.05, 1e30, np.inf):
            got = check(b, x, threshold, f"special values, threshold {threshold}")
        got = check(b, x, 0.0, "special values, threshold 0")
        assert got["nonfinite"].tolist() == [1, 1, 1, 0, 0, 0, 3, frames, 0, 0, 2, 0]
        assert got["peak"][0, 1] < 1 and np.isnan(got["sumsq"][0, 1]) and np.isfinite(got["sumsq"][0, 0])
        assert got["peak"][1, 0] == np.inf and got["quiet_run"][1] == 0
        assert got["peak"][3, 0].tobytes() == f32(1e-41).tobytes() and got["sumsq"][3].view(np.uint32).max() == 0
        assert got[4].tobytes()[:68] == bytes(68) and got["quiet_run"][4] == frames      # -0.0: peak, sums and hold +0.0f, all quiet at 0
        assert got["sumsq"][5, 0] != 0 and got["sumsq"][5, 0] < f32(1e-38)
        assert got["peak"][7, 0].tobytes() == f32(0.0).tobytes() and got["quiet_run"][7] == 0
        assert got["quiet_run"][8] == frames - 1 - 150
        assert got["sumsq"][9, 0] == np.inf and got["nonfinite"][9] == 0


@pytest.mark.parametrize("frames", [64, 65, 200, 2049])
def test_quiet_tails_around_lane_and_block_boundaries(frames):
    """One row per tail length T: the last loud frame is loud in one channel only and only just (the next float above the threshold),
    the tail is as loud as a quiet frame may be."""
    threshold = f32(0.01)
    tails = sorted({t for t in (0, 1, 2, 62, 63, 64, 65, 127, 128, 129, frames - 65, frames - 64, frames - 2, frames - 1, frames) if 0 <= t <= frames})
    r = np.random.default_rng(frames)
    x = r.uniform(0.02, 1.0, (len(tails), frames, 2)).astype(f32) * r.choice(np.array([-1, 1], dtype=f32), (len(tails), frames, 2))
    for k, t in enumerate(tails):
        x[k, frames - t:, :] = threshold * r.choice(np.array([-1, 1, 0.5, 0], dtype=f32), (t, 2))
        if t < frames:
            x[k, frames - 1 - t, :] = [0.0, -np.nextafter(threshold, f32(1))] if k % 2 else [np.nextafter(threshold, f32(1)), 0.001]
    with Batch(4, desc.FMT_STEREO, 48000, 1) as b:
        got = check(b, x, threshold, f"tails in {frames} frames")
        assert got["quiet_run"].tolist() == tails
        # continued from records that had 1000 quiet frames: only the all-quiet row goes on counting
        old = np.zeros(len(tails), METER_DTYPE)
        old["quiet_run"] = 1000
        got = check(b, x, threshold, "tails with carry", carry=True, old=old)
        assert got["quiet_run"].tolist() == [t if t < frames else 1000 + frames for t in tails]


def test_carry_over_a_sequence_of_calls():
    rows = 130
    r = np.random.default_rng(7)
    threshold = f32(0.05)
    with Batch(4, desc.FMT_STEREO, 48000, 1) as b:
        running = np.zeros(rows, METER_DTYPE)
        want = running.copy()
        garbage = np.frombuffer(np.full(rows * RECORD, GARBAGE, np.uint8).tobytes(), dtype=METER_DTYPE)
        for k, frames in enumerate([256, 64, 37, 441, 256, 1, 2048, 256, 65, 256]):
            x = (r.standard_normal((rows, frames, 2)) * 0.5).astype(f32)
            x[r.random(rows) < 0.6] *= f32(0.001)         # most rows are quiet throughout in a given call
            x[5] = 0.0
            if k == 3:
                x[6, 17, 0] = np.nan
            want = meter_ref.meter(x, threshold, want)
            running = device_meter(b, x, threshold, carry=True, old=running)
            expect(running, want, f"call {k} with carry")
            # the same call without carry never reads the destination: the garbage there is gone, and the record is the call's own
            alone = device_meter(b, x, threshold, carry=False, old=garbage)
            expect(alone, meter_ref.meter(x, threshold), f"call {k} without carry over garbage")
            assert (alone["quiet_run"] <= frames).all()
        assert running["quiet_run"][5] == 256 + 64 + 37 + 441 + 256 + 1 + 2048 + 256 + 65 + 256
        assert (running["peak_hold"] >= running["peak"].max(axis=1)).all()
        # saturation
        old = np.zeros(3, METER_DTYPE)
        old["quiet_run"] = [0xFFFFFFFF - 10, 0xFFFFFFFF - 64, 0xFFFFFFFF]
        old["peak_hold"] = [np.nan, 3.0, 0.0]
        got = check(b, np.zeros((3, 64, 2), f32), threshold, "saturation", carry=True, old=old)
        assert got["quiet_run"].tolist() == [0xFFFFFFFF] * 3 and got["peak_hold"].tolist() == [0.0, 3.0, 0.0]


def reverb_batch(n):
    b = Batch(n, desc.FMT_STEREO, 48000, 1)
    b.set_effect(0, [preset_effect((5 * i) % 113) for i in range(n)])
    b.apply_changes()
    return b


@pytest.mark.parametrize("own_stream", [True, False])
def test_on_real_outputs_and_the_effect_path_is_untouched(own_stream):
    """72 EAX reverbs of mixed presets, an impulse and then silence: mix_device -> downmix_device -> meter_device on the voices and on the
    buses, on the batch's stream or on a caller's; the records equal the restatement over the outputs copied out, quiet_run with carry
    grows by `frames` per call once a tail is under the threshold, and outputs and states are those of a run without any meter call."""
    torch = _torch()
    n, frames, n_buses, calls = 72, 256, 3, 40
    threshold = f32(0.005)
    r = np.random.default_rng(80)
    bus = r.integers(0, n_buses, n)
    gain = r.uniform(0.2, 1, n).astype(f32)
    impulse = np.zeros((n, frames, 2), f32)
    impulse[:, 3:11, :] = 0.9
    outs, blobs = [], []
    for metered in (True, False):
        with reverb_batch(n) as b:
            b.set_routing(bus, gain)
            side = torch.cuda.Stream()
            stream = None if own_stream else side.cuda_stream
            vm = torch.zeros(n * RECORD, dtype=torch.uint8, device="cuda")
            bm = torch.zeros(n_buses * RECORD, dtype=torch.uint8, device="cuda")
            want_v, want_b = np.zeros(n, METER_DTYPE), np.zeros(n_buses, METER_DTYPE)
            ys, grown = [], 0
            for k in range(calls):
                d = torch.from_numpy(impulse if k == 0 else np.zeros_like(impulse)).cuda()
                y = torch.empty_like(d)
                out = torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                b.mix_device(frames, d.data_ptr(), y.data_ptr())
                if metered:
                    b.downmix_device(frames, y.data_ptr(), n_buses, out.data_ptr(), stream=stream)
                    b.meter_device(n, frames, y.data_ptr(), vm.data_ptr(), threshold, carry=True, stream=stream)
                    b.meter_device(n_buses, frames, out.data_ptr(), bm.data_ptr(), threshold, carry=True, stream=stream)
                    if stream:
                        side.synchronize()
                b.synchronize()
                ys.append(y.cpu().numpy())
                if metered:
                    before = want_v["quiet_run"].copy()
                    want_v = meter_ref.meter(ys[-1], threshold, want_v)
                    want_b = meter_ref.meter(downmix(ys[-1], bus, gain, n_buses), threshold, want_b)
                    assert same_bits(out.cpu().numpy(), downmix(ys[-1], bus, gain, n_buses))
                    got_v = vm.cpu().numpy().view(METER_DTYPE)
                    expect(got_v, want_v, f"call {k}, voices")
                    expect(bm.cpu().numpy().view(METER_DTYPE), want_b, f"call {k}, buses")
                    silent = np.abs(ys[-1]).max(axis=(1, 2)) <= threshold
                    assert (got_v["quiet_run"][silent] == before[silent] + frames).all()
                    grown += int((silent & (before >= frames)).sum())
            if metered:
                print("voices that went on being quiet, summed over the calls:", grown, "peak_hold:", want_v["peak_hold"].min(), want_v["peak_hold"].max())
                assert grown > 0, "no tail went under the threshold: the test did not see quiet_run grow over calls"
                assert (want_v["peak_hold"] > threshold).any() and (want_v["nonfinite"] == 0).all()
            nbytes = b.snapshot_bytes()
            blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            b.snapshot(None, blob.data_ptr(), nbytes)
            b.synchronize()
            outs.append(ys)
            blobs.append(blob.cpu().numpy())
    for k, (a, c) in enumerate(zip(*outs)):
        assert a.tobytes() == c.tobytes(), f"call {k}: the outputs differ from a run without meters"
    assert blobs[0].tobytes() == blobs[1].tobytes(), "the states differ from a run without meters"


def test_mix_downmix_meter():
    """Against a twin batch given the same calls through mix and mix_downmix: the buses are mix_downmix's, the voice records those of
    the restatement over mix's outputs -- also for a call of more than 2048 frames --, either meter left out, carry from call to call."""
    n, n_buses = 40, 4
    r = np.random.default_rng(90)
    bus = r.integers(-1, n_buses, n)
    gain = r.uniform(-1, 1, n).astype(f32)
    threshold = f32(0.1)
    with reverb_batch(n) as b, reverb_batch(n) as plain, reverb_batch(n) as twin:
        for t in (b, plain):
            t.set_routing(bus, gain)
        vm, bm = np.zeros(n, METER_DTYPE), np.zeros(n_buses, METER_DTYPE)
        want_v, want_b = vm.copy(), bm.copy()
        for k, frames in enumerate([256, 2500, 100, 4096 + 37, 256, 256]):
            x = r.uniform(-1, 1, (n, frames, 2)).astype(f32) * f32(0.0 if k >= 4 else 1.0)
            y = twin.mix(x)
            want_buses = plain.mix_downmix(x, n_buses)
            assert same_bits(want_buses, downmix(y, bus, gain, n_buses))
            if k == 2:      # without carry, into garbage, the voices only
                garbage = np.frombuffer(np.full(n * RECORD, GARBAGE, np.uint8).tobytes(), dtype=METER_DTYPE).copy()
                got_buses, gv, gb = b.mix_downmix_meter(x, n_buses, threshold, voice_meters=garbage, buses=False)
                assert gb is None and gv is garbage
                expect(gv, meter_ref.meter(y, threshold), f"call {k}: voices only, no carry")
            elif k == 3:    # the buses only, fresh records
                got_buses, gv, gb = b.mix_downmix_meter(x, n_buses, threshold, voices=False)
                assert gv is None
                expect(gb, meter_ref.meter(want_buses, threshold), f"call {k}: buses only")
            else:
                got_buses, gv, gb = b.mix_downmix_meter(x, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
                assert gv is vm and gb is bm
                want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
                expect(vm, want_v, f"call {k} ({frames} frames): voices")
                expect(bm, want_b, f"call {k} ({frames} frames): buses")
            assert got_buses.tobytes() == want_buses.tobytes(), f"call {k}: the buses differ from mix_downmix's"
        assert (vm["frames"] == 256).all()
        # both meters left out: mix_downmix itself
        x = r.uniform(-1, 1, (n, 64, 2)).astype(f32)
        got_buses, gv, gb = b.mix_downmix_meter(x, n_buses, threshold, voices=False, buses=False)
        assert gv is None and gb is None and got_buses.tobytes() == plain.mix_downmix(x, n_buses).tobytes()
        twin.mix(x)
        x = r.uniform(-1, 1, (n, 300, 2)).astype(f32)
        # one array for the voices and the buses behind them
        both = np.zeros(n + n_buses, METER_DTYPE)
        y = twin.mix(x)
        got_buses, gv, gb = b.mix_downmix_meter(x, n_buses, threshold, voice_meters=both[:n], bus_meters=both[n:])
        want_buses = plain.mix_downmix(x, n_buses)
        expect(both, np.concatenate([meter_ref.meter(y, threshold), meter_ref.meter(want_buses, threshold)]), "one array for both")


def test_group_of_two_shards_against_one_batch():
    n, frames, n_buses = 90, 256, 3
    r = np.random.default_rng(70)
    bus = r.integers(-1, n_buses, n)
    gain = r.uniform(-1, 1, n).astype(f32)
    threshold = f32(0.3)
    with Group(n, [0, 0], desc.FMT_STEREO, 48000, 1) as g, Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        for t in (g, b):
            t.set_effect_type(0, desc.ECHO)
            t.apply_changes()
            t.set_routing(bus, gain)
        assert [(f, c) for _, f, c in g.shards] == [(0, 45), (45, 45)]
        gm, vm = np.zeros(n, METER_DTYPE), np.zeros(n, METER_DTYPE)
        for k in range(4):
            x = r.uniform(-1, 1, (n, frames, 2)).astype(f32) * f32(k < 2)
            x[50] *= f32(0.01)
            group_buses, got = g.mix_downmix_meter(x, n_buses, threshold, carry=True, voice_meters=gm)
            _, want, _ = b.mix_downmix_meter(x, n_buses, threshold, carry=True, voice_meters=vm, buses=False)
            assert got is gm and got.tobytes() == want.tobytes(), f"call {k}: the group's voice records differ from one batch's"
        assert gm["quiet_run"][50] >= 2 * frames
        fp = C.POINTER(C.c_float)
        for threshold, flags, what in ((-1.0, 0, "threshold"), (float("nan"), 0, "threshold"), (0.5, 2, "Unknown meter flags")):
            before = gm.tobytes()
            assert not lib.load().oalsfx_group_mix_downmix_meter(g._h, frames, x.ctypes.data_as(fp), n_buses, group_buses.ctypes.data_as(fp), threshold, flags,
                                                                 C.c_void_p(gm.ctypes.data))
            assert what in lib.load().oalsfx_group_error(g._h).decode() and gm.tobytes() == before


def test_refusals_leave_the_records_and_the_batch_alone():
    torch = _torch()
    rows, frames = 64, 32
    x = np.random.default_rng(50).standard_normal((rows, frames, 2)).astype(f32)
    so = lib.load()
    with Batch(rows, desc.FMT_STEREO, 48000, 1) as b:
        src = torch.from_numpy(x).cuda()
        dst = torch.full((rows * RECORD,), GARBAGE, dtype=torch.uint8, device="cuda")
        s, d = src.data_ptr(), dst.data_ptr()

        def refused(message, rows_=rows, frames_=frames, src_=s, threshold=0.5, flags=0, dst_=d):
            ok = so.oalsfx_batch_meter_device(b._h, rows_, frames_, C.c_void_p(src_), threshold, flags, C.c_void_p(dst_), None)
            assert not ok and message in b.error, (message, b.error)

        refused("No source samples", src_=0)
        refused("No meter records", dst_=0)
        refused("Row count", rows_=0)
        refused("Row count", rows_=-1)
        refused("Frame count is negative", frames_=-1)
        refused("threshold", threshold=-1e-30)
        refused("threshold", threshold=float("nan"))
        refused("threshold", threshold=float("-inf"))
        refused("Unknown meter flags", flags=2)
        refused("Unknown meter flags", flags=-2)
        refused("4-byte aligned", src_=s + 2)
        refused("16-byte aligned", dst_=d + 8)
        refused("overlap", dst_=s + 16 * 10)                                  # the records inside the source
        refused("overlap", src_=d + 16, frames_=1, rows_=4)                   # the source inside the records
        refused("too large for one launch", rows_=1 << 30, frames_=1)
        b.meter_device(rows, 0, 0, 0, 0.5)      # no frames: succeeds, writes nothing
        with pytest.raises(BatchError, match="threshold"):
            b.mix_downmix_meter(x, 1, -1.0)
        assert not so.oalsfx_batch_mix_downmix_meter(b._h, frames, x.ctypes.data_as(C.POINTER(C.c_float)), 1, x.ctypes.data_as(C.POINTER(C.c_float)),
                                                     0.5, 8, C.c_void_p(0), C.c_void_p(0)) and "Unknown meter flags" in b.error
        b.synchronize()
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == GARBAGE).all(), "a refused call wrote to the records"
        check(b, x, 0.5, "the batch after the refusals")
        check(b, x, 0.5, "on the batch's stream by name", stream=b.stream)


def test_api_array_meters(tmp_path):
    """tests/cpp/api_array_meters.cpp: both forms of ApiArray::mix_to_buses_metered against records the program computes itself, in the
    stated order, from forty separate oalsfxpp::Api objects' outputs."""
    exe = str(tmp_path / "api_array_meters")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "api_array_meters.cpp"),
                    "-L", libdir, "-loalsfx_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
