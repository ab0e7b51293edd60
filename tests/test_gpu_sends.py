"""GPU: the bus sends (oalsfx_batch_set_send_routing, _get_send_routing, _set_send_ramps and what they do to every downmix call;
include/oalsfx_hip.h, "bus sends") against their NumPy restatement (tests/sends_ref.py).  Every comparison is on the bit patterns (NaNs
by position) and on the exact integers; there is no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import meter_ref
import sampler_ref
import sends_ref
from downmix_ref import downmix
from harness import ROOT, ShadowArmy, preset_effect
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, Batch, BatchError
from sends_ref import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = {1: desc.FMT_MONO, 2: desc.FMT_STEREO, 6: desc.FMT_5POINT1, 7: desc.FMT_6POINT1, 8: desc.FMT_7POINT1}


def _torch():
    import torch
    return torch


class Pair:
    """A batch and the restatement of its sends, given the same calls."""

    def __init__(self, b):
        self.b, self.ref = b, sends_ref.Sends(b.n)

    def route(self, send, first, bus=None, gain=None):
        self.b.set_routing(bus, gain, first=first, send=send)
        self.ref.set_routing(send, first, bus, None if gain is None else np.asarray(gain, f32))

    def ramp(self, send, first, gain_to, frames):
        self.b.set_send_ramps(gain_to, frames, first=first, send=send)
        self.ref.set_ramps(send, first, np.asarray(gain_to, f32), frames)

    def check_get(self, label):
        for i in range(self.b.n):
            for send in range(sends_ref.SENDS):
                got, want = self.b.get_send(i, send), self.ref.get(i, send)
                same = got[0] == want[0] and got[3] == want[3] and f32(got[1]).tobytes() == f32(want[1]).tobytes() and f32(got[2]).tobytes() == f32(want[2]).tobytes()
                assert same, f"{label}: instance {i}, send {send}: {got} for {want}"
        assert [self.b.get_routing(i) for i in range(self.b.n)] == [self.b.get_send(i, 0)[:2] for i in range(self.b.n)]

    def downmix(self, x, n_buses, label, offset=0, stream=None):
        """One downmix_device call over host x, [n][frames][channels], `offset` floats off the allocations, against the restatement."""
        torch = _torch()
        frames = x.shape[1]
        src = torch.empty(x.size + offset, dtype=torch.float32, device="cuda")
        src[offset:] = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(-1)
        count = n_buses * frames * self.b.channels
        dst = torch.full((count + offset + 8,), 777.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.b.downmix_device(frames, src.data_ptr() + 4 * offset, n_buses, dst.data_ptr() + 4 * offset, stream=stream)
        self.b.synchronize()
        torch.cuda.synchronize()
        host = dst.cpu().numpy()
        assert (host[:offset] == 777.0).all() and (host[offset + count:] == 777.0).all(), "the downmix wrote outside the bus buffer"
        got = host[offset:offset + count].reshape(n_buses, frames, self.b.channels)
        want = self.ref.downmix(x, n_buses)
        bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        assert bad.size == 0, f"{label}: {len(bad)} of {got.size} elements differ, first at (bus, frame, channel) {bad[0].tolist()}"
        return got


def random_routing(pair, rng, buses=3):
    """Send 0 mostly to bus 0, the others anywhere or nowhere; bus `buses` gets exactly 33 members through sends 1..3 of the first eleven
    instances, bus `buses + 1` none; instance 20 is in bus 0 twice."""
    n = pair.b.n
    for send in range(sends_ref.SENDS):
        weights = np.asarray([1.0, 7.0] + [1.0] * (buses - 1) if send == 0 else [4.0] + [2.0] * buses)
        bus = rng.choice(np.arange(-1, buses), n, p=weights / weights.sum())
        if send:
            bus[:11] = buses
        pair.route(send, 0, bus, rng.uniform(-1, 1, n).astype(f32))
    pair.route(0, 20, [0])
    pair.route(1, 20, [0])
    pair.route(2, 11, [0])  # (bus `buses` keeps its 33: instance 11 was never in it)


def test_sends_without_ramps():
    """70 instances, random sends into three buses, a bus of 33 members and one of none; misaligned buffers at every vector width; the
    table is uploaded once."""
    n, frames, n_buses = 70, 65, 5
    rng = np.random.default_rng(1)
    so = lib.load()
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        pair = Pair(b)
        random_routing(pair, rng)
        assert len(pair.ref.members(3)) == 33 and not pair.ref.members(4) and len(pair.ref.members(0)) > 32
        assert pair.ref.members(0).count((20, 0)) == 1 and pair.ref.members(0).count((20, 1)) == 1
        pair.check_get("as set")
        x = rng.standard_normal((n, frames, 2)).astype(f32)
        first = pair.downmix(x, n_buses, "first call")
        assert first[4].view(np.uint32).max() == 0, "a bus without members is +0.0f"
        uploads = b.downmix_uploads()
        again = pair.downmix(x, n_buses, "second call")
        assert same_bits(first, again) and b.downmix_uploads() == uploads, "an unchanged call sent the table again"
        try:
            for width in (1, 2, 4):
                so.oalsfx_debug_downmix_vector(width)
                for offset in (0, 1, 2, 3):
                    x4 = rng.standard_normal((n, 64, 2)).astype(f32)
                    pair.downmix(x4, n_buses, f"{width} floats per access, {offset} floats off", offset=offset)
        finally:
            so.oalsfx_debug_downmix_vector(4)
        assert b.downmix_uploads() == uploads
        with pytest.raises(BatchError, match=r"Instance 0, send 1 is routed to bus 3; the call has 3\."):
            b.downmix_device(frames, 0x1000, 3, 0x100000)
        pair.route(0, 0, [4])
        with pytest.raises(BatchError, match=r"Instance 0 is routed to bus 4; the call has 3\."):
            b.downmix_device(frames, 0x1000, 3, 0x100000)
        c = __import__("ctypes")
        assert not so.oalsfx_batch_set_send_routing(b._h, 4, 0, 1, (c.c_int * 1)(0), None) and b.error == "Send out of range."
        assert not so.oalsfx_batch_set_send_routing(b._h, 1, 0, 2, (c.c_int * 2)(1, -2), None) and b.error == "Bus number is out of range."
        assert not so.oalsfx_batch_set_send_ramps(b._h, 1, 0, 1, (c.c_float * 1)(0.5), 2 ** 24 + 1) and b.error == "Ramp length out of range."
        assert not so.oalsfx_batch_set_send_ramps(b._h, 1, n - 1, 2, (c.c_float * 2)(0.5, 0.5), 16)
        pair.check_get("after the refusals")


@pytest.mark.parametrize("channels", [1, 2, 6, 7, 8])
def test_ramps_over_calls_and_in_one(channels):
    """Ramps of 0, 1, 5, 64, 100 and 1000 frames over calls of 7, 64, 1 and 228 frames and over one call of 300: the same bits.  Then a
    gain that cancels a ramp, a ramp restarted in mid-ramp and a new bus alone, which keeps its ramp running."""
    n, n_buses, lengths = 70, 3, (0, 1, 5, 64, 100, 1000)
    rng = np.random.default_rng(20 + channels)
    with Batch(n, FORMATS[channels], 48000, 1) as b, Batch(n, FORMATS[channels], 48000, 1) as whole:
        pair, one = Pair(b), Pair(whole)
        for p in (pair, one):
            r = np.random.default_rng(30 + channels)
            random_routing(p, r, buses=2)
            for send in range(sends_ref.SENDS):
                for i in range(n):
                    if (i + send) % 3:
                        p.ramp(send, i, [r.uniform(-1, 1)], lengths[(i + 2 * send) % len(lengths)])
        pair.check_get("as set")
        x = rng.standard_normal((n, 300, channels)).astype(f32)
        parts, at = [], 0
        for frames in (7, 64, 1, 228):
            parts.append(pair.downmix(x[:, at:at + frames], n_buses, f"the call of {frames} frames"))
            at += frames
            pair.check_get(f"after the call of {frames} frames")
        together = one.downmix(x, n_buses, "one call of 300 frames")
        one.check_get("after one call of 300 frames")
        assert same_bits(np.concatenate(parts, axis=1), together)
        still = [(i, s) for s in range(sends_ref.SENDS) for i in range(n) if pair.ref.frames[s, i]]
        assert len(still) >= 6 and all(pair.ref.frames[s, i] == 1000 and pair.ref.done[s, i] == 300 for i, s in still)
        routed = [(i, s) for i, s in still if pair.ref.bus[s, i] >= 0]
        (i0, s0), (i1, s1), (i2, s2) = routed[:3]
        pair.route(s0, i0, None, [0.25])                                  # a gain: the ramp is gone
        pair.ramp(s1, i1, [-0.5], 100)                                   # restarted in mid-ramp: from where it was
        pair.route(s2, i2, [(int(pair.ref.bus[s2, i2]) + 1) % n_buses])    # a new bus alone: the ramp runs on
        assert pair.ref.get(i0, s0)[3] == 0 and pair.ref.get(i1, s1)[3] == 100 and pair.ref.get(i2, s2)[3] == 700
        pair.check_get("after the three changes")
        for frames in (99, 1, 65):
            pair.downmix(rng.standard_normal((n, frames, channels)).astype(f32), n_buses, f"after the changes, {frames} frames")
            pair.check_get(f"after the changes, {frames} frames")
        # every ramp ended or cancelled: the table goes back to the plain kernels with one more upload, then stays
        for p in (pair,):
            for s in range(sends_ref.SENDS):
                p.route(s, 0, None, np.linspace(-1, 1, n).astype(f32))
        pair.downmix(x[:, :64], n_buses, "no ramp left")
        uploads = b.downmix_uploads()
        pair.downmix(x[:, 64:129], n_buses, "no ramp left, again")
        assert b.downmix_uploads() == uploads


def test_the_table_goes_back_to_the_plain_pass_when_the_last_ramp_has_ended():
    n = 40
    rng = np.random.default_rng(5)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        pair = Pair(b)
        pair.route(1, 0, [0] * n, rng.uniform(0, 1, n).astype(f32))
        pair.ramp(1, 0, rng.uniform(0, 1, n).astype(f32), 100)
        pair.ramp(2, 0, [0.5], 1000)                      # routed nowhere: it runs, and keeps no kernel waiting
        x = rng.standard_normal((n, 64, 2)).astype(f32)
        pair.downmix(x, 1, "frames 0 .. 63")
        uploads = b.downmix_uploads()
        pair.downmix(x, 1, "frames 64 .. 127: the ramps end in this call")
        assert b.downmix_uploads() == uploads
        pair.downmix(x, 1, "the ramps have ended")
        assert b.downmix_uploads() == uploads + 1
        pair.downmix(x, 1, "and again")
        assert b.downmix_uploads() == uploads + 1
        assert pair.ref.get(0, 2)[3] == 1000 - 256
        pair.check_get("at the end")


def test_send_0_alone_is_the_downmix_of_before():
    n, frames = 300, 129
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n, frames, 2)).astype(f32)
    bus, gain = rng.integers(-1, 4, n), rng.uniform(-1, 1, n).astype(f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        pair = Pair(b)
        pair.route(0, 0, bus, gain)
        got = pair.downmix(x, 4, "send 0 only")
        assert same_bits(got, downmix(x, bus, gain, 4))
        pair.downmix(x, 4, "again")
        assert b.downmix_uploads() == 1


def test_the_kernels_a_downmix_launches(tmp_path):
    """What the bits cannot show -- rows of no frames give the plain kernels' bits -- a kernel trace does: tests/sends_launches.py, a
    child process under `rocprofv3 --kernel-trace`, makes downmix calls with send 0 only, with four sends and no ramp, with a ramp
    running and ended, and with a ramp on a send routed nowhere; the downmix kernels of the trace in launch order must be the old two
    wherever no routed send ramps, and k_downmix_ramp_chunks with the old level 2 while one does."""
    import csv
    import glob
    import re
    import shutil
    import sys

    import sends_launches
    tool = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    assert os.path.exists(tool), "no rocprofv3 here"
    r = subprocess.run([tool, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "-o", "sends", "--", sys.executable,
                        os.path.join(ROOT, "tests", "sends_launches.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    (trace,) = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    launches = []
    for row in csv.DictReader(open(trace)):
        name = re.search(r"k_downmix_\w+<\d+>", row["Kernel_Name"])
        if name:
            launches.append((int(row["Start_Timestamp"]), name.group(0)))
    got = [name for _, name in sorted(launches)]
    assert got == sends_launches.EXPECTED, got


def test_the_host_entry_points_advance_the_ramps():
    """mix_downmix_meter and play_downmix_meter with bus meters: the buses over the twin's per-instance outputs, the ramps moved on by the
    call's frames."""
    from test_gpu_sampler import playing
    n, n_buses, threshold = 24, 3, f32(0.05)
    rng = np.random.default_rng(7)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b, Batch(n, desc.FMT_STEREO, 48000, 1) as twin:
        for t in (b, twin):
            t.set_effect_type(0, desc.ECHO)
            t.apply_changes()
        pair = Pair(b)
        random_routing(pair, rng, buses=2)
        pair.ramp(0, 0, rng.uniform(0, 1, n).astype(f32), 300)
        pair.ramp(2, 0, rng.uniform(0, 1, n).astype(f32), 64)
        bm = np.zeros(n_buses, METER_DTYPE)
        want_b = np.zeros(n_buses, METER_DTYPE)
        records, pcm, assets = playing(rng, n, 2, asset_frames=(3000, 12000), max_step=2 * sampler_ref.ONE)
        b.set_samplers(records)
        state = records
        for k, frames in enumerate((100, 256, 37)):
            if k == 1:
                x, state = sampler_ref.render(state, pcm, frames, 2)
                got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, bus_meters=bm, voices=False)
            else:
                x = rng.uniform(-1, 1, (n, frames, 2)).astype(f32)
                got, _, _ = b.mix_downmix_meter(x, n_buses, threshold, carry=True, bus_meters=bm, voices=False)
            y = twin.mix(x)
            want = pair.ref.downmix(y, n_buses)
            want_b = meter_ref.meter(want, threshold, want_b)
            assert same_bits(got, want), f"call {k} ({frames} frames): the buses differ"
            assert meter_ref.same_records(bm, want_b), f"call {k}: the bus meters differ"
            pair.check_get(f"call {k}")
        assert pair.ref.get(0, 0)[3] == 0 and np.abs(got).max() > 0
        got = b.mix_downmix(x, n_buses)
        assert same_bits(got, pair.ref.downmix(twin.mix(x), n_buses))


def test_the_shared_reverb_topology():
    """Eight voices send to a master bus and to two room buses; the room buses are the device input of a second batch of two EAX reverbs,
    whose own downmix is the rooms' share of the master.  Two calls of 256 frames, nothing leaving the device in between, against the
    CPU oracle fed with the restatement's buses."""
    torch = _torch()
    n, frames = 8, 256
    rng = np.random.default_rng(8)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as a, Batch(2, desc.FMT_STEREO, 48000, 1) as rooms:
        rooms.set_effect(0, [preset_effect(5), preset_effect(26)])
        rooms.apply_changes()
        voices, wet = Pair(a), Pair(rooms)
        voices.route(0, 0, [0] * n, rng.uniform(0.5, 1, n).astype(f32))                 # dry, to the master
        voices.route(1, 0, [1] * n, rng.uniform(0, 0.5, n).astype(f32))                 # a send level per voice into room 1
        voices.route(2, 0, [2 if i % 2 else -1 for i in range(n)], rng.uniform(0, 0.5, n).astype(f32))
        voices.ramp(1, 0, [0.0] * 4, 300)                                               # four voices leave room 1, without a zipper
        wet.route(0, 0, [0, 0], [0.7, 0.4])
        voice_army, room_army = ShadowArmy(a), ShadowArmy(rooms)
        buses = torch.empty((3, frames, 2), dtype=torch.float32, device="cuda")
        for k in range(2):
            x = rng.uniform(-1, 1, (n, frames, 2)).astype(f32)
            d = torch.from_numpy(x).cuda()
            y = torch.empty_like(d)
            wet_out = torch.empty((2, frames, 2), dtype=torch.float32, device="cuda")
            share = torch.empty((1, frames, 2), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            a.mix_device(frames, d.data_ptr(), y.data_ptr())
            a.downmix_device(frames, y.data_ptr(), 3, buses.data_ptr())
            a.synchronize()
            rooms.mix_device(frames, buses[1:].data_ptr(), wet_out.data_ptr())
            rooms.downmix_device(frames, wet_out.data_ptr(), 1, share.data_ptr())
            rooms.synchronize()
            torch.cuda.synchronize()
            want_buses = voices.ref.downmix(voice_army.mix(x), 3)
            assert same_bits(buses.cpu().numpy(), want_buses), f"call {k}: the voices' buses"
            want_wet = room_army.mix(np.ascontiguousarray(want_buses[1:]))
            assert not room_army.differing(wet_out.cpu().numpy(), want_wet), f"call {k}: the rooms"
            assert same_bits(share.cpu().numpy(), wet.ref.downmix(want_wet, 1)), f"call {k}: the rooms' share of the master"
            voices.check_get(f"call {k}")
        assert np.abs(share.cpu().numpy()).max() > 0


def test_api_array_sends(tmp_path):
    """tests/cpp/api_array_sends.cpp: ApiArray::set_send, ramp_send and get_send against sums the program computes itself."""
    exe = str(tmp_path / "api_array_sends")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "api_array_sends.cpp"),
                    "-L", libdir, "-loalsfx_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
