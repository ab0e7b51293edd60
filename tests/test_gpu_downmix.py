"""GPU: the bus downmix (oalsfx_batch_set_routing, oalsfx_batch_downmix_device, oalsfx_batch_mix_downmix, the group and ApiArray forms;
include/oalsfx_hip.h, "bus downmix") against its NumPy restatement (tests/downmix_ref.py).  Every comparison is on the bit patterns (NaNs
by position); there is no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from downmix_ref import downmix, downmix_shards, same_bits
from harness import ROOT, ShadowArmy, make_effect, preset_effect
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch, BatchError, Group

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_5POINT1_REAR, desc.FMT_6POINT1, desc.FMT_7POINT1]


def _torch():
    import torch
    return torch


def device_downmix(b, x, n_buses, stream=None, offset=0):
    """x: host [n][frames][channels]; `offset`: floats by which the source and the bus buffer are shifted from their allocations."""
    torch = _torch()
    frames = x.shape[1]
    src = torch.empty(x.size + offset, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(-1)
    count = n_buses * frames * b.channels
    dst = torch.full((count + offset + 8,), 777.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.downmix_device(frames, src.data_ptr() + 4 * offset, n_buses, dst.data_ptr() + 4 * offset, stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:offset] == 777.0).all() and (host[offset + count:] == 777.0).all(), "the downmix wrote outside the bus buffer"
    return host[offset:offset + count].reshape(n_buses, frames, b.channels)


def check(b, x, bus, gain, n_buses, label, **kw):
    got = device_downmix(b, x, n_buses, **kw)
    want = downmix(x, bus, gain, n_buses)
    bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, f"{label}: {len(bad)} of {got.size} elements differ, first at (bus, frame, channel) {bad[0].tolist()}"
    return got


def test_members_per_bus_from_none_to_4096():
    """Buses of 0, 1, 31, 32, 33, 1000 and 4096 members in one call, the members of each scattered over the batch, some instances nowhere."""
    sizes = [0, 1, 31, 32, 33, 1000, 4096]
    r = np.random.default_rng(10)
    bus = np.concatenate([np.full(c, k) for k, c in enumerate(sizes)] + [np.full(57, -1)])
    r.shuffle(bus)
    n = len(bus)
    x = r.standard_normal((n, 37, 2)).astype(f32)
    gain = r.uniform(-1.5, 1.5, n).astype(f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(bus, gain)
        assert b.get_routing(5) == (int(bus[5]), float(gain[5]))
        got = check(b, x, bus, gain, len(sizes), "members per bus")
        assert got[0].view(np.uint32).max() == 0, "a bus without members is +0.0f"
        # more buses than anything is routed to: zeros behind the routed ones
        got = check(b, x, bus, gain, len(sizes) + 3, "three more empty buses")
        assert got[len(sizes):].view(np.uint32).max() == 0


@pytest.mark.parametrize("fmt, frames, n_buses, clustered", [
    (desc.FMT_MONO, 3000, 1, False), (desc.FMT_STEREO, 441, 64, False), (desc.FMT_QUAD, 256, 7, True), (desc.FMT_5POINT1, 37, 2, False),
    (desc.FMT_5POINT1_REAR, 2048, 7, False), (desc.FMT_6POINT1, 1, 64, True), (desc.FMT_7POINT1, 3000, 2, True), (desc.FMT_STEREO, 2048, 1, True),
    (desc.FMT_MONO, 1, 7, False), (desc.FMT_6POINT1, 441, 1, False), (desc.FMT_7POINT1, 256, 64, False), (desc.FMT_QUAD, 37, 64, True)])
def test_formats_frames_and_buses(fmt, frames, n_buses, clustered):
    n = 300
    r = np.random.default_rng(100 * fmt + n_buses)
    ch = desc.FORMAT_CHANNELS[fmt]
    x = r.standard_normal((n, frames, ch)).astype(f32)
    gain = r.uniform(-2, 2, n).astype(f32)
    if clustered:   # neighbours share a bus, in runs of uneven length
        bus = np.sort(r.integers(0, n_buses, n))
    else:
        bus = r.integers(0, n_buses, n)
    bus[r.integers(0, n, 20)] = -1
    with Batch(n, fmt, 48000, 1) as b:
        b.set_routing(bus, gain)
        check(b, x, bus, gain, n_buses, f"format {fmt}, {frames} frames, {n_buses} buses")


def test_special_gains_and_values():
    """Gains of 0, negative, denormal and 1e30; inputs with denormals, infinities, NaNs and -0.0: every member takes part, nothing is flushed."""
    n, frames = 200, 64
    r = np.random.default_rng(3)
    x = r.standard_normal((n, frames, 2)).astype(f32)
    specials = np.array([1e-40, -1e-42, np.inf, -np.inf, np.nan, -0.0, 0.0, 3e38, -3e38, 1e-38], dtype=f32)
    where = r.random(x.shape) < 0.05
    x[where] = r.choice(specials, where.sum())
    x[7] = f32(1e-41)           # a whole row of denormals ...
    gain = r.choice(np.array([0.0, -0.0, -1.0, 1e-40, 1e30, 0.5, -1e30, 1.0], dtype=f32), n)
    gain[7] = f32(0.5)          # ... halved: still denormal, must not be flushed
    bus = r.integers(-1, 3, n)
    bus[7] = 2
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(bus, gain)
        got = check(b, x, bus, gain, 3, "special values")
        assert np.isnan(got).any() and np.isfinite(got).any()
    # one member, a denormal times a half, alone on its bus: the exact bits
    with Batch(2, desc.FMT_MONO, 48000, 1) as b:
        b.set_routing([0, 1], [0.5, 0.0])
        x = np.array([[[1e-41], [-0.0]], [[np.inf], [1.0]]], dtype=f32)
        got = device_downmix(b, x, 2)
        assert got[0, 0, 0].tobytes() == f32(f32(1e-41) * f32(0.5)).tobytes() and got[0, 0, 0] != 0
        assert got[0, 1, 0].tobytes() == f32(0.0).tobytes()     # +0 + (-0 * 0.5) = +0
        assert np.isnan(got[1, 0, 0]) and got[1, 1, 0].tobytes() == f32(0.0).tobytes()   # 0 * Inf; 0 * 1


@pytest.mark.parametrize("fmt, offset", [(desc.FMT_MONO, 1), (desc.FMT_MONO, 3), (desc.FMT_5POINT1, 1), (desc.FMT_5POINT1, 5), (desc.FMT_STEREO, 2),
                                         (desc.FMT_STEREO, 6), (desc.FMT_QUAD, 2)])
def test_buffers_off_the_wide_alignment(fmt, offset):
    """Mono and 5.1 at an odd float, stereo at an odd frame: the narrower loads give the bits of the aligned call."""
    n, frames = 150, 129
    r = np.random.default_rng(offset)
    ch = desc.FORMAT_CHANNELS[fmt]
    x = r.standard_normal((n, frames, ch)).astype(f32)
    gain = r.uniform(-1, 1, n).astype(f32)
    bus = r.integers(-1, 4, n)
    with Batch(n, fmt, 48000, 1) as b:
        b.set_routing(bus, gain)
        shifted = check(b, x, bus, gain, 4, f"offset {offset}", offset=offset)
        aligned = check(b, x, bus, gain, 4, "aligned")
        assert same_bits(shifted, aligned)


def test_every_access_width_gives_the_same_bits():
    n, frames = 500, 256
    r = np.random.default_rng(5)
    x = r.standard_normal((n, frames, 2)).astype(f32)
    gain = r.uniform(-1, 1, n).astype(f32)
    bus = r.integers(0, 3, n)
    so = lib.load()
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(bus, gain)
        try:
            for width in (1, 2, 4):
                so.oalsfx_debug_downmix_vector(width)
                check(b, x, bus, gain, 3, f"{width} floats per access")
        finally:
            so.oalsfx_debug_downmix_vector(4)


def test_repeats_routing_changes_and_table_reuse():
    n, frames = 400, 100
    r = np.random.default_rng(6)
    x = r.standard_normal((n, frames, 2)).astype(f32)
    gain = r.uniform(-1, 1, n).astype(f32)
    bus = r.integers(0, 5, n)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        assert b.get_routing(n - 1) == (0, 1.0)
        check(b, x, np.zeros(n, int), np.ones(n, f32), 1, "the default routing: everything on bus 0, gain 1")
        b.set_routing(bus, gain)
        first = check(b, x, bus, gain, 5, "first call")
        uploads = b.downmix_uploads()
        again = check(b, x, bus, gain, 5, "second call")
        assert same_bits(first, again) and b.downmix_uploads() == uploads, "an unchanged call sent the table again"
        bus[10:20] = 4
        b.set_routing(bus[10:20], None, first=10)       # buses only
        gain[30:35] = f32(-3.0)
        b.set_routing(None, gain[30:35], first=30)      # gains only
        changed = check(b, x, bus, gain, 5, "after a routing change")
        assert not same_bits(first, changed) and b.downmix_uploads() == uploads + 1
        check(b, x, bus, gain, 5, "unchanged again")
        assert b.downmix_uploads() == uploads + 1
        check(b, x, bus, gain, 6, "another bus count")    # the table carries the buses the second level zeroes
        assert b.downmix_uploads() == uploads + 2


def mixed_setup(n):
    def effect(i):
        k = i % 4
        return preset_effect((7 * i) % 113) if k < 2 else make_effect([desc.CHORUS, desc.ECHO][k - 2])
    return lambda b: b.set_effect(0, [effect(i) for i in range(n)])


def routing_for(n, n_buses, seed):
    r = np.random.default_rng(seed)
    bus = r.integers(-1, n_buses, n)
    return bus, r.uniform(-1, 1, n).astype(f32)


def test_downmix_behind_a_chained_run():
    """EAX reverbs, proven steady, so that consecutive mix_device calls overlap; the downmix with hip_stream NULL must come behind the
    last of them (the join is what is tested: chained_calls has to have advanced) and equal the restatement over the oracle's outputs."""
    torch = _torch()
    n, frames, n_buses = 72, 256, 3
    bus, gain = routing_for(n, n_buses, 20)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect(0, [preset_effect((3 * i) % 113) for i in range(n)])
        b.apply_changes()
        b.set_routing(bus, gain)
        army = ShadowArmy(b)
        r = np.random.default_rng(21)
        xs = [r.uniform(-1, 1, (n, frames, 2)).astype(f32) for _ in range(8)]
        ref = None
        for x in xs[:3]:
            b.mix(x)                  # through the start-up cross-fade; proven
            army.mix(x)
        before = b.chained_calls
        dx = [torch.from_numpy(x).cuda() for x in xs[3:]]
        dy = [torch.empty_like(d) for d in dx]
        out = torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for d, y in zip(dx, dy):
            b.mix_device(frames, d.data_ptr(), y.data_ptr())
        b.downmix_device(frames, dy[-1].data_ptr(), n_buses, out.data_ptr())
        b.synchronize()
        assert b.chained_calls - before >= 3, "the calls did not overlap: the test would not see a missing join"
        for x in xs[3:]:
            ref = army.mix(x)
        assert not army.differing(dy[-1].cpu().numpy(), ref)
        assert same_bits(out.cpu().numpy(), downmix(ref, bus, gain, n_buses))


def test_downmix_on_a_callers_stream_and_from_host_buffers():
    """Mixed effects and EAX reverbs: mix_device on the batch's stream with the downmix on a caller's stream right behind it, then
    mix_downmix from host buffers with a call longer than 2048 frames."""
    torch = _torch()
    n, n_buses = 40, 4
    bus, gain = routing_for(n, n_buses, 30)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        mixed_setup(n)(b)
        b.apply_changes()
        b.set_routing(bus, gain)
        army = ShadowArmy(b)
        r = np.random.default_rng(31)
        side = torch.cuda.Stream()
        ref = None
        for k, frames in enumerate([256, 441, 256]):
            x = r.uniform(-1, 1, (n, frames, 2)).astype(f32)
            d = torch.from_numpy(x).cuda()
            y = torch.empty_like(d)
            out = torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            b.mix_device(frames, d.data_ptr(), y.data_ptr())
            b.downmix_device(frames, y.data_ptr(), n_buses, out.data_ptr(), stream=side.cuda_stream)
            side.synchronize()
            ref = army.mix(x)
            assert not army.differing(y.cpu().numpy(), ref), f"call {k}"
            assert same_bits(out.cpu().numpy(), downmix(ref, bus, gain, n_buses)), f"call {k}: downmix on the caller's stream"
        for frames in (2500, 256):
            x = r.uniform(-1, 1, (n, frames, 2)).astype(f32)
            got = b.mix_downmix(x, n_buses)
            ref = army.mix(x)
            assert same_bits(got, downmix(ref, bus, gain, n_buses)), f"mix_downmix, {frames} frames"


@pytest.mark.parametrize("n_buses", [1, 64])
def test_full_size(n_buses):
    n, frames = 4096, 256
    r = np.random.default_rng(40 + n_buses)
    x = r.standard_normal((n, frames, 2)).astype(f32)
    gain = r.uniform(0, 1, n).astype(f32)
    bus = np.arange(n) % n_buses
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(bus, gain)
        check(b, x, bus, gain, n_buses, f"4096 instances into {n_buses} buses")


def test_refusals_leave_the_buffer_and_the_batch_alone():
    torch = _torch()
    n, frames = 64, 32
    x = np.random.default_rng(50).standard_normal((n, frames, 2)).astype(f32)
    bus = np.arange(n) % 3
    gain = np.ones(n, f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(bus, gain)
        src = torch.from_numpy(x).cuda()
        dst = torch.full((3, frames, 2), 5.0, dtype=torch.float32, device="cuda")
        with pytest.raises(BatchError, match=r"Instance 2 is routed to bus 2; the call has 2\."):
            b.downmix_device(frames, src.data_ptr(), 2, dst.data_ptr())
        with pytest.raises(BatchError, match="overlaps"):
            b.downmix_device(frames, src.data_ptr(), 3, src.data_ptr() + 4 * frames * 2 * 10)
        with pytest.raises(BatchError, match="overlaps"):
            b.downmix_device(frames, src.data_ptr() + 4 * frames * 2, 3, src.data_ptr())   # the bus buffer ends inside the source
        with pytest.raises(BatchError, match="No source samples"):
            b.downmix_device(frames, 0, 3, dst.data_ptr())
        with pytest.raises(BatchError, match="No destination samples"):
            b.downmix_device(frames, src.data_ptr(), 3, 0)
        with pytest.raises(BatchError, match="routed to bus 2"):
            b.mix_downmix(x, 2)
        so = lib.load()
        assert not so.oalsfx_batch_downmix_device(b._h, -1, src.data_ptr(), 3, dst.data_ptr(), None) and b.error == "Frame count is negative."
        assert not so.oalsfx_batch_downmix_device(b._h, frames, src.data_ptr(), 0, dst.data_ptr(), None) and b.error == "Bus count is out of range."
        import ctypes as C
        assert not so.oalsfx_batch_set_routing(b._h, 0, 2, (C.c_int * 2)(1, -2), None) and b.get_routing(0) == (0, 1.0)
        assert not so.oalsfx_batch_set_routing(b._h, n - 1, 2, (C.c_int * 2)(1, 1), None)
        b.downmix_device(0, 0, 3, 0)    # no frames: succeeds, does nothing
        b.synchronize()
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 5.0).all(), "a refused call wrote to the bus buffer"
        check(b, x, bus, gain, 3, "the batch after the refusals")


def test_routing_leaves_the_effect_path_and_the_blob_alone():
    """With routing set, mix_device outputs and a snapshot are byte-identical to those of a batch that never heard of routing, and reset
    leaves the routing as it was."""
    torch = _torch()
    n, frames = 48, 256
    bus, gain = routing_for(n, 3, 60)
    r = np.random.default_rng(61)
    xs = [r.uniform(-1, 1, (n, frames, 2)).astype(f32) for _ in range(3)]
    outs, blobs = [], []
    for routed in (False, True):
        with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
            mixed_setup(n)(b)
            b.apply_changes()
            if routed:
                b.set_routing(bus, gain)
            ys = []
            for x in xs:
                d = torch.from_numpy(x).cuda()
                y = torch.empty_like(d)
                b.mix_device(frames, d.data_ptr(), y.data_ptr())
                if routed:
                    bus_out = torch.empty((3, frames, 2), dtype=torch.float32, device="cuda")
                    b.downmix_device(frames, y.data_ptr(), 3, bus_out.data_ptr())
                b.synchronize()
                ys.append(y.cpu().numpy())
            nbytes = b.snapshot_bytes()
            blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            b.snapshot(None, blob.data_ptr(), nbytes)
            b.synchronize()
            outs.append(ys)
            blobs.append(blob.cpu().numpy())
            if routed:
                b.reset([1, 5])
                b.restore(None, blob.data_ptr(), nbytes)
                assert [b.get_routing(i) for i in range(n)] == [(int(bus[i]), float(gain[i])) for i in range(n)]
    for a, c in zip(*outs):
        assert a.tobytes() == c.tobytes()
    assert blobs[0].tobytes() == blobs[1].tobytes()


def test_group_adds_the_shards_in_shard_order():
    n, frames, n_buses = 90, 256, 3
    bus, gain = routing_for(n, n_buses, 70)
    bus[45:][bus[45:] == 2] = 1         # bus 2: members in shard 0 only
    r = np.random.default_rng(71)
    with Group(n, [0, 0], desc.FMT_STEREO, 48000, 1) as g, Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        for t in (g, b):
            t.set_effect_type(0, desc.ECHO)
            t.apply_changes()
            t.set_routing(bus, gain)
        shards = [(f, c) for _, f, c in g.shards]
        assert shards == [(0, 45), (45, 45)]
        for k in range(3):
            x = r.uniform(-1, 1, (n, frames, 2)).astype(f32)
            y = b.mix(x)
            got = g.mix_downmix(x, n_buses)
            assert same_bits(got, downmix_shards(y, bus, gain, n_buses, shards)), f"call {k}"
            assert same_bits(got[2], downmix(y, bus, gain, n_buses)[2]), "a bus of shard 0 alone equals the one-batch sum"
        with pytest.raises(BatchError, match=r"is routed to bus \d; the call has 1\."):
            g.mix_downmix(x, 1)


def test_api_array_buses(tmp_path):
    """tests/cpp/api_array_buses.cpp: ApiArray::set_routing and both forms of mix_to_buses against sums the program computes itself, in
    the stated order, from forty separate oalsfxpp::Api objects' outputs."""
    exe = str(tmp_path / "api_array_buses")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "api_array_buses.cpp"),
                    "-L", libdir, "-loalsfx_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
