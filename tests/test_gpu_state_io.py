"""GPU: instance state snapshot, restore and reset (oalsfx_batch_snapshot / _restore / _reset, include/oalsfx_hip.h).

The check is a twin: a snapshotted batch goes on, and a batch (or instance) restored from the snapshot must go on bit for bit the same --
outputs, read_slot states (update stamps aside: they are renumbered), delay lines, send-filter histories and the API-visible properties.
The uninterrupted batch is followed by CPU oracle shadows where the test says so, which anchors the twin to the reference."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from harness import ROOT, ShadowArmy, make_effect, preset_effect
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import Batch, BatchError

pytestmark = pytest.mark.gpu

E = make_effect
FRAMES = 256


def _torch():
    import torch
    return torch


def kinds_setup(n, slots=2):
    """EAX presets i % 113, chorus, echo, equalizer and Null across the instances and slots."""
    def effect(i, s):
        k = (i + 2 * s) % 5
        if k == 0:
            return preset_effect(i % 113)
        return E([None, desc.CHORUS, desc.ECHO, desc.EQUALIZER, desc.NULL][k])

    def setup(b):
        for s in range(slots):
            b.set_effect(s, [effect(i, s) for i in range(n)])
    return setup


def reverb_setup(n):
    return lambda b: b.set_effect(0, [preset_effect((3 * i) % 113) for i in range(n)])


def make(n, setup, fmt=desc.FMT_STEREO, slots=1, rate=48000):
    b = Batch(n, fmt, rate, slots)
    setup(b)
    b.apply_changes()
    return b


class Inputs:
    """Seeded device inputs, one per call, and one output buffer per call and batch."""

    def __init__(self, n, channels, seed=0):
        self.n, self.ch, self.rng = n, channels, np.random.default_rng(seed)

    def make(self, frames=FRAMES):
        torch = _torch()
        x = self.rng.uniform(-1.0, 1.0, size=(self.n, frames, self.ch)).astype(np.float32)
        return x, torch.from_numpy(x).cuda()


def run(b, xs, frames=FRAMES):
    """Consecutive mix_device calls on the batch's own stream (chained where the batch allows), no synchronisation between them."""
    torch = _torch()
    outs = [torch.empty_like(d) for _, d in xs]
    for (_, d), o in zip(xs, outs):
        b.mix_device(frames, d.data_ptr(), o.data_ptr())
    return outs


def host(b, outs):
    _torch().cuda.synchronize()
    b.synchronize()
    return [o.cpu().numpy() for o in outs]


def snapshot(b, instances=None):
    torch = _torch()
    nbytes = b.snapshot_bytes(instances)
    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b.snapshot(instances, blob.data_ptr(), nbytes)
    b.synchronize()
    return blob


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_out(a, b, label, rows_a=None, rows_b=None):
    a = a if rows_a is None else a[rows_a]
    b = b if rows_b is None else b[rows_b]
    bad = np.nonzero((bits(a) != bits(b)).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, f"{label}: rows {bad[:8].tolist()} differ"


def view(b, i):
    """What the API shows of instance i: properties (active, deferred), slot parameters and states without their update stamps, rings,
    source parameters and state."""
    out = []
    for s in range(b.effect_count):
        p, st = b.read_slot(i, s)
        out += [bytes(b.get_effect(i, s)), bytes(b.get_effect(i, s, deferred=True)), bytes(b.get_send_props(i, s)),
                bytes(b.get_send_props(i, s, deferred=True)), p.type, bytes(p)[8:], bytes(st)[4:], b.read_ring(i, s).tobytes()]
    sp, sst = b.read_source(i)
    out += [bytes(b.get_send_props(i, -1)), bytes(b.get_send_props(i, -1, deferred=True)), bytes(sp), bytes(sst)]
    return out


def same_view(a, i, b, j, label):
    va, vb = view(a, i), view(b, j)
    names = ["effect", "deferred effect", "send", "deferred send", "type", "params", "state", "ring"]
    for k, (x, y) in enumerate(zip(va, vb)):
        what = names[k % 8] if k < 8 * a.effect_count else ["direct send", "deferred direct send", "source params", "source state"][k - 8 * a.effect_count]
        assert x == y, f"{label}: instance {i} vs {j}: {what} differs"


def test_continuation_of_a_chained_run():
    """256 instances, two slots of EAX presets, chorus, echo, equalizer and Null: 12 calls without synchronising, a snapshot, a fresh
    batch restored from it, 6 more calls on both -- identical, and the source anchored to the oracle on every 8th instance."""
    n = 256
    setup = kinds_setup(n)
    a = make(n, setup, slots=2)
    inp = Inputs(n, a.channels, seed=1)
    army = ShadowArmy(a, list(range(0, n, 8)))
    army.sync()
    first = [inp.make() for _ in range(12)]
    outs = run(a, first)
    blob = snapshot(a)
    ya = host(a, outs)
    for k, (x, _) in enumerate(first):
        assert not army.differing(ya[k], army.mix(x)), f"source call {k} differs from the oracle"
    b = make(n, lambda _: None, slots=2)
    b.restore(None, blob.data_ptr(), blob.numel())
    for i in range(0, n, 5):
        same_view(a, i, b, i, "right after the restore")
    more = [inp.make() for _ in range(6)]
    ya, yb = host(a, run(a, more)), host(b, run(b, more))
    for k in range(6):
        same_out(ya[k], yb[k], f"continuation call {k}")
        assert not army.differing(ya[k], army.mix(more[k][0])), f"source continuation call {k} differs from the oracle"
    for i in range(0, n, 3):
        same_view(a, i, b, i, "after the continuation")
    a.close(); b.close()


def test_rollback_into_the_same_batch():
    n = 64
    a = make(n, reverb_setup(n))
    inp = Inputs(n, a.channels, seed=2)
    host(a, run(a, [inp.make() for _ in range(8)]))
    blob = snapshot(a)
    later = [inp.make() for _ in range(6)]
    y1 = host(a, run(a, later))
    a.restore(None, blob.data_ptr(), blob.numel())
    y2 = host(a, run(a, later))
    for k in range(6):
        same_out(y1[k], y2[k], f"rolled-back call {k}")
    a.close()


def test_permuted_targets_and_a_forked_voice():
    torch = _torch()
    n = 48
    setup = kinds_setup(n, 1)
    a = make(n, setup)
    inp = Inputs(n, a.channels, seed=3)
    host(a, run(a, [inp.make() for _ in range(5)]))
    blob = snapshot(a)
    b = make(n, lambda _: None)
    rev = list(range(n - 1, -1, -1))
    b.restore(rev, blob.data_ptr(), blob.numel())
    one = snapshot(a, [5])
    c = make(n, setup)
    c.restore([10], one.data_ptr(), one.numel())
    c.restore([20], one.data_ptr(), one.numel())
    xs = [inp.make() for _ in range(4)]
    xs_rev = [(x[::-1].copy(), torch.flip(d, [0]).contiguous()) for x, d in xs]
    xs_c = []
    for x, _ in xs:
        x2 = x.copy()
        x2[10] = x2[20] = x[5]
        xs_c.append((x2, torch.from_numpy(x2).cuda()))
    ya, yb, yc = host(a, run(a, xs)), host(b, run(b, xs_rev)), host(c, run(c, xs_c))
    for k in range(4):
        same_out(ya[k][::-1], yb[k], f"reversed targets, call {k}")
        same_out(ya[k], yc[k], f"fork to 10, call {k}", rows_a=[5], rows_b=[10])
        same_out(ya[k], yc[k], f"fork to 20, call {k}", rows_a=[5], rows_b=[20])
    for i in (0, 7, 5):
        same_view(a, i, b, n - 1 - i, "reversed targets")
    same_view(a, 5, c, 10, "fork")
    same_view(a, 5, c, 20, "fork")
    for x in (a, b, c):
        x.close()


def _mid(case, b, n):
    if case == "applied preset":
        b.set_effect(0, [preset_effect((7 * i + 11) % 113) for i in range(n)])
        b.apply_changes()
    elif case == "inside the cross-fade":
        b.set_effect(0, [preset_effect((7 * i + 11) % 113) for i in range(n)])
        b.apply_changes()
        return 64   # frames of the call in front of the snapshot
    elif case == "type change":
        b.set_effect(0, E(desc.CHORUS), first=0, count=n // 2)
        b.apply_changes()
    elif case == "deferred only":
        b.set_effect(0, preset_effect(40), first=0, count=n // 2)
        b.set_send_props(-1, 0.5, 0.7, 1.0, first=n // 4, count=n // 2)
    elif case == "modulated":
        pass
    return 0


@pytest.mark.parametrize("case", ["applied preset", "inside the cross-fade", "type change", "deferred only", "modulated"])
def test_snapshots_taken_mid_transition(case):
    n = 32
    if case == "modulated":
        def setup(b):
            b.set_effect(0, [make_effect(desc.EAX_REVERB, modulation_depth=0.6, modulation_time=0.3 + 0.01 * i) for i in range(n)])
    else:
        setup = reverb_setup(n)
    a = make(n, setup)
    inp = Inputs(n, a.channels, seed=4)
    host(a, run(a, [inp.make() for _ in range(6)]))
    if case == "modulated":
        a.set_effect(0, E(desc.EAX_REVERB), first=0, count=n // 2)   # depth back to 0: the smoother keeps moving (mod_ever)
        a.apply_changes()
        host(a, run(a, [inp.make()]))
    frames = _mid(case, a, n)
    if frames:
        host(a, run(a, [inp.make(frames)], frames))
    blob = snapshot(a)
    b = make(n, lambda _: None)
    b.restore(None, blob.data_ptr(), blob.numel())
    for i in range(n):
        for s in range(a.effect_count):
            assert bytes(a.get_effect(i, s, deferred=True)) == bytes(b.get_effect(i, s, deferred=True)), f"instance {i}: deferred effect"
        assert bytes(a.get_send_props(i, -1, deferred=True)) == bytes(b.get_send_props(i, -1, deferred=True)), f"instance {i}: deferred send"
    if case == "deferred only":
        a.apply_changes(); b.apply_changes()
    xs = [inp.make(f) for f in (FRAMES, 100, FRAMES, FRAMES)]
    ya = [host(a, run(a, [x], x[0].shape[1]))[0] for x in xs]
    yb = [host(b, run(b, [x], x[0].shape[1]))[0] for x in xs]
    for k in range(len(xs)):
        same_out(ya[k], yb[k], f"{case}: call {k}")
    for i in (0, 1, n // 2, n - 1):
        same_view(a, i, b, i, case)
    a.close(); b.close()


@pytest.mark.parametrize("rotate", [1, 2])
def test_restore_onto_other_types_and_sizes(rotate):
    """Instances 0..7 reverbs, 8..15 chorus, 16..23 Null, restored into a batch whose groups are rotated: every image lands on a slot of
    another type (reverb onto chorus / Null, chorus onto Null / reverb, Null onto reverb / chorus)."""
    n = 24
    kinds = [lambda i: preset_effect(i % 113), lambda i: E(desc.CHORUS, delay=0.004 + 0.0005 * i), lambda i: E(desc.NULL)]
    a = make(n, lambda b: b.set_effect(0, [kinds[i // 8](i) for i in range(n)]))
    b = make(n, lambda b: b.set_effect(0, [kinds[(i // 8 + rotate) % 3](i) for i in range(n)]))
    inp = Inputs(n, a.channels, seed=5)
    warm = [inp.make() for _ in range(4)]
    host(a, run(a, warm)); host(b, run(b, warm))
    blob = snapshot(a)
    b.restore(None, blob.data_ptr(), blob.numel())
    xs = [inp.make() for _ in range(4)]
    ya, yb = host(a, run(a, xs)), host(b, run(b, xs))
    for k in range(4):
        same_out(ya[k], yb[k], f"rotation {rotate}, call {k}")
    for i in (0, 9, 17, 23):
        same_view(a, i, b, i, f"rotation {rotate}")
    a.close(); b.close()


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_5POINT1])
def test_channel_formats_and_send_filters(fmt):
    n = 40
    setup = kinds_setup(n, 2)

    def with_filters(b):
        setup(b)
        b.set_send_props(-1, 0.9, 0.5, 0.8, first=0, count=n // 2)
        b.set_send_props(0, 0.8, 0.6, 0.9, first=n // 4, count=n // 2)
    a = make(n, with_filters, fmt=fmt, slots=2)
    army = ShadowArmy(a, list(range(0, n, 3)))
    inp = Inputs(n, a.channels, seed=6)
    first = [inp.make() for _ in range(4)]
    for x in first:
        assert not army.differing(host(a, run(a, [x]))[0], army.mix(x[0])), "source differs from the oracle"
    blob = snapshot(a)
    b = make(n, lambda _: None, fmt=fmt, slots=2)
    b.restore(None, blob.data_ptr(), blob.numel())
    for x in [inp.make() for _ in range(4)]:
        ya, yb = host(a, run(a, [x]))[0], host(b, run(b, [x]))[0]
        same_out(ya, yb, "continuation")
        assert not army.differing(ya, army.mix(x[0])), "source continuation differs from the oracle"
    for i in range(0, n, 7):
        same_view(a, i, b, i, "filters")
    a.close(); b.close()


def test_multi_buffer_after_a_restore():
    """After a restore mix_device_multi stays bit-identical to single calls, and its multi-buffer passes come back once the device has
    proven the restored instances steady again."""
    torch = _torch()
    n = 128
    a = make(n, reverb_setup(n))
    inp = Inputs(n, a.channels, seed=7)
    for _ in range(6):
        host(a, run(a, [inp.make() for _ in range(3)]))
        if a.plan(0)[1] == n:
            break
    blob = snapshot(a)
    b = make(n, lambda _: None)
    b.restore(None, blob.data_ptr(), blob.numel())
    calls, resumed = 0, None
    for rnd in range(12):
        xs = [inp.make() for _ in range(4)]
        ya = host(a, run(a, xs))
        outs = [torch.empty_like(d) for _, d in xs]
        before = b.multi_counts()[1]
        b.mix_device_multi(FRAMES, [d.data_ptr() for _, d in xs], [o.data_ptr() for o in outs])
        yb = host(b, outs)
        for k in range(4):
            same_out(ya[k], yb[k], f"round {rnd} buffer {k}")
        calls += 4
        if b.multi_counts()[1] > before:
            resumed = calls
            break
    assert resumed is not None, f"no multi-buffer pass within {calls} calls after the restore (plan {b.plan(0)})"
    print(f"multi-buffer passes resumed {resumed} calls after the restore")
    a.close(); b.close()


def test_full_size_4096_eax_reverbs():
    """BASELINE configs[1]'s shape: 4096 EAX reverbs, stereo, 48 kHz.  Snapshot, restore into a second batch, 4 calls on both: every
    output identical, and a second snapshot of both identical in every device record (update stamps aside) and delay line."""
    torch = _torch()
    n = 4096
    a = make(n, lambda b: b.set_effect_type(0, desc.EAX_REVERB))
    inp = Inputs(n, a.channels, seed=8)
    host(a, run(a, [inp.make() for _ in range(6)]))
    blob = snapshot(a)
    b = make(n, lambda _: None)
    b.restore(None, blob.data_ptr(), blob.numel())
    del blob
    xs = [inp.make() for _ in range(4)]
    ya, yb = host(a, run(a, xs)), host(b, run(b, xs))
    for k in range(4):
        same_out(ya[k], yb[k], f"call {k}")
    sa, sb = snapshot(a), snapshot(b)
    assert sa.numel() == sb.numel()
    hdr = struct.unpack_from("<IIiiiiQQQQQ", sa[:256].cpu().numpy().tobytes())
    prefix, stride = hdr[8], hdr[9]
    for blob in (sa, sb):
        blob[prefix: prefix + n * stride].view(n, stride)[:, :4] = 0   # the slot state's update stamp (seen_seq) is renumbered
    assert torch.equal(sa[prefix:], sb[prefix:]), "device records or delay lines differ after the continuation"
    for i in (0, 1, 2047, 4095):
        same_view(a, i, b, i, "full size")
    a.close(); b.close()


def test_blob_portability_through_the_host():
    """The blob copied to host memory, saved and loaded (torch.save / torch.load) and copied back restores identically; so does a blob
    written straight into page-locked host memory."""
    torch = _torch()
    n = 40
    a = make(n, kinds_setup(n, 1))
    inp = Inputs(n, a.channels, seed=9)
    host(a, run(a, [inp.make() for _ in range(5)]))
    blob = snapshot(a)
    f = io.BytesIO()
    torch.save(blob.cpu(), f)
    f.seek(0)
    back = torch.load(f).cuda()
    nbytes = a.snapshot_bytes()
    l = lib.load()
    pinned = l.oalsfx_pinned_alloc(nbytes)
    assert pinned
    try:
        a.snapshot(None, pinned, nbytes)
        a.synchronize()
        b, c = make(n, lambda _: None), make(n, lambda _: None)
        b.restore(None, back.data_ptr(), back.numel())
        c.restore(None, pinned, nbytes)
        c.synchronize()
    finally:
        l.oalsfx_pinned_free(C.c_void_p(pinned))
    xs = [inp.make() for _ in range(3)]
    ya, yb, yc = host(a, run(a, xs)), host(b, run(b, xs)), host(c, run(c, xs))
    for k in range(3):
        same_out(ya[k], yb[k], f"through torch.save, call {k}")
        same_out(ya[k], yc[k], f"through page-locked memory, call {k}")
    for x in (a, b, c):
        x.close()


def test_refusals_leave_the_target_untouched():
    torch = _torch()
    n = 16
    a = make(n, reverb_setup(n))
    inp = Inputs(n, a.channels, seed=10)
    host(a, run(a, [inp.make() for _ in range(3)]))
    blob = snapshot(a)
    nbytes = blob.numel()
    target, twin = make(n, kinds_setup(n, 1)), make(n, kinds_setup(n, 1))
    warm = [inp.make() for _ in range(2)]
    host(target, run(target, warm)); host(twin, run(twin, warm))
    bad_magic = blob.clone()
    bad_magic[0] ^= 0xFF
    cases = [(target, None, blob.data_ptr(), nbytes - 16, "larger than the bytes"), (target, None, bad_magic.data_ptr(), nbytes, "magic"),
             (target, [1, 2, 1] + list(range(3, 16)), blob.data_ptr(), nbytes, "twice"),
             (target, list(range(8)), blob.data_ptr(), nbytes, "number of instances")]
    for fmt, rate, slots in ((desc.FMT_MONO, 48000, 1), (desc.FMT_STEREO, 44100, 1), (desc.FMT_STEREO, 48000, 2)):
        cases.append((Batch(n, fmt, rate, slots), None, blob.data_ptr(), nbytes, "differs from the batch"))
    for b, targets, ptr, size, what in cases:
        with pytest.raises(BatchError, match=what):
            b.restore(targets, ptr, size)
    tiny = torch.empty(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(BatchError, match="too small"):
        target.snapshot(None, tiny.data_ptr(), 1024)
    xs = [inp.make() for _ in range(3)]
    yt, yw = host(target, run(target, xs)), host(twin, run(twin, xs))
    for k in range(3):
        same_out(yt[k], yw[k], f"refused target, call {k}")
    for i in range(0, n, 5):
        same_view(target, i, twin, i, "refused target")
    for b, *_ in cases:
        b.close()
    a.close(); twin.close()


def test_reset_half_the_instances():
    n = 32
    setup = kinds_setup(n, 2)

    def with_sends(b):
        setup(b)
        b.set_send_props(-1, 0.7, 0.5, 1.0)
        b.set_send_props(1, 0.6, 0.9, 0.8)
    a, twin = make(n, with_sends, slots=2), make(n, with_sends, slots=2)
    inp = Inputs(n, a.channels, seed=11)
    warm = [inp.make() for _ in range(4)]
    host(a, run(a, warm)); host(twin, run(twin, warm))
    half = list(range(0, n, 2))
    a.reset(half)
    default = bytes(desc.SendProps(1.0, 1.0, 1.0))
    for i in half:
        for s in range(2):
            for deferred in (False, True):
                assert a.get_effect(i, s, deferred).type == desc.NULL, f"instance {i} slot {s}"
                assert bytes(a.get_send_props(i, s, deferred)) == default
        assert bytes(a.get_send_props(i, -1)) == default and bytes(a.get_send_props(i, -1, True)) == default
    fresh = make(n, lambda _: None, slots=2)
    for b in (a, fresh):
        b.set_effect_at(0, half, [preset_effect(i % 113) for i in half])
        b.set_effect_at(1, half, E(desc.ECHO))
        b.apply_changes()
    xs = [inp.make() for _ in range(4)]
    ya, yf, yt = host(a, run(a, xs)), host(fresh, run(fresh, xs)), host(twin, run(twin, xs))
    others = list(range(1, n, 2))
    for k in range(4):
        same_out(ya[k], yf[k], f"reset instances against a fresh batch, call {k}", rows_a=half, rows_b=half)
        same_out(ya[k], yt[k], f"untouched instances against the twin, call {k}", rows_a=others, rows_b=others)
    for i in (0, 2, 30):
        same_view(a, i, fresh, i, "reset")
    for i in (1, 31):
        same_view(a, i, twin, i, "untouched")
    for b in (a, fresh, twin):
        b.close()


def test_api_array_reset_matches_a_fresh_api(tmp_path):
    """tests/cpp/api_array_reset.cpp: oalsfxpp::ApiArray::reset(index) is Api::initialize for that voice -- it then mixes like a fresh
    oalsfxpp::Api given the same calls, and the other voices like an array that was not reset."""
    exe = str(tmp_path / "api_array_reset")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "api_array_reset.cpp"),
                    "-L", libdir, "-loalsfx_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout


def test_state_io_is_ordered_before_a_mix_on_a_caller_stream():
    """A snapshot (then a restore) queued on the batch's stream with a mix_device on a caller's stream right behind it and nothing
    synchronised in between: the caller's launch must wait for the copy.  The blob's delay lines equal those of a twin's snapshot taken
    while idle, a batch restored from it continues like the twin, and the mix behind the restore equals the mix behind the snapshot."""
    torch = _torch()
    n = 4096
    setup = lambda b: b.set_effect_type(0, desc.EAX_REVERB)
    a, twin = make(n, setup), make(n, setup)
    inp = Inputs(n, a.channels, seed=12)
    warm = [inp.make() for _ in range(3)]
    host(a, run(a, warm)); host(twin, run(twin, warm))
    want = snapshot(twin)
    nbytes = want.numel()
    got = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    x, xd = inp.make()
    side = torch.cuda.Stream()
    outs = [torch.empty_like(xd), torch.empty_like(xd)]
    a.snapshot(None, got.data_ptr(), nbytes)
    a.mix_device(FRAMES, xd.data_ptr(), outs[0].data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    a.synchronize()
    a.restore(None, want.data_ptr(), nbytes)
    a.mix_device(FRAMES, xd.data_ptr(), outs[1].data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    a.synchronize()
    hdr = struct.unpack_from("<IIiiiiQQQQQ", want[:256].cpu().numpy().tobytes())
    rings = hdr[8] + n * hdr[9]
    assert torch.equal(got[rings:], want[rings:]), "the snapshot read delay lines the caller's mix had already advanced"
    y = [o.cpu().numpy() for o in outs]
    same_out(y[0], y[1], "the mix behind the restore against the mix behind the snapshot")
    c = make(n, lambda _: None)
    c.restore(None, got.data_ptr(), nbytes)
    xs = [inp.make() for _ in range(2)]
    yc, yt = host(c, run(c, xs)), host(twin, run(twin, xs))
    for k in range(2):
        same_out(yc[k], yt[k], f"restored from the raced snapshot, call {k}")
    for i in (0, 4095):
        same_view(c, i, twin, i, "raced snapshot")
    for b in (a, twin, c):
        b.close()
