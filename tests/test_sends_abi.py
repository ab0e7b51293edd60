"""CPU checks of the bus sends: the C ABI declares and exports them, the Python mirror binds them and refuses bad arguments before the
library is reached, the number of sends is one constant everywhere, and the NumPy restatement (tests/sends_ref.py) computes what the
header states -- member order, chunks, the ramp's formula at its ends and across a restart -- and tells the stated order of a ramp's
arithmetic from the two nearest others.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import downmix_ref
import sends_ref
from oalsfxpp_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_set_send_routing", "oalsfx_batch_get_send_routing", "oalsfx_batch_set_send_ramps")
f32 = np.float32


def test_header_declares_and_the_mirror_binds_the_send_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in lib.SIGNATURES, name
    assert re.search(r"int oalsfx_batch_set_send_routing\(oalsfx_batch\* b, int send, int first, int count, const int\* bus, const float\* gain\);", header)
    assert re.search(r"int oalsfx_batch_get_send_routing\(const oalsfx_batch\* b, int instance, int send, int\* bus, float\* gain, float\* gain_to, "
                     r"uint32_t\* frames_left\);", header)
    assert re.search(r"int oalsfx_batch_set_send_ramps\(oalsfx_batch\* b, int send, int first, int count, const float\* gain_to, uint32_t frames\);", header)
    assert len(lib.SIGNATURES["oalsfx_batch_set_send_routing"][1]) == 6 and len(lib.SIGNATURES["oalsfx_batch_get_send_routing"][1]) == 7
    assert len(lib.SIGNATURES["oalsfx_batch_set_send_ramps"][1]) == 6


def test_the_library_exports_the_send_calls():
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(so, name), name


def test_the_number_of_sends_is_one_constant():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    (value,) = re.findall(r"^#define OALSFX_BUS_SENDS (\d+)$", header, flags=re.M)
    assert int(value) == api.BUS_SENDS == sends_ref.SENDS == 4
    assert api.SEND_RAMP_MAX_FRAMES == sends_ref.MAX_RAMP == 2 ** 24


def test_the_array_header_declares_the_send_methods():
    header = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool set_send\(int index, int send, int bus, float gain\);", header)
    assert re.search(r"bool ramp_send\(int index, int send, float gain_to, uint32_t frames\);", header)
    assert re.search(r"bool get_send\(int index, int send, int& bus, float& gain, float& gain_to, uint32_t& frames_left\);", header)


def test_the_ramp_kernel_is_a_file_of_its_own_and_built():
    from oalsfxpp_amd import build
    assert "hip/bus_sends.hip" in build.HIP_SOURCES
    kernel = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "bus_sends.hip")).read())
    assert "#pragma clang fp contract(off)" in kernel and "__shared__" not in kernel and "atomic" not in kernel and "__shfl" not in kernel


def _unopened(n=8, channels=2):
    """A Batch whose handle was never created: a check that let a call through would fail on the missing library, not with BatchError."""
    b = api.Batch.__new__(api.Batch)
    b.n = n
    b.channels = channels
    b._h = None
    b._lib = None
    return b


@pytest.mark.parametrize("kwargs, what", [
    (dict(bus=[0], send=4), "Send out of range"), (dict(bus=[0], send=-1), "Send out of range"), (dict(bus=[0, -2], send=1), "Bus number"),
    (dict(bus=[0] * 9, send=2), "out of bounds"), (dict(bus=[0, 1], first=7, send=3), "out of bounds"), (dict(send=1), "buses, gains or both"),
    (dict(bus=[0, 1], gain=[1.0], send=1), "2 buses but 1 gains"), (dict(gain=[None], send=2), "sequence")])
def test_send_routing_is_checked(kwargs, what):
    with pytest.raises(api.BatchError, match=what):
        _unopened().set_routing(**kwargs)


@pytest.mark.parametrize("args, kwargs, what", [
    (([1.0], 16), dict(send=4), "Send out of range"), (([1.0], 2 ** 24 + 1), dict(), "Ramp length out of range"), (([1.0], -1), dict(), "Ramp length"),
    (([1.0] * 9, 16), dict(), "out of bounds"), (([1.0, 1.0], 16), dict(first=7, send=1), "out of bounds"), (([1.0], 16), dict(first=-1), "out of bounds"),
    ((3.0, 16), dict(), "sequence of gains")])
def test_send_ramps_are_checked(args, kwargs, what):
    with pytest.raises(api.BatchError, match=what):
        _unopened().set_send_ramps(*args, **kwargs)


def test_get_routing_checks_the_send_and_the_instance():
    for kwargs, what in ((dict(instance=0, send=4), "Send out of range"), (dict(instance=8, send=1), "out of bounds"), (dict(instance=-1, send=3), "out of bounds")):
        with pytest.raises(api.BatchError, match=what):
            _unopened().get_routing(**kwargs)
        with pytest.raises(api.BatchError, match=what):
            _unopened().get_send(**kwargs)


# ---- the restatement against sums worked out by hand ----
def _ones(n, frames=1):
    return np.ones((n, frames, 1), f32)


def test_a_fresh_batch_is_the_routing_of_before():
    s = sends_ref.Sends(5)
    assert [s.get(2, k) for k in range(4)] == [(0, f32(1.0), f32(1.0), 0)] + [(-1, f32(1.0), f32(1.0), 0)] * 3
    x = np.random.default_rng(0).standard_normal((5, 9, 2)).astype(f32)
    assert sends_ref.same_bits(s.downmix(x, 2), downmix_ref.downmix(x, [0] * 5, np.ones(5, f32), 2))


def test_one_instance_twice_in_one_bus_in_send_order():
    small = f32(2.0 ** -24)  # half an ulp of 1: 1 + small is a tie and rounds to even, back to 1
    s = sends_ref.Sends(1)
    for send, gain in enumerate([1.0, small, small]):
        s.set_routing(send, 0, [0], [gain])
    assert s.members(0) == [(0, 0), (0, 1), (0, 2)]
    assert s.downmix(_ones(1), 1)[0, 0, 0] == f32(1.0)              # (+0 + 1) + 2^-24, a tie, 1; and again
    for send, gain in enumerate([small, small, 1.0]):
        s.set_routing(send, 0, None, [gain])
    assert s.downmix(_ones(1), 1)[0, 0, 0] == f32(1.0 + 2.0 ** -23)  # the two halves of an ulp first: they carry
    # the instance's other sends go elsewhere: instance 1 comes before instance 0's ... no: by instance first, then by send
    s = sends_ref.Sends(2)
    s.set_routing(0, 0, [0, 0], [small, 1.0])
    s.set_routing(3, 0, [0, -1], [small, 1.0])
    assert s.members(0) == [(0, 0), (0, 3), (1, 0)]
    assert s.downmix(_ones(2), 1)[0, 0, 0] == f32(1.0 + 2.0 ** -23)


def test_thirty_three_members_through_sends_1_to_3_make_a_second_chunk():
    small = f32(2.0 ** -24)
    s = sends_ref.Sends(11)
    s.set_routing(0, 0, [-1] * 11)
    for send in (1, 2, 3):
        s.set_routing(send, 0, [0] * 11, [small] * 11)
    assert len(s.members(0)) == 33 and s.members(0)[:4] == [(0, 1), (0, 2), (0, 3), (1, 1)] and s.members(0)[32] == (10, 3)
    # the big member first: 1 and thirty-one ties, 1; the second chunk is the last member alone; 1 + 2^-24: a tie, 1
    s.set_routing(1, 0, None, [1.0])
    assert s.downmix(_ones(11), 1)[0, 0, 0] == f32(1.0)
    # the big member last, (10, 3): the first chunk is 32 * 2^-24 = 2^-19 exactly, the second chunk 1, the bus 1 + 2^-19 exactly
    s.set_routing(1, 0, None, [small])
    s.set_routing(3, 10, None, [1.0])
    assert s.downmix(_ones(11), 1)[0, 0, 0] == f32(1.0 + 2.0 ** -19)
    # a thirty-fourth member, (0, 0) in front: 1, then thirty-one ties; the second chunk holds two small ones, 2^-23, a whole ulp
    s.set_routing(3, 10, None, [small])
    s.set_routing(0, 0, [0], [1.0])
    assert s.members(0)[0] == (0, 0) and len(s.members(0)) == 34
    assert s.downmix(_ones(11), 1)[0, 0, 0] == f32(1.0 + 2.0 ** -23)
    assert s.downmix(_ones(11), 1, chunk=34)[0, 0, 0] == f32(1.0)  # as one chain every addition is a tie


def test_a_ramp_at_its_ends():
    """n = 0, R - 1, R, R + 1: the formula up to the last frame of the ramp, gain_to from there on -- not the formula at n = R."""
    s = sends_ref.Sends(1)
    start, target, frames = f32(0.1), f32(0.5), 3
    s.set_routing(0, 0, None, [start])
    s.set_ramps(0, 0, [target], frames)
    step = f32(f32(target - start) / f32(frames))
    assert s.get(0) == (0, start, target, 3) and s.step[0, 0] == step
    out = s.downmix(_ones(1, 5), 1, advance=False)[0, :, 0]
    assert out[0].tobytes() == f32(f32(0.0) + f32(1.0) * f32(start + f32(0.0) * step)).tobytes() == start.tobytes()
    assert out[2].tobytes() == f32(start + f32(f32(2.0) * step)).tobytes()
    assert out[3].tobytes() == out[4].tobytes() == target.tobytes()
    # ... which the formula would miss here: 0.1f + 3 * step is not 0.5f
    assert f32(start + f32(f32(3.0) * step)) != target
    # the same frames in calls of 2, 1 and 2: the same bits, and the get call follows
    parts = [s.downmix(_ones(1, 2), 1)[0, :, 0]]
    assert s.get(0) == (0, f32(start + f32(f32(2.0) * step)), target, 1)
    parts.append(s.downmix(_ones(1, 1), 1)[0, :, 0])
    assert s.get(0) == (0, target, target, 0) and s.gain[0, 0] == target and not s.frames[0, 0]
    parts.append(s.downmix(_ones(1, 2), 1)[0, :, 0])
    assert np.concatenate(parts).tobytes() == out.tobytes()
    # a ramp of one frame: that frame still has the old gain
    s.set_ramps(0, 0, [0.25], 1)
    assert s.downmix(_ones(1, 2), 1)[0, :, 0].tolist() == [target, f32(0.25)]
    # a ramp of no frames sets the gain at once
    s.set_ramps(0, 0, [0.5], 0)
    assert s.get(0) == (0, f32(0.5), f32(0.5), 0)


def test_a_restarted_ramp_continues_from_the_value_its_predecessor_had():
    s = sends_ref.Sends(2)
    s.set_routing(1, 0, [-1, -1], [0.0, 0.0])
    s.set_ramps(1, 0, [1.0, 1.0], 100)
    s.downmix(_ones(2, 37), 1)  # the clock runs whatever the send's bus
    step = f32(f32(1.0) / f32(100.0))
    held = f32(f32(0.0) + f32(f32(37.0) * step))
    assert s.get(0, 1) == (-1, held, f32(1.0), 63)
    s.set_ramps(1, 0, [0.25], 10)
    assert s.get(0, 1) == (-1, held, f32(0.25), 10) and s.frm[1, 0] == held and s.step[1, 0] == f32(f32(f32(0.25) - held) / f32(10.0))
    # a new bus alone keeps the other ramp running; a gain cancels it
    s.set_routing(1, 1, [0], None)
    assert s.get(1, 1) == (0, held, f32(1.0), 63)
    s.set_routing(1, 1, None, [0.5])
    assert s.get(1, 1) == (0, f32(0.5), f32(0.5), 0)


def test_the_order_is_observable():
    """64 random ramps of 1000 frames: the reference's running sum gain += step and a fused from + n * step each differ from the stated
    form in enough elements that a kernel built either way cannot pass the GPU tests by luck (seed 3: 0.99 and 0.36 of the bus's elements)."""
    r = np.random.default_rng(3)
    n, frames = 64, 1000
    s = sends_ref.Sends(n)
    s.set_routing(0, 0, None, r.uniform(0, 1, n).astype(f32))
    s.set_ramps(0, 0, r.uniform(0, 1, n).astype(f32), frames)
    x = r.standard_normal((n, frames, 2)).astype(f32)
    stated = s.downmix(x, 1, advance=False)
    running = s.downmix(x, 1, form="running", advance=False)
    fused = s.downmix(x, 1, form="fused", advance=False)
    print((running != stated).mean(), (fused != stated).mean())
    assert (running != stated).mean() > 0.5
    assert (fused != stated).mean() > 0.05
    assert sends_ref.same_bits(stated, s.downmix(x, 1))
