"""CPU checks of the bus downmix: the C ABI declares and exports it, the Python mirror binds it and refuses bad arguments before the
library is reached, the chunk size is one constant everywhere, the NumPy restatement computes what the header states (and an order other
than the stated one shows), and the kernels keep nothing in scratch memory -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import downmix_ref
from oalsfxpp_amd import api, lib
from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_set_routing", "oalsfx_batch_get_routing", "oalsfx_batch_downmix_device", "oalsfx_batch_mix_downmix",
         "oalsfx_group_set_routing", "oalsfx_group_mix_downmix")
DEBUG_NAMES = ("oalsfx_debug_downmix_uploads", "oalsfx_debug_downmix_vector")
f32 = np.float32


def test_header_declares_and_the_mirror_binds_the_downmix_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in lib.SIGNATURES, name
    for name in DEBUG_NAMES:
        assert re.search(r"\b" + name + r"\(", debug), name
        assert name in lib.SIGNATURES, name


def test_the_library_exports_the_downmix_calls():
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + DEBUG_NAMES:
        assert hasattr(so, name), name


def test_the_array_header_declares_the_bus_methods():
    header = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool set_routing\(int index, int bus, float gain\);", header)
    assert re.search(r"bool mix_to_buses\(int sample_count, const float\* src_samples, int bus_count, float\* dst_buses\);", header)
    assert re.search(r"bool mix_to_buses\(int sample_count, const float\* const\* src_samples, int bus_count, float\* dst_buses\);", header)


def test_the_chunk_size_is_one_constant():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    (value,) = re.findall(r"^#define OALSFX_DOWNMIX_CHUNK (\d+)$", header, flags=re.M)
    assert int(value) == api.DOWNMIX_CHUNK == downmix_ref.CHUNK
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "downmix.hip")).read()
    assert "kChunk = OALSFX_DOWNMIX_CHUNK" in kernel


def _unopened(n=8, channels=2):
    """A Batch whose handle was never created: a check that let a call through would fail on the missing library, not with BatchError."""
    b = api.Batch.__new__(api.Batch)
    b.n = n
    b.channels = channels
    b._h = None
    b._lib = None
    return b


def _unopened_group(n=8, channels=2):
    g = api.Group.__new__(api.Group)
    g.n = n
    g.channels = channels
    g._h = None
    g._lib = None
    return g


@pytest.mark.parametrize("kwargs, what", [
    (dict(bus=[0] * 9), "out of bounds"), (dict(bus=[0, 1], first=7), "out of bounds"), (dict(bus=[0], first=-1), "out of bounds"),
    (dict(bus=[0, -2]), "Bus number"), (dict(bus=[0, 1], gain=[1.0]), "2 buses but 1 gains"), (dict(gain=[1.0] * 9), "out of bounds"),
    (dict(), "buses, gains or both"), (dict(bus=[0.5]), "sequence"), (dict(bus=3), "sequence"), (dict(gain=[None]), "sequence")])
def test_routing_arrays_are_checked(kwargs, what):
    for target in (_unopened(), _unopened_group()):
        with pytest.raises(api.BatchError, match=what):
            target.set_routing(**kwargs)


def test_get_routing_checks_the_instance():
    for i in (-1, 8):
        with pytest.raises(api.BatchError, match="out of bounds"):
            _unopened().get_routing(i)


@pytest.mark.parametrize("frames, n_buses, what", [(-1, 1, "Frame count is negative"), (16, 0, "Bus count"), (16, -3, "Bus count")])
def test_downmix_device_checks_its_counts(frames, n_buses, what):
    with pytest.raises(api.BatchError, match=what):
        _unopened().downmix_device(frames, 0x1000, n_buses, 0x100000)


def test_mix_downmix_checks_its_arrays():
    b, g = _unopened(), _unopened_group()
    good = np.zeros((8, 16, 2), f32)
    for target in (b, g):
        with pytest.raises(api.BatchError, match="Bus count"):
            target.mix_downmix(good, 0)
        for bad in (np.zeros((7, 16, 2), f32), np.zeros((8, 16, 1), f32), np.zeros((8, 32), f32)):
            with pytest.raises(api.BatchError, match="the source is"):
                target.mix_downmix(bad, 1)
    for dst in (np.zeros((2, 16, 2), f32), np.zeros((1, 16, 2), np.float64), np.zeros((1, 15, 2), f32)):
        with pytest.raises(api.BatchError, match="the bus array is"):
            b.mix_downmix(good, 1, dst)


# ---- the restatement against sums worked out by hand ----
def _col(values):
    """Members with one element each: [n][1][1]."""
    return np.asarray(values, dtype=f32).reshape(-1, 1, 1)


def test_three_members_in_the_stated_order():
    x, g = _col([1.0, 2.0 ** -24, 2.0 ** -24]), np.ones(3, f32)
    # (+0 + 1) + 2^-24 rounds back to 1 (a tie, to even), and again: 1.  Summed from the small end the two halves of an ulp would carry.
    assert downmix_ref.downmix(x, [0, 0, 0], g, 1)[0, 0, 0] == f32(1.0)
    assert f32(f32(2.0 ** -24) + f32(2.0 ** -24)) + f32(1.0) == f32(1.0 + 2.0 ** -23)
    # gains are applied before the sum, each product rounded on its own: 3 * (1 + 2^-23) is not representable
    x, g = _col([1.0 + 2.0 ** -23, 5.0, 7.0]), np.asarray([3.0, -1.0, 0.5], f32)
    t0 = f32(f32(1.0 + 2.0 ** -23) * f32(3.0))
    assert t0 == f32(3.0 + 2.0 ** -21)  # 3 + 3 * 2^-23 rounds to even at an ulp of 2^-22: up to 3 + 2^-21
    want = f32(f32(f32(f32(0.0) + t0) + f32(-5.0)) + f32(3.5))
    assert downmix_ref.downmix(x, [1, 1, 1], g, 2)[1, 0, 0].tobytes() == want.tobytes()
    assert downmix_ref.downmix(x, [1, 1, 1], g, 2)[0, 0, 0].tobytes() == f32(0.0).tobytes()  # a bus without members: +0.0f


def test_thirty_three_members_make_a_second_chunk():
    small = f32(2.0 ** -24)  # half an ulp of 1: 1 + small is a tie and rounds to even, back to 1
    g = np.ones(34, f32)
    # 1, then thirty-two small ones.  First chunk: 1 and thirty-one ties, 1.  Second chunk: the last member alone.  1 + 2^-24: a tie, 1.
    assert downmix_ref.downmix(_col([1.0] + [small] * 32), [0] * 33, g[:33], 1)[0, 0, 0] == f32(1.0)
    # The big member last: the first chunk is 32 * 2^-24 = 2^-19 exactly, the second chunk 1, the bus 1 + 2^-19 exactly.
    assert downmix_ref.downmix(_col([small] * 32 + [1.0]), [0] * 33, g[:33], 1)[0, 0, 0] == f32(1.0 + 2.0 ** -19)
    # The big member just inside the first chunk: 31 * 2^-24 + 1 = 1 + 15.5 ulps, a tie, to even: 1 + 16 ulps = 1 + 2^-19; the second
    # chunk is 2^-24 alone, half an ulp onto an even mantissa: stays.
    x = _col([small] * 31 + [1.0, small])
    assert downmix_ref.downmix(x, [0] * 33, g[:33], 1)[0, 0, 0] == f32(1.0 + 2.0 ** -19)
    # Thirty-four members tell the chunk sizes apart: 1 and thirty-three small ones.  In chunks of 32 the second chunk holds two small
    # ones, 2^-23, a whole ulp: 1 + 2^-23.  As one chain every addition is a tie: 1.  In chunks of 16: 1, then 16 * 2^-24 = 2^-20, then
    # 2^-23: 1 + 2^-20 + 2^-23, every step exact.
    x = _col([1.0] + [small] * 33)
    assert downmix_ref.downmix(x, [0] * 34, g, 1)[0, 0, 0] == f32(1.0 + 2.0 ** -23)
    assert downmix_ref.downmix(x, [0] * 34, g, 1, chunk=34)[0, 0, 0] == f32(1.0)
    assert downmix_ref.downmix(x, [0] * 34, g, 1, chunk=16)[0, 0, 0] == f32(1.0 + 2.0 ** -20 + 2.0 ** -23)


def test_negative_zero_does_not_survive_a_sum_from_positive_zero():
    nz = f32(-0.0)
    got = downmix_ref.downmix(_col([nz, nz]), [0, 0], np.ones(2, f32), 1)[0, 0, 0]
    assert got.tobytes() == f32(0.0).tobytes()  # +0 + -0 = +0 in round-to-nearest
    got = downmix_ref.downmix(_col([1.0]), [0], np.asarray([nz]), 1)[0, 0, 0]
    assert got.tobytes() == f32(0.0).tobytes()  # 1 * -0 = -0, +0 + -0 = +0


def test_a_gain_of_zero_times_inf_is_nan():
    x = _col([np.inf, 1.0, 2.0])
    out = downmix_ref.downmix(x, [0, 0, 1], np.asarray([0.0, 1.0, 1.0], f32), 2)
    assert np.isnan(out[0, 0, 0]) and out[1, 0, 0] == f32(2.0)
    out = downmix_ref.downmix(x, [-1, 0, 1], np.asarray([0.0, 1.0, 1.0], f32), 2)
    assert out[0, 0, 0] == f32(1.0)  # routed nowhere: takes no part


def test_the_order_is_observable():
    """4096 random members: the plain sequential sum, a chunk of 16 and numpy.sum each differ from the stated order in most elements, so a
    kernel that sums in another order cannot pass the GPU tests by luck."""
    r = np.random.default_rng(1)
    n = 4096
    x = r.standard_normal((n, 64, 2)).astype(f32)
    g = r.uniform(0, 1, n).astype(f32)
    bus = np.zeros(n, int)
    stated = downmix_ref.downmix(x, bus, g, 1)
    for other in (downmix_ref.downmix(x, bus, g, 1, chunk=n), downmix_ref.downmix(x, bus, g, 1, chunk=16),
                  (x * g[:, None, None]).sum(0, dtype=f32)[None]):
        assert (other != stated).mean() > 0.5
    assert downmix_ref.same_bits(stated, downmix_ref.downmix(x, bus, g, 1))


def test_shards_add_in_shard_order():
    r = np.random.default_rng(2)
    x = r.standard_normal((70, 8, 2)).astype(f32)
    g = r.uniform(-1, 1, 70).astype(f32)
    bus = r.integers(-1, 3, 70)
    shards = [(0, 35), (35, 35)]
    want = (np.zeros((3, 8, 2), f32) + downmix_ref.downmix(x[:35], bus[:35], g[:35], 3)) + downmix_ref.downmix(x[35:], bus[35:], g[35:], 3)
    assert downmix_ref.same_bits(downmix_ref.downmix_shards(x, bus, g, 3, shards), want)
    # a bus whose members all lie in shard 0 comes out as from one batch
    bus0 = np.where(np.arange(70) < 35, bus, -1)
    assert downmix_ref.same_bits(downmix_ref.downmix_shards(x, bus0, g, 3, shards), downmix_ref.downmix(x, bus0, g, 3))


def test_the_downmix_kernels_keep_nothing_in_scratch():
    ks = {k: v for k, v in kernels().items() if k.startswith(("k_downmix_chunks<", "k_downmix_sums<"))}
    assert len(ks) == 6, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
