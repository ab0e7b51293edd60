"""CPU checks of the level meters: the C ABI declares and exports them, the record is 80 bytes with the same offsets in C, ctypes and
NumPy, the Python mirror binds the calls and refuses bad arguments before the library is reached, the lane count is one constant
everywhere, the NumPy restatement computes what the header states (and an order other than the stated one shows), and the kernels keep
nothing in scratch memory -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import meter_ref
from oalsfxpp_amd import api, desc, lib
from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_meter_device", "oalsfx_batch_mix_downmix_meter", "oalsfx_group_mix_downmix_meter")
f32 = np.float32
FIELDS = ("peak", "sumsq", "peak_hold", "quiet_run", "nonfinite", "frames")


def test_header_declares_and_the_mirror_binds_the_meter_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in lib.SIGNATURES, name
    assert "no bus meters" in header    # the group's limit is stated where the call is declared


def test_the_library_exports_the_meter_calls():
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(so, name), name


def test_the_array_header_declares_the_metered_methods():
    header = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    tail = r", int bus_count, float\* dst_buses, float threshold, bool carry,\s+oalsfx_meter\* voice_meters, oalsfx_meter\* bus_meters\);"
    assert re.search(r"bool mix_to_buses_metered\(int sample_count, const float\* src_samples" + tail, header)
    assert re.search(r"bool mix_to_buses_metered\(int sample_count, const float\* const\* src_samples" + tail, header)


def test_the_record_is_80_bytes_with_the_same_offsets_everywhere():
    src = r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "oalsfx_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(oalsfx_meter), offsetof(oalsfx_meter, peak), offsetof(oalsfx_meter, sumsq),
               offsetof(oalsfx_meter, peak_hold), offsetof(oalsfx_meter, quiet_run), offsetof(oalsfx_meter, nonfinite),
               offsetof(oalsfx_meter, frames), OALSFX_METER_LANES, OALSFX_METER_CARRY);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "m.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "m")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 80 == C.sizeof(desc.Meter) == api.METER_DTYPE.itemsize == meter_ref.DTYPE.itemsize
    assert got[1:7] == [0, 32, 64, 68, 72, 76]
    assert [getattr(desc.Meter, f).offset for f in FIELDS] == got[1:7]
    for dtype in (api.METER_DTYPE, meter_ref.DTYPE):
        assert dtype.names == FIELDS and [dtype.fields[f][1] for f in FIELDS] == got[1:7]
    assert got[7] == api.METER_LANES and got[8] == api.METER_CARRY == meter_ref.CARRY


def test_the_lane_count_is_one_constant():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    (value,) = re.findall(r"^#define OALSFX_METER_LANES (\d+)$", header, flags=re.M)
    assert int(value) == api.METER_LANES == meter_ref.LANES == 64
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "meter.hip")).read()
    assert "kWave = OALSFX_METER_LANES" in kernel


def test_the_header_states_the_arithmetic():
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read())
    for phrase in ("p = fmaxf(p, fabsf(x[f][c]))", "q_l = q_l + (x[f][c] * x[f][c])", "for s = 32, 16, 8, 4, 2, 1: for every l < s, q_l = q_l + q_{l+s}",
                   "!(fabsf(x) < INFINITY)", "fabsf(x[f][c]) <= threshold", "min(old.quiet_run + F, UINT32_MAX)",
                   "fmaxf(old.peak_hold, max_c peak[c])"):
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


def _unopened_group(n=8, channels=2):
    g = api.Group.__new__(api.Group)
    g.n = n
    g.channels = channels
    g._h = None
    g._lib = None
    return g


@pytest.mark.parametrize("kwargs, what", [
    (dict(rows=0), "Row count"), (dict(rows=-4), "Row count"), (dict(frames=-1), "Frame count is negative"),
    (dict(threshold=-1e-30), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=None), "threshold"),
    (dict(carry=2), "Unknown meter flags"), (dict(carry=-1), "Unknown meter flags"),
    (dict(src_ptr=0), "No source samples"), (dict(meters_ptr=0), "No meter records"), (dict(src_ptr=0x1002), "4-byte aligned"),
    (dict(meters_ptr=0x100008), "16-byte aligned")])
def test_meter_device_checks_its_arguments(kwargs, what):
    args = dict(rows=8, frames=16, src_ptr=0x1000, meters_ptr=0x100000, threshold=0.001)
    args.update(kwargs)
    with pytest.raises(api.BatchError, match=what):
        _unopened().meter_device(**args)


def test_mix_downmix_meter_checks_its_arrays():
    b, g = _unopened(), _unopened_group()
    good = np.zeros((8, 16, 2), f32)
    for target in (b, g):
        with pytest.raises(api.BatchError, match="Bus count"):
            target.mix_downmix_meter(good, 0, 0.0)
        for bad in (np.zeros((7, 16, 2), f32), np.zeros((8, 16, 1), f32), np.zeros((8, 32), f32)):
            with pytest.raises(api.BatchError, match="the source is"):
                target.mix_downmix_meter(bad, 1, 0.0)
        for threshold in (-0.5, float("nan"), "loud"):
            with pytest.raises(api.BatchError, match="threshold"):
                target.mix_downmix_meter(good, 1, threshold)
        with pytest.raises(api.BatchError, match="Unknown meter flags"):
            target.mix_downmix_meter(good, 1, 0.0, carry=4)
        for meters in (np.zeros(7, api.METER_DTYPE), np.zeros(8 * 20, f32), np.zeros((8, 1), api.METER_DTYPE), np.zeros(16, api.METER_DTYPE)[::2], [0] * 8):
            with pytest.raises(api.BatchError, match="the meter array"):
                target.mix_downmix_meter(good, 1, 0.0, voice_meters=meters)
    with pytest.raises(api.BatchError, match="the meter array"):
        b.mix_downmix_meter(good, 3, 0.0, bus_meters=np.zeros(2, api.METER_DTYPE))
    for dst in (np.zeros((2, 16, 2), f32), np.zeros((1, 16, 2), np.float64), np.zeros((1, 15, 2), f32)):
        with pytest.raises(api.BatchError, match="the bus array is"):
            b.mix_downmix_meter(good, 1, 0.0, dst=dst)


# ---- the restatement against values worked out by hand ----
def _row(values):
    """One mono row: [1][frames][1]."""
    return np.asarray(values, dtype=f32).reshape(1, -1, 1)


def _bits(value):
    return np.asarray(value, dtype=f32).tobytes()


SMALL = 2.0 ** -12  # its square, 2^-24, is half an ulp of 1: 1 + 2^-24 is a tie and rounds to even, back to 1


def test_a_tie_rounds_differently_in_lane_order_than_in_frame_order():
    values = np.zeros(66)
    values[0], values[1], values[65] = 1.0, SMALL, SMALL
    x = _row(values)
    # frame order: (1 + 2^-24) + 2^-24, two ties: 1.  Lane order: lane 0 holds 1, lane 1 holds 2^-24 + 2^-24 = 2^-23 (frames 1 and 65),
    # and the tree's last step adds them: 1 + 2^-23 exactly.
    assert meter_ref.meter(x, 0.0)["sumsq"][0, 0] == f32(1.0 + 2.0 ** -23)
    assert meter_ref.sumsq(x, lanes=1)[0, 0] == f32(1.0)
    # with the two small frames a lane apart (1 and 2) the tree adds lane 2 into lane 0 first (s = 2), then lane 1 (s = 1): two ties, 1
    values = np.zeros(66)
    values[0], values[1], values[2] = 1.0, SMALL, SMALL
    assert meter_ref.meter(_row(values), 0.0)["sumsq"][0, 0] == f32(1.0)


def test_fewer_frames_than_lanes():
    m = meter_ref.meter(_row([1.0, SMALL, SMALL]), 0.5)[0]
    # s = 2: q_0 = 1 + 2^-24 (frame 2), a tie: 1; s = 1: q_0 = 1 + 2^-24 (frame 1): 1.  Adding lanes 1 and 2 first would give 1 + 2^-23.
    assert m["sumsq"][0] == f32(1.0) and m["sumsq"][1:].view(np.uint32).max() == 0
    assert m["peak"][0] == f32(1.0) and m["peak"][1:].view(np.uint32).max() == 0      # channels the format lacks: +0.0f
    assert m["peak_hold"] == f32(1.0) and m["frames"] == 3 and m["nonfinite"] == 0
    assert m["quiet_run"] == 2    # frames 1 and 2 are within 0.5
    assert meter_ref.meter(_row([0.25]), 0.5)[0]["quiet_run"] == 1 and meter_ref.meter(_row([0.75]), 0.5)[0]["quiet_run"] == 0
    assert meter_ref.meter(_row([0.5]), 0.5)[0]["quiet_run"] == 1     # |x| == threshold is quiet


def test_sixty_five_frames_give_lane_zero_a_second_frame():
    values = np.zeros(65)
    values[0], values[64] = SMALL, 1.0
    m = meter_ref.meter(_row(values), 0.5)[0]
    assert m["sumsq"][0] == f32(1.0)        # lane 0: (+0 + 2^-24) + 1, a tie: 1
    assert m["quiet_run"] == 0 and m["frames"] == 65
    values[0], values[64] = 1.0, SMALL
    m = meter_ref.meter(_row(values), 0.5)[0]
    assert m["sumsq"][0] == f32(1.0) and m["quiet_run"] == 64
    values[63] = SMALL                      # lane 63 comes in at s = 32, onto lane 31, and reaches lane 0 as 2^-24: still a tie
    assert meter_ref.meter(_row(values), 0.5)[0]["sumsq"][0] == f32(1.0)
    values[63] = 0.0
    values[1] = SMALL                       # frames 1 and 64: lane 1 and lane 0's second frame; lane 0 = 1 (tie), + lane 1: 1 (tie)
    assert meter_ref.meter(_row(values), 0.5)[0]["sumsq"][0] == f32(1.0)


def test_a_nan_is_ignored_by_the_peak_counted_and_loud():
    m = meter_ref.meter(_row([0.5, np.nan, 0.25]), 1.0)[0]
    assert m["peak"][0] == f32(0.5) and m["peak_hold"] == f32(0.5)
    assert m["nonfinite"] == 1 and m["quiet_run"] == 1 and np.isnan(m["sumsq"][0])
    m = meter_ref.meter(_row([np.nan, np.nan]), 1.0)[0]
    assert _bits(m["peak"][0]) == _bits(0.0) and m["nonfinite"] == 2 and m["quiet_run"] == 0
    m = meter_ref.meter(_row([-np.inf, 0.0, 0.0]), 1.0)[0]
    assert m["peak"][0] == f32(np.inf) and m["sumsq"][0] == f32(np.inf) and m["nonfinite"] == 1 and m["quiet_run"] == 2
    x = np.zeros((1, 4, 2), f32)            # stereo: all channels count
    x[0, 1, 1], x[0, 2, 0] = np.nan, np.inf
    m = meter_ref.meter(x, 1.0)[0]
    assert m["nonfinite"] == 2 and m["quiet_run"] == 1 and m["peak"][0] == f32(np.inf) and _bits(m["peak"][1]) == _bits(0.0)
    assert m["peak_hold"] == f32(np.inf)


def test_negative_zero():
    m = meter_ref.meter(_row([-0.0] * 70), 0.0)[0]
    assert _bits(m["peak"][0]) == _bits(0.0) and _bits(m["sumsq"][0]) == _bits(0.0) and _bits(m["peak_hold"]) == _bits(0.0)
    assert m["quiet_run"] == 70 and m["nonfinite"] == 0    # |-0| <= 0: quiet at a threshold of 0


def test_a_denormal_whose_square_underflows():
    tiny, denormal = f32(1e-30), f32(1e-40)
    assert f32(tiny * tiny) == 0 and denormal != 0
    m = meter_ref.meter(_row([tiny, denormal, 0.0]), 0.0)[0]
    assert m["peak"][0] == tiny and _bits(m["sumsq"][0]) == _bits(0.0)
    assert m["quiet_run"] == 1              # the denormal is above a threshold of 0: nothing is flushed
    m = meter_ref.meter(_row([denormal]), 0.0)[0]
    assert _bits(m["peak"][0]) == _bits(denormal) and m["quiet_run"] == 0
    # squares that are denormal themselves add up without a flush: thirty-three times (2^-70)^2
    m = meter_ref.meter(_row([2.0 ** -70, 0.0] * 32 + [2.0 ** -70]), 1.0)[0]
    assert _bits(m["sumsq"][0]) == _bits(33 * 2.0 ** -140) and m["sumsq"][0] != 0


def test_carry_adds_up_saturates_and_restarts():
    old = np.zeros(1, meter_ref.DTYPE)
    quiet, loud_then_quiet = _row([0.0] * 64), _row([0.0, 0.9] + [0.0] * 5)
    m = meter_ref.meter(quiet, 0.5, old)
    assert m[0]["quiet_run"] == 64
    m = meter_ref.meter(quiet, 0.5, m)
    assert m[0]["quiet_run"] == 128
    m = meter_ref.meter(loud_then_quiet, 0.5, m)
    assert m[0]["quiet_run"] == 5 and m[0]["peak_hold"] == f32(0.9)      # a loud frame: the run starts again behind it
    m = meter_ref.meter(quiet, 0.5, m)
    assert m[0]["quiet_run"] == 69 and m[0]["peak_hold"] == f32(0.9) and _bits(m[0]["peak"][0]) == _bits(0.0)
    old["quiet_run"] = meter_ref.UINT32_MAX - 10
    assert meter_ref.meter(quiet, 0.5, old)[0]["quiet_run"] == meter_ref.UINT32_MAX
    old["quiet_run"] = meter_ref.UINT32_MAX - 64
    assert meter_ref.meter(quiet, 0.5, old)[0]["quiet_run"] == meter_ref.UINT32_MAX
    old["quiet_run"] = meter_ref.UINT32_MAX - 65
    assert meter_ref.meter(quiet, 0.5, old)[0]["quiet_run"] == meter_ref.UINT32_MAX - 1
    # without carry what is at the destination does not matter
    assert meter_ref.meter(quiet, 0.5)[0]["quiet_run"] == 64


def test_peak_hold_replaces_an_old_nan():
    old = np.zeros(1, meter_ref.DTYPE)
    old["peak_hold"] = np.nan
    assert meter_ref.meter(_row([0.25, -0.5]), 0.0, old)[0]["peak_hold"] == f32(0.5)
    old["peak_hold"] = 2.0
    assert meter_ref.meter(_row([0.25, -0.5]), 0.0, old)[0]["peak_hold"] == f32(2.0)
    assert meter_ref.meter(_row([np.nan]), 0.0, old)[0]["peak_hold"] == f32(2.0)


def _sumsq_fused(x, lanes):
    """The stated order with q = fma(x, x, q): the product is exact in float64, and the one rounding of the sum to float32 is what a
    fused multiply-add does (but for double roundings, which are rare and only lower the share this is used for)."""
    rows, frames, channels = x.shape
    q = np.zeros((rows, lanes, channels), dtype=f32)
    for base in range(0, frames, lanes):
        block = x[:, base:base + lanes].astype(np.float64)
        q[:, :block.shape[1]] = (q[:, :block.shape[1]].astype(np.float64) + block * block).astype(f32)
    s = lanes // 2
    while s >= 1:
        q[:, :s] = q[:, :s] + q[:, s:2 * s]
        s //= 2
    return q[:, 0]


def test_the_order_is_observable():
    """4096 random stereo rows of 256 frames: the frame-by-frame sum, numpy.sum, 32 lanes and a fused multiply-add each differ from the
    stated order in a clear share of the values, so a kernel that sums another way cannot pass the GPU tests by luck."""
    x = np.random.default_rng(1).standard_normal((4096, 256, 2)).astype(f32)
    stated = meter_ref.sumsq(x)
    shares = {"frame by frame": (meter_ref.sumsq(x, lanes=1) != stated).mean(),
              "numpy.sum": ((x * x).sum(axis=1, dtype=f32) != stated).mean(),
              "32 lanes": (meter_ref.sumsq(x, lanes=32) != stated).mean(),
              "fused multiply-add": (_sumsq_fused(x, 64) != stated).mean()}
    print(shares)
    assert shares["frame by frame"] > 0.5 and shares["numpy.sum"] > 0.5 and shares["32 lanes"] > 0.1 and shares["fused multiply-add"] > 0.05, shares
    assert meter_ref.same_bits(stated, meter_ref.meter(x, 0.0)["sumsq"][:, :2])
    # up to 64 frames 32 lanes are the same sum by construction (lane l + 32 is added into lane l either way)
    assert meter_ref.same_bits(meter_ref.sumsq(x[:, :64], lanes=32), meter_ref.sumsq(x[:, :64]))


def test_the_meter_kernels_are_built_and_keep_nothing_in_scratch():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_meter_rows<")}
    # channels x floats per load: mono 1; stereo 1, 2; quad 1, 2, 4; 5.1 1, 2; 6.1 1; 7.1 1, 2, 4
    assert sorted(ks) == sorted(f"k_meter_rows<{c}, {v}>" for c, vs in ((1, (1,)), (2, (1, 2)), (4, (1, 2, 4)), (6, (1, 2)), (7, (1,)), (8, (1, 2, 4)))
                                for v in vs), sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
