"""CPU checks of the voice filter sweeps: the header's declarations and the mirror's bindings, the contract's wording, the record's size
and offsets on both sides, and the host helper's arithmetic against sweep_ref.make.  (What the library refuses in a set call needs a
batch, and so a device: tests/test_gpu_sweeps.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import sweep_ref as wref
from oalsfxpp_amd import api, desc, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("oalsfx_batch_set_sweeps", "oalsfx_batch_get_sweeps", "oalsfx_batch_set_lane_sweeps", "oalsfx_batch_get_lane_sweeps")
HOST = ("oalsfx_host_filter_sweep", "oalsfx_host_filter_sweep_check")


def test_header_declares_and_the_mirror_binds_the_sweep_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES + HOST:
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "#define OALSFX_SWEEP_ACTIVE 1" in header and desc.SWEEP_ACTIVE == 1 == wref.ACTIVE
    assert header.index("---- envelope programs") > header.index("---- voice filter sweeps") > header.index("---- voice filters")
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert "long long oalsfx_debug_sweep_uploads(" in debug and '"k_sweep_rows"' in debug and '"k_sweep_program_rows"' in debug
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + HOST + ("oalsfx_debug_sweep_uploads",):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    for verb in ("set", "get"):
        restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_sweeps"]
        old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_sweeps"]
        assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:]
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("from[k] + ((float)n * step[k]) for n < R and to[k] for n >= R", "no fused multiply-add and no running sum", "all five coefficients frame f's",
                   "done = min(R, done + F)", "clears the sweep's ACTIVE", "is a triangle and therefore convex", "the device checks nothing",
                   "linear in the COEFFICIENTS", "also cancel the voice's sweep", "it may err on the late side") + tuple(f'"{m}"' for m in wref.MESSAGES.values()):
        assert phrase in flat, phrase
    code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "sweep.hip")).read())
    assert "__syncthreads" not in code and "atomic" not in code and "fma" not in code and "#pragma clang fp contract(off)" in code
    assert '"hip/sweep.hip"' in open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()


def test_the_record_is_80_bytes_on_both_sides():
    offsets = dict(flags=0, frames=4, done=8, reserved=12, step=36, to=56, reserved1=76)
    assert api.SWEEP_DTYPE.itemsize == C.sizeof(desc.FilterSweep) == 80
    for name, at in offsets.items():
        assert api.SWEEP_DTYPE.fields[name][1] == at == getattr(desc.FilterSweep, name).offset, name
    assert api.SWEEP_DTYPE.fields["from"][1] == 16 == desc.FilterSweep.from_.offset
    text = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "sweep.hip")).read()
    assert "sizeof(oalsfx_filter_sweep) == 80" in text and "offsetof(oalsfx_filter_sweep, from) == 16" in text and "offsetof(oalsfx_filter_sweep, to) == 56" in text


@pytest.mark.parametrize("frames", [1, 2, 3, 100, 48000, 1 << 24])
def test_the_helper_is_one_subtraction_and_one_division(frames):
    rng = np.random.default_rng(frames % 1000)
    a, b = bcases.filt(bcases.low_pass(rng.uniform(0.01, 0.4))), bcases.filt(bcases.band_pass(rng.uniform(0.01, 0.4)), flags=0, x=rng.uniform(-1, 1, (8, 2)))
    got = api.filter_sweep(a, b, frames)
    want = wref.make(bref.coefficients(a[0]), bref.coefficients(b[0]), frames)
    assert got.tobytes() == want.tobytes()
    assert got["flags"][0] == wref.ACTIVE and got["done"][0] == 0 and api.filter_sweep_check(got) is None


def test_the_helper_refuses_a_length_out_of_range():
    a = bcases.filt()
    for frames in (0, (1 << 24) + 1):
        with pytest.raises(api.BatchError):
            api.filter_sweep(a, a, frames)
    assert "No filter sweep record." == _check_null()


def _check_null():
    message = C.c_char_p()
    assert lib.load().oalsfx_host_filter_sweep_check(None, C.byref(message)) == 0
    return message.value.decode()
