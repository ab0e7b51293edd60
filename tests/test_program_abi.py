"""CPU checks of the envelope programs: the header's declarations and the mirror's bindings, the contract's wording, the queue's row on
both sides, what the Python layer refuses before the library is asked, and oalsfx_host_envelope_adsr against voice_ref.ramp.  (What the
library itself refuses needs a batch, and so a device: tests/test_gpu_programs.py.)"""
import ctypes as C
import os
import re

import numpy as np

import voice_ref as vref
from oalsfxpp_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("oalsfx_batch_set_env_programs", "oalsfx_batch_get_env_programs", "oalsfx_batch_set_lane_env_programs", "oalsfx_batch_get_lane_env_programs")


def test_header_declares_and_the_mirror_binds_the_program_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "#define OALSFX_ENV_PROGRAM_MAX 8" in header and api.ENV_PROGRAM_MAX == 8
    assert header.index("---- envelope programs") > header.index("---- voice filters")
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert "long long oalsfx_debug_program_uploads(" in debug and '"k_program_rows"' in debug and '"k_program_biquad_rows"' in debug
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + ("oalsfx_debug_program_uploads", "oalsfx_host_envelope_adsr"):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    for verb in ("set", "get"):
        restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_env_programs"]
        old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_env_programs"]
        assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:]
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("it is ACTIVE, delay == 0 and ramp_done == ramp_frames", "s = min(F - t, delay + (ramp_frames - ramp_done))", "This check also runs at t == F",
                   "Several zero-length segments go in a row", "the same two records and the same queue as one render of F", "a -0.0f stays negative",
                   "\"Envelope program length out of range.\"", "\"A program's segment is not active.\"", "\"A program's segment glides.\"",
                   "also empty the voice's queue", "is not offered", "it may err on the late side"):
        assert phrase in flat, phrase
    for name in ("program.hip", "program_rows_body.hpp"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", name)).read())
        assert "__syncthreads" not in code and "atomic" not in code and "__shared__" not in code, name
    assert '"hip/program.hip"' in open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()


def test_the_queue_row_is_a_kilobyte():
    text = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "program.hpp")).read()
    assert "sizeof(EnvProgram) == 1024" in text
    assert 16 + (api.ENV_PROGRAM_MAX - 1) * api.ENVELOPE_DTYPE.itemsize == 1024


def test_adsr_is_four_ramps_of_the_ramp_helper():
    rng = np.random.default_rng(1)
    for channels in (1, 2, 6, 8):
        peak, sustain = rng.uniform(0.1, 2, channels).astype(f32), rng.uniform(0, 1, channels).astype(f32)
        attack, decay, hold, release = (int(v) for v in rng.integers(0, 5000, 4))
        got = api.envelope_adsr(peak, sustain, attack, decay, hold, release)
        zero = np.zeros(channels, f32)
        for k, (a, b, frames, flags) in enumerate(((zero, peak, attack, vref.ACTIVE), (peak, peak, hold, vref.ACTIVE), (peak, sustain, decay, vref.ACTIVE),
                                                   (sustain, zero, release, vref.ACTIVE | vref.STOP))):
            want = np.zeros(1, vref.DTYPE)
            want["flags"] = flags
            vref.ramp(want[0], a, b, frames)
            assert got[k].tobytes() == want[0].tobytes(), (channels, k)
    assert lib.load().oalsfx_host_envelope_check(C.c_void_p(got.ctypes.data), 4096, None)


def test_the_mirror_refuses_what_needs_no_library():
    """Batch.set_env_programs on a Batch whose handle was never created: what the Python layer can decide by itself is refused there, with
    the library's words where the library has them; a check that let the call through would fail on the missing library, not with
    BatchError.  (That a program's segments are ACTIVE and do not GLIDE is left to the library: tests/test_gpu_programs.py.)"""
    import pytest

    from test_voice_abi import _unopened, env
    b = _unopened(n=4)
    seg = lambda **kw: env(**kw)[0]
    good = [seg(ramp_frames=5), seg(ramp_frames=7)]
    for programs, kw, what in (
            ([[]], {}, "Envelope program length out of range."),
            ([[seg()] * 9], {}, "Envelope program length out of range."),
            (np.zeros((2, 9), api.ENVELOPE_DTYPE), {}, "Envelope program length out of range."),
            ([good] * 5, {}, "Instance range is out of bounds."),
            ([good, good], dict(instances=[1, 1]), "An instance is listed twice as an envelope target."),
            ([good], dict(instances=[1, 2]), "2 instances but 1 programs"),
            ([good], dict(instances=[4]), "out of bounds"),
            ([[seg(), seg(flags=8 | vref.ACTIVE)]], {}, "Unknown envelope flags."),
            ([[seg(ramp_frames=3, ramp_done=4)]], {}, "The envelope's ramp_done is beyond its ramp."),
            ([[seg(), seg(reserved=[0, 1, 0])]], {}, "The envelope's reserved fields are not 0."),
            (np.array([[seg(), seg(sub=65536)]], api.ENVELOPE_DTYPE), {}, "The envelope's sub is beyond 65535."),
            ([[1, 2]], {}, "envelopes are an array of ENVELOPE_DTYPE")):
        with pytest.raises(api.BatchError, match=what.replace(".", r"\.")):
            b.set_env_programs(programs, **kw)
