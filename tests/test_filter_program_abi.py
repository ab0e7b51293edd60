"""CPU checks of the filter programs through the host-only entry points of the library: the header's declarations and the mirror's
bindings, the contract's wording, the record's and the queue row's sizes on both sides, every refusal's text (in the header, in the
restatement and in the library), what the Python layer refuses before the library is asked, and the two host helpers:
oalsfx_host_filter_program against sweep_ref.make byte for byte, oalsfx_host_filter_sweep_log's lengths, continuity, ends, node
frequencies and refusals.  (What a set call refuses needs a batch, and so a device: tests/test_gpu_filter_programs.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import filter_program_ref as fref
import sweep_ref as wref
from oalsfxpp_amd import api, desc, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("oalsfx_batch_set_filter_programs", "oalsfx_batch_get_filter_programs", "oalsfx_batch_set_lane_filter_programs", "oalsfx_batch_get_lane_filter_programs")
HOST = ("oalsfx_host_filter_program", "oalsfx_host_filter_sweep_log")
TEXTS = tuple(fref.MESSAGES.values()) + ("An instance is listed twice as a filter program target.", "No filter program lengths.")


def test_header_declares_and_the_mirror_binds_the_filter_program_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES + HOST:
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "#define OALSFX_FILTER_PROGRAM_MAX 8" in header and api.FILTER_PROGRAM_MAX == desc.FILTER_PROGRAM_MAX == fref.MAX == 8
    assert header.index("---- filter programs") > header.index("---- envelope programs") > header.index("---- voice filter sweeps")
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert "long long oalsfx_debug_filter_program_uploads(" in debug and '"k_filter_program_rows"' in debug and '"k_filter_program_env_rows"' in debug
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + HOST + ("oalsfx_debug_filter_program_uploads",):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    for verb in ("set", "get"):
        restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_filter_programs"]
        old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_filter_programs"]
        assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:]
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("not OALSFX_SWEEP_ACTIVE, or done == frames", "s = min(F - t, frames - done)", "This check also runs at t == F", "the new one has done == 0",
                   "the same filter record, sweep record and queue as one render of F", "are `to` of segment k - 1", "takes its `from` (index 0)",
                   "only the filter stage looks at the queue", "A length of 1 is oalsfx_batch_set_lane_sweeps exactly", "also empty the voice's queue",
                   "every refusal of oalsfx_batch_set_sweeps, for every segment", "it may err on the late side") + tuple(f'"{m}"' for m in fref.MESSAGES.values()):
        assert phrase in flat, phrase
    code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "filter_program.hip")).read())
    assert "__syncthreads" not in code and "atomic" not in code and "fma" not in code and "__shared__" not in code and "#pragma clang fp contract(off)" in code
    assert '"hip/filter_program.hip"' in open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()


def test_every_refusal_has_its_text_in_the_library():
    blob = open(lib.LIB_PATH, "rb").read()
    for text in TEXTS:
        assert text.encode() + b"\0" in blob, text
    assert len(set(TEXTS)) == len(TEXTS)
    # (the refusals of a record by itself are oalsfx_host_filter_sweep_check's, for every segment: tests/test_sweep_ref.py)
    assert lib.load().oalsfx_batch_set_filter_programs(None, None, 0, None, None) == 0
    assert lib.load().oalsfx_batch_get_lane_filter_programs(None, 0, None, 0, None, None) == 0


def test_the_queue_row_is_576_bytes_on_both_sides():
    text = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "filter_program.hpp")).read()
    assert "sizeof(FilterProgram) == 576" in text
    assert api.FILTER_QUEUE_DTYPE.itemsize == C.sizeof(desc.FilterProgramQueue) == 16 + (api.FILTER_PROGRAM_MAX - 1) * api.SWEEP_DTYPE.itemsize == 576
    for name, at in dict(head=0, count=4, reserved=8, queue=16).items():
        assert api.FILTER_QUEUE_DTYPE.fields[name][1] == at == getattr(desc.FilterProgramQueue, name).offset, name
    assert api.SWEEP_DTYPE.itemsize == 80 and 576 % 16 == 0


@pytest.mark.parametrize("segments", [1, 2, 3, 8])
def test_the_program_helper_is_the_sweep_helper_per_segment(segments):
    rng = np.random.default_rng(segments)
    nodes = np.concatenate([bcases.filt(bcases.low_pass(rng.uniform(0.01, 0.4)), x=rng.uniform(-1, 1, (8, 2))) for _ in range(segments + 1)])
    frames = [int(v) for v in rng.integers(1, 5000, segments)]
    got = api.filter_program(nodes, frames)
    for k in range(segments):
        assert got[k].tobytes() == wref.make(bref.coefficients(nodes[k]), bref.coefficients(nodes[k + 1]), frames[k])[0].tobytes(), k
        assert got[k:k + 1].tobytes() == api.filter_sweep(nodes[k], nodes[k + 1], frames[k]).tobytes(), k
        if k + 1 < segments:
            assert got[k]["to"].tobytes() == got[k + 1]["from"].tobytes()
    assert np.asarray(fref.chain([bref.coefficients(n) for n in nodes], frames), wref.DTYPE).tobytes() == got.tobytes()
    assert fref.check(list(got)) is None


def test_the_program_helper_refuses():
    node = bcases.filt()
    for nodes, frames in ((np.concatenate([node] * 10), [5] * 9), (np.concatenate([node] * 3), [5, 0]), (np.concatenate([node] * 3), [5, (1 << 24) + 1]),
                          (np.concatenate([node] * 2), [5, 5]), (node, [])):
        with pytest.raises(api.BatchError):
            api.filter_program(nodes, frames)
    assert lib.load().oalsfx_host_filter_program(None, None, 1, None) == 0


def ulps(a, b):
    """The distance of two positive float32 in units of the last place."""
    return abs(int(np.asarray(a, f32).view(np.int32)) - int(np.asarray(b, f32).view(np.int32)))


@pytest.mark.parametrize("kind, f0, f1, frames, segments", [
    (desc.VF_LOW_PASS, 0.004, 0.4, 48000, 8), (desc.VF_LOW_PASS, 0.3, 0.01, 1001, 3), (desc.VF_BAND_PASS, 0.02, 0.02, 7, 7),
    (desc.VF_HIGH_PASS, 0.05, 0.25, 100, 1), (desc.VF_PEAKING, 0.01, 0.45, 1 << 24, 5), (desc.VF_LOW_PASS, 0.1, 0.2, 13, 8)])
def test_the_log_sweep(kind, f0, f1, frames, segments):
    gain, rcp_q = 2.0, 0.9
    out, freq = api.filter_sweep_log(kind, gain, f0, f1, rcp_q, frames, segments)
    assert len(out) == segments and len(freq) == segments + 1
    lengths = out["frames"].astype(np.int64)
    assert lengths.sum() == frames and (lengths[:frames % segments] == frames // segments + 1).all() and (lengths[frames % segments:] == frames // segments).all()
    assert (out["flags"] == wref.ACTIVE).all() and (out["done"] == 0).all() and fref.check(list(out)) is None
    for k in range(segments - 1):
        assert out[k]["to"].tobytes() == out[k + 1]["from"].tobytes(), k
    # the ends as given, every node within 2 ulp of the float64 power, and every node's design the design routine's
    assert freq[0].tobytes() == f32(f0).tobytes() and freq[-1].tobytes() == f32(f1).tobytes()
    a, b = np.float64(f32(f0)), np.float64(f32(f1))
    for k in range(segments + 1):
        assert ulps(freq[k], f32(a * (b / a) ** (k / segments))) <= 2, (k, freq[k])
        node = np.zeros(1, api.FILTER_DTYPE)
        assert lib.load().oalsfx_host_voice_filter(kind, gain, float(freq[k]), rcp_q, C.c_void_p(node.ctypes.data))
        coef = out[k]["from"] if k < segments else out[k - 1]["to"]
        assert coef.tobytes() == bref.coefficients(node[0]).tobytes(), k


def test_the_log_sweep_refuses():
    for args in ((desc.VF_LOW_PASS, 1.0, 0.01, 0.2, 1.0, 3, 4), (desc.VF_LOW_PASS, 1.0, 0.01, 0.2, 1.0, 100, 0), (desc.VF_LOW_PASS, 1.0, 0.01, 0.2, 1.0, 100, 9),
                 (desc.VF_LOW_PASS, 1.0, 0.0, 0.2, 1.0, 100, 4), (desc.VF_LOW_PASS, 1.0, 0.01, -0.2, 1.0, 100, 4), (desc.VF_LOW_PASS, 1.0, 0.01, 0.6, 1.0, 100, 4),
                 (9, 1.0, 0.01, 0.2, 1.0, 100, 4), (desc.VF_LOW_PASS, 1.0, 0.01, 0.2, 1.0, (1 << 24) + 1, 4)):
        with pytest.raises(api.BatchError):
            api.filter_sweep_log(*args)
    # nothing written where it refuses; node_freq_out may be NULL
    buf = np.zeros(4, api.SWEEP_DTYPE)
    buf["frames"] = 77
    assert lib.load().oalsfx_host_filter_sweep_log(desc.VF_LOW_PASS, 1.0, 0.01, 0.6, 1.0, 100, 4, C.c_void_p(buf.ctypes.data), None) == 0 and (buf["frames"] == 77).all()
    assert lib.load().oalsfx_host_filter_sweep_log(desc.VF_LOW_PASS, 1.0, 0.01, 0.2, 1.0, 100, 4, C.c_void_p(buf.ctypes.data), None) == 1 and buf["frames"].sum() == 100


def test_the_mirror_refuses_what_needs_no_library():
    """Batch.set_filter_programs on a Batch whose handle was never created: what the Python layer can decide by itself is refused there, with
    the library's words where the library has them."""
    from test_voice_abi import _unopened
    b = _unopened(n=4)
    seg = wref.make((1, 0, 0, 0, 0), (0.5, 0.1, 0, -0.2, 0.1), 100)[0]
    good = [seg, seg]
    for programs, kw, what in (
            ([[]], {}, "Filter program length out of range."),
            ([[seg] * 9], {}, "Filter program length out of range."),
            (np.zeros((2, 9), api.SWEEP_DTYPE), {}, "Filter program length out of range."),
            ([good] * 5, {}, "Instance range is out of bounds."),
            ([good, good], dict(instances=[1, 1]), "An instance is listed twice as a filter program target."),
            ([good], dict(instances=[1, 2]), "2 instances but 1 programs"),
            ([good], dict(instances=[4]), "out of bounds"),
            ([[1, 2]], {}, "sweeps are an array of SWEEP_DTYPE")):
        with pytest.raises(api.BatchError, match=what.replace(".", r"\.")):
            b.set_filter_programs(programs, **kw)
