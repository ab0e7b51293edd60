"""CPU checks of polyphony: the C ABI declares and exports the eight calls and the mirror binds them, OALSFX_MAX_POLYPHONY is 16 on both
sides, the header states the contract, and the layers above offer the lanes -- no GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

import polyphony_ref as pref
from oalsfxpp_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_CALLS = ("samplers", "envelopes", "resamplers")
NAMES = ("oalsfx_batch_set_polyphony", "oalsfx_batch_get_polyphony") + tuple(f"oalsfx_batch_{verb}_lane_{what}" for what in RECORD_CALLS for verb in ("set", "get"))


def test_header_declares_and_the_mirror_binds_the_polyphony_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    assert len(NAMES) == 8
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
    assert header.index("---- polyphony") > header.index("---- resamplers")
    assert re.search(r"#define OALSFX_MAX_POLYPHONY 16\b", header) and api.MAX_POLYPHONY == pref.MAX_POLYPHONY == 16
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in lib.SIGNATURES and hasattr(so, name), name
    for what in RECORD_CALLS:
        # the lane forms take the lane in front of the instances and are otherwise the calls they generalise
        for verb in ("set", "get"):
            restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_{what}"]
            old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_{what}"]
            assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:], (verb, what)
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("in[f][c] = (((+0.0f + o_0) + o_1) + ...) + o_(K-1)", "Lanes are summed ascending, every addition is rounded by itself",
                   "last product is not fused into the sum", "may be added or left out", "a lone voice's -0.0f therefore reaches the input as +0.0f",
                   "the reason K == 1 keeps its own path", "voice row = lane * instances + instance", "the same 3 * K records as one render of F",
                   "\"Polyphony out of range.\"", "\"A lane that would be dropped is still in use.\"", "\"Lane out of range.\"",
                   "oalsfx_batch_reset, _snapshot and _restore neither touch nor carry it", "checked against the sampler of the same lane and instance"):
        assert phrase in flat, phrase
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert '"k_mix_rows"' in debug
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "polyphony.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "__shared__" not in kernel and "__syncthreads" not in kernel and "atomicAdd" not in kernel


def test_the_layers_above_offer_the_lanes():
    assert callable(api.Batch.set_polyphony) and isinstance(api.Batch.polyphony, property)
    for what in RECORD_CALLS:
        for verb in ("set", "get"):
            lane = inspect.signature(getattr(api.Batch, f"{verb}_{what}")).parameters["lane"]
            assert lane.default == 0, (verb, what)
    array = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    for declaration in (r"bool set_polyphony\(int lanes\);", r"int get_polyphony\(\) const;",
                        r"bool set_sampler\(int index, int lane, const oalsfx_sampler& sampler\);", r"bool get_sampler\(int index, int lane, oalsfx_sampler& sampler\);",
                        r"bool set_envelope\(int index, int lane, const oalsfx_envelope& envelope\);", r"bool get_envelope\(int index, int lane, oalsfx_envelope& envelope\);",
                        r"bool set_resampler\(int index, int lane, int table\);", r"bool get_resampler\(int index, int lane, int& table\);",
                        # ... beside the signatures that mean lane 0
                        r"bool set_sampler\(int index, const oalsfx_sampler& sampler\);", r"bool get_resampler\(int index, int& table\);"):
        assert re.search(declaration, array), declaration
    build = open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()
    assert '"hip/polyphony.hip"' in build


def test_what_the_mirror_refuses_without_the_library():
    unopened = api.Batch.__new__(api.Batch)
    unopened.n, unopened.channels, unopened._h, unopened._lib = 8, 2, None, None
    for lanes in (0, -1, 17):
        with pytest.raises(api.BatchError, match="Polyphony out of range."):
            unopened.set_polyphony(lanes)
