"""CPU checks of the sampler streams: the ring row's layout on both sides, the header's declarations and contract phrases, the mirror's
bindings, what the layers above offer, and the refusals that are decided without a device.  (The refusals that need one -- a ring that is
full by the device's own count, an asset outside its allocation, the glide and filter rules -- are in tests/test_gpu_streams.py.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sampler_ref as sref
import stream_ref as stref
from oalsfxpp_amd import api, desc, lib
from test_sampler_abi import rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERBS = ("set", "append", "get")
NAMES = tuple(f"oalsfx_batch_{v}_{lane}streams" for v in VERBS for lane in ("", "lane_")) + ("oalsfx_batch_get_stream_state", "oalsfx_batch_get_lane_stream_state")


def test_the_ring_row_is_656_bytes_on_both_sides(tmp_path):
    src = r'''
    #include <cstddef>
    #include <cstdio>
    #include "stream.hpp"
    int main() {
        using oalsfx_hip::StreamRing;
        std::printf("%zu %zu %zu %zu %zu %d\n", sizeof(StreamRing), offsetof(StreamRing, queued), offsetof(StreamRing, reset), offsetof(StreamRing, entry),
                    sizeof(oalsfx_sampler), OALSFX_STREAM_QUEUE);
        return 0;
    }'''
    cpp, exe = str(tmp_path / "s.cpp"), str(tmp_path / "s")
    open(cpp, "w").write(src)
    hip = os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", hip, "-I", os.path.join(ROOT, "oalsfxpp_amd", "csrc", "host"),
                    "-x", "hip", "--offload-arch=gfx950", cpp, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [656, 0, 4, 16, 80, 8]
    t = api.STREAM_RING_DTYPE
    assert t.itemsize == C.sizeof(desc.StreamRing) == 656 and [t.fields[k][1] for k in ("queued", "reset", "reserved", "entry")] == [0, 4, 8, 16]
    assert desc.StreamRing.entry.offset == 16 and api.STREAM_QUEUE == desc.STREAM_QUEUE == stref.QUEUE == 8


def test_header_declares_and_the_mirror_binds_the_stream_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in lib.SIGNATURES and hasattr(so, name), name
    assert "#define OALSFX_STREAM_QUEUE 8" in header and header.index("---- sampler streams") > header.index("---- filter programs")
    for verb in VERBS:
        restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_streams"]
        old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_streams"]
        assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:] and old_args == lib.SIGNATURES["oalsfx_batch_set_env_programs"][1]
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("position >= E, whether or not it is PLAYING", "at position wrap(entry.position + over)", "chains of takes are bounded by the ring",
                   "is replaced in that render, with its over", "position = E and PLAYING cleared", "is replaced with over = 0",
                   "the envelope runs on across a take untouched", "an intro and its loop are two entries", "Nothing interpolates across the seam",
                   "provided the appends fall at the same frames", "plays the whole asset's bits at any step and any start", "\"The stream queue is full.\"",
                   "\"A queued sampler is not playing.\"", "\"Stream length out of range.\"", "\"The streaming voice's envelope glides.\"", "\"The gliding voice streams.\"",
                   "\"An instance is listed twice as a stream target.\"", "also empty the voice's ring and zero taken", "taken > j", "_snapshot and _restore neither touch nor carry them",
                   "a dropped lane whose ring holds an entry is refused", "Not done: interpolation across the seam", "k_stream_filter_rows if any voice filter is ACTIVE"):
        assert phrase in flat, phrase
    for phrase in ("not offered while",):
        assert phrase not in flat, phrase
    for phrase in ():
        assert phrase in flat, phrase
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "stream.hip")).read()
    code = re.sub(r"//[^\n]*", "", kernel + open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "stream_rows_body.hpp")).read())
    assert "#pragma clang fp contract(off)" in code and "__syncthreads" not in code and "atomic" not in code and "__shared__" not in code
    assert '"hip/stream.hip"' in open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()


def test_the_layers_above_offer_the_streams():
    for name in ("set_streams", "append_streams", "get_streams", "get_stream_state"):
        assert inspect.signature(getattr(api.Batch, name)).parameters["lane"].default == 0


def test_the_array_and_the_helper():
    array = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    for declaration in (r"bool set_stream\(int index, int lane, const oalsfx_sampler\* records, int length\);", r"bool set_stream\(int index, const oalsfx_sampler\* records, int length\);",
                        r"bool queue_sampler\(int index, int lane, const oalsfx_sampler& record\);", r"bool queue_sampler\(int index, const oalsfx_sampler& record\);",
                        r"bool stream_state\(int index, int lane, uint32_t& taken, uint32_t& queued\);", r"bool stream_state\(int index, uint32_t& taken, uint32_t& queued\);"):
        assert re.search(declaration, array), declaration
    assert "oalsfx_host_stream_chunks" in lib.SIGNATURES and re.search(r"\bint oalsfx_host_stream_chunks\(", open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read())
    r = rec(frames=96, step=5096, position=777, format=sref.PCM_F32, channels=2, data=0x1000)
    for length in (1, 20, 32, 95, 96, 500):
        got = api.stream_chunks(r, length)
        want = stref.chunks(r[0], [min(length, 96 - at) for at in range(0, 96, length)])
        assert got.tobytes() == want.tobytes(), length
    for bad, length in ((r, 0), (rec(frames=96, flags=sref.PLAYING | sref.LOOP, loop_end=9), 20), (rec(frames=96, position=20 << 12), 20), (rec(frames=0), 20), (rec(format=3), 20)):
        with pytest.raises(api.BatchError):
            api.stream_chunks(bad, length)


def test_what_is_refused_without_a_device():
    unopened = api.Batch.__new__(api.Batch)
    unopened.n, unopened.channels, unopened._h, unopened._lib = 8, 2, None, None
    good = np.concatenate([rec(), rec(), rec()])
    for call, streams, message in ((unopened.set_streams, [good[:0]], "Stream length out of range."),
                                   (unopened.set_streams, [np.concatenate([good] * 4)[:10]], "Stream length out of range."),
                                   (unopened.append_streams, [np.concatenate([good] * 3)], "Stream length out of range."),
                                   (unopened.set_streams, [np.concatenate([good[:2], rec(flags=8 | sref.PLAYING)])], "Unknown sampler flags."),
                                   (unopened.append_streams, [rec(format=3)], "Unknown sampler format."),
                                   (unopened.set_streams, [np.concatenate([good[:1], rec(position=100 << 12)])], "The sampler's position is past its end."),
                                   (unopened.append_streams, [rec(channels=4)], "The sampler's channel count is neither 1 nor the batch's.")):
        with pytest.raises(api.BatchError, match=re.escape(message)):
            call(streams)
    for call in (unopened.set_streams, unopened.append_streams):
        with pytest.raises(api.BatchError, match="An instance is listed twice as a stream target."):
            call([good, good], instances=[3, 3])
        with pytest.raises(api.BatchError, match="2 instances but 1 streams"):
            call([good], instances=[3, 4])
