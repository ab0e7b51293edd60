"""CPU: the envelope programs' two kernels themselves, compiled for the host (tests/cpp/program_rows_host.cpp includes
oalsfxpp_amd/csrc/hip/program.hip and biquad.hip behind the shim of biquad_rows_host.cpp), against the restatement
(tests/program_ref.py): outputs on their bits, both records, the filter and the queue of every voice after every call.  The lanes of a
wavefront run one after the other, lane 0 last; tests/cpp/program_rows_host.cpp says why that stands in for the device.  The program
is a stand-alone one with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler has their
runtime, and is run directly: the assets, the output, the scratch rows and the queues are heap blocks of exactly their size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import polyphony_cases as pcases
import program_cases as gcases
import program_ref as gref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from oalsfxpp_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "program_rows_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CALLS = gcases.CALLS
f32 = np.float32
# a queue's row as the kernels keep it (oalsfxpp_amd/csrc/hip/program.hpp, EnvProgram)
QUEUE = np.dtype([("head", np.uint32), ("count", np.uint32), ("reserved", np.uint32, (2,)), ("queue", vref.DTYPE, (gref.PROGRAM_MAX - 1,))])
assert QUEUE.itemsize == 1024


def queues(programs):
    rows = np.zeros((len(programs), len(programs[0])), QUEUE)
    for k, lane in enumerate(programs):
        for i, p in enumerate(lane):
            rows[k][i]["count"] = len(p) - 1
            for j, e in enumerate(p[1:]):
                rows[k][i]["queue"][j] = e
    return rows


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("program_rows_host") / "program_rows_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    compilers = ["g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")]
    flags = ["-std=c++17", "-O0", "-g", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
             "-I", os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip"), SOURCE, "-o", exe]
    errors = []
    for sanitize in (SANITIZE, []):
        for cxx in compilers:
            # (the runtimes linked statically, as clang does anyway: the program then runs whatever else the process has loaded)
            static = ["-static-libasan", "-static-libubsan"] if sanitize and cxx == "g++" else []
            try:
                r = subprocess.run([cxx] + sanitize + static + flags, capture_output=True, text=True)
            except OSError as e:
                errors.append(f"{cxx}: {e}")
                continue
            if r.returncode == 0:
                return exe, bool(sanitize)
            errors.append(f"{cxx} {' '.join(sanitize)}: {r.stderr[-400:]}")
    pytest.fail("no host compiler builds tests/cpp/program_rows_host.cpp:\n" + "\n".join(errors))


def run(program, tmp_path, records, programs, resamplers, filters, tables, pcm, channels, calls, offset=0):
    """Writes the job, runs the program, returns [(out [n][frames][channels], records, envelopes, filters, queues [lanes][n])] per call.
    filters None: k_program_rows; else k_program_biquad_rows."""
    exe, _ = program
    lanes, n = records.shape
    distinct, asset_of = [], []
    for p in [p for lane in pcm for p in lane]:
        for k, q in enumerate(distinct):
            if q is p:
                break
        else:
            distinct.append(p)
            k = len(distinct) - 1
        asset_of.append(k)
    job, result = str(tmp_path / "job.bin"), str(tmp_path / "result.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("<7i", n, lanes, channels, len(calls), len(distinct), offset, filters is not None))
        f.write(np.asarray(calls, np.int32).tobytes())
        for t in range(ref.FIR_TABLES):
            coef = tables.get(t)
            if coef is None:
                f.write(struct.pack("<2i", 0, 0))
            else:
                f.write(struct.pack("<2i", *api.fir_shape(coef)))
                f.write(np.ascontiguousarray(coef, f32).tobytes())
        for p in distinct:
            raw = np.ascontiguousarray(p).tobytes()
            f.write(struct.pack("<q", len(raw)))
            f.write(raw)
        f.write(np.asarray(asset_of, np.int32).tobytes())
        f.write(np.ascontiguousarray(records).tobytes())
        f.write(np.ascontiguousarray(gcases.first_segments(programs)).tobytes())
        f.write(np.ascontiguousarray(resamplers, np.int32).tobytes())
        f.write(np.ascontiguousarray(np.zeros((lanes, n), bref.DTYPE) if filters is None else filters).tobytes())
        f.write(queues(programs).tobytes())
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        out = np.frombuffer(raw, f32, n * frames * channels, at).reshape(n, frames, channels)
        at += out.nbytes
        after = []
        for dtype in (sref.DTYPE, vref.DTYPE, bref.DTYPE, QUEUE):
            after.append(np.frombuffer(raw, dtype, lanes * n, at).copy().reshape(lanes, n))
            at += after[-1].nbytes
        got.append((out, *after))
    assert at == len(raw)
    return got


def compare(got, records, programs, resamplers, filters, tables, pcm, channels, calls):
    lanes, n = records.shape
    state, p_state, f_state, outs = records, programs, filters, []
    for k, frames in enumerate(calls):
        want, state, p_state, f_state = gref.render(state, p_state, resamplers, f_state, tables, pcm, frames, channels)
        out, rec_after, env_after, f_after, q_after = got[k]
        bad = [i for i in range(n) if not sref.same_floats(out[i], want[i])[0]]
        assert not bad, f"call {k} ({frames} frames): the outputs of the instances {bad[:6]} differ"
        rec_after["data"] = state["data"]               # (the program's own addresses)
        bad = []
        for v in range(lanes):
            for i in range(n):
                q, p = q_after[v][i], np.asarray(p_state[v][i], vref.DTYPE)
                left = q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])]
                same = rec_after[v][i].tobytes() == state[v][i].tobytes() and env_after[v][i].tobytes() == p[0].tobytes() and left.tobytes() == p[1:].tobytes()
                if filters is not None:
                    same = same and f_after[v][i].tobytes() == f_state[v][i].tobytes()
                if not same:
                    bad.append((v, i))
        assert not bad, f"call {k}: the records or queues of the voices (lane, instance) {bad[:6]} differ"
        outs.append(out)
    return np.concatenate(outs, axis=1), state, p_state


def both_ways(program, tmp_path, records, programs, resamplers, filters, tables, pcm, channels, offset):
    """The calls one after the other and one call of their sum: each against the restatement, and the two against each other."""
    got = run(program, tmp_path, records, programs, resamplers, filters, tables, pcm, channels, CALLS, offset=offset)
    parts, after, p_after = compare(got, records, programs, resamplers, filters, tables, pcm, channels, CALLS)
    total = sum(CALLS)
    whole = run(program, tmp_path, records, programs, resamplers, filters, tables, pcm, channels, [total], offset=offset)
    one, after_one, p_one = compare(whole, records, programs, resamplers, filters, tables, pcm, channels, [total])
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes()
    assert all(np.asarray(a).tobytes() == np.asarray(c).tobytes() for la, lc in zip(p_after, p_one) for a, c in zip(la, lc))
    return one, after, p_after


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernels: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("program_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("offset", [0, 1, 2])
def test_the_voices_the_contract_names(program, tmp_path, offset, filtered):
    """program_cases.named_programs: 8 stereo instances of 4 lanes in calls of 1, 63, 64, 65, 256 and 7 frames, and in one call of their
    sum; the destination 0, 1 and 2 floats off a 16-byte boundary; with and without biquad_cases.named_filters."""
    names, records, programs, resamplers, pcm, which = gcases.named_programs(2)
    filters = bcases.named_filters(names) if filtered else None
    out, after, p_after = both_ways(program, tmp_path, records, programs, resamplers, filters, cases.tables(), pcm, 2, offset)
    k, i = which["STOP in mid-program"]
    assert not after[k][i]["flags"] & sref.PLAYING and len(p_after[k][i]) == 1
    assert all(len(p_after[k][i]) == 1 for k, i in (which["eight segments used up in one call"], which["two zero-length segments in a row"]))
    assert np.abs(out).max() > 0


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_random_programs_in_four_lanes(program, tmp_path, channels, filtered):
    """20 instances of 4 lanes, half of the voices with a random program of 2 .. 8 segments."""
    rng = np.random.default_rng(3300 + channels)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 20, 4, channels, True, calls=CALLS, asset_frames=(1, 300))
    programs = gcases.random_programs(rng, envelopes, channels)
    filters = bcases.random_filters(rng, 4, 20) if filtered else None
    out, _, _ = both_ways(program, tmp_path, records, programs, resamplers, filters, cases.tables(), pcm, channels, channels % 3)
    assert np.abs(out).max() > 0


def test_one_lane_stores_its_spans(program, tmp_path):
    """K = 1: a voice's spans are stored, a -0.0f among them included, and an idle instance is filled with +0.0f."""
    rng = np.random.default_rng(37)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 10, 1, 2, True, calls=CALLS, asset_frames=(1, 300))
    programs = gcases.random_programs(rng, envelopes, 2, share=0.8)
    records[0][7], programs[0][7] = np.zeros(1, sref.DTYPE)[0], [np.zeros(1, vref.DTYPE)[0]]
    out, _, _ = both_ways(program, tmp_path, records, programs, resamplers, None, cases.tables(), pcm, 2, 1)
    assert (out[7].view(np.uint32) == 0).all() and np.abs(out).max() > 0
