"""CPU: the filter programs' kernels themselves, compiled for the host (tests/cpp/filter_program_rows_host.cpp includes
oalsfxpp_amd/csrc/hip/filter_program.hip behind the shim of biquad_rows_host.cpp), against the restatement
(tests/filter_program_ref.py): outputs on their bits, and all records and both queues of every voice after every call.  The program is
a stand-alone one with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler has their
runtime, their runtimes linked statically, and is run directly: the assets, the output, the scratch rows and every table are heap blocks
of exactly their size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import biquad_ref as bref
import filter_program_cases as fcases
import filter_program_ref as fref
import sampler_ref as sref
import sweep_cases as wcases
import sweep_ref as wref
import voice_ref as vref
from oalsfxpp_amd.api import FILTER_QUEUE_DTYPE
from test_program_host import QUEUE, queues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "filter_program_rows_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
INSTANCES = 5
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("filter_program_rows_host") / "filter_program_rows_host")
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
    pytest.fail("no host compiler builds tests/cpp/filter_program_rows_host.cpp:\n" + "\n".join(errors))


def filter_queues(filter_programs):
    rows = np.zeros((len(filter_programs), len(filter_programs[0])), FILTER_QUEUE_DTYPE)
    for k, lane in enumerate(filter_programs):
        for i, p in enumerate(lane):
            rows[k][i]["count"] = len(p) - 1
            for j, s in enumerate(p[1:]):
                rows[k][i]["queue"][j] = s
    return rows


def run(program, tmp_path, case, calls, programmed, offset=0):
    """Writes the job, runs the program, returns [(out [n][frames][channels], records, envelopes, filters, sweeps, envelope queues,
    filter queues [lanes][n])] per call."""
    exe, _ = program
    lanes, n, channels = case.lanes, case.n, case.channels
    job, result = str(tmp_path / "job.bin"), str(tmp_path / "result.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("<7i", n, lanes, channels, len(calls), len(case.pool), offset, programmed))
        f.write(np.asarray(calls, np.int32).tobytes())
        for _, _, pcm in case.pool:
            raw = np.ascontiguousarray(pcm).tobytes()
            f.write(struct.pack("<q", len(raw)))
            f.write(raw)
        asset_of = np.asarray(case.keys, np.int32)
        asset_of[(case.records["flags"] & sref.PLAYING) == 0] = -1
        f.write(asset_of.tobytes())
        f.write(np.ascontiguousarray(case.records).tobytes())
        f.write(np.ascontiguousarray(wcases.first_segments(case)).tobytes())
        f.write(np.ascontiguousarray(case.resamplers, np.int32).tobytes())
        f.write(np.ascontiguousarray(case.filters).tobytes())
        f.write(np.ascontiguousarray(case.sweeps).tobytes())
        f.write(queues(case.programs).tobytes())
        f.write(filter_queues(case.filter_programs).tobytes())
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        out = np.frombuffer(raw, f32, n * frames * channels, at).reshape(n, frames, channels)
        at += out.nbytes
        after = []
        for dtype in (sref.DTYPE, vref.DTYPE, bref.DTYPE, wref.DTYPE, QUEUE, FILTER_QUEUE_DTYPE):
            after.append(np.frombuffer(raw, dtype, lanes * n, at).copy().reshape(lanes, n))
            at += after[-1].nbytes
        got.append((out, *after))
    assert at == len(raw)
    return got


def compare(got, case, calls):
    lanes, n = case.lanes, case.n
    state, p_state, f_state, fp_state, outs = case.records, case.programs, case.filters, case.filter_programs, []
    for k, frames in enumerate(calls):
        want, state, p_state, f_state, fp_state = fref.render(state, p_state, case.resamplers, f_state, fp_state, {}, case.pcm, frames, case.channels)
        out, rec_after, env_after, f_after, s_after, q_after, fq_after = got[k]
        bad = [i for i in range(n) if not sref.same_floats(out[i], want[i])[0]]
        assert not bad, f"call {k} ({frames} frames): the outputs of the instances {bad[:6]} differ: {[case.what.get((v, bad[0])) for v in range(lanes)]}"
        rec_after["data"] = state["data"]               # (the program's own addresses)
        bad = []
        for v in range(lanes):
            for i in range(n):
                q, p = q_after[v][i], np.asarray(p_state[v][i], vref.DTYPE)
                left = q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])]
                fq, fp = fq_after[v][i], np.asarray(fp_state[v][i], wref.DTYPE)
                f_left = fq["queue"][int(fq["head"]):int(fq["head"]) + int(fq["count"])]
                same = (rec_after[v][i].tobytes() == state[v][i].tobytes() and env_after[v][i].tobytes() == p[0].tobytes() and left.tobytes() == p[1:].tobytes() and
                        f_after[v][i].tobytes() == f_state[v][i].tobytes() and s_after[v][i].tobytes() == fp[0].tobytes() and
                        f_left.tobytes() == fp[1:].tobytes())
                if not same:
                    bad.append((v, i))
        assert not bad, f"call {k}: the records or queues of the voices (lane, instance) {bad[:6]} differ: {case.what.get(bad[0])}"
        outs.append(out)
    return np.concatenate(outs, axis=1), f_state, fp_state


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("filter_program_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("programmed", [False, True])
@pytest.mark.parametrize("channels", sorted(fcases.SHAPES))
def test_five_instances_against_the_restatement(program, tmp_path, channels, programmed):
    """5 instances of 1, 2 or 3 lanes: the 300 frames in one call and split as 1 + 63 + 64 + 65 + 107, each against the restatement and
    the two against each other; the destination 0, 1 or 2 floats off its allocation.  programmed: k_filter_program_env_rows, the
    programmed voices under envelope programs that switch segment inside the renders as well."""
    case = fcases.build(channels, program=programmed, n=INSTANCES)
    offset = channels % 3
    whole, f0, fp0 = compare(run(program, tmp_path, case, (300,), programmed, offset), case, (300,))
    parts, f1, fp1 = compare(run(program, tmp_path, case, fcases.SPLIT, programmed, offset), case, fcases.SPLIT)
    assert sref.same_floats(whole, parts)[0] and f0.tobytes() == f1.tobytes()
    assert all(np.asarray(a, wref.DTYPE).tobytes() == np.asarray(c, wref.DTYPE).tobytes() for la, lc in zip(fp0, fp1) for a, c in zip(la, lc))
    assert np.abs(whole).max() > 0 and len(case.programmed) >= 3
    assert any(len(fp0[k][i]) < len(case.filter_programs[k][i]) for k, i in case.programmed), "no queue was walked"


@pytest.mark.parametrize("frames", [1, 63, 64, 65])
def test_the_short_renders(program, tmp_path, frames):
    case = fcases.build(2, n=INSTANCES)
    compare(run(program, tmp_path, case, (frames, frames), False, 1), case, (frames, frames))
