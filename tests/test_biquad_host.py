"""CPU: the voice filters' kernel itself, compiled for the host (tests/cpp/biquad_rows_host.cpp includes oalsfxpp_amd/csrc/hip/biquad.hip
behind the shim of mix_rows_host.cpp), against the restatement (tests/biquad_ref.py): outputs on their bits, the four records of every
voice after every call.  The filter stage exchanges values between lanes, so the kernel is written as per-lane phase functions between
its wavefront syncs and the host build runs each phase over all 64 lanes before the next; the zero fill, the renders and the sums between
two filter stages still run lane by lane, so the run also proves the ownership rule of k_mix_rows.  The program is a stand-alone one
with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler has their runtime, and is run
directly: the assets, the output and the scratch rows are heap blocks of exactly their size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
import polyphony_cases as pcases
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from oalsfxpp_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "biquad_rows_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CALLS = (1, 2, 63, 64, 65, 256, 7)
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("biquad_rows_host") / "biquad_rows_host")
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
    pytest.fail("no host compiler builds tests/cpp/biquad_rows_host.cpp:\n" + "\n".join(errors))


def run(program, tmp_path, records, envelopes, resamplers, filters, tables, pcm, channels, calls, offset=0):
    """Writes the job, runs the program, returns [(out [n][frames][channels], records, envelopes, filters [lanes][n])] per call."""
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
        f.write(struct.pack("<6i", n, lanes, channels, len(calls), len(distinct), offset))
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
        f.write(np.ascontiguousarray(envelopes).tobytes())
        f.write(np.ascontiguousarray(resamplers, np.int32).tobytes())
        f.write(np.ascontiguousarray(filters).tobytes())
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        out = np.frombuffer(raw, f32, n * frames * channels, at).reshape(n, frames, channels)
        at += out.nbytes
        after = []
        for dtype in (sref.DTYPE, vref.DTYPE, bref.DTYPE):
            after.append(np.frombuffer(raw, dtype, lanes * n, at).copy().reshape(lanes, n))
            at += after[-1].nbytes
        got.append((out, *after))
    assert at == len(raw)
    return got


def compare(got, records, envelopes, resamplers, filters, tables, pcm, channels, calls, names=None):
    lanes, n = records.shape
    state, env_state, f_state, outs = records, envelopes, filters, []
    for k, frames in enumerate(calls):
        want, state, env_state, f_state = bref.render(state, env_state, resamplers, f_state, tables, pcm, frames, channels)
        out, rec_after, env_after, f_after = got[k]
        bad = [i for i in range(n) if not sref.same_floats(out[i], want[i])[0]]
        assert not bad, f"call {k} ({frames} frames): the outputs of the instances {bad[:6]} differ" + (f": {[names[v][bad[0]] for v in range(lanes)]}" if names else "")
        rec_after["data"] = state["data"]               # (the program's own addresses)
        bad = [(v, i) for v in range(lanes) for i in range(n)
               if rec_after[v][i].tobytes() != state[v][i].tobytes() or env_after[v][i].tobytes() != env_state[v][i].tobytes() or f_after[v][i].tobytes() != f_state[v][i].tobytes()]
        assert not bad, f"call {k}: the records of the voices (lane, instance) {bad[:6]} differ"
        outs.append(out)
    return np.concatenate(outs, axis=1), state, env_state, f_state


def both_ways(program, tmp_path, records, envelopes, resamplers, filters, tables, pcm, channels, offset, names=None):
    """The calls one after the other and one call of their sum: each against the restatement, and the two against each other."""
    got = run(program, tmp_path, records, envelopes, resamplers, filters, tables, pcm, channels, CALLS, offset=offset)
    parts, after, env_after, f_after = compare(got, records, envelopes, resamplers, filters, tables, pcm, channels, CALLS, names)
    total = sum(CALLS)
    whole = run(program, tmp_path, records, envelopes, resamplers, filters, tables, pcm, channels, [total], offset=offset)
    one, after_one, env_one, f_one = compare(whole, records, envelopes, resamplers, filters, tables, pcm, channels, [total], names)
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes() and f_after.tobytes() == f_one.tobytes()
    return one, after, env_after, f_after


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("biquad_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("offset", [0, 1, 2])
def test_the_voices_the_contract_names(program, tmp_path, offset):
    """polyphony_cases.named_voices under biquad_cases.named_filters: 8 stereo instances of 4 lanes in calls of 1, 2, 63, 64, 65, 256 and
    7 frames, and in one call of their sum; the destination 0, 1 and 2 floats off a 16-byte boundary."""
    names, records, envelopes, resamplers, pcm = pcases.named_voices(2)
    filters = bcases.named_filters(names)
    out, after, _, f_after = both_ways(program, tmp_path, records, envelopes, resamplers, filters, cases.tables(), pcm, 2, offset, names)
    where = {names[k][i]: (k, i) for k in range(pcases.LANES) for i in range(pcases.INSTANCES)}
    alone, _ = bref.filter_one(filters[1][5], np.zeros((sum(CALLS), 2), f32), 2)
    assert sref.same_floats(out[5], alone + f32(0.0))[0] and np.abs(out[5, :300]).min() > 0, bcases.RINGING
    assert not after[where["a one-shot that ends in mid-call"]]["flags"] & sref.PLAYING
    assert f_after[2][6].tobytes() == filters[2][6].tobytes(), "a record that is not ACTIVE is not touched"


@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_200_random_voices_in_four_lanes(program, tmp_path, channels):
    """50 instances of 4 lanes, six voices in ten filtered, random histories in all eight channels."""
    rng = np.random.default_rng(2700 + channels)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 50, 4, channels, True, calls=CALLS, asset_frames=(1, 300))
    filters = bcases.random_filters(rng, 4, 50)
    out, _, _, f_after = both_ways(program, tmp_path, records, envelopes, resamplers, filters, cases.tables(), pcm, channels, channels % 3)
    assert np.abs(out).max() > 0
    assert f_after["x"][:, :, channels:].tobytes() == filters["x"][:, :, channels:].tobytes() and f_after["y"][:, :, channels:].tobytes() == filters["y"][:, :, channels:].tobytes()


def test_one_lane_filtered_and_unfiltered_side_by_side(program, tmp_path):
    """K = 1: a voice's frames are stored, by its render or by its filter, and an idle instance is filled with +0.0f."""
    rng = np.random.default_rng(31)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 10, 1, 2, True, calls=CALLS, asset_frames=(1, 300))
    filters = bcases.random_filters(rng, 1, 10, share=0.5)
    records[0][7], envelopes[0][7], filters["flags"][0, 7] = np.zeros(1, sref.DTYPE)[0], np.zeros(1, vref.DTYPE)[0], 0
    filters["flags"][0, 2] = bref.ACTIVE
    out, _, _, _ = both_ways(program, tmp_path, records, envelopes, resamplers, filters, cases.tables(), pcm, 2, 1)
    assert (out[7].view(np.uint32) == 0).all() and np.abs(out).max() > 0
