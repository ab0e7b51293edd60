"""CPU: the polyphony kernel itself, compiled for the host (tests/cpp/mix_rows_host.cpp includes oalsfxpp_amd/csrc/hip/polyphony.hip behind
the shim of fir_rows_host.cpp and runs the lanes of a wavefront one after the other, each through all of its instance's voices), against
the restatement (tests/polyphony_ref.py): outputs on their bits, the 3 * K records of every instance after every call.  Because the lanes
run one after the other, the run also proves the kernel's ownership rule: were an element of an instance's row written by one lane and
read by another, the sums would be wrong here.  The program is a stand-alone one with its own main, built with AddressSanitizer and
UndefinedBehaviorSanitizer where the host compiler has their runtime, and is run directly: the assets are heap blocks of exactly their
size, so a read one element outside an asset ends the run."""
import os
import struct
import subprocess

import numpy as np
import pytest

import polyphony_cases as pcases
import polyphony_ref as pref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from oalsfxpp_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "mix_rows_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("mix_rows_host") / "mix_rows_host")
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
    pytest.fail("no host compiler builds tests/cpp/mix_rows_host.cpp:\n" + "\n".join(errors))


def run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, calls, offset=0):
    """Writes the job, runs the program, returns [(out [n][frames][channels], records [lanes][n], envelopes [lanes][n])] per call."""
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
                taps, bits = api.fir_shape(coef)
                f.write(struct.pack("<2i", taps, bits))
                f.write(np.ascontiguousarray(coef, f32).tobytes())
        for p in distinct:
            raw = np.ascontiguousarray(p).tobytes()
            f.write(struct.pack("<q", len(raw)))
            f.write(raw)
        f.write(np.asarray(asset_of, np.int32).tobytes())
        f.write(np.ascontiguousarray(records).tobytes())
        f.write(np.ascontiguousarray(envelopes).tobytes())
        f.write(np.ascontiguousarray(resamplers, np.int32).tobytes())
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        out = np.frombuffer(raw, f32, n * frames * channels, at).reshape(n, frames, channels)
        at += out.nbytes
        rec_after = np.frombuffer(raw, sref.DTYPE, lanes * n, at).copy().reshape(lanes, n)
        at += rec_after.nbytes
        env_after = np.frombuffer(raw, vref.DTYPE, lanes * n, at).copy().reshape(lanes, n)
        at += env_after.nbytes
        got.append((out, rec_after, env_after))
    assert at == len(raw)
    return got


def compare(got, records, envelopes, resamplers, tables, pcm, channels, calls, names=None):
    lanes, n = records.shape
    state, env_state, outs = records, envelopes, []
    for k, frames in enumerate(calls):
        want, state, env_state = pref.render(state, env_state, resamplers, tables, pcm, frames, channels)
        out, rec_after, env_after = got[k]
        bad = [i for i in range(n) if not sref.same_floats(out[i], want[i])[0]]
        assert not bad, f"call {k} ({frames} frames): the outputs of the instances {bad[:6]} differ" + (f": {[names[v][bad[0]] for v in range(lanes)]}" if names else "")
        rec_after["data"] = state["data"]               # (the program's own addresses)
        bad = [(v, i) for v in range(lanes) for i in range(n)
               if rec_after[v][i].tobytes() != state[v][i].tobytes() or env_after[v][i].tobytes() != env_state[v][i].tobytes()]
        assert not bad, f"call {k}: the records of the voices (lane, instance) {bad[:6]} differ"
        outs.append(out)
    return np.concatenate(outs, axis=1), state, env_state


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("mix_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("offset", [0, 1, 2])
def test_the_voices_the_contract_names(program, tmp_path, offset):
    """polyphony_cases.named_voices: 8 stereo instances of 4 lanes in calls of 1, 63, 64, 65, 256 and 7 frames, and in one call of their
    sum; the destination 0, 1 and 2 floats off a 16-byte boundary, so that every store width's kernel runs."""
    names, records, envelopes, resamplers, pcm = pcases.named_voices(2)
    tables = cases.tables()
    got = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, 2, pcases.CALLS, offset=offset)
    parts, after, env_after = compare(got, records, envelopes, resamplers, tables, pcm, 2, pcases.CALLS, names)
    total = sum(pcases.CALLS)
    whole = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, 2, [total], offset=offset)
    one, after_one, env_one = compare(whole, records, envelopes, resamplers, tables, pcm, 2, [total], names)
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes()
    where = {names[k][i]: (k, i) for k in range(pcases.LANES) for i in range(pcases.INSTANCES)}
    assert (parts[5] == 0).all() and not np.signbit(parts[5]).any(), "an instance whose lanes are all idle is +0.0f"
    assert np.abs(parts[3]).max() > 0, "a lone voice in the last lane"
    for name in ("a STOP ramp that ends in mid-call", "a one-shot that ends in mid-call", "a one-shot without a table that ends", "delay 70 and a STOP of 200"):
        assert not after[where[name]]["flags"] & sref.PLAYING, name
    for name in ("a delay longer than the calls", "T = 8, delay 449", "a loop shorter than the taps"):
        assert after[where[name]]["flags"] & sref.PLAYING, name
    assert env_after[where["a delay longer than the calls"]]["delay"] == 1000 - total
    assert after[where["a delay longer than the calls"]]["position"] == records[where["a delay longer than the calls"]]["position"]
    assert env_after[where["an envelope on a voice that does not play"]]["ramp_done"] == 80


@pytest.mark.parametrize("enveloped", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_200_random_voices_in_four_lanes(program, tmp_path, channels, enveloped):
    """50 instances of 4 lanes."""
    rng = np.random.default_rng(1700 + 10 * channels + enveloped)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 50, 4, channels, enveloped, asset_frames=(1, 300))
    tables = cases.tables()
    got = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, pcases.CALLS, offset=channels % 3)
    parts, after, env_after = compare(got, records, envelopes, resamplers, tables, pcm, channels, pcases.CALLS)
    total = sum(pcases.CALLS)
    whole = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, [total])
    one, after_one, env_one = compare(whole, records, envelopes, resamplers, tables, pcm, channels, [total])
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes()
    assert np.abs(one).max() > 0
