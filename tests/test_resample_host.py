"""CPU: the resamplers' kernel itself, compiled for the host (tests/cpp/fir_rows_host.cpp includes oalsfxpp_amd/csrc/hip/resample.hip behind a
small shim and runs the lanes one after the other), against the restatement (tests/resample_ref.py): outputs on their bits, both records
after every call.  The same program renders jobs that name no table through voice.hip's k_voice_rows as well (its `voice` mode).  The program is built with AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler has their runtime,
and is run directly: the assets are heap blocks of exactly their size, so a tap read one element outside an asset ends the run."""
import os
import struct
import subprocess

import numpy as np
import pytest

import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from oalsfxpp_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "fir_rows_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("fir_rows_host") / "fir_rows_host")
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
    pytest.fail("no host compiler builds tests/cpp/fir_rows_host.cpp:\n" + "\n".join(errors))


def run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, calls, offset=0, voice=False):
    """Writes the job, runs the program (voice: through k_voice_rows), returns [(out, records, envelopes)] per call."""
    exe, _ = program
    distinct, asset_of = [], []
    for p in pcm:
        for k, q in enumerate(distinct):
            if q is p:
                break
        else:
            distinct.append(p)
            k = len(distinct) - 1
        asset_of.append(k)
    job, result = str(tmp_path / "job.bin"), str(tmp_path / "result.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("<5i", len(records), channels, len(calls), len(distinct), offset))
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
        f.write(records.tobytes())
        f.write(envelopes.tobytes())
        f.write(np.asarray(resamplers, np.int32).tobytes())
    r = subprocess.run([exe, job, result] + (["voice"] if voice else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        size = len(records) * frames * channels * 4
        out = np.frombuffer(raw, f32, len(records) * frames * channels, at).reshape(len(records), frames, channels)
        at += size
        rec_after = np.frombuffer(raw, sref.DTYPE, len(records), at).copy()
        at += rec_after.nbytes
        env_after = np.frombuffer(raw, vref.DTYPE, len(records), at).copy()
        at += env_after.nbytes
        got.append((out, rec_after, env_after))
    assert at == len(raw)
    return got


def compare(got, records, envelopes, resamplers, tables, pcm, channels, calls, names=None):
    names = names or [f"row {r}" for r in range(len(records))]
    state, env_state = records, envelopes
    outs = []
    for k, frames in enumerate(calls):
        want, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, frames, channels)
        out, rec_after, env_after = got[k]
        bad = [names[r] for r in range(len(names)) if not sref.same_floats(out[r], want[r])[0]]
        assert not bad, f"call {k}: the outputs of {bad[:6]} differ"
        rec_after["data"] = state["data"]               # (the program's own addresses)
        bad = [names[r] for r in range(len(names)) if rec_after[r].tobytes() != state[r].tobytes() or env_after[r].tobytes() != env_state[r].tobytes()]
        assert not bad, f"call {k}: the records of {bad[:6]} differ"
        outs.append(out)
    return np.concatenate(outs, axis=1), state, env_state


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the run below had AddressSanitizer under it."""
    exe, sanitized = program
    print("fir_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("fmt", [sref.PCM_U8, sref.PCM_S16, sref.PCM_F32])
@pytest.mark.parametrize("taps", [4, 8])
def test_the_rows_the_contract_names(program, tmp_path, taps, fmt):
    tables = cases.tables()
    for channels, width in ((1, 1), (2, 1), (2, 2), (8, 8), (6, 1)):
        names, records, resamplers, pcm = cases.named_rows(taps, fmt, width, channels)
        envelopes = np.zeros(len(records), vref.DTYPE)
        where = tmp_path / f"{channels}_{width}"
        where.mkdir()
        got = run(program, where, records, envelopes, resamplers, tables, pcm, channels, cases.CALLS)
        parts, after, _ = compare(got, records, envelopes, resamplers, tables, pcm, channels, cases.CALLS, names)
        whole = run(program, where, records, envelopes, resamplers, tables, pcm, channels, [sum(cases.CALLS)], offset=1)
        one, after_one, _ = compare(whole, records, envelopes, resamplers, tables, pcm, channels, [sum(cases.CALLS)], names)
        assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes()
        row = dict(zip(names, range(len(names))))
        assert not after["flags"][row["a one-shot that ends in mid-call"]] & sref.PLAYING and after["flags"][row["the last H frames of a one-shot"]] & sref.PLAYING
        assert np.abs(parts[row["a looping voice at i == loop_start == 0 reads +0.0f"]]).max() > 0
        if fmt == sref.PCM_F32:
            assert np.isnan(parts[row["NaN and Inf samples under a zero coefficient"]]).any(), "0 * Inf was skipped"
            assert not np.isnan(parts[row["NaN and Inf samples under a zero coefficient"]]).all()
            quiet = parts[row["denormal products"]]
            assert (quiet != 0).any() and np.abs(quiet).max() < np.finfo(f32).tiny


@pytest.mark.parametrize("enveloped", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_200_random_rows(program, tmp_path, channels, enveloped):
    rng = np.random.default_rng(900 + 10 * channels + enveloped)
    records, envelopes, resamplers, pcm, _, _ = cases.random_rows(rng, 200, channels, enveloped)
    tables = cases.tables()
    kinds = [int((resamplers == ref.NONE).sum()), int(np.isin(resamplers, (0, 2, 4, 6)).sum()), int(np.isin(resamplers, (1, 3, 5, 7)).sum())]
    assert min(kinds) >= 60, kinds
    got = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, cases.CALLS, offset=channels % 3)
    parts, after, env_after = compare(got, records, envelopes, resamplers, tables, pcm, channels, cases.CALLS)
    whole = run(program, tmp_path, records, envelopes, resamplers, tables, pcm, channels, [sum(cases.CALLS)])
    one, after_one, env_one = compare(whole, records, envelopes, resamplers, tables, pcm, channels, [sum(cases.CALLS)])
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes()
    assert np.abs(one).max() > 0


# ---- k_voice_rows: the same row body compiled without tables (voice.hip) ----
@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_200_random_enveloped_rows_through_k_voice_rows(program, tmp_path, channels):
    """The enveloped rows of test_200_random_rows with no row naming a table, through launch_voice.  At 8 channels this is the only host
    run of the tile of 4 frames a lane that the body takes without tables (k_fir_rows: 3)."""
    rng = np.random.default_rng(900 + 10 * channels + 1)
    records, envelopes, resamplers, pcm, _, _ = cases.random_rows(rng, 200, channels, True)
    resamplers[:] = ref.NONE
    assert int((envelopes["flags"] & vref.ACTIVE != 0).sum()) >= 60
    got = run(program, tmp_path, records, envelopes, resamplers, {}, pcm, channels, cases.CALLS, offset=channels % 3, voice=True)
    parts, after, env_after = compare(got, records, envelopes, resamplers, {}, pcm, channels, cases.CALLS)
    whole = run(program, tmp_path, records, envelopes, resamplers, {}, pcm, channels, [sum(cases.CALLS)], voice=True)
    one, after_one, env_one = compare(whole, records, envelopes, resamplers, {}, pcm, channels, [sum(cases.CALLS)])
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes()
    assert np.abs(one).max() > 0 and (after_one["step"] != records["step"]).any() and (env_one["sub"] != 0).any()


def test_the_rows_the_envelopes_contract_names_through_k_voice_rows(program, tmp_path):
    """The rows "voice envelopes" names one by one (tests/test_gpu_voice.py: required_rows), in its calls of 256, 256 and 1024 stereo frames
    and in one of 1536, a float off the allocation's alignment."""
    from test_gpu_voice import required_rows
    names, records, envelopes, pcm = required_rows(lambda asset: 0)
    resamplers = np.full(len(records), ref.NONE)
    sizes = [256, 256, 1024]
    got = run(program, tmp_path, records, envelopes, resamplers, {}, pcm, 2, sizes, voice=True)
    parts, after, env_after = compare(got, records, envelopes, resamplers, {}, pcm, 2, sizes, names)
    whole = run(program, tmp_path, records, envelopes, resamplers, {}, pcm, 2, [sum(sizes)], offset=1, voice=True)
    one, after_one, env_one = compare(whole, records, envelopes, resamplers, {}, pcm, 2, [sum(sizes)], names)
    assert sref.same_floats(parts, one)[0] and after.tobytes() == after_one.tobytes() and env_after.tobytes() == env_one.tobytes()
    row = dict(zip(names, range(len(names))))
    assert not parts[row["delay == F"]][:256].view(np.uint32).any() and not after["flags"][row["STOP completes in mid-call"]] & sref.PLAYING
    assert np.isnan(parts[row["NaN and Inf samples under a ramp"]]).any()
