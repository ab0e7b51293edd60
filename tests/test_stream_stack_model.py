"""CPU: the host model of the whole voice stack as it stands now (tests/stream_stack_model.py), which tests/test_gpu_stream_stack.py
replays on a GPU.  Checked here, without one: the generated sequences hold every named stretch and meet their conditions, and nothing in
them is out of the device's bounds; the real kernel bodies, built for the host as stand-alone programs under AddressSanitizer and
UndefinedBehaviorSanitizer where a host compiler has their runtime and run directly (tests/cpp/stream_rows_host.cpp through
tests/test_stream_host.py, tests/cpp/filter_program_rows_host.cpp through tests/test_filter_program_host.py), leave the renders of a
sequence the way the model says, from the states the sequence reaches, as far as those programs cover the tables in play: the rings'
kernel for the renders without an ACTIVE filter, the filter programs' for the renders without an open ring and without a FIR table."""
import fcntl
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import program_cases as gcases
import resample_ref as ref
import sampler_ref as sref
import stream_ref as stref
import stream_stack_model as ssm
import sweep_ref as wref
import test_filter_program_host as fhost
import test_stream_host as shost
import voice_ref as vref

f32 = np.float32
SHAPE_IDS = dict(argnames="shape", argvalues=ssm.SHAPES, ids=lambda s: f"{s[0]}ch-{s[1]}x{s[2]}")


def built_once(tmp_path_factory, name, source):
    """The stand-alone host program `name`, built as tests/test_stream_host.py builds it -- with the sanitizers by the first of g++ and
    clang++ (ROCm's among them) that has their runtime, else without -- once per test run: parallel workers share the one build, in the
    directory above their own, and wait for it.  Returns (the program, whether it has the sanitizers)."""
    base = tmp_path_factory.getbasetemp()
    where = (base.parent if os.environ.get("PYTEST_XDIST_WORKER") else base) / ("built_" + name)
    where.mkdir(exist_ok=True)
    exe, done = str(where / name), where / "done"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    flags = ["-std=c++17", "-O0", "-g", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(shost.ROOT, "include"),
             "-I", os.path.join(shost.ROOT, "oalsfxpp_amd", "csrc", "hip"), source, "-o", exe]
    with open(where / "lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        errors = []
        for sanitize in (fhost.SANITIZE, []):
            for cxx in ("g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")):
                if done.exists():
                    break
                static = ["-static-libasan", "-static-libubsan"] if sanitize and cxx == "g++" else []
                try:
                    r = subprocess.run([cxx] + sanitize + static + flags, capture_output=True, text=True)
                except OSError as e:
                    errors.append(f"{cxx}: {e}")
                    continue
                if r.returncode == 0:
                    done.write_text("sanitized" if sanitize else "plain")
                else:
                    errors.append(f"{cxx} {' '.join(sanitize)}: {r.stderr[-400:]}")
        if not done.exists():
            pytest.fail(f"no host compiler builds {source}:\n" + "\n".join(errors))
    return exe, done.read_text() == "sanitized"


@pytest.fixture(scope="module")
def stream_rows_host(tmp_path_factory):
    return built_once(tmp_path_factory, "stream_rows_host", shost.SOURCE)


@pytest.fixture(scope="module")
def filter_program_host(tmp_path_factory):
    return built_once(tmp_path_factory, "filter_program_rows_host", fhost.SOURCE)


def test_the_host_programs_are_built_with_the_sanitizers(stream_rows_host, filter_program_host):
    """Not a property of the kernels: says in the test report whether the replays below had AddressSanitizer under them."""
    for exe, sanitized in (stream_rows_host, filter_program_host):
        print(os.path.basename(exe), "built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
        assert os.path.exists(exe)


def script(seed, n, channels, lanes_max, pool_seed=None, **kw):
    pool = ssm.pool_for(seed if pool_seed is None else pool_seed, channels)
    return ssm.build(seed, n, channels, lanes_max, pool, [0x40000000 + 0x1000000 * k for k in range(len(pool))], **kw)


@pytest.fixture(scope="module")
def scripts():
    made = {}

    def get(shape):
        if shape not in made:
            channels, n, lanes_max, seed = shape
            made[shape] = script(seed, n, channels, lanes_max)
        return made[shape]
    return get


@pytest.mark.parametrize(**SHAPE_IDS)
def test_the_generator_holds_its_stretches_and_meets_its_conditions(scripts, shape):
    s = scripts(shape)
    missing = [what for what, there in ssm.present(s.ops).items() if not there]
    unmet = [what for what, met in ssm.conditions(s.ops).items() if not met]
    print(ssm.summary(s.ops))
    assert not missing and not unmet, (missing, unmet, ssm.summary(s.ops))
    assert max(op["lanes"] for op in s.ops) == shape[2] and all(len(op["want"]) == shape[1] for op in s.ops if op["kind"] in ("render", "play"))


@pytest.mark.parametrize(**SHAPE_IDS)
def test_nothing_is_out_of_the_devices_bounds(scripts, shape):
    assert ssm.check_bounds(scripts(shape).ops) > 100


def test_a_lone_voices_negative_zero_is_in_the_mono_sequence(scripts):
    """The store sink of one lane: the reference itself holds a -0.0f somewhere in a render at one lane."""
    s = scripts(ssm.SHAPES[-1])
    assert s.channels == 1 and any(op["lanes"] == 1 and (op["want"].view(np.uint32) == 0x80000000).any() for op in s.ops if op["kind"] == "render")


@pytest.mark.parametrize("seed", [41, 42])
def test_the_short_sequences_hold_their_stretches(seed):
    """The two sequences tests/test_gpu_stream_stack.py interleaves on one stream."""
    s = script(seed, 5, 2, 3, pool_seed=41, only=ssm.SHORT)
    found = ssm.present(s.ops)
    assert 30 <= len(s.ops) <= 90, len(s.ops)
    assert all(found[ssm.STRETCHES[k]] for k in (0, 1, 2, 3, 4, 5, 6, 7, 11, 18)), found
    ssm.check_bounds(s.ops)


@pytest.mark.parametrize(**SHAPE_IDS)
def test_the_rings_kernel_follows_the_model_on_the_host(scripts, stream_rows_host, tmp_path, shape):
    """Every render of every shape's sequence that k_stream_rows runs on the device (no filter is ACTIVE): the model's state in front of it
    handed to the host build of that kernel, one call; outputs on their bits, the current record, the ring, the taken count and the
    envelope program behind it on their bytes.  The unfiltered life of a stream and the ring of 17 entries alone are 10 such renders with
    24 takes in every sequence."""
    program = stream_rows_host
    s = scripts(shape)
    renders = [op for op in s.ops if op["kind"] in ("render", "play") and op["kernel"] == "k_stream_rows"]
    print(shape, len(renders), "renders,", sum(len(t) for op in renders for t in op["takes"].values()), "takes")
    assert len(renders) >= 10 and sum(len(t) for op in renders for t in op["takes"].values()) >= 24
    for k, op in enumerate(renders):
        before, after = op["before"], op["after"]
        got = shost.run(program, tmp_path, before["streams"], before["prog"], before["res"], before["tables"], s.assets, s.channels, [op["frames"]], {},
                        offset=op["offset"], queued=True)[0]
        out, rec_after, env_after, q_after, ring_after, taken_after = got
        assert not ssm.bits_differ(out, op["want"]), f"render {k} ({op['frames']} frames): the outputs differ at {ssm.bits_differ(out, op['want'])}"
        bad = []
        for v in range(before["lanes"]):
            for i in range(s.n):
                q, p, st, ring, t = q_after[v][i], np.asarray(after["prog"][v][i], vref.DTYPE), after["streams"][v][i], ring_after[v][i], int(taken_after[v][i])
                left = q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])]
                waiting = [ring["entry"][(t + j) % stref.QUEUE] for j in range(int(ring["queued"]) - t)]
                same = (shost.nowhere(rec_after[v][i:i + 1]) == shost.nowhere(st[:1]) and env_after[v][i].tobytes() == p[0].tobytes() and
                        left.tobytes() == p[1:].tobytes() and t == int(after["taken"][v][i]) - int(before["taken"][v][i]) and
                        len(waiting) == len(st) - 1 and shost.nowhere(waiting) == shost.nowhere(st[1:]))
                if not same:
                    bad.append((v, i))
        assert not bad, f"render {k}: the records, rings, taken counts or queues of the voices (lane, instance) {bad[:6]} differ"


@pytest.mark.parametrize(**SHAPE_IDS)
def test_the_filter_programs_kernels_follow_the_model_on_the_host(scripts, filter_program_host, tmp_path, shape):
    """Every render of every shape's sequence that a filter program kernel runs on the device while no voice names a FIR table and every
    voice plays a whole asset or nothing: the model's state in front of it handed to the host build of k_filter_program_rows or
    k_filter_program_env_rows, one call; outputs, the records of all four tables and both queues behind it.  The two horizons to the frame
    alone are three such renders of either kernel in every sequence."""
    program = filter_program_host
    s = scripts(shape)
    pool = s.pool
    key_of = {int(a): k for k, a in enumerate(s.addresses)}
    renders = [op for op in s.ops if op["kind"] == "render" and op["kernel"].startswith("k_filter_program") and (op["before"]["res"] == ref.NONE).all() and
               all(len(st) == 1 and (not int(st[0]["flags"]) & sref.PLAYING or int(st[0]["data"]) in key_of) for lane in op["before"]["streams"] for st in lane)]
    print(shape, len(renders), "renders")
    assert len(renders) >= 6 and {op["kernel"] for op in renders} == {"k_filter_program_rows", "k_filter_program_env_rows"}
    assert any(op["filter_switches"] for op in renders)
    for k, op in enumerate(renders):
        before, after = op["before"], op["after"]
        lanes = before["lanes"]
        records = np.array([[st[0] for st in lane] for lane in before["streams"]], sref.DTYPE)
        keys = np.array([[key_of.get(int(r["data"]), 0) for r in lane] for lane in records])
        # (a record over the first frames of an asset reads no further than its own frames: the whole asset stands in)
        case = SimpleNamespace(lanes=lanes, n=s.n, channels=s.channels, pool=pool, keys=keys, records=records, programs=before["prog"], resamplers=before["res"],
                               filters=before["filt"], sweeps=np.array([[p[0] for p in lane] for lane in before["fprog"]], wref.DTYPE), filter_programs=before["fprog"])
        programmed = op["kernel"] == "k_filter_program_env_rows"
        out, rec_after, env_after, f_after, s_after, q_after, fq_after = fhost.run(program, tmp_path, case, (op["frames"],), programmed, op["offset"])[0]
        assert not ssm.bits_differ(out, op["want"]), f"render {k} ({op['frames']} frames, {op['kernel']}): the outputs differ at {ssm.bits_differ(out, op['want'])}"
        want_rec = np.array([[st[0] for st in lane] for lane in after["streams"]], sref.DTYPE)
        rec_after["data"] = want_rec["data"]
        bad = {"records": ssm.records_differ(rec_after, want_rec), "envelopes": ssm.records_differ(env_after, gcases.first_segments(after["prog"])),
               "filters": ssm.records_differ(f_after, after["filt"]), "sweeps": ssm.records_differ(s_after, np.array([[p[0] for p in lane] for lane in after["fprog"]], wref.DTYPE))}
        for v in range(lanes):
            for i in range(s.n):
                fq, fp = fq_after[v][i], np.asarray(after["fprog"][v][i], wref.DTYPE)
                q, p = q_after[v][i], np.asarray(after["prog"][v][i], vref.DTYPE)
                if fq["queue"][int(fq["head"]):int(fq["head"]) + int(fq["count"])].tobytes() != fp[1:].tobytes() or \
                        (programmed and q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])].tobytes() != p[1:].tobytes()):
                    bad.setdefault("queues", []).append((v, i))
        bad = {what: where for what, where in bad.items() if where}
        assert not bad, f"render {k} ({op['kernel']}): {bad}"


def test_the_kernel_names_depend_on_the_hosts_reading(scripts):
    """The predictions are not vacuous: in every sequence renders walk rings that are dry on the device, because the host cannot know,
    and renders leave the rings' kernels while the device's counts have not changed since, because the host has read them."""
    for shape in ssm.SHAPES:
        renders = [op for op in scripts(shape).ops if op["kind"] == "render"]
        assert sum(op["kernel"] in ssm.STREAM_KERNELS and op["device_open"] == 0 for op in renders) >= 2       # (the life of a stream, with a filter and without)
        assert sum(op["kernel"] not in ssm.STREAM_KERNELS and op["before"]["taken"].any() for op in renders) >= 2
