"""CPU: the ramp kernel of the bus sends and the table builder, compiled for the host (tests/cpp/bus_sends_host.cpp includes
oalsfxpp_amd/csrc/hip/downmix.hip and bus_sends.hip behind the shim of mix_rows_host.cpp), against the restatement (tests/sends_ref.py),
bit for bit.  The program is a stand-alone one with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer where the
host compiler has their runtime, and is run directly: the source, the buses, the partials and the table's arrays are heap blocks of
exactly their size.  One table serves five calls of 1, 63, 64, 65 and 300 frames, so the ramps are met at every `since`."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sends_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "bus_sends_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CALLS = (1, 63, 64, 65, 300)
INSTANCES, BUSES = 70, 3
RAMP = np.dtype([("from", "<f4"), ("step", "<f4"), ("to", "<f4"), ("frames", "<u4"), ("done", "<u4")])
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("bus_sends_host") / "bus_sends_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    compilers = ["g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")]
    flags = ["-std=c++17", "-O0", "-g", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
             "-I", os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip"), SOURCE, "-o", exe]
    errors = []
    for sanitize in (SANITIZE, []):
        for cxx in compilers:
            static = ["-static-libasan", "-static-libubsan"] if sanitize and cxx == "g++" else []
            try:
                r = subprocess.run([cxx] + sanitize + static + flags, capture_output=True, text=True)
            except OSError as e:
                errors.append(f"{cxx}: {e}")
                continue
            if r.returncode == 0:
                return exe, bool(sanitize)
            errors.append(f"{cxx} {' '.join(sanitize)}: {r.stderr[-400:]}")
    pytest.fail("no host compiler builds tests/cpp/bus_sends_host.cpp:\n" + "\n".join(errors))


def random_sends(rng, n=INSTANCES, buses=BUSES):
    """Send 0 mostly to bus 0 (three chunks with the others' share), sends 1..3 anywhere or nowhere, bus 2 a handful (one short chunk);
    four sends in ten ramp, at every stage from not begun to one frame left."""
    s = sends_ref.Sends(n)
    for send in range(sends_ref.SENDS):
        bus = rng.choice([-1, 0, 1, 2], n, p=[0.1, 0.8, 0.1, 0.0] if send == 0 else [0.45, 0.25, 0.25, 0.05])
        s.set_routing(send, 0, bus, rng.uniform(-1, 1, n).astype(f32))
        for i in np.nonzero(rng.random(n) < 0.4)[0]:
            frames = int(rng.choice([1, 5, 64, 100, 1000]))
            s.set_ramps(send, i, [f32(rng.uniform(-1, 1))], frames)
            s.done[send, i] = rng.integers(0, frames)
    s.set_routing(1, 3, [0], None)  # instance 3 is in bus 0 twice whatever was drawn
    s.set_routing(0, 3, [0], None)
    return s


def run(program, tmp_path, sends, x_calls, channels, max_vector, offset=0):
    """Writes the job from the sends as they stand, runs the program, returns [(vector, buses [BUSES][frames][channels])] per call."""
    exe, _ = program
    rows = np.zeros((sends_ref.SENDS, sends.n), RAMP)
    rows["from"], rows["step"], rows["to"], rows["frames"], rows["done"] = sends.frm, sends.step, sends.to, sends.frames, sends.done
    job, result = str(tmp_path / "job.bin"), str(tmp_path / "result.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("<6i", sends.n, BUSES, channels, len(x_calls), max_vector, offset))
        f.write(np.asarray([x.shape[1] for x in x_calls], np.int32).tobytes())
        f.write(sends.bus.astype(np.int32).tobytes())
        f.write(sends.gain.astype(f32).tobytes())
        f.write(rows.tobytes())
        for x in x_calls:
            f.write(np.ascontiguousarray(x, f32).tobytes())
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw, got, at = open(result, "rb").read(), [], 0
    for x in x_calls:
        (vector,) = struct.unpack_from("<i", raw, at)
        out = np.frombuffer(raw, f32, BUSES * x.shape[1] * channels, at + 4).reshape(BUSES, x.shape[1], channels)
        at += 4 + out.nbytes
        got.append((vector, out))
    assert at == len(raw)
    return got


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("bus_sends_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("max_vector", [1, 2, 4])
@pytest.mark.parametrize("channels", [1, 2, 6, 7, 8])
def test_70_instances_into_3_buses(program, tmp_path, channels, max_vector):
    rng = np.random.default_rng(100 * channels + max_vector)
    sends = random_sends(rng)
    assert len(sends.members(0)) > 64 and 1 <= len(sends.members(2)) <= 32 and (3, 0) in sends.members(0) and (3, 1) in sends.members(0)
    x_calls = [rng.standard_normal((INSTANCES, frames, channels)).astype(f32) for frames in CALLS]
    got = run(program, tmp_path, sends, x_calls, channels, max_vector)
    widths = set()
    for k, x in enumerate(x_calls):
        want = sends.downmix(x, BUSES)
        vector, out = got[k]
        widths.add(vector)
        fits = max(v for v in (1, 2, 4) if (x.shape[1] * channels) % v == 0)
        assert vector == min(max_vector, fits)
        assert sends_ref.same_bits(out, want), f"call {k} ({x.shape[1]} frames, {vector} floats per lane): the buses differ"
    assert max_vector in widths  # (the call of 64 frames takes the widest in every channel count)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_buffers_off_a_16_byte_boundary(program, tmp_path, offset):
    rng = np.random.default_rng(offset)
    sends = random_sends(rng)
    x_calls = [rng.standard_normal((INSTANCES, frames, 2)).astype(f32) for frames in (64, 65)]
    got = run(program, tmp_path, sends, x_calls, 2, 4, offset)
    for k, x in enumerate(x_calls):
        want = sends.downmix(x, BUSES)
        assert got[k][0] == (2 if offset == 2 else 1)
        assert sends_ref.same_bits(got[k][1], want), f"call {k}"


def test_no_send_ramps_and_an_empty_bus(program, tmp_path):
    """Rows of frames == 0 for every member: the plain sum, which downmix_ref states; bus 1 has no member and is +0.0f."""
    import downmix_ref
    rng = np.random.default_rng(9)
    sends = sends_ref.Sends(INSTANCES)
    bus = np.where(np.arange(INSTANCES) % 5 == 0, 2, 0)
    gain = rng.uniform(-1, 1, INSTANCES).astype(f32)
    sends.set_routing(0, 0, bus, gain)
    x = rng.standard_normal((INSTANCES, 65, 2)).astype(f32)
    ((vector, out),) = run(program, tmp_path, sends, [x], 2, 4)
    assert vector == 2 and sends_ref.same_bits(out, downmix_ref.downmix(x, bus, gain, BUSES)) and (out[1].view(np.uint32) == 0).all()
