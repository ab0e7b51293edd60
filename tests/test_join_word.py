"""The join word on the CPU ("calls that join a queued launch"): the protocol of oalsfxpp_amd/csrc/hip/join_word.hpp has no HIP
types in it, so a stand-alone program (tests/join_word_race.cpp, its own main) runs both sides on two host threads -- one appends buffers
as mix_device does, one closes at a random moment as the gate does -- and checks over many rounds that every buffer is counted exactly
once and that the closer copies the entries that were published.  Built with -fsanitize=thread where the toolchain has the runtime (the
release / acquire pairs of the header are then checked too), plain otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "join_word_race.cpp")
INC = os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip")


def _build(tmp_path, flags, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-pthread", "-I", INC] + flags + [SRC, "-o", out], capture_output=True, text=True)
    return out, r


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("join_word")
    out, r = _build(tmp, ["-fsanitize=thread"], "join_word_race_tsan")
    sanitized = r.returncode == 0
    if not sanitized:
        out, r = _build(tmp, [], "join_word_race")
        assert r.returncode == 0, r.stderr
    return out, sanitized


def test_every_buffer_is_counted_exactly_once(program):
    exe, sanitized = program
    rounds = 20000
    r = subprocess.run([exe, str(rounds)], capture_output=True, text=True, timeout=300)
    print(("thread sanitizer build: " if sanitized else "plain build: ") + r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == rounds, r.stdout
    # both outcomes happened: buffers that joined, and buffers the close turned away
    assert int(words[2]) > 0 and int(words[3]) > 0, r.stdout


def test_the_header_has_no_hip_in_it():
    """A host-only program can drive both sides: the header includes nothing of HIP and compiles with the host compiler alone (the
    program above is the proof); what it shares with the kernels is the table's layout, asserted in common.hpp."""
    with open(os.path.join(INC, "join_word.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "hipStream" not in text
