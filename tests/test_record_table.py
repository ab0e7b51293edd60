"""The record table on the CPU: oalsfxpp_amd/csrc/hip/record_table.hpp -- the host's bookkeeping for samplers, envelopes and resamplers: which
rows were set since they last went to the device, how large the staging buffer is, what a read-back may overwrite -- has no HIP types in
it, so a stand-alone program (tests/record_table_check.cpp, its own main) drives it against a naive model over a few thousand random
sequences of set, drain and scatter, render and merge.  Built with AddressSanitizer and UndefinedBehaviorSanitizer where a host compiler
has their runtime (the staging arrays are heap blocks of exactly the size the header's rule gives), plain otherwise, and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "record_table_check.cpp")
INC = os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SIZES, TYPES = 6, 2   # tables of 1, 2, 63, 64, 65 and 200 rows; an int and an 80-byte struct


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("record_table") / "record_table_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    errors = []
    for sanitize in (SANITIZE, []):
        for cxx in ("g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")):
            # g++ links libasan and libubsan as shared libraries unless told otherwise, and such a program refuses to start ("ASan runtime
            # does not come first in initial library list") wherever the environment preloads any other library.  Linked statically, which
            # is clang's default, the same checks are compiled into the program and it starts everywhere (tests/test_resample_host.py
            # builds its program the same way).
            static = ["-static-libasan", "-static-libubsan"] if sanitize and cxx == "g++" else []
            try:
                r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", INC] + sanitize + static + [SRC, "-o", exe],
                                   capture_output=True, text=True)
            except OSError as e:
                errors.append(f"{cxx}: {e}")
                continue
            if r.returncode == 0:
                return exe, bool(sanitize)
            errors.append(f"{cxx} {' '.join(sanitize)}: {r.stderr[-400:]}")
    pytest.fail("no host compiler builds tests/record_table_check.cpp:\n" + "\n".join(errors))


def test_the_table_follows_the_model(program):
    """No row listed twice and as many as were set; a capacity between that count and the table's size; after the scatter the device holds
    what was set; after a merge unmarked rows are the device's and marked rows the host's; a drain with nothing pending writes nothing
    (the program's checks, each named in its output when it fails)."""
    exe, sanitized = program
    sequences = 300
    r = subprocess.run([exe, str(sequences)], capture_output=True, text=True, timeout=300)
    print(("address and undefined-behaviour sanitizer build: " if sanitized else "plain build: ") + r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == sequences * SIZES * TYPES, r.stdout
    # every operation happened: drains, among them drains with nothing pending, and merges
    assert int(words[2]) > int(words[3]) > 0 and int(words[4]) > 0, r.stdout


def test_the_header_has_no_hip_in_it():
    """A host-only program can drive the table: the header includes nothing of HIP and compiles with the host compiler alone (the program
    above is the proof)."""
    with open(os.path.join(INC, "record_table.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "hipStream" not in text
