"""CPU: the sampler streams' render kernel itself, compiled for the host (tests/cpp/stream_rows_host.cpp includes
oalsfxpp_amd/csrc/hip/stream.hip behind the shim of program_rows_host.cpp), against the restatement (tests/stream_ref.py): outputs on
their bits, the current record, the ring, the taken count and the envelope program of every voice after every call, appends between
the calls included.  The lanes of a wavefront run one after the other, lane 0 last; tests/cpp/stream_rows_host.cpp says why that stands
in for the device.  The program is a stand-alone one with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer
where the host compiler has their runtime, and is run directly: every record's PCM -- every chunk by itself --, the output, the
records, the rings, the queues and the taken counts are heap blocks of exactly their size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import stream_cases as scases
import stream_ref as stref
import voice_ref as vref
from oalsfxpp_amd import api
from test_program_host import QUEUE, SANITIZE, queues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "stream_rows_host.cpp")
f32 = np.float32
RING = api.STREAM_RING_DTYPE


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program and whether it was built with the sanitizers: the first of g++ and clang++ (ROCm's among them) that builds it with
    them, else the first that builds it without."""
    exe = str(tmp_path_factory.mktemp("stream_rows_host") / "stream_rows_host")
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
    pytest.fail("no host compiler builds tests/cpp/stream_rows_host.cpp:\n" + "\n".join(errors))


class Blocks:
    """The PCM of every record as a block of its own: a chunk's neighbours in its asset are not behind it."""

    def __init__(self, assets):
        self.assets, self.number, self.raw = assets, {}, []

    def of(self, record):
        if not int(record["flags"]) & sref.PLAYING:
            return -1
        key = stref.asset_key(record)
        if key not in self.number:
            self.number[key] = len(self.raw)
            self.raw.append(np.ascontiguousarray(self.assets[key]).tobytes())
        return self.number[key]


def run(program, tmp_path, streams, programs, resamplers, tables, assets, channels, calls, appends, offset=0, queued=True):
    """Writes the job, runs the program, returns [(out [n][frames][channels], records, envelopes, queues, rings, taken [lanes][n])] per
    call.  appends: {call: [(lane, instance, entries)]}, put in behind that call."""
    exe, _ = program
    lanes, n = len(streams), len(streams[0])
    blocks = Blocks(assets)
    flat = [s for lane in streams for s in lane]
    block_of = [blocks.of(s[0]) for s in flat]
    rings, ring_block = np.zeros(lanes * n, RING), np.full((lanes * n, stref.QUEUE), -1, np.int32)
    for v, s in enumerate(flat):
        rings[v]["queued"] = len(s) - 1
        for j, e in enumerate(s[1:]):
            rings[v]["entry"][j] = e
            ring_block[v][j] = blocks.of(e)
    tail = b""
    for c in range(len(calls)):
        items = appends.get(c, ())
        tail += struct.pack("<i", len(items))
        for k, i, entries in items:
            tail += struct.pack("<2i", k * n + i, len(entries))
            for e in entries:
                tail += struct.pack("<i", blocks.of(e)) + np.asarray(e, sref.DTYPE).tobytes()
    job, result = str(tmp_path / "job.bin"), str(tmp_path / "result.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("<7i", n, lanes, channels, len(calls), len(blocks.raw), offset, queued))
        f.write(np.asarray(calls, np.int32).tobytes())
        for t in range(ref.FIR_TABLES):
            coef = tables.get(t)
            if coef is None:
                f.write(struct.pack("<2i", 0, 0))
            else:
                f.write(struct.pack("<2i", *api.fir_shape(coef)))
                f.write(np.ascontiguousarray(coef, f32).tobytes())
        for raw in blocks.raw:
            f.write(struct.pack("<q", len(raw)))
            f.write(raw)
        f.write(np.asarray(block_of, np.int32).tobytes())
        f.write(np.ascontiguousarray(scases.firsts(streams)).tobytes())
        f.write(np.ascontiguousarray(np.array([[p[0] for p in lane] for lane in programs], dtype=vref.DTYPE)).tobytes())
        f.write(np.ascontiguousarray(resamplers, np.int32).tobytes())
        f.write(queues(programs).tobytes())
        f.write(ring_block.tobytes())
        f.write(rings.tobytes())
        f.write(tail)
    r = subprocess.run([exe, job, result], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stderr + r.stdout)[-3000:]
    raw = open(result, "rb").read()
    got, at = [], 0
    for frames in calls:
        out = np.frombuffer(raw, f32, n * frames * channels, at).reshape(n, frames, channels)
        at += out.nbytes
        after = []
        for dtype in (sref.DTYPE, vref.DTYPE, QUEUE, RING, np.uint32):
            after.append(np.frombuffer(raw, dtype, lanes * n, at).copy().reshape(lanes, n))
            at += after[-1].nbytes
        got.append((out, *after))
    assert at == len(raw)
    return got


def nowhere(records):
    """The records without their addresses, which are the program's own."""
    r = np.array(records, dtype=sref.DTYPE).copy()
    r["data"] = 0
    return r.tobytes()


def compare(got, streams, programs, resamplers, tables, assets, channels, calls, appends):
    lanes, n = len(streams), len(streams[0])
    taken, outs = np.zeros((lanes, n), np.uint32), []
    for c, frames in enumerate(calls):
        want, streams, taken, programs = stref.render(streams, taken, programs, resamplers, tables, assets, frames, channels)
        out, rec_after, env_after, q_after, ring_after, taken_after = got[c]
        bad = [i for i in range(n) if not sref.same_floats(out[i], want[i])[0]]
        assert not bad, f"call {c} ({frames} frames): the outputs of the instances {bad[:6]} differ"
        bad = []
        for v in range(lanes):
            for i in range(n):
                q, p, s, ring, t = q_after[v][i], np.asarray(programs[v][i], vref.DTYPE), streams[v][i], ring_after[v][i], int(taken_after[v][i])
                left = q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])]
                waiting = [ring["entry"][(t + j) % stref.QUEUE] for j in range(int(ring["queued"]) - t)]
                same = (nowhere(rec_after[v][i:i + 1]) == nowhere(s[:1]) and env_after[v][i].tobytes() == p[0].tobytes() and left.tobytes() == p[1:].tobytes() and
                        t == int(taken[v][i]) and len(waiting) == len(s) - 1 and nowhere(waiting) == nowhere(s[1:]))
                if not same:
                    bad.append((v, i))
        assert not bad, f"call {c}: the records, rings, taken counts or queues of the voices (lane, instance) {bad[:6]} differ"
        for k, i, entries in appends.get(c, ()):
            streams[k][i] = stref.append(streams[k][i], entries)
            assert streams[k][i] is not None
        outs.append(out)
    return np.concatenate(outs, axis=1), taken


def test_the_program_is_built_with_the_sanitizers(program):
    """Not a property of the kernel: says in the test report whether the runs below had AddressSanitizer under them."""
    exe, sanitized = program
    print("stream_rows_host built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers: no host compiler here has their runtime")
    assert os.path.exists(exe)


@pytest.mark.parametrize("offset", [0, 1, 2])
def test_the_voices_the_contract_names(program, tmp_path, offset):
    """stream_cases.named_streams: 6 stereo instances of 2 lanes in calls of 1, 63, 64, 65, 256, 7 and 200 frames with the appends behind
    the first and the fifth; the destination 0, 1 and 2 floats off a 16-byte boundary."""
    names, streams, programs, resamplers, pool, appends = scases.named_streams(2)
    bases = scases.fake_bases(pool)
    streams, assets = scases.resolve_streams(streams, pool, bases)
    appends = {c: [(k, i, scases.resolve(e, pool, bases, assets)) for k, i, e in v] for c, v in appends.items()}
    got = run(program, tmp_path, streams, programs, resamplers, cases.tables(), assets, 2, scases.CALLS, appends, offset=offset)
    out, taken = compare(got, streams, programs, resamplers, cases.tables(), assets, 2, scases.CALLS, appends)
    assert taken[0][0] == 7 and taken[0][4] == 9 and taken[0][5] == 3 and np.abs(out).max() > 0


@pytest.mark.parametrize("channels", [1, 2, 4, 6, 7, 8])
def test_random_streams_in_three_lanes(program, tmp_path, channels):
    """12 instances of 3 lanes, most one-shots cut into 2 .. 8 random chunks, loops behind an intro, random envelopes and tables; in four
    calls and in one call of their sum: the same bits, records and counts.  With one channel the kernel gets no queue table."""
    rng = np.random.default_rng(5200 + channels)
    calls = (70, 200, 3, 330)
    streams, programs, resamplers, pool = scases.random_streams(rng, 12, 3, channels, calls)
    streams, assets = scases.resolve_streams(streams, pool, scases.fake_bases(pool))
    args = (streams, programs, resamplers, cases.tables(), assets, channels)
    queued = channels != 1
    parts, taken = compare(run(program, tmp_path, *args, calls, {}, offset=channels % 3, queued=queued), *args, calls, {})
    whole, taken1 = compare(run(program, tmp_path, *args, [sum(calls)], {}, offset=channels % 3, queued=queued), *args, [sum(calls)], {})
    assert sref.same_floats(parts, whole)[0] and (taken == taken1).all() and taken.sum() > 10 and np.abs(parts).max() > 0


def test_one_lane_stores_its_spans(program, tmp_path):
    """K = 1: a voice's spans are stored, and an idle instance is filled with +0.0f."""
    rng = np.random.default_rng(41)
    calls = (70, 200, 3, 330)
    streams, programs, resamplers, pool = scases.random_streams(rng, 10, 1, 2, calls, share=0.9)
    streams[0][7], programs[0][7] = np.zeros(1, sref.DTYPE), [np.zeros(1, vref.DTYPE)[0]]
    streams, assets = scases.resolve_streams(streams, pool, scases.fake_bases(pool))
    args = (streams, programs, resamplers, cases.tables(), assets, 2)
    out, taken = compare(run(program, tmp_path, *args, calls, {}, offset=1), *args, calls, {})
    assert (out[7].view(np.uint32) == 0).all() and np.abs(out).max() > 0 and taken.sum() > 5
