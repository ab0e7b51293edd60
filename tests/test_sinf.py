"""The two restatements of the reference's libm sinf -- the oracle's (oracle/ref_sinf.h) and the device's (glibc_sinf, csrc/hip/common.hpp)
-- and the device's lround (lround_away).

CPU: ref_sinf.h against the bits recorded from the build container's libm (tests/golden/sinf_bits.npz), and against the local libm on
every argument the process path can form, where the local libm is that libm.
GPU: the device copies themselves, through oalsfx_debug_sinf, on every float of that domain against ref_sinf.h compiled on the host,
bit for bit.  Through the effects they show only behind a truncation (`static_cast<int>(sin * depth)` in the chorus), a rounding
(the reverb's modulated tap) or an addition (`* 0.5F + 0.5F` in the ring modulator), which hide a wrong last bit almost everywhere.

The domain: the ring modulator forms [-pi, pi), the chorus and the flanger [0, 2 pi], the reverb [0, 2 pi).  Covered: every float in
[2^-13, 8) and in (-4, -2^-13], +-0, a sample of |y| < 2^-13 (the branch that returns y) and the recorded arguments."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HELPER = r"""
#include "ref_sinf.h"
#include <math.h>
#include <stddef.h>
float one(float x) { return oracle_sinf(x); }
float libm_one(float x) { return sinf(x); }
void sweep(const float* in, float* out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = oracle_sinf(in[i]); }
void sweep_lround(const float* in, int32_t* out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = (int32_t)lroundf(in[i]); }
/* floats whose bit patterns are first .. last: how many does ref_sinf.h give other bits than the local libm, and the first such */
unsigned long long differ_from_libm(uint32_t first, uint32_t last, uint32_t* where)
{
    unsigned long long bad = 0;
    for (uint64_t b = first; b <= last; ++b) {
        const uint32_t u = (uint32_t)b;
        float x, mine, theirs;
        uint32_t m, t;
        memcpy(&x, &u, 4);
        mine = oracle_sinf(x); theirs = sinf(x);
        memcpy(&m, &mine, 4); memcpy(&t, &theirs, 4);
        if (m != t && bad++ == 0) *where = u;
    }
    return bad;
}
"""

# bit patterns, both ends included
POSITIVE = (0x39000000, 0x40FFFFFF)   # [2^-13, 8): 134 217 728 floats
NEGATIVE = (0xB9000000, 0xC07FFFFF)   # (-4, -2^-13]
TINY = 0x39000000                     # |y| below 2^-13
CHUNK = 1 << 24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """ref_sinf.h, the local libm's sinf and lroundf, compiled on the host."""
    d = tmp_path_factory.mktemp("sinf")
    c, so = str(d / "s.c"), str(d / "s.so")
    with open(c, "w") as f:
        f.write(HELPER)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-builtin-sinf", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"), c, "-o", so, "-lm"], check=True)
    lib = C.CDLL(so)
    lib.one.restype = lib.libm_one.restype = C.c_float
    lib.one.argtypes = lib.libm_one.argtypes = [C.c_float]
    lib.sweep.argtypes = lib.sweep_lround.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.differ_from_libm.restype = C.c_ulonglong
    lib.differ_from_libm.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return lib


def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "sinf_bits.npz"))


def test_restated_sinf_matches_recorded_libm_bits(host):
    g = gold()
    got = np.array([host.one(float(a)) for a in g["args"]], dtype=np.float32).view(np.uint32)
    assert np.array_equal(got, g["bits"])


def _slices(first, last, parts):
    edges = np.linspace(first, last + 1, parts + 1).astype(np.uint64)
    return [(int(a), int(b) - 1) for a, b in zip(edges[:-1], edges[1:]) if b > a]


@pytest.mark.parametrize("span", [POSITIVE, NEGATIVE], ids=["positive", "negative"])
def test_restated_sinf_matches_the_local_libm_on_the_whole_domain(host, span):
    """Asserted only where the local libm is the one the reference's results were recorded with (it reproduces sinf_bits.npz)."""
    g = gold()
    local = np.array([host.libm_one(float(a)) for a in g["args"]], dtype=np.float32).view(np.uint32)
    if not np.array_equal(local, g["bits"]):
        import platform
        pytest.skip(f"the local libm ({' '.join(platform.libc_ver())}) gives other bits than the recorded one on {int((local != g['bits']).sum())} "
                    f"of {local.size} recorded arguments")

    def part(s):
        where = C.c_uint32(0)
        return host.differ_from_libm(s[0], s[1], C.byref(where)), where.value

    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:   # (plain C calls: ctypes drops the interpreter lock)
        results = list(pool.map(part, _slices(span[0], span[1], 32)))
    bad = sum(r[0] for r in results)
    first = next((f"{r[1]:#010x}" for r in results if r[0]), None)
    assert bad == 0, f"ref_sinf.h differs from the local libm on {bad} floats, the first {first}"


# ---- the device copies ----
def _device(mode, args):
    from oalsfxpp_amd import lib
    args = np.ascontiguousarray(args, dtype=np.float32)
    out = np.empty(args.size, dtype=np.int32 if mode else np.float32)
    assert lib.load().oalsfx_debug_sinf(0, mode, args.ctypes.data, out.ctypes.data, args.size) == 1
    return out


def _host(fn, args, dtype, pool):
    args = np.ascontiguousarray(args, dtype=np.float32)
    out = np.empty(args.size, dtype=dtype)
    cuts = np.linspace(0, args.size, 17).astype(np.int64)

    def part(k):
        a, b = int(cuts[k]), int(cuts[k + 1])
        if b > a:
            fn(args.ctypes.data + 4 * a, out.ctypes.data + 4 * a, b - a)

    list(pool.map(part, range(16)))
    return out


def _sweep(host, mode, spans):
    """Every float of the spans of bit patterns, CHUNK at a time: the device against the host."""
    total = 0
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        for first, last in spans:
            for lo in range(first, last + 1, CHUNK):
                n = min(CHUNK, last + 1 - lo)
                args = np.arange(lo, lo + n, dtype=np.uint32).view(np.float32)
                got = _device(mode, args).view(np.uint32)
                want = _host(host.sweep_lround if mode else host.sweep, args, np.int32 if mode else np.float32, pool).view(np.uint32)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (f"{'lround_away' if mode else 'glibc_sinf'}: {bad.size} of the {n} floats from {lo:#010x} differ, the first "
                                       f"{lo + int(bad[0]):#010x}: device {int(got[bad[0]]):#010x}, host {int(want[bad[0]]):#010x}")
                total += n
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("span", [POSITIVE, NEGATIVE], ids=["positive", "negative"])
def test_device_sinf_on_the_whole_domain(host, span):
    assert _sweep(host, 0, [span]) == span[1] - span[0] + 1


@pytest.mark.gpu
def test_device_sinf_small_and_recorded_arguments(host):
    """+-0, a million of |y| < 2^-13 in either sign (returned as they are) with the ends of that range, and the recorded arguments
    (which reach +-100: the quadrant reduction far outside the process path's range) against the recorded bits."""
    rng = np.random.default_rng(20261021)
    bits = rng.integers(0, TINY, size=1 << 20, dtype=np.uint32)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000), np.array([0, 0x80000000, 1, 0x80000001, TINY - 1, (TINY - 1) | 0x80000000], dtype=np.uint32)])
    got = _device(0, bits.view(np.float32)).view(np.uint32)
    assert np.array_equal(got, bits), "glibc_sinf changes an argument below 2^-13"
    with ThreadPoolExecutor(max_workers=4) as pool:
        assert np.array_equal(got, _host(host.sweep, bits.view(np.float32), np.float32, pool).view(np.uint32))
    g = gold()
    got = _device(0, g["args"]).view(np.uint32)
    assert np.array_equal(got, g["bits"]), f"{int((got != g['bits']).sum())} of the recorded arguments differ"


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [0, 0x80000000], ids=["positive", "negative"])
def test_device_lround_where_the_reverb_uses_it(host, sign):
    """Every float with 0.25 <= |x| < 4096 (the modulated tap is a depth of at most a few hundred samples times a sine) against lroundf."""
    span = (0x3E800000 | sign, 0x457FFFFF | sign)
    assert _sweep(host, 1, [span]) == 0x07000000


@pytest.mark.gpu
def test_device_lround_on_the_rest_of_the_integers(host):
    """A million floats drawn from the rest of |x| < 2^24: below a quarter (zeros and denormals included) and from 4096 up."""
    rng = np.random.default_rng(20261022)
    bits = np.concatenate([rng.integers(0, 0x3E800000, size=1 << 19, dtype=np.uint32), rng.integers(0x45800000, 0x4B800000, size=1 << 19, dtype=np.uint32),
                           np.array([0, 0x3E7FFFFF, 0x3EFFFFFF, 0x3F000000, 0x45800000, 0x4B7FFFFF], dtype=np.uint32)])
    bits = bits | (rng.integers(0, 2, size=bits.size, dtype=np.uint32) << np.uint32(31))
    args = bits.view(np.float32)
    got = _device(1, args)
    with ThreadPoolExecutor(max_workers=4) as pool:
        want = _host(host.sweep_lround, args, np.int32, pool)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} differ, the first {args[bad[0]]!r}: device {got[bad[0]]}, lroundf {want[bad[0]]}"
