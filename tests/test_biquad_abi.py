"""CPU checks of the voice filters: the record's layout on both sides, the header's declarations and the mirror's bindings, every refusal's
text, the host helpers against code already held to the reference and against the cookbook formulas in double precision, and what the
restatement (tests/biquad_ref.py) promises by itself: split invariance, and that another order of evaluation shows in the bits."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import biquad_cases as bcases
import biquad_ref as bref
from oalsfxpp_amd import api, desc, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("oalsfx_batch_set_filters", "oalsfx_batch_get_filters", "oalsfx_batch_set_lane_filters", "oalsfx_batch_get_lane_filters")
HOST = ("oalsfx_host_voice_filter", "oalsfx_host_rcp_q_from_slope", "oalsfx_host_rcp_q_from_bandwidth", "oalsfx_host_voice_filter_check")
# the largest difference between oalsfx_host_voice_filter and the cookbook formulas evaluated in double, relative to the record's largest
# coefficient, over the grid of test_the_six_kinds_against_the_cookbook_in_double (measured with this build's libm)
MEASURED = 7.62e-7


def test_the_record_is_160_bytes_on_both_sides(tmp_path):
    src = r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "oalsfx_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(oalsfx_voice_filter), offsetof(oalsfx_voice_filter, flags), offsetof(oalsfx_voice_filter, reserved0),
               offsetof(oalsfx_voice_filter, b0), offsetof(oalsfx_voice_filter, a2), offsetof(oalsfx_voice_filter, reserved1), offsetof(oalsfx_voice_filter, x),
               offsetof(oalsfx_voice_filter, y), OALSFX_VF_ACTIVE, OALSFX_VF_LOAD);
        return 0;
    }'''
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [160, 0, 4, 8, 24, 28, 32, 96, 1, 2]
    t = api.FILTER_DTYPE
    assert t.itemsize == C.sizeof(desc.VoiceFilter) == 160
    assert [t.fields[k][1] for k in ("flags", "reserved0", "b0", "b1", "b2", "a1", "a2", "reserved1", "x", "y")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 96]
    assert [getattr(desc.VoiceFilter, k).offset for k in ("flags", "b0", "a2", "reserved1", "x", "y")] == [0, 8, 24, 28, 32, 96]
    assert t["x"].shape == t["y"].shape == (8, 2)
    assert (desc.VF_ACTIVE, desc.VF_LOAD) == (bref.ACTIVE, bref.LOAD) == (1, 2)


def test_header_declares_and_the_mirror_binds_the_filter_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES + HOST[:1] + HOST[3:]:
        assert re.search(r"\bint " + name + r"\(", header), name
    for name in HOST[1:3]:
        assert re.search(r"\bfloat " + name + r"\(float ", header), name
    assert header.index("---- voice filters") > header.index("---- polyphony")
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert "long long oalsfx_debug_filter_uploads(" in debug and '"k_biquad_rows"' in debug
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + HOST + ("oalsfx_debug_filter_uploads",):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    for verb in ("set", "get"):
        restype, args = lib.SIGNATURES[f"oalsfx_batch_{verb}_lane_filters"]
        old_restype, old_args = lib.SIGNATURES[f"oalsfx_batch_{verb}_filters"]
        assert restype is old_restype and args == [old_args[0], C.c_int] + old_args[1:] and old_args == lib.SIGNATURES[f"oalsfx_batch_{verb}_envelopes"][1]
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("y_f = ((((b0 * x_f) + (b1 * x_(f-1))) + (b2 * x_(f-2))) - (a1 * y_(f-1))) - (a2 * y_(f-2))", "a stopped voice rings out",
                   "F == 1 shifts them, F == 0 leaves them", "a -0.0f stays negative", "is not read past its flags", "LOAD is consumed by the upload",
                   "keeps the pending histories and LOAD", "\"Unknown voice filter flags.\"", "\"Non-finite voice filter coefficient.\"",
                   "\"Non-finite voice filter history.\"", "also covers a dropped lane with an ACTIVE filter", "_snapshot and _restore neither touch nor carry them"):
        assert phrase in flat, phrase
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "biquad.hip")).read()
    code = re.sub(r"//[^\n]*", "", kernel)
    assert "#pragma clang fp contract(off)" in code and "__syncthreads" not in code and "atomicAdd" not in code and "__builtin_amdgcn_wave_barrier" in code
    assert "filter_recurrence" in code and "filter_recurrence(float* row" not in open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "support_kernels.hip")).read()
    assert '"hip/biquad.hip"' in open(os.path.join(ROOT, "oalsfxpp_amd", "build.py")).read()


def test_the_layers_above_offer_the_filters():
    for verb in ("set", "get"):
        assert inspect.signature(getattr(api.Batch, f"{verb}_filters")).parameters["lane"].default == 0
    assert callable(api.Batch.filter_uploads)
    array = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    for declaration in (r"bool set_voice_filter\(int index, int lane, const oalsfx_voice_filter& filter\);", r"bool get_voice_filter\(int index, int lane, oalsfx_voice_filter& filter\);",
                        r"bool set_voice_filter\(int index, const oalsfx_voice_filter& filter\);", r"bool get_voice_filter\(int index, oalsfx_voice_filter& filter\);"):
        assert re.search(declaration, array), declaration


def test_every_refusal_has_its_text():
    good = bcases.filt(bcases.low_pass(0.1), bref.ACTIVE | bref.LOAD, x=np.ones((8, 2), f32), y=-np.ones((8, 2), f32))
    assert api.voice_filter_check(good) is None and api.voice_filter_check(np.zeros(1, bref.DTYPE)) is None

    def changed(**fields):
        r = good.copy()
        for k, v in fields.items():
            r[k] = v
        return r

    unopened = api.Batch.__new__(api.Batch)
    unopened.n, unopened.channels, unopened._h, unopened._lib = 8, 2, None, None
    cases = [(changed(flags=4), "Unknown voice filter flags."), (changed(flags=0x80000001), "Unknown voice filter flags."),
             (changed(reserved0=1), "The voice filter's reserved fields are not 0."), (changed(reserved1=-0.0), "The voice filter's reserved fields are not 0.")]
    for name in bref.COEFFICIENTS:
        for bad in (np.inf, -np.inf, np.nan):
            cases.append((changed(**{name: bad}), "Non-finite voice filter coefficient."))
    for name in ("x", "y"):
        for c, j, bad in ((0, 0, np.nan), (7, 1, np.inf), (3, 0, -np.inf)):
            h = good[name].copy()
            h[0, c, j] = bad
            cases.append((changed(**{name: h}), "Non-finite voice filter history."))
    for record, message in cases:
        assert api.voice_filter_check(record) == message
        with pytest.raises(api.BatchError, match=re.escape(message)):
            unopened.set_filters(record)
    # (the largest finite and the denormal values are taken)
    assert api.voice_filter_check(changed(b0=3.4e38, a2=1e-45, x=np.full((8, 2), -3.4e38, f32))) is None
    with pytest.raises(api.BatchError, match="listed twice as a voice filter target"):
        unopened.set_filters(np.concatenate([good, good]), instances=[3, 3])


def test_the_helper_refuses_what_it_cannot_design():
    for kind, gain, freq in ((-1, 1, 0.1), (6, 1, 0.1), (0, 0.00001, 0.1), (3, 0, 0.1), (0, np.nan, 0.1), (0, 1, 0.0), (0, 1, 0.5), (0, 1, -0.1), (0, 1, np.nan)):
        r = bcases.filt((9, 9, 9, 9, 9))
        assert not lib.load().oalsfx_host_voice_filter(kind, gain, freq, 1.0, C.c_void_p(r.ctypes.data)), (kind, gain, freq)
        assert r.tobytes() == bcases.filt((9, 9, 9, 9, 9)).tobytes()
    r = api.voice_filter(desc.VF_PEAKING, 2.0, 0.1, 1.0, bcases.filt(flags=bref.ACTIVE, x=np.ones((8, 2), f32)))
    assert r["flags"] == bref.ACTIVE and (r["x"] == 1).all() and (r["y"] == 0).all() and r["reserved1"] == 0, "nothing but the coefficients is written"


@pytest.mark.parametrize("rate", [44100, 48000])
def test_the_shelves_are_the_send_filters_bit_for_bit(rate):
    """oalsfx_host_voice_filter for the high and the low shelf with rcp_q_from_slope(gain, 1) is direct.lp and direct.hp of
    oalsfx_host_derive_source for the same gain_hf / gain_lf (whose corner frequencies are 250 and 5000 Hz, crossed by name as in the
    reference): the helper is tied to code already held to the reference."""
    for gain_hf, gain_lf in ((0.5, 0.25), (0.001, 1.0), (0.9, 0.05), (1.0, 0.7), (0.123, 0.999)):
        sp = lib.derive_source(desc.FMT_STEREO, rate, desc.SendProps(1, gain_hf, gain_lf), [desc.SendProps(1, 1, 1)], [desc.NULL])
        for kind, gain, hz, theirs in ((desc.VF_HIGH_SHELF, gain_hf, 250.0, sp.direct.lp), (desc.VF_LOW_SHELF, gain_lf, 5000.0, sp.direct.hp)):
            gain = f32(gain)
            mine = api.voice_filter(kind, gain, f32(hz) / f32(rate), api.rcp_q_from_slope(gain, 1.0))
            for name in bref.COEFFICIENTS:
                assert f32(mine[name][0]).tobytes() == f32(getattr(theirs, name)).tobytes(), (kind, gain, name)


def cookbook(kind, gain, f, rcp_q):
    """The RBJ cookbook in double: (b0, b1, b2, a1, a2) / a0."""
    w0 = 2 * np.pi * f
    s, c = np.sin(w0), np.cos(w0)
    alpha = s / 2 * rcp_q
    A = gain
    if kind == desc.VF_LOW_PASS:
        b, a = [(1 - c) / 2, 1 - c, (1 - c) / 2], [1 + alpha, -2 * c, 1 - alpha]
    elif kind == desc.VF_HIGH_PASS:
        b, a = [(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + alpha, -2 * c, 1 - alpha]
    elif kind == desc.VF_BAND_PASS:
        b, a = [alpha, 0.0, -alpha], [1 + alpha, -2 * c, 1 - alpha]
    elif kind == desc.VF_PEAKING:
        q = np.sqrt(A)
        b, a = [1 + alpha * q, -2 * c, 1 - alpha * q], [1 + alpha / q, -2 * c, 1 - alpha / q]
    else:
        sg = 2 * np.sqrt(A) * alpha
        if kind == desc.VF_HIGH_SHELF:
            b = [A * ((A + 1) + (A - 1) * c + sg), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - sg)]
            a = [(A + 1) - (A - 1) * c + sg, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - sg]
        else:
            b = [A * ((A + 1) - (A - 1) * c + sg), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - sg)]
            a = [(A + 1) + (A - 1) * c + sg, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - sg]
    return np.array(b + a[1:]) / a[0]


def test_the_six_kinds_against_the_cookbook_in_double():
    """The five coefficients of every kind over a grid of gains, corner frequencies and Qs, against the cookbook formulas evaluated in
    double on the same float32 arguments.  The largest difference, relative to the record's largest coefficient, was measured here at
    7.62e-7 (a few float32 roundings of the formula's terms); four times that is asserted, because libm's sinf and cosf differ from numpy's
    by an ulp from one build to the next."""
    worst = 0.0
    for kind in range(6):
        for gain in (0.05, 0.5, 1.0, 2.0, 8.0):
            for f in (0.001, 0.01, 0.05, 0.2, 0.45):
                for rcp_q in (0.1, 0.7071, 1.4142, 3.0):
                    gain, f, rcp_q = f32(gain), f32(f), f32(rcp_q)
                    got = api.voice_filter(kind, gain, f, rcp_q)
                    want = cookbook(kind, float(gain), float(f), float(rcp_q))
                    mine = np.array([got[name][0] for name in bref.COEFFICIENTS], np.float64)
                    worst = max(worst, float(np.abs(mine - want).max() / np.abs(want).max()))
    print(f"largest relative difference to the cookbook in double: {worst:.3g}")
    assert worst <= 4 * MEASURED
    # the two ways to rcp_q, as the reference writes them (src/oalsfxpp.cpp:842-865)
    for gain, slope in ((0.5, 1.0), (2.0, 0.75), (0.001, 1.0)):
        want = np.sqrt((gain + 1 / gain) * (1 / slope - 1) + 2)
        assert abs(float(api.rcp_q_from_slope(gain, slope)) - want) <= 4e-7 * want
    for f, bandwidth in ((0.01, 1.0), (0.1, 2.0), (0.3, 0.5)):
        w0 = 2 * np.pi * f
        want = 2 * np.sinh(np.log(2) / 2 * bandwidth * w0 / np.sin(w0))
        assert abs(float(api.rcp_q_from_bandwidth(f, bandwidth)) - want) <= 2e-6 * want


def test_any_split_of_a_render_gives_the_same_bits_and_records():
    """1000 random records over 2500 frames in one piece and in pieces of 441, 256, 1, 2 and 1800."""
    rng = np.random.default_rng(2500)
    records = bcases.random_filters(rng, 1, 1000)[0]
    coef = bref.coefficients(records)
    x = rng.uniform(-1, 1, (1000, 2500, 8)).astype(f32)
    x[:, 900:1400] = 0                          # (a silent stretch: the filters ring)
    whole, xh, yh = bref.process(coef, x, records["x"], records["y"])
    parts, at, xs, ys = [], 0, records["x"], records["y"]
    for frames in (441, 256, 1, 2, 1800):
        y, xs, ys = bref.process(coef, x[:, at:at + frames], xs, ys)
        parts.append(y)
        at += frames
    assert at == 2500
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes() and xs.tobytes() == xh.tobytes() and ys.tobytes() == yh.tobytes()
    assert (xh[:, :, 0] == x[:, -1]).all() and (xh[:, :, 1] == x[:, -2]).all() and (yh[:, :, 0] == whole[:, -1]).all() and (yh[:, :, 1] == whole[:, -2]).all()
    # no frames leave the histories, one frame shifts them
    _, x0, y0 = bref.process(coef, x[:, :0], records["x"], records["y"])
    assert x0.tobytes() == records["x"].tobytes() and y0.tobytes() == records["y"].tobytes()
    y1, x1, _ = bref.process(coef, x[:, :1], records["x"], records["y"])
    assert (x1[:, :, 1] == records["x"][:, :, 0]).all() and (x1[:, :, 0] == x[:, 0]).all()
    # ... and filter_one, the form the renders use, touches no channel at or above the channel count
    y, after = bref.filter_one(records[0], x[0, :100, :2], 2)
    assert y.tobytes() == whole[0, :100, :2].tobytes() and after["x"][2:].tobytes() == records[0]["x"][2:].tobytes() and after["y"][2:].tobytes() == records[0]["y"][2:].tobytes()


def test_another_order_shows():
    """4096 frames of random 16-bit samples through low-passes at freq_mult 0.01, 0.05 and 0.2: the share of outputs whose bits differ
    from the stated value for a fused multiply-add chain, for u - ((a1 * y1) + (a2 * y2)), and for the feed-forward sum taken from the
    right.  Every cell is far above 10 %: a kernel that evaluated the filter in another order would not pass a test on the bits."""
    rng = np.random.default_rng(4096)
    x = (rng.integers(-32768, 32768, 4096).astype(f32) / f32(32768.0)).astype(f32)
    print("share of differing outputs   fma   grouped   from the right")
    for freq_mult in (0.01, 0.05, 0.2):
        coef = np.array(bcases.low_pass(freq_mult), f32)
        stated, _, _ = bref.process(coef, x[:, None], np.zeros((1, 2), f32), np.zeros((1, 2), f32))
        shares = [float((bref.process_other(coef, x, how).view(np.uint32) != stated[:, 0].view(np.uint32)).mean()) for how in ("fma", "grouped", "from the right")]
        print(f"freq_mult {freq_mult:<5}              " + "   ".join(f"{100 * s:5.1f} %" for s in shares))
        assert min(shares) > 0.10, (freq_mult, shares)
