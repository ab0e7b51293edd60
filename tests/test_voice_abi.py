"""CPU checks of the voice envelopes: the C ABI declares and exports them, the record is 144 bytes with the same offsets in C, ctypes and
NumPy, every refusal is one in the library's own check, in the Python mirror and in the restatement, the host helpers compute what the
header states, the NumPy restatement (tests/voice_ref.py) is the samplers' where no envelope is active, holds the split law, stays inside
63 bits at the extremes, agrees with a tile-by-tile model of the kernel's position arithmetic, and orders other than the stated one show
-- no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sampler_ref as sref
import voice_ref as ref
from oalsfxpp_amd import api, desc, lib
from test_sampler_abi import random_records, rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_set_envelopes", "oalsfx_batch_get_envelopes")
HOST_NAMES = ("oalsfx_host_envelope_ramp", "oalsfx_host_envelope_glide", "oalsfx_host_envelope_check")
f32 = np.float32
ONE = sref.ONE
M64 = (1 << 64) - 1


def test_header_declares_and_the_mirror_binds_the_envelope_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES + HOST_NAMES[2:]:
        assert re.search(r"\bint " + name + r"\(", header), name
    for name in HOST_NAMES[:2]:
        assert re.search(r"\bvoid " + name + r"\(", header), name
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert re.search(r"\blong long oalsfx_debug_envelope_uploads\(", debug) and re.search(r"\bconst char\* oalsfx_debug_last_render_kernel\(", debug)
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + HOST_NAMES + ("oalsfx_debug_envelope_uploads", "oalsfx_debug_last_render_kernel"):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("e_c = gain_from[c] + ((float)n * gain_step[c])", "out[f][c] = (v_k * gain[c]) * e_c", "PHI = (position << 16) | sub",
                   "S_g = (step << 16) + g * glide_slope", "m * S_g0 + glide_slope * m * (m - 1) / 2 + (f' - m) * (step_to << 16)",
                   "Any split of F frames into consecutive renders gives the same outputs and the same two final records",
                   "oalsfx_batch_reset, _snapshot and _restore neither touch nor carry envelopes", "a group (oalsfx_group_*) offers no envelopes",
                   "the device clamps nothing"):
        assert phrase in flat, phrase
    for method in ("set_envelopes", "get_envelopes", "envelope_uploads", "last_render_kernel"):
        assert callable(getattr(api.Batch, method))
    array = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool set_envelope\(int index, const oalsfx_envelope& envelope\);", array)
    assert re.search(r"bool get_envelope\(int index, oalsfx_envelope& envelope\);", array)


def test_the_record_is_144_bytes_with_the_same_offsets_everywhere():
    src = r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "oalsfx_hip.h"
    #define O(f) offsetof(oalsfx_envelope, f)
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(oalsfx_envelope), O(flags), O(delay), O(ramp_frames), O(ramp_done),
               O(gain_from), O(gain_step), O(gain_to), O(glide_frames), O(glide_done), O(glide_slope), O(step_to), O(sub), O(reserved),
               _Alignof(oalsfx_envelope));
        printf("%d %d %d %d\n", OALSFX_ENV_ACTIVE, OALSFX_ENV_STOP, OALSFX_ENV_GLIDE, OALSFX_ENV_SUB_BITS);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "e.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "e")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 144 == C.sizeof(desc.Envelope) == api.ENVELOPE_DTYPE.itemsize == ref.DTYPE.itemsize
    assert got[1:14] == ref.OFFSETS and got[14] == 4
    assert [getattr(desc.Envelope, f).offset for f in ref.FIELDS] == ref.OFFSETS
    for dtype in (api.ENVELOPE_DTYPE, ref.DTYPE):
        assert dtype.names == ref.FIELDS and [dtype.fields[f][1] for f in ref.FIELDS] == ref.OFFSETS
    assert api.ENVELOPE_DTYPE == ref.DTYPE
    assert got[15:18] == [desc.ENV_ACTIVE, desc.ENV_STOP, desc.ENV_GLIDE] == [ref.ACTIVE, ref.STOP, ref.GLIDE] == [1, 2, 4]
    assert got[18] == desc.ENV_SUB_BITS == ref.SUB_BITS == 16
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "voice.hip")).read()
    body = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "voice_rows_body.hpp")).read()
    assert "kSub = OALSFX_ENV_SUB_BITS" in body and "#pragma clang fp contract(off)" in kernel


# ---- refusals: the library's check, the Python mirror and the restatement say the same ----
def env(**fields):
    """One envelope: active, no delay, no ramp, gains of 1, unless told otherwise."""
    e = np.zeros(1, ref.DTYPE)
    base = dict(flags=ref.ACTIVE, gain_from=1.0, gain_to=1.0)
    base.update(fields)
    for k, v in base.items():
        e[k] = v
    return e


def library_check(e, step):
    message = C.c_char_p()
    ok = lib.load().oalsfx_host_envelope_check(C.c_void_p(e.ctypes.data), step, C.byref(message))
    return ok, (message.value or b"").decode()


def _unopened(n=8, channels=2):
    """A Batch whose handle was never created: a check that let a call through would fail on the missing library, not with BatchError."""
    b = api.Batch.__new__(api.Batch)
    b.n = n
    b.channels = channels
    b._h = None
    b._lib = None
    return b


GLIDING = ref.ACTIVE | ref.GLIDE
REFUSALS = [
    (dict(flags=8 | ref.ACTIVE), ONE, "Unknown envelope flags", True), (dict(flags=0x80000000), ONE, "Unknown envelope flags", True),
    (dict(reserved=[0, 0, 1]), ONE, "reserved", True), (dict(reserved=[7, 0, 0], flags=0), ONE, "reserved", True),
    (dict(ramp_frames=2 ** 24 + 1), ONE, "ramp is longer", True),
    (dict(ramp_frames=10, ramp_done=11), ONE, "ramp_done", True),
    (dict(sub=65536), ONE, "sub is beyond", True),
    (dict(flags=GLIDING, glide_frames=2 ** 20 + 1), ONE, "glide is longer", True),
    (dict(flags=GLIDING, glide_frames=5, glide_done=6), ONE, "glide_done", True),
    (dict(flags=GLIDING, step_to=2 ** 20), ONE, "step_to", True),
    (dict(flags=ref.GLIDE, step_to=2 ** 20), ONE, "step_to", True),                       # GLIDE is checked whether or not ACTIVE
    (dict(flags=GLIDING, step_to=ONE), 2 ** 20, "gliding sampler's step", False),
    (dict(flags=GLIDING, glide_frames=100, glide_slope=-((ONE << 16) // 100) - 1, step_to=0), ONE, "leaves the range", False),     # S_G < 0
    (dict(flags=GLIDING, glide_frames=2 ** 20, glide_slope=2 ** 16, step_to=ONE), 0, "leaves the range", False)]                 # S_G == 2^36


@pytest.mark.parametrize("fields, step, what, seen_by_mirror", REFUSALS)
def test_set_envelopes_refuses(fields, step, what, seen_by_mirror):
    e = env(**fields)
    ok, message = library_check(e, step)
    assert not ok and what in message, message
    assert ref.check(e[0], step) == what
    if seen_by_mirror:
        with pytest.raises(api.BatchError, match=what):
            _unopened().set_envelopes(e)
        with pytest.raises(api.BatchError, match=what):
            _unopened().set_envelopes(np.concatenate([env(), e, env()]), instances=[5, 1, 2])


def test_what_the_check_takes():
    for fields, step in ((dict(), 2 ** 32 - 1), (dict(ramp_frames=2 ** 24, ramp_done=2 ** 24, sub=65535), 2 ** 32 - 1),      # no glide: any step
                         (dict(flags=GLIDING, glide_frames=2 ** 20, glide_done=2 ** 20, step_to=2 ** 20 - 1), 2 ** 20 - 1),
                         (dict(flags=GLIDING, glide_frames=2 ** 20, glide_slope=2 ** 16 - 1, step_to=ONE), 0),                # S_G = 2^36 - 2^20
                         (dict(flags=GLIDING, glide_frames=100, glide_slope=-((ONE << 16) // 100), step_to=0), ONE),          # S_G = 56
                         (dict(flags=0, step_to=2 ** 31, glide_frames=2 ** 31, glide_done=7), ONE)):                           # idle glide fields
        e = env(**fields)
        ok, message = library_check(e, step)
        assert ok and message == "" and ref.check(e[0], step) is None, (fields, message)
    assert lib.load().oalsfx_host_envelope_check(C.c_void_p(env(sub=65536).ctypes.data), ONE, None) == 0           # no message wanted


def test_set_envelopes_checks_its_instances_and_arrays():
    b = _unopened()
    for instances in ([8], [-1], [0, 9]):
        with pytest.raises(api.BatchError, match="out of bounds"):
            b.set_envelopes(np.concatenate([env()] * len(instances)), instances=instances)
    with pytest.raises(api.BatchError, match="out of bounds"):
        b.set_envelopes(np.concatenate([env()] * 9))
    with pytest.raises(api.BatchError, match="listed twice"):
        b.set_envelopes(np.concatenate([env()] * 3), instances=[1, 2, 1])
    with pytest.raises(api.BatchError, match="3 instances but 2 envelopes"):
        b.set_envelopes(np.concatenate([env()] * 2), instances=[1, 2, 3])
    for bad in (np.zeros(2, api.SAMPLER_DTYPE), np.zeros((1, 2), ref.DTYPE), np.zeros(4, ref.DTYPE)[::2]):
        with pytest.raises(api.BatchError, match="the envelope array"):
            b.set_envelopes(bad, instances=[0, 1])
    with pytest.raises(api.BatchError, match="sequence of desc.Envelope"):
        b.set_envelopes([1.5, 2.5], instances=[0, 1])
    with pytest.raises(api.BatchError, match="out of bounds"):
        b.get_envelopes([8])


# ---- the host helpers ----
def test_the_host_helpers_compute_what_the_header_states():
    so = lib.load()
    rng = np.random.default_rng(3)
    fp = C.POINTER(C.c_float)
    for trial in range(300):
        channels = int(rng.integers(1, 9))
        frames = int((0, 1, 3, 480, 2 ** 24, rng.integers(1, 2 ** 24))[trial % 6])
        a, b = rng.uniform(-2, 2, channels).astype(f32), rng.uniform(-2, 2, channels).astype(f32)
        got = env(flags=ref.ACTIVE | ref.STOP, ramp_done=5, gain_step=9.0, gain_from=7.0, gain_to=7.0, delay=3)
        so.oalsfx_host_envelope_ramp(a.ctypes.data_as(fp), b.ctypes.data_as(fp), channels, frames, C.c_void_p(got.ctypes.data))
        want = env(flags=ref.ACTIVE | ref.STOP, gain_step=9.0, gain_from=7.0, gain_to=7.0, delay=3)
        ref.ramp(want[0], a, b, frames)
        assert got.tobytes() == want.tobytes()
        step = ((b - a) / f32(frames)).astype(f32) if frames else np.zeros(channels, f32)     # one subtraction, one division
        assert sref.same_bits(got["gain_step"][0, :channels], step) and (got["gain_step"][0, channels:] == 9.0).all()
    cases = [(ONE, 2 * ONE, 48000), (2 * ONE, ONE, 48000), (ONE, ONE, 100), (5000, 4000, 7), (4000, 5000, 7), (0, 2 ** 20 - 1, 1), (2 ** 20 - 1, 0, 1),
             (2 ** 20 - 1, 0, 2 ** 20), (0, 2 ** 20 - 1, 2 ** 20), (ONE, 3 * ONE, 0), (1, 0, 3), (0, 1, 3)]
    cases += [tuple(int(x) for x in (rng.integers(0, 2 ** 20), rng.integers(0, 2 ** 20), rng.integers(1, 2 ** 20 + 1))) for _ in range(300)]
    for step, step_to, frames in cases:
        got = env(glide_done=9, delay=3)
        so.oalsfx_host_envelope_glide(step, step_to, frames, C.c_void_p(got.ctypes.data))
        want = env(delay=3)
        ref.glide(want[0], step, step_to, frames)
        assert got.tobytes() == want.tobytes(), (step, step_to, frames)
        slope = int(got["glide_slope"][0])
        if frames:
            exact = (step_to - step) * 65536
            if abs(exact) // frames < 2 ** 31:
                assert abs(slope) * frames <= abs(exact) < (abs(slope) + 1) * frames and slope * exact >= 0      # truncated toward zero
            else:
                assert abs(slope) == 2 ** 31 - 1 and slope * exact > 0                                          # the steepest the record holds
        # ... and what the helper gives is a glide the check takes: it never leaves [step, step_to]
        assert library_check(got, step)[0] and ref.check(got[0], step) is None
    assert int(env(glide_slope=0)["glide_slope"][0]) == 0 and ref.glide_slope(ONE, 2 * ONE, 0) == 0
    assert ref.glide_slope(1, 0, 3) == -(65536 // 3) and ref.glide_slope(0, 1, 3) == 65536 // 3


# ---- values worked out by hand ----
def _mono(values, dtype=f32):
    return np.asarray(values, dtype=dtype).reshape(-1, 1)


def test_delay_ramp_and_stop_by_hand():
    asset = _mono([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    r = rec(format=sref.PCM_F32, frames=8, gain=0.5)
    e = env(flags=ref.ACTIVE | ref.STOP, delay=2, ramp_frames=4, gain_from=1.0, gain_step=-0.25, gain_to=99.0)
    out, after, e_after = ref.render_one(r[0], e[0], asset, 8, 1)
    # two frames of delay, four of the fade (e = 1, 0.75, 0.5, 0.25 on v * gain = 0.5, 1, 2, 4), then the voice has stopped: +0.0f
    assert out[:, 0].tolist() == [0.0, 0.0, 0.5, 0.75, 1.0, 1.0, 0.0, 0.0] and not out[6:].view(np.uint32).any()
    assert after["position"] == 4 * ONE and after["flags"] == 0 and e_after["delay"] == 0 and e_after["ramp_done"] == 4 and e_after["sub"] == 0
    # without STOP the ramp ends on gain_to and the voice goes on
    e = env(delay=2, ramp_frames=4, gain_from=1.0, gain_step=-0.25, gain_to=-1.0)
    out, after, e_after = ref.render_one(r[0], e[0], asset, 8, 1)
    assert out[:, 0].tolist() == [0.0, 0.0, 0.5, 0.75, 1.0, 1.0, -8.0, -16.0]
    assert after["position"] == 6 * ONE and after["flags"] == sref.PLAYING and e_after["ramp_done"] == 4
    # R == 0 with STOP: silent at once, stopped, nothing advanced
    out, after, e_after = ref.render_one(r[0], env(flags=ref.ACTIVE | ref.STOP)[0], asset, 3, 1)
    assert not out.view(np.uint32).any() and after["flags"] == 0 and after["position"] == 0
    # a delay as long as the call: nothing but the delay moves
    out, after, e_after = ref.render_one(r[0], env(delay=3, ramp_frames=4)[0], asset, 3, 1)
    assert not out.view(np.uint32).any() and after.tobytes() == r[0].tobytes() and e_after["delay"] == 0 and e_after["ramp_done"] == 0
    # a negative factor on the frames past a one-shot's end: +0.0f, not -0.0f
    out, after, _ = ref.render_one(rec(format=sref.PCM_F32, frames=8, position=6 * ONE)[0], env(gain_to=-1.0)[0], asset, 4, 1)
    assert out[:, 0].tolist() == [-64.0, -128.0, 0.0, 0.0] and not out[2:].view(np.uint32).any() and after["flags"] == 0
    # a sampler that is not PLAYING: zeros, its record as it is, the counters run
    idle = rec(format=sref.PCM_F32, frames=8, flags=0, position=3 * ONE)
    e = env(flags=GLIDING, delay=1, ramp_frames=10, glide_frames=2, step_to=77, sub=5)
    out, after, e_after = ref.render_one(idle[0], e[0], asset, 4, 1)
    assert not out.view(np.uint32).any() and after["position"] == 3 * ONE and after["step"] == 77 and after["flags"] == 0
    assert (e_after["delay"], e_after["ramp_done"], e_after["glide_done"], e_after["sub"]) == (0, 3, 2, 5)


def test_a_glide_by_hand():
    asset = _mono(np.arange(64.0))
    # from a step of 1 to a step of 2 over four frames: fine steps 1, 1.25, 1.5, 1.75, then 2: positions 0, 1, 2.25, 3.75, 5.5, 7.5, 9.5
    r = rec(format=sref.PCM_F32, frames=64, flags=sref.PLAYING | sref.LINEAR)
    e = env(flags=GLIDING)
    ref.glide(e[0], ONE, 2 * ONE, 4)
    assert e["glide_slope"][0] == (ONE << 16) // 4
    out, after, e_after = ref.render_one(r[0], e[0], asset, 7, 1)
    assert out[:, 0].tolist() == [0.0, 1.0, 2.25, 3.75, 5.5, 7.5, 9.5]
    assert after["position"] == int(11.5 * ONE) and after["step"] == 2 * ONE and e_after["glide_done"] == 4 and e_after["sub"] == 0
    # the 16 bits below the 12: a slope of one fine unit moves the position by one 12-bit unit only after 362 frames (362 * 361 / 2 < 65536 <= 363 * 362 / 2)
    e = env(flags=GLIDING, glide_frames=1000, glide_slope=1, step_to=0)
    out, after, e_after = ref.render_one(rec(format=sref.PCM_F32, frames=64, step=0, flags=sref.PLAYING | sref.LINEAR)[0], e[0], asset, 364, 1)
    assert not out[:363].any() and out[363, 0] == f32(1.0 / ONE)
    assert after["position"] == 1 and e_after["sub"] == 364 * 363 // 2 - 65536 and after["step"] == 0 and e_after["glide_done"] == 364
    # a one-frame loop under a glide holds its frame whatever the step
    r = rec(format=sref.PCM_F32, frames=64, flags=sref.PLAYING | sref.LOOP, loop_start=9, loop_end=10, position=9 * ONE)
    e = env(flags=GLIDING)
    ref.glide(e[0], ONE, 7 * ONE, 50)
    out, after, _ = ref.render_one(r[0], e[0], asset, 80, 1)
    assert (out == 9.0).all() and 9 * ONE <= after["position"] < 10 * ONE and after["step"] == 7 * ONE


# ---- no envelope: the samplers' arithmetic ----
def test_inactive_envelopes_leave_the_samplers_arithmetic():
    rng = np.random.default_rng(11)
    records, assets, _, _ = random_records(rng, 1000, 2)
    records["flags"][::13] &= ~np.uint32(sref.PLAYING)
    envelopes = np.zeros(1000, ref.DTYPE)
    noise = rng.integers(0, 2 ** 32, (1000, ref.DTYPE.itemsize // 4), dtype=np.uint64).astype(np.uint32)
    envelopes[500:] = noise[500:].view(ref.DTYPE).reshape(-1)
    envelopes["flags"] &= ~np.uint32(ref.ACTIVE)           # anything but ACTIVE, in every field
    for frames in (1, 700):
        want, want_after = sref.render(records, assets, frames, 2)
        got, after, env_after = ref.render(records, envelopes, assets, frames, 2)
        assert sref.same_bits(got, want) and after.tobytes() == want_after.tobytes() and env_after.tobytes() == envelopes.tobytes()


# ---- the split law ----
def covered(records, envelopes, after, env_after, calls):
    """What the pairs of a split test must contain, looked up in the records themselves."""
    edges = np.cumsum(calls)
    active = (envelopes["flags"] & ref.ACTIVE) != 0
    stop = active & ((envelopes["flags"] & ref.STOP) != 0)
    gliding = active & ((envelopes["flags"] & ref.GLIDE) != 0)
    playing = (records["flags"] & sref.PLAYING) != 0
    one_shot = playing & ((records["flags"] & sref.LOOP) == 0)
    delay = envelopes["delay"].astype(np.int64)
    ramp_end = delay + envelopes["ramp_frames"].astype(np.int64) - envelopes["ramp_done"].astype(np.int64)
    glide_end = delay + envelopes["glide_frames"].astype(np.int64) - envelopes["glide_done"].astype(np.int64)
    inside = lambda x: (x > 0) & (x < edges[-1]) & ~np.isin(x, edges)
    ended = one_shot & ((after["flags"] & sref.PLAYING) == 0) & (after["position"] == after["frames"].astype(np.uint64) * ONE)
    return {
        "a delay across a call boundary": (active & (delay > edges[0])).any(), "a delay that ends on a boundary": (active & np.isin(delay, edges)).any(),
        "a ramp that ends inside a call": (active & inside(ramp_end)).any(), "a ramp that ends between calls": (active & np.isin(ramp_end, edges[:-1])).any(),
        "a glide that ends inside a call": (gliding & inside(glide_end)).any(), "a glide that ends between calls": (gliding & np.isin(glide_end, edges[:-1])).any(),
        "STOP that completes": (stop & playing & (ramp_end < edges[-1])).any(), "STOP that does not": (stop & (ramp_end > edges[-1])).any(),
        "a one-shot that ends in mid-ramp": (ended & active & ~stop & (env_after["ramp_done"] < env_after["ramp_frames"])).any(),
        "a glide down to a hold": (gliding & (envelopes["step_to"] == 0) & (after["step"] == 0)).any(),
        "rows with no envelope": (~active).any(), "samplers that do not play": (active & ~playing).any(),
        "a sub that is not 0 afterwards": (env_after["sub"] != 0).any()}


def test_any_split_of_a_render_gives_the_same_outputs_and_records():
    rng = np.random.default_rng(21)
    total = sum(ref.CALLS)
    assert ref.CALLS == (441, 256, 1, 1802) and total == 2500
    for channels in (2, 1, 6):
        count = 1000 if channels == 2 else 96
        records, envelopes, assets, _, _ = ref.random_pairs(rng, count, channels)
        whole, after_whole, env_whole = ref.render(records, envelopes, assets, total, channels)
        parts, state, env_state = [], records, envelopes
        for frames in ref.CALLS:
            out, state, env_state = ref.render(state, env_state, assets, frames, channels)
            parts.append(out)
        assert sref.same_bits(np.concatenate(parts, axis=1), whole)
        assert state.tobytes() == after_whole.tobytes() and env_state.tobytes() == env_whole.tobytes()
        if channels == 2:
            missing = [what for what, there in covered(records, envelopes, after_whole, env_whole, ref.CALLS).items() if not there]
            assert not missing, missing
            assert np.abs(whole).max() > 0


# ---- the extremes ----
def running_sum(record, e, frames):
    """PHI of every frame and behind the last by adding one fine step after the other, in Python's integers; the largest sum formed."""
    flags = int(e["flags"])
    env_glide = (int(e["glide_frames"]), int(e["glide_slope"]), int(e["step_to"])) if flags & ref.GLIDE else None
    g = int(e["glide_done"]) if flags & ref.GLIDE else 0
    phi = (int(record["position"]) << 16) | int(e["sub"])
    seen, largest = [], phi
    for _ in range(frames):
        seen.append(ref.wrap_fine(phi, record))
        s = ref.fine_step(int(record["step"]), env_glide, g)
        assert 0 <= s < 2 ** 36 or env_glide is None
        phi += s
        g += 1
        largest = max(largest, phi)
    return seen, ref.wrap_fine(phi, record), largest


@pytest.mark.parametrize("name, record, e, frames", [
    ("the largest steps", dict(frames=2 ** 31 - 1, step=2 ** 20 - 1, position=(2 ** 31 - 1) * ONE - 1),
     dict(flags=GLIDING, glide_frames=3000, step_to=2 ** 20 - 1, sub=65535), 5000),
    ("the fine step at 0", dict(frames=1000, step=ONE), dict(flags=GLIDING, glide_frames=128, glide_slope=-((ONE << 16) // 128), step_to=0), 300),
    ("the fine step just below 2^36", dict(frames=2 ** 31 - 1, step=0, flags=sref.PLAYING | sref.LOOP, loop_start=5, loop_end=2 ** 31 - 1),
     dict(flags=GLIDING, glide_frames=2 ** 20, glide_slope=2 ** 16 - 1, glide_done=2 ** 20 - 2000, step_to=2 ** 20 - 1), 4000),
    ("a one-frame loop under a glide", dict(frames=2 ** 31 - 1, step=2 ** 20 - 1, flags=sref.PLAYING | sref.LOOP | sref.LINEAR, loop_start=2 ** 31 - 2,
                                             loop_end=2 ** 31 - 1, position=(2 ** 31 - 2) * ONE + 4095),
     dict(flags=GLIDING, glide_frames=1500, glide_slope=-(((2 ** 20 - 1) << 16) // 1500), step_to=3, sub=65535), 3000),
    ("no glide, the largest step", dict(frames=2 ** 31 - 1, step=2 ** 32 - 1, flags=sref.PLAYING | sref.LOOP, loop_start=0, loop_end=2 ** 31 - 1,
                                         position=(2 ** 31 - 1) * ONE - 1), dict(sub=65535, ramp_frames=2 ** 24, ramp_done=2 ** 24 - 100), 2000)])
def test_extremes_stay_inside_63_bits(name, record, e, frames):
    r, e = rec(format=sref.PCM_U8, **record), env(**e)
    assert ref.check(e[0], int(r["step"][0])) is None and library_check(e, int(r["step"][0]))[0]
    seen, end, largest = running_sum(r[0], e[0], frames)
    flags = int(e["flags"][0])
    env_glide = (int(e["glide_frames"][0]), int(e["glide_slope"][0]), int(e["step_to"][0])) if flags & ref.GLIDE else None
    g0 = int(e["glide_done"][0]) if flags & ref.GLIDE else 0
    phi0 = (int(r["position"][0]) << 16) | int(e["sub"][0])
    assert largest < 2 ** 63
    # the closed form is the running sum, frame by frame
    assert ref.fine_positions(r[0], env_glide, phi0, g0, frames).tolist() == seen
    assert ref.wrap_fine(phi0 + ref.advance(int(r["step"][0]), env_glide, g0, frames), r[0]) == end
    # ... and the kernel's tile-by-tile way, in 64-bit modular arithmetic, gets there too
    loop, E = bool(int(r["flags"][0]) & sref.LOOP), int(r["frames"][0]) << 28
    for tile in (512, 256):
        got, got_end = kernel_positions(r[0], e[0], frames, tile)
        assert got == [s if loop or s < E else None for s in seen] and got_end == (end if loop else min(end, E))


def test_the_bounds_leave_room_for_a_render_of_2_to_the_24_frames():
    """The largest sums the contract allows, with Python's integers: a glide of 2^20 frames at the largest slope from the last position of
    the longest asset, then 2^24 frames at the largest step; ramp indices up to 2^24 are exact in float32."""
    phi0 = (((2 ** 31 - 1) << 12) - 1) << 16 | 65535
    assert phi0 < 2 ** 59
    worst = phi0 + ref.advance(0, (2 ** 20, 2 ** 16 - 1, 2 ** 20 - 1), 0, 2 ** 24)
    assert worst < phi0 + 2 ** 24 * 2 ** 36 < 2 ** 61
    down = ref.advance(2 ** 20 - 1, (2 ** 20, -(((2 ** 20 - 1) << 16) // 2 ** 20), 0), 0, 2 ** 24)
    assert 0 <= down < 2 ** 56
    # one tile's advance without a glide, at any step: what the kernel adds to a wrapped position
    assert phi0 + 512 * ((2 ** 32 - 1) << 16) < 2 ** 60
    assert int(f32(2 ** 24 - 1)) == 2 ** 24 - 1 and int(f32(2 ** 24)) == 2 ** 24


# ---- the kernel's way to the positions ----
def kernel_positions(record, e, frames, tile):
    """voice_rows_body.hpp's arithmetic for one playing row with an active envelope, in Python integers masked to 64 bits: the tile's base wrapped
    once per tile (a one-shot's held at its end), a frame's offset from it in closed form.  Returns (PHI of every frame as the kernel
    uses it -- None where it is past a one-shot's end --, PHI behind the last frame)."""
    flags, eflags = int(record["flags"]), int(e["flags"])
    loop = bool(flags & sref.LOOP)
    E, L0, L1 = int(record["frames"]) << 28, int(record["loop_start"]) << 28, int(record["loop_end"]) << 28
    step = int(record["step"])
    G, g, slope, step_to = (int(e["glide_frames"]), int(e["glide_done"]), int(e["glide_slope"]), int(e["step_to"])) if eflags & ref.GLIDE else (0, 0, 0, step)
    sigma, sigma_to = step << 16, step_to << 16

    def advance(g, m):
        inside = min(m, G - g)
        sg = (sigma + g * (slope & M64)) & M64
        return (inside * sg + (inside * ((inside - 1) & 0xFFFFFFFF) & 0xFFFFFFFF) // 2 * (slope & M64) + (m - inside) * sigma_to) & M64

    def wrap_past(q):
        r = q - L1
        return L0 + (r % (L1 - L0) if r >= L1 - L0 else r)

    base = (int(record["position"]) << 16) | int(e["sub"])
    if loop and base >= L1:
        base = wrap_past(base)
    seen = []
    for f0 in range(0, frames, tile):
        for t in range(min(tile, frames - f0)):
            q = (base + advance(g, t)) & M64
            if loop and q >= L1:
                q = wrap_past(q)
            seen.append(q if loop or q < E else None)
        m = min(tile, frames - f0)
        base = (base + advance(g, m)) & M64
        g = min(G, g + m)
        if loop:
            if base >= L1:
                base = wrap_past(base)
        elif base > E:
            base = E
    return seen, base


def test_the_kernels_tiles_reach_the_restatements_positions():
    rng = np.random.default_rng(5)
    records, envelopes, _, _, _ = ref.random_pairs(rng, 400, 2, max_step=40 * ONE)
    checked = 0
    for r, e in zip(records, envelopes):
        if not int(e["flags"]) & ref.ACTIVE or not int(r["flags"]) & sref.PLAYING:
            continue
        frames = 1300
        env_glide = (int(e["glide_frames"]), int(e["glide_slope"]), int(e["step_to"])) if int(e["flags"]) & ref.GLIDE else None
        g0 = int(e["glide_done"]) if env_glide else 0
        phi0 = (int(r["position"]) << 16) | int(e["sub"])
        want = ref.fine_positions(r, env_glide, phi0, g0, frames).tolist()
        end = ref.wrap_fine(phi0 + ref.advance(int(r["step"]), env_glide, g0, frames), r)
        loop = bool(int(r["flags"]) & sref.LOOP)
        E = int(r["frames"]) << 28
        for tile in (512, 256):
            got, got_end = kernel_positions(r, e, frames, tile)
            assert got == [w if loop or w < E else None for w in want]
            assert got_end == (end if loop else min(end, E))
        checked += 1
    assert checked > 250


# ---- the order is observable ----
def test_the_order_is_observable():
    """2^20 random inputs: four other ways of computing a frame each differ from the stated one in a share of the outputs that is above
    zero (DESIGN.md 4f has the shares measured), so a kernel that computes another way cannot pass the GPU tests by luck."""
    rng = np.random.default_rng(9)
    count = 1 << 20
    v = rng.standard_normal(count).astype(f32)
    gain = rng.uniform(0.2, 1.0, count).astype(f32)
    R = 4800
    start, target = rng.uniform(0.0, 1.0, count).astype(f32), rng.uniform(0.0, 1.0, count).astype(f32)
    step = ((target - start) / f32(R)).astype(f32)
    n = rng.integers(1, R, count)
    nf = n.astype(f32)
    e = start + (nf * step)
    stated = (v * gain) * e
    fused = (nf.astype(np.float64) * step.astype(np.float64) + start.astype(np.float64)).astype(f32)            # the product exact, rounded once
    # a running sum: the steps added one after the other in float32 (the first 64 frames of every ramp; n drawn anew below that)
    short = rng.integers(1, 64, count)
    running = start.copy()
    for k in range(1, 64):
        running = np.where(short >= k, running + step, running)
    shares = {"fma(n, step, from)": float((((v * gain) * fused).view(np.uint32) != stated.view(np.uint32)).mean()),
              "a running sum of the step": float((((v * gain) * running).view(np.uint32) != ((v * gain) * (start + (short.astype(f32) * step))).view(np.uint32)).mean()),
              "v * (gain * e)": float(((v * (gain * e)).view(np.uint32) != stated.view(np.uint32)).mean())}
    # a glide evaluated at 12-bit positions: the slope rounded to the samplers' fixed point first
    step0, step1 = rng.integers(ONE // 2, 2 * ONE, count), rng.integers(ONE // 2, 2 * ONE, count)
    G = 4800
    slope = np.asarray([ref.glide_slope(int(a), int(b), G) for a, b in zip(step0[:4096], step1[:4096])], dtype=np.int64).repeat(count // 4096)
    step0 = step0[:4096].repeat(count // 4096)
    t = rng.integers(1, G, count).astype(np.int64)
    fine = t * (step0 << 16) + slope * (t * (t - 1) // 2)
    coarse = t * step0 + (slope >> 16) * (t * (t - 1) // 2)
    shares["a glide at 12-bit positions"] = float(((fine >> 16) != coarse).mean())
    print(shares)
    for name, share in shares.items():
        assert share > 0, (name, shares)
    # ... and the restatement computes the stated one
    asset = v[:2000].reshape(-1, 1).copy()
    for k in range(0, 2000, 131):
        r = rec(format=sref.PCM_F32, frames=2000, position=k * ONE, step=0, gain=gain[k])
        en = env(ramp_frames=R, ramp_done=int(n[k]), gain_from=start[k], gain_step=step[k], gain_to=target[k])
        assert np.asarray(ref.render_one(r[0], en[0], asset, 1, 1)[0][0, 0], f32).tobytes() == np.asarray(stated[k], f32).tobytes()
