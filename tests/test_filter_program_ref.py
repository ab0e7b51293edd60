"""CPU: the restatement of the filter programs by itself (tests/filter_program_ref.py) -- a split of a render changes nothing, the
stated form by hand, the refusals -- and the proof that the bit comparison of tests/test_gpu_filter_programs.py and
tests/test_filter_program_host.py discriminates: on the very voices those tests render (tests/filter_program_cases.py), a kernel that
switched a frame late, one that did not reset the index at a switch, and one that chose the segment per 64-frame tile would each differ
from the stated form.

What cannot differ is asserted as well, so that nobody counts it as coverage:
  * a program with no switch inside the frames rendered is one sweep there, under every form;
  * the per-tile form is the stated form wherever every switch falls on a tile boundary of the render ((64, 64) and (128, 172) in a
    render of 300 frames): the tile's first frame is then the segment's first.  It is held to differ only where a switch falls inside a
    tile with LONG frames of the new segment left in that tile."""
import numpy as np
import pytest

import biquad_ref as bref
import filter_program_cases as fcases
import filter_program_ref as fref
import sweep_ref as wref

f32 = np.float32
WRONG = ("late", "index", "tile")
FRAMES = 300


def render_calls(case, sizes):
    state = (case.records, case.programs, case.filters, case.filter_programs)
    outs = []
    for frames in sizes:
        out, r, p, f, fp = fref.render(state[0], state[1], case.resamplers, state[2], state[3], {}, case.pcm, frames, case.channels)
        state = (r, p, f, fp)
        outs.append(out)
    return np.concatenate(outs, axis=1), state


def same_programs(a, b):
    return all(len(x) == len(y) and all(s.tobytes() == t.tobytes() for s, t in zip(x, y)) for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("channels", sorted(fcases.SHAPES))
def test_a_split_of_the_reference_changes_nothing(channels, program):
    case = fcases.build(channels, program=program)
    whole, (r0, p0, f0, fp0) = render_calls(case, (FRAMES,))
    parts, (r1, p1, f1, fp1) = render_calls(case, fcases.SPLIT)
    assert whole.tobytes() == parts.tobytes() and r0.tobytes() == r1.tobytes() and f0.tobytes() == f1.tobytes() and same_programs(fp0, fp1)
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    for v in case.programmed:
        k, i = v
        shape, before, after = case.shape[v], case.filter_programs[k][i], fp0[k][i]
        ends = np.cumsum([length - done for length, done in shape])
        inside = int((ends <= FRAMES).sum())          # segments that complete inside the render
        if inside == len(shape):
            assert len(after) == 1 and not after[0]["flags"] & wref.ACTIVE and after[0]["done"] == after[0]["frames"], case.what[v]
            assert bref.coefficients(f0[k][i]).tobytes() == before[-1]["to"].tobytes()
        else:
            assert len(after) == len(shape) - inside and after[0]["flags"] & wref.ACTIVE, case.what[v]
            assert after[0]["done"] == (shape[inside][1] if inside else shape[0][1]) + FRAMES - (ends[inside - 1] if inside else 0), case.what[v]
            want = before[inside - 1]["to"] if inside else bref.coefficients(case.filters[k][i])
            assert bref.coefficients(f0[k][i]).tobytes() == np.asarray(want, f32).tobytes(), case.what[v]


def test_the_stated_form_by_hand():
    """Two segments of two frames and one, one channel, every operation written out: frame 2 takes the second segment's `from`."""
    a = wref.make((0.5, 0.25, 0.125, -0.3, 0.1), (0.1, 0.7, 0.3, 0.2, -0.05), 2)[0]
    b = wref.make((0.9, -0.2, 0.05, 0.1, 0.3), (0.3, 0.3, 0.3, -0.1, 0.2), 1)[0]
    f = np.zeros(1, bref.DTYPE)[0]
    f["flags"] = bref.ACTIVE
    x = np.asarray([[0.7], [-0.4], [0.9], [0.2]], f32)
    y, f_after, after = fref.filter_one(f, [a, b], x, 1)
    c = [a["from"], (a["from"] + (f32(1) * a["step"]).astype(f32)).astype(f32), b["from"], b["to"]]
    want, x1, x2, y1, y2 = [], f32(0), f32(0), f32(0), f32(0)
    for t in range(4):
        u = f32(f32(f32(c[t][0] * x[t, 0]) + f32(c[t][1] * x1)) + f32(c[t][2] * x2))
        yt = f32(f32(u - f32(c[t][3] * y1)) - f32(c[t][4] * y2))
        want.append(yt)
        x2, x1, y2, y1 = x1, x[t, 0], y1, yt
    assert y[:, 0].tobytes() == np.asarray(want, f32).tobytes()
    assert len(after) == 1 and after[0]["done"] == 1 and after[0]["flags"] == 0 and bref.coefficients(f_after).tobytes() == b["to"].tobytes()
    # three frames: the first segment completes on the render's last frame and is replaced in that render
    _, f3, after3 = fref.filter_one(f, [a, b], x[:2], 1)
    assert len(after3) == 1 and after3[0]["done"] == 0 and after3[0]["flags"] == wref.ACTIVE and bref.coefficients(f3).tobytes() == a["to"].tobytes()


def test_refusals_of_a_program():
    ok = wref.make((1, 0, 0, 0, 0), (0.5, 0.1, 0, -0.2, 0.1), 100)[0]
    idle, started = ok.copy(), ok.copy()
    idle["flags"], started["done"] = 0, 1
    assert fref.check([ok]) is None and fref.check([ok] * 8) is None and fref.check([started, ok]) is None and fref.check([idle]) is None
    assert fref.check([]) == fref.check([ok] * 9) == fref.MESSAGES["length"]
    assert fref.check([ok, idle]) == fref.check([idle, ok]) == fref.MESSAGES["active"]
    assert fref.check([ok, started]) == fref.MESSAGES["started"]
    bad = ok.copy()
    bad["step"] = np.nan
    assert fref.check([ok, bad]) == wref.MESSAGES["finite"]
    assert len(set(fref.MESSAGES.values())) == len(fref.MESSAGES)


def behind(shape, a):
    """The ramp frames of the segment that starts on frame a of the render, inside the render."""
    at = 0
    for j, (length, done) in enumerate(shape[:-1]):
        at += length - done
        if at == a:
            return min(shape[j + 1][0], FRAMES - a)
    raise ValueError(a)


@pytest.mark.parametrize("channels", sorted(fcases.SHAPES))
def test_three_wrong_kernels_would_show(channels):
    case = fcases.build(channels)
    stated = fcases.programmed_voice_outputs(case, (FRAMES,), "stated")
    share = {}
    for how in WRONG:
        wrong = fcases.programmed_voice_outputs(case, (FRAMES,), how)
        share[how] = {v: float((wrong[v].view(np.uint32) != stated[v].view(np.uint32)).mean()) for v in case.programmed}
    held = {how: [] for how in WRONG}
    for v in case.programmed:
        shape = case.shape[v]
        switches = fcases.switches_inside(shape, FRAMES)
        if not switches:
            # the known blind spot: one sweep inside these frames, under every form
            assert all(share[how][v] == 0 for how in WRONG), case.what[v]
            continue
        if any(behind(shape, a) >= fcases.LONG for a in switches):
            for how in ("late", "index"):
                assert share[how][v] > 0, f"{case.what[v]}: a kernel that switched '{how}' would pass"
                held[how].append(share[how][v])
        if all(a % fref.TILE == 0 for a in switches):
            assert share["tile"][v] == 0, case.what[v]          # the second blind spot: every switch on a tile boundary
        elif any(a % fref.TILE != 0 and min(behind(shape, a), fref.TILE - a % fref.TILE) >= fcases.LONG for a in switches):
            assert share["tile"][v] > 0, f"{case.what[v]}: a kernel that chose the segment per tile would pass"
            held["tile"].append(share["tile"][v])
    for how in WRONG:
        print(channels, how, "voices held to differ", len(held[how]), "least share", min(held[how]) if held[how] else None)
    assert len(held["late"]) >= 3 and len(held["tile"]) >= 2
