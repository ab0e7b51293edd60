"""CPU: the restatement of the voice filter sweeps by itself (tests/sweep_ref.py) -- a split of a render changes nothing, the refusals
and their texts agree with the library's -- and the proof that the bit comparison of tests/test_gpu_sweeps.py and
tests/test_sweep_host.py discriminates: on the very voices those tests render (tests/sweep_cases.py), a kernel that kept a running sum,
one that fused the product and the sum, and one that held the coefficients over a 64-frame tile would each differ from the stated form
in the output of every swept voice."""
import numpy as np
import pytest

import biquad_ref as bref
import sweep_cases as wcases
import sweep_ref as wref
from oalsfxpp_amd import api

f32 = np.float32
WRONG = ("running", "fma", "tile")


def render_calls(case, sizes):
    state = (case.records, case.programs, case.filters, case.sweeps)
    outs = []
    for frames in sizes:
        out, r, p, f, s = wref.render(state[0], state[1], case.resamplers, state[2], state[3], {}, case.pcm, frames, case.channels)
        state = (r, p, f, s)
        outs.append(out)
    return np.concatenate(outs, axis=1), state


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("channels", sorted(wcases.SHAPES))
def test_a_split_of_the_reference_changes_nothing(channels, program):
    case = wcases.build(channels, program=program)
    whole, (r0, p0, f0, s0) = render_calls(case, (300,))
    parts, (r1, p1, f1, s1) = render_calls(case, wcases.SPLIT)
    assert whole.tobytes() == parts.tobytes() and r0.tobytes() == r1.tobytes() and f0.tobytes() == f1.tobytes() and s0.tobytes() == s1.tobytes()
    assert all(np.asarray(a).tobytes() == np.asarray(c).tobytes() for la, lc in zip(p0, p1) for a, c in zip(la, lc))
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    for k, i in case.swept:
        length, done = int(case.sweeps[k][i]["frames"]), int(case.sweeps[k][i]["done"])
        if done + 300 >= length:
            assert not s0[k][i]["flags"] & wref.ACTIVE and s0[k][i]["done"] == length, case.what[(k, i)]
            assert bref.coefficients(f0[k][i]).tobytes() == case.sweeps[k][i]["to"].tobytes()
        else:
            assert s0[k][i]["flags"] & wref.ACTIVE and s0[k][i]["done"] == done + 300
            assert bref.coefficients(f0[k][i]).tobytes() == bref.coefficients(case.filters[k][i]).tobytes()


def test_the_stated_form_by_hand():
    """Three frames of one channel, every operation written out."""
    s = wref.make((0.5, 0.25, 0.125, -0.3, 0.1), (0.1, 0.7, 0.3, 0.2, -0.05), 2)[0]
    f = np.zeros(1, bref.DTYPE)[0]
    f["flags"] = bref.ACTIVE
    x = np.asarray([[0.7], [-0.4], [0.9]], f32)
    y, f_after, s_after = wref.filter_one(f, s, x, 1)
    c0 = s["from"]
    c1 = (s["from"] + (f32(1) * s["step"]).astype(f32)).astype(f32)
    c2 = s["to"]
    y0 = f32(c0[0] * x[0, 0])
    y1 = f32(f32(f32(c1[0] * x[1, 0]) + f32(c1[1] * x[0, 0])) - f32(c1[3] * y0))
    y2 = f32(f32(f32(f32(f32(c2[0] * x[2, 0]) + f32(c2[1] * x[1, 0])) + f32(c2[2] * x[0, 0])) - f32(c2[3] * y1)) - f32(c2[4] * y0))
    assert y[:, 0].tobytes() == np.asarray([y0, y1, y2], f32).tobytes()
    assert s_after["done"] == 2 and s_after["flags"] == 0 and bref.coefficients(f_after).tobytes() == s["to"].tobytes()


REFUSED = [
    (dict(flags=3), "flags"), (dict(flags=0x80000001), "flags"), (dict(reserved=1), "reserved"), (dict(reserved1=-0.0), "reserved"),
    (dict(frames=0), "frames"), (dict(frames=(1 << 24) + 1), "frames"), (dict(flags=0, frames=(1 << 24) + 1), "frames"), (dict(done=101), "done"),
    (dict(step=np.nan), "finite"), (dict(to=np.inf), "finite"), (dict(**{"from": -np.inf}), "finite"),
]


@pytest.mark.parametrize("fields, why", REFUSED)
def test_refusals_and_their_texts(fields, why):
    s = wref.make((1, 0, 0, 0, 0), (0.5, 0.1, 0, -0.2, 0.1), 100)
    for k, v in fields.items():
        s[k] = v
    assert wref.check(s[0]) == wref.MESSAGES[why] == api.filter_sweep_check(s)


def test_records_that_are_taken():
    for s in (np.zeros(1, wref.DTYPE), wref.make((1, 0, 0, 0, 0), (0, 0, 0, 0, 0), 1 << 24), wref.make((1, 0, 0, 0, 0), (0, 0, 0, 0, 0), 7, done=7)):
        assert wref.check(s[0]) is None and api.filter_sweep_check(s) is None
    assert len(set(wref.MESSAGES.values())) == len(wref.MESSAGES), "every refusal has a message of its own"


def shares(channels, sizes):
    """{how: {(lane, instance): the share of the swept voice's output elements that differ from the stated form}}."""
    case = wcases.build(channels)
    stated = wcases.swept_voice_outputs(case, sizes, "stated")
    out = {}
    for how in WRONG:
        wrong = wcases.swept_voice_outputs(case, sizes, how)
        out[how] = {v: float((wrong[v].view(np.uint32) != stated[v].view(np.uint32)).mean()) for v in case.swept}
    return case, out


@pytest.mark.parametrize("sizes", [(300,), wcases.SPLIT], ids=["300", "split"])
@pytest.mark.parametrize("channels", sorted(wcases.SHAPES))
def test_three_wrong_kernels_would_show(channels, sizes):
    """Every swept voice with sweep_cases.LONG frames of ramp or more inside the 300 frames differs under all three wrong forms.  The
    shorter sweeps (R = 1 and R = 2) cannot differ under a running sum or a fused product: with n in {0, 1, 2}
    the product n * step is exact and the running sum has made at most one addition.  R = 2 still differs under coefficients held per
    tile; R = 1 has one frame of ramp, whose coefficients are `from` under every form (held over a tile they show only where the tile
    goes on behind that frame)."""
    case, share = shares(channels, sizes)
    for how in WRONG:
        print(channels, sizes, how, "least share among the long sweeps", min(share[how][v] for v in case.swept if ramp_left(case, v) >= wcases.LONG),
              "mean", float(np.mean(list(share[how].values()))))
    for v in case.swept:
        left = ramp_left(case, v)
        if left >= wcases.LONG:
            for how in WRONG:
                assert share[how][v] > 0, f"{case.what[v]}: a kernel with '{how}' coefficients would pass"
        elif left == 2:
            assert share["tile"][v] > 0 and share["running"][v] == 0 and share["fma"][v] == 0, case.what[v]
        else:
            assert left == 1 and share["running"][v] == 0 and share["fma"][v] == 0, case.what[v]
            # (`from` held over the frames behind the sweep's one frame, where the stated form has `to`: in one render of 300 the tile
            # goes on for 63 frames behind it; in the split the first render is that one frame alone, and the next tile starts on `to`)
            assert (share["tile"][v] > 0) == (sizes == (300,)), case.what[v]
    assert sum(ramp_left(case, v) >= wcases.LONG for v in case.swept) >= 3


def ramp_left(case, v):
    s = case.sweeps[v[0]][v[1]]
    return min(300, int(s["frames"]) - int(s["done"]))
