"""CPU: `harness.OracleApi` against the compiled reference on whole call sequences of the Api surface.

The GPU tests trust `OracleApi` to say what the reference's `Api` would have derived after any sequence of setters, applies and
mixes.  These programs pin that model to the reference beyond "set everything, apply once, mix": same-type and cross-type
effect changes, `set_effect_type` to NULL or to the type a slot already has, `set_effect_props` with the union of another type,
direct and auxiliary sends inside and outside [0, 1] (the reference clamps only the direct one), sends set back to exactly
(1, 1, 1), sends written between an apply and the next mix, applies with nothing pending, and every `get_*` read.

What the reference computes is stored in tests/golden/reference_digests.json under `sequence[...]` keys (written by
tests/golden/generate.py): a digest of each mix's output, each `get_*` result, and digests of the final slot parameters,
state and rings and of the source.  Where oracle/_ref/libref.so is built each program also runs on the live reference."""
import hashlib
import random

import pytest

from harness import OracleApi, make_effect, preset_effect
from oalsfxpp_amd import desc
from oalsfxpp_amd.workloads import FIELDS, random_effect
from oracle import oracle as orc
from test_oracle_vs_reference import _leaves, _member, digest_floats, digest_struct, stored

INPUT_SEED = 9
FRAMES = (1, 64, 100, 256, 441, 2049)
MULTI_FORMATS = (desc.FMT_5POINT1, desc.FMT_6POINT1, desc.FMT_7POINT1)


def any_effect(rng, t):
    return random_effect(rng, t) if t in FIELDS else make_effect(t)


def send_value(rng):
    """A send gain: inside [0, 1], above it, negative, or exactly 0 or 1."""
    return rng.choice((lambda: rng.uniform(0.0, 1.0), lambda: rng.uniform(1.0, 2.5), lambda: rng.uniform(-1.0, 0.0),
                       lambda: 0.0, lambda: 1.0))()


def random_program(seed):
    """(fmt, rate, slots, ops) of a seeded program.  Ops: ("effect", slot, Effect), ("type", slot, t), ("props", slot, EffectPropsU),
    ("send", slot, g, ghf, glf), ("apply",), ("get_effect", slot, deferred), ("get_send", slot, deferred), ("mix", frames)."""
    rng = random.Random(7000 + seed)
    fmt = (desc.FMT_STEREO, desc.FMT_MONO, desc.FMT_STEREO, rng.choice(MULTI_FORMATS))[seed % 4]
    rate = rng.choice((44100, 48000))
    slots = rng.randint(1, 4)
    types = [rng.choice((desc.EAX_REVERB, desc.REVERB, rng.randrange(12))) for _ in range(slots)]
    ops = [("effect", s, any_effect(rng, t)) for s, t in enumerate(types)] + [("apply",)]
    for _ in range(rng.randint(14, 22)):
        s = rng.randrange(slots)
        r = rng.random()
        if r < 0.12:     # same type, other properties
            ops.append(("effect", s, any_effect(rng, types[s])))
        elif r < 0.18:   # another type
            types[s] = rng.randrange(12)
            ops.append(("effect", s, any_effect(rng, types[s])))
        elif r < 0.26:   # NULL, the type the slot has, or another one
            t = rng.choice((desc.NULL, types[s], rng.randrange(12)))
            types[s] = t
            ops.append(("type", s, t))
        elif r < 0.34:   # the props union of the slot's type, or of another type than the deferred one
            t = rng.choice((types[s], rng.randrange(1, 12)))
            ops.append(("props", s, any_effect(rng, t).props))
        elif r < 0.50:
            d = rng.choice((-1, -1, s))
            if rng.random() < 0.25:
                ops.append(("send", d, 1.0, 1.0, 1.0))
            else:
                ops.append(("send", d, send_value(rng), send_value(rng), send_value(rng)))
        elif r < 0.60:
            ops.append(("apply",))
            if rng.random() < 0.3:
                ops.append(("apply",))
        elif r < 0.70:
            if rng.random() < 0.5:
                ops.append(("get_effect", s, rng.random() < 0.5))
            else:
                ops.append(("get_send", rng.choice((-1, s)), rng.random() < 0.5))
        elif r < 0.82:
            ops.append(("mix", rng.choice(FRAMES)))
        else:            # a run of buffers long enough for reverbs to settle
            ops += [("mix", 256)] * rng.randint(4, 10)
    ops += [("get_send", -1, False), ("get_send", 0, False), ("get_send", 0, True), ("get_effect", 0, True), ("mix", 256)]
    return fmt, rate, slots, ops


def _aux_to_unity(second_change):
    """The sequence the batch once got wrong: an aux send set to 0.5, applied and mixed; then set back to exactly (1, 1, 1) while
    the slot changes -- the reference re-derives the sends from the active aux props on any slot change (src/oalsfxpp.cpp:3397-3412)."""
    ops = [("effect", 0, make_effect(desc.EAX_REVERB)), ("send", 0, 0.5, 0.5, 0.5), ("apply",)] + [("mix", 256)] * 3
    ops += [("send", 0, 1.0, 1.0, 1.0), ("get_send", 0, False), ("get_send", 0, True)] + second_change + [("apply",)]
    return ops + [("mix", 256)] * 4 + [("get_send", 0, False)]


def directed_programs():
    S, R = desc.FMT_STEREO, 48000
    props = preset_effect(8).props
    return {
        "aux_to_unity_same_type": (S, R, 1, _aux_to_unity([("effect", 0, preset_effect(112))])),
        "aux_to_unity_props": (S, R, 1, _aux_to_unity([("props", 0, props)])),
        "aux_to_unity_type_change": (S, R, 1, _aux_to_unity([("effect", 0, make_effect(desc.REVERB))])),
        # the aux send of slot 0 back to unity while only slot 1 changes
        "aux_to_unity_other_slot": (S, R, 2, [("effect", 1, make_effect(desc.ECHO))] + _aux_to_unity([("effect", 1, make_effect(desc.ECHO, delay=0.05))])),
        # an aux send written after the apply and before the mix that refreshes the slot
        "aux_between_apply_and_mix": (desc.FMT_MONO, 44100, 1, [("effect", 0, make_effect(desc.CHORUS)), ("apply",), ("mix", 256),
                                      ("effect", 0, make_effect(desc.CHORUS, rate=3.0)), ("apply",), ("send", 0, 0.3, 1.0, 0.6),
                                      ("mix", 256), ("mix", 256), ("send", 0, 1.0, 1.0, 1.0), ("apply",), ("apply",), ("mix", 256)]),
    }


SEEDS = range(36)


def all_programs():
    out = {f"sequence[{k}]": v for k, v in directed_programs().items()}
    for s in SEEDS:
        out[f"sequence[random{s}]"] = random_program(s)
    return out


def digest_effect(e):
    """An Effect as get_effect returns it: the type and every member of the props union, field by field (padding ignored)."""
    members = [name for name, *_ in desc.EffectPropsU._fields_ if name != "raw"]
    leaves = [e.type] + [v for m in members for v in _leaves(getattr(e.props, m))]
    return hashlib.sha256(repr(leaves).encode()).hexdigest()[:16]


def send_list(p):
    return [float(p[0]), float(p[1]), float(p[2])] if isinstance(p, tuple) else [p.gain, p.gain_hf, p.gain_lf]


def run_program(api, program):
    """Runs the ops on a `Reference` or an `OracleApi`; returns one record per mix or read."""
    fmt, rate, slots, ops = program
    is_ref = isinstance(api, orc.Reference)
    out, k = [], 0
    for op in ops:
        kind = op[0]
        if kind == "effect":
            api.set_effect(op[1], op[2])
        elif kind == "type":
            api.set_effect_type(op[1], op[2])
        elif kind == "props":
            api.set_effect_props(op[1], op[2])
        elif kind == "send":
            api.set_send_props(*op[1:])
        elif kind == "apply":
            api.apply_changes()
        elif kind == "get_effect":
            e = api.get_effect(op[1], op[2])
            out.append(["effect", digest_effect(e[1] if is_ref else e)])
        elif kind == "get_send":
            p = api.get_send_props(op[1], op[2])
            out.append(["send", send_list(p[1] if is_ref else p)])
        elif kind == "mix":
            ch = desc.FORMAT_CHANNELS[fmt]
            x = orc.synth(INPUT_SEED, k, op[1] * ch).reshape(op[1], ch)
            out.append(["mix", digest_floats(api.mix(x))])
            k += 1
    return out


def reference_sequence_record(program):
    fmt, rate, slots, _ = program
    ref = orc.Reference(fmt, rate, slots)
    rec = {"ops": run_program(ref, program), "slots": []}
    for s in range(slots):
        rp, rs = ref.dump_slot(s)
        rec["slots"].append({"type": rp.type, "params": _member(rp.u, desc.PARAMS_MEMBER, rp.type),
                             "state": _member(rs.u, desc.STATE_MEMBER, rp.type), "ring": digest_floats(ref.dump_rings(s, rp))})
    sp, ss = ref.dump_source()
    rec["source_params"], rec["source_state"] = digest_struct(sp), digest_struct(ss)
    return rec


def test_programs_cover_the_surface():
    """The generated programs use every operation and edge the model has to get right."""
    progs = all_programs()
    ops = [op for _, _, _, p in progs.values() for op in p]
    kinds = {op[0] for op in ops}
    assert kinds == {"effect", "type", "props", "send", "apply", "get_effect", "get_send", "mix"}
    assert {op[1] for op in ops if op[0] == "mix"} == set(FRAMES)
    assert any(op[0] == "type" and op[2] == desc.NULL for op in ops)
    sends = [op for op in ops if op[0] == "send"]
    assert any(op[1] >= 0 and op[2:] == (1.0, 1.0, 1.0) for op in sends) and any(op[1] < 0 and op[2:] == (1.0, 1.0, 1.0) for op in sends)
    assert any(min(op[2:]) < 0 for op in sends if op[1] >= 0) and any(max(op[2:]) > 1 for op in sends if op[1] >= 0)
    assert any(min(op[2:]) < 0 for op in sends if op[1] < 0) and any(max(op[2:]) > 1 for op in sends if op[1] < 0)
    assert any(a[0] == "apply" and b[0] == "apply" for _, _, _, p in progs.values() for a, b in zip(p, p[1:]))
    assert {(op[1] < 0, op[2]) for op in ops if op[0] == "get_send"} == {(True, False), (True, True), (False, False), (False, True)}
    assert {op[2] for op in ops if op[0] == "get_effect"} == {False, True}
    fmts = {p[0] for p in progs.values()}
    assert {desc.FMT_MONO, desc.FMT_STEREO} <= fmts and fmts & set(MULTI_FORMATS)
    assert {p[1] for p in progs.values()} == {44100, 48000} and {p[2] for p in progs.values()} == {1, 2, 3, 4}


@pytest.mark.parametrize("key", list(all_programs()))
def test_call_sequence(key):
    program = all_programs()[key]
    exp = stored(key)
    if orc.have_reference():
        assert reference_sequence_record(program) == exp, f"{key}: the compiled reference no longer gives the stored digests (tests/golden/generate.py)"
    fmt, rate, slots, ops = program
    mine = OracleApi(fmt, rate, slots)
    got = run_program(mine, program)
    assert len(got) == len(exp["ops"]), key
    reads = [op for op in ops if op[0] in ("mix", "get_effect", "get_send")]
    for k, (g, e, op) in enumerate(zip(got, exp["ops"], reads)):
        assert g == e, f"{key}: record {k} ({op[0]} {op[1:]}) differs from the reference's: {g} != {e}"
    for s, e in enumerate(exp["slots"]):
        t = e["type"]
        assert mine.active[s].type == t, f"{key}: slot {s} type"
        assert _member(mine.params[s].u, desc.PARAMS_MEMBER, t) == e["params"], f"{key}: slot {s} derived parameters differ from the reference's"
        assert _member(mine.oracle.state(s).u, desc.STATE_MEMBER, t) == e["state"], f"{key}: slot {s} final state differs from the reference's"
        assert digest_floats(mine.oracle.ring(s)) == e["ring"], f"{key}: slot {s} delay rings differ from the reference's"
    assert digest_struct(mine.source_params) == exp["source_params"], f"{key}: source parameters differ from the reference's"
    assert digest_struct(mine.oracle.source_state()) == exp["source_state"], f"{key}: source state differs from the reference's"
