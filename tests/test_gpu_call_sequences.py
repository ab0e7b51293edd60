"""GPU: the batch's setters, apply_changes and upload pass against one `harness.OracleApi` per instance.

The parity tests feed the oracle the descriptors the batch derived itself (`OracleShadow`), so they cannot see a descriptor the
batch derived wrongly from a sequence of calls.  Here every instance has a model of the reference's `Api` (pinned to the compiled
reference by tests/test_oracle_call_sequences.py) that is driven with the same calls, each applied to the instances it touches:
ranges of one instance, a run or all; `set_effect` with stride 0, the record size and a wider stride (records inside a caller's
struct); `set_effect_at` with unsorted, repeated indices; `set_effect_props` broadcast and per instance; sends over ranges;
`apply_changes` on sub-ranges, which leaves other instances' changes pending.

Checks: every mix output bit for bit; every `get_effect` / `get_send_props`, current and deferred; the derived slot and source
parameters (`update_seq` included) after applies, after mixes and at the end; and at the end the state and delay lines.  Reading
parameters back makes the batch derive what is pending (`sync_params`), as the reference's next mix would: the model refreshes at
the same point, and an apply is followed by a read-back only some of the time, so sends written between an apply and the next
mix are also covered."""
import ctypes as C
import random

import numpy as np
import pytest

from harness import OracleApi, make_effect, preset_effect, same_bits, struct_diff
from oalsfxpp_amd import desc
from oalsfxpp_amd.api import Batch, Group
from oalsfxpp_amd.workloads import FIELDS, random_effect
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FRAMES = (1, 64, 100, 256, 441, 2049)


def any_effect(rng, t):
    return random_effect(rng, t) if t in FIELDS else make_effect(t)


def pick_type(rng):
    return rng.choice((desc.EAX_REVERB, desc.EAX_REVERB, desc.REVERB, rng.randrange(12)))


def send_value(rng):
    return rng.choice((lambda: rng.uniform(0.0, 1.0), lambda: rng.uniform(1.0, 2.5), lambda: rng.uniform(-1.0, 0.0), lambda: 1.0))()


def effect_diff(a, b):
    """Effects field by field: the type and every member of the props union (the reverb member's padding bytes are not state)."""
    out = [] if a.type == b.type else [f".type: {a.type} != {b.type}"]
    for name, *_ in desc.EffectPropsU._fields_:
        if name != "raw":
            out += struct_diff(getattr(a.props, name), getattr(b.props, name), f".props.{name}")
    return out


class Wide(C.Structure):
    """A caller's record with an effect inside it: set_effect / set_effect_props with a stride wider than the effect."""
    _fields_ = [("tag", C.c_uint32 * 5), ("effect", desc.Effect), ("tail", C.c_float * 3)]


def _wide(effects):
    arr = (Wide * len(effects))()
    for k, e in enumerate(effects):
        arr[k].tag[0], arr[k].effect, arr[k].tail[0] = 0xDEADBEEF, e, float("nan")
    return arr


class Driver:
    """A batch (or group) and one model per instance, driven op by op."""

    def __init__(self, target, fmt, rate, slots):
        self.t, self.fmt, self.slots = target, fmt, slots
        self.n = target.n
        self.models = [OracleApi(fmt, rate, slots) for _ in range(self.n)]
        self.ch = desc.FORMAT_CHANNELS[fmt]
        self.k = 0
        self.is_batch = isinstance(target, Batch)

    def lib(self):
        return self.t._lib

    def do(self, op):
        kind = op[0]
        if kind == "effect":                       # ("effect", slot, first, effects, stride): effects one per instance
            _, s, first, effects, stride = op
            if stride == "zero":
                self.t.set_effect(s, effects[0], first, len(effects)) if self.is_batch else self.t.set_effect(s, effects[0], first)
                effects = [effects[0]] * (len(effects) if self.is_batch else self.n - first)
            elif stride == "packed":
                self.t.set_effect(s, effects, first, len(effects)) if self.is_batch else self.t.set_effect(s, effects, first)
            else:
                arr = _wide(effects)
                fn = self.lib().oalsfx_batch_set_effect if self.is_batch else self.lib().oalsfx_group_set_effect
                self.t._check(fn(self.t._h, first, len(effects), s, C.addressof(arr) + Wide.effect.offset, C.sizeof(Wide)))
            for k, e in enumerate(effects):
                self.models[first + k].set_effect(s, e)
        elif kind == "effect_at":                  # ("effect_at", slot, instances, effects or one effect)
            _, s, idx, effects = op
            self.t.set_effect_at(s, idx, effects)
            for k, i in enumerate(idx):
                self.models[i].set_effect(s, effects if isinstance(effects, desc.Effect) else effects[k])
        elif kind == "type":                       # ("type", slot, first, count, t)
            _, s, first, count, t = op
            self.t.set_effect_type(s, t, first, count)
            for i in range(first, first + count):
                self.models[i].set_effect_type(s, t)
        elif kind == "props":                      # ("props", slot, first, props list, stride)
            _, s, first, props, stride = op
            if stride == "zero":
                self.t.set_effect_props(s, props[0], first, len(props))
                props = [props[0]] * len(props)
            elif stride == "packed":
                self.t.set_effect_props(s, props, first, len(props))
            else:
                arr = _wide([desc.Effect(0, p) for p in props])
                fn = self.lib().oalsfx_batch_set_effect_props if self.is_batch else self.lib().oalsfx_group_set_effect_props
                self.t._check(fn(self.t._h, first, len(props), s, C.addressof(arr) + Wide.effect.offset + desc.Effect.props.offset, C.sizeof(Wide)))
            for k, p in enumerate(props):
                self.models[first + k].set_effect_props(s, p)
        elif kind == "send":                       # ("send", slot, first, count, g, ghf, glf)
            _, s, first, count, *g = op
            self.t.set_send_props(s, *g, first, count)
            for i in range(first, first + count):
                self.models[i].set_send_props(s, *g)
        elif kind == "apply":                      # ("apply", first, count, read back)
            _, first, count, read = op
            self.t.apply_changes(first, count)
            for i in range(first, first + count):
                self.models[i].apply_changes()
            if read:
                self.check_params(f"after apply({first}, {count})")
        elif kind == "get":                        # ("get", instances)
            for i in op[1]:
                self.check_gets(i)
        elif kind == "mix":
            frames = op[1]
            x = np.stack([orc.synth(100 + i, self.k, frames * self.ch).reshape(frames, self.ch) for i in range(self.n)])
            y = self.t.mix(x)
            for i in range(self.n):
                ok, nbad = same_bits(y[i], self.models[i].mix(x[i]))
                assert ok, f"mix {self.k} ({frames} frames): instance {i}: {nbad} samples differ from its model"
            self.k += 1
            if self.is_batch:
                self.check_params(f"after mix {self.k - 1}")

    def check_gets(self, i):
        b, m = self.t, self.models[i]
        for s in range(self.slots):
            for d in (False, True):
                diff = effect_diff(b.get_effect(i, s, d), m.get_effect(s, d))
                assert not diff, f"instance {i} get_effect({s}, deferred={d}): {diff[:4]}"
        for s in range(-1, self.slots):
            for d in (False, True):
                got, want = b.get_send_props(i, s, d), m.get_send_props(s, d)
                assert bytes(got) == bytes(want), f"instance {i} get_send_props({s}, deferred={d}): {struct_diff(got, want)}"

    def check_params(self, where):
        """The derived records against the models' (reading them back derives what is pending; the models refresh alike)."""
        for i, m in enumerate(self.models):
            m.refresh()
            for s in range(self.slots):
                p, _ = self.t.read_slot(i, s)
                d = struct_diff(p, m.params[s])
                assert not d, f"{where}: instance {i} slot {s} parameters differ from the model's: {d[:4]}"
            sp, _ = self.t.read_source(i)
            d = struct_diff(sp, m.source_params)
            assert not d, f"{where}: instance {i} source parameters differ from the model's: {d[:4]}"

    def check_state(self):
        for i, m in enumerate(self.models):
            diffs = []
            for s in range(self.slots):
                p, st = self.t.read_slot(i, s)
                if p.type in desc.STATE_MEMBER:
                    mem = desc.STATE_MEMBER[p.type]
                    diffs += struct_diff(getattr(st.u, mem), getattr(m.oracle.state(s).u, mem), f"slot{s}.{mem}")
                ok, nbad = same_bits(self.t.read_ring(i, s), m.oracle.ring(s))
                if not ok:
                    diffs.append(f"slot{s}.ring: {nbad} words differ")
            _, sst = self.t.read_source(i)
            diffs += struct_diff(sst, m.oracle.source_state(), "source_state")
            assert not diffs, f"instance {i}: state differs from the model's: {diffs[:4]}"

    def run(self, ops):
        for op in ops:
            self.do(op)

    def finish(self):
        if self.is_batch:    # (a group has no read-back: its outputs were checked)
            for i in range(self.n):
                self.check_gets(i)
            self.check_params("at the end")
            self.check_state()


# ---- programs ----
def pick_range(rng, n):
    r = rng.random()
    if r < 0.3:
        return rng.randrange(n), 1
    if r < 0.75:
        a = rng.randrange(n)
        return a, rng.randint(1, n - a)
    return 0, n


def batch_program(seed, n, slots, group=False):
    """Seeded ops over the batch forms; a group takes set_effect ranges that run to the end (its wrapper's form)."""
    rng = random.Random(9100 + seed)
    ops = [("effect", s, 0, [any_effect(rng, pick_type(rng)) for _ in range(n)], "packed") for s in range(slots)]
    ops += [("apply", 0, n, True), ("mix", 256)]
    last_aux = None
    for _ in range(rng.randint(18, 26)):
        s = rng.randrange(slots)
        first, count = pick_range(rng, n)
        r = rng.random()
        if r < 0.14:
            if group:
                count = n - first
            t = pick_type(rng)
            same = rng.random() < 0.5   # one type for the range (properties may still differ) or a type per instance
            effects = [any_effect(rng, t if same else pick_type(rng)) for _ in range(count)]
            ops.append(("effect", s, first, effects, rng.choice(("zero", "packed", "wide"))))
        elif r < 0.22 and not group:
            idx = [rng.randrange(n) for _ in range(rng.randint(1, 8))]
            idx += [idx[0]] * rng.randint(0, 2)          # repeated: the later record wins
            rng.shuffle(idx)
            t = pick_type(rng)
            ops.append(("effect_at", s, idx, any_effect(rng, t) if rng.random() < 0.3 else [any_effect(rng, t) for _ in idx]))
        elif r < 0.30:
            ops.append(("type", s, first, count, rng.choice((desc.NULL, desc.EAX_REVERB, desc.REVERB, rng.randrange(12)))))
        elif r < 0.40:
            t = rng.choice((desc.EAX_REVERB, rng.randrange(1, 12)))
            ops.append(("props", s, first, [any_effect(rng, t).props for _ in range(count)], rng.choice(("zero", "packed", "wide"))))
        elif r < 0.56:
            d = rng.choice((-1, s, s))
            if last_aux and rng.random() < 0.4:
                # an aux send set before goes back to exactly (1, 1, 1), often with a properties-only change of the same instances
                d, first, count = last_aux
                ops.append(("send", d, first, count, 1.0, 1.0, 1.0))
                if rng.random() < 0.6:
                    t = rng.choice((desc.EAX_REVERB, rng.randrange(1, 12)))
                    ops += [("props", rng.randrange(slots), first, [any_effect(rng, t).props] * count, "zero"), ("apply", first, count, False)]
                continue
            g = (1.0, 1.0, 1.0) if rng.random() < 0.2 else (send_value(rng), send_value(rng), send_value(rng))
            ops.append(("send", d, first, count) + g)
            if d >= 0:
                last_aux = (d, first, count)
        elif r < 0.70:
            ops.append(("apply", first, count, rng.random() < 0.5))
            if rng.random() < 0.2:
                ops.append(("apply", first, count, False))
        elif r < 0.76:
            ops.append(("get", rng.sample(range(n), 3)))
        elif r < 0.88:
            ops.append(("mix", rng.choice(FRAMES)))
        else:
            ops += [("mix", 256)] * rng.randint(3, 8)
    return ops + [("apply", 0, n, False), ("mix", 256), ("mix", 256)]


def aux_to_unity(first, count, second_change):
    """Aux send 0.5, apply, mix; the send back to exactly (1, 1, 1) while the slot changes, apply, mix: the reference re-derives the
    sends from the active aux props on any slot change (src/oalsfxpp.cpp:3397-3412) and mixes at send gain 1 from then on."""
    ops = [("send", 0, first, count, 0.5, 0.5, 0.5), ("apply", first, count, False)] + [("mix", 256)] * 3
    ops += [("send", 0, first, count, 1.0, 1.0, 1.0), ("get", [first])] + second_change + [("apply", first, count, False)]
    return ops + [("mix", 256)] * 4


def _setup(n, t=desc.EAX_REVERB):
    return [("effect", 0, 0, [make_effect(t)] * n, "zero"), ("apply", 0, n, False), ("mix", 256)]


@pytest.mark.parametrize("change", ["same_type", "props", "type_change"])
def test_aux_send_back_to_unity_one_instance(change):
    """The directed sequence at one instance; a change of type (which re-derived the sends already) is the control."""
    second = {"same_type": [("effect", 0, 0, [preset_effect(112)], "packed")],
              "props": [("props", 0, 0, [preset_effect(8).props], "packed")],
              "type_change": [("effect", 0, 0, [make_effect(desc.REVERB)], "packed")]}[change]
    with Batch(1, desc.FMT_STEREO, 48000, 1) as b:
        d = Driver(b, desc.FMT_STEREO, 48000, 1)
        d.run(_setup(1) + aux_to_unity(0, 1, second))
        d.finish()


def test_aux_send_back_to_unity_inside_a_batch():
    """The same inside 32 instances: a run of them takes the sequence, one of them has its other slot change instead, and the
    rest keep their 0.5 send (for good: an aux send once set keeps its instance on the apply list)."""
    n = 32
    with Batch(n, desc.FMT_STEREO, 48000, 2) as b:
        d = Driver(b, desc.FMT_STEREO, 48000, 2)
        ops = _setup(n) + [("effect", 1, 0, [make_effect(desc.ECHO)] * n, "zero"), ("apply", 0, n, True)]
        ops += [("send", 0, 0, n, 0.5, 0.5, 0.5), ("apply", 0, n, False), ("mix", 256), ("mix", 256)]
        ops += [("send", 0, 5, 9, 1.0, 1.0, 1.0), ("send", 0, 20, 1, 1.0, 1.0, 1.0)]
        ops += [("props", 0, 5, [preset_effect(8).props] * 9, "packed"), ("effect", 1, 20, [make_effect(desc.ECHO, delay=0.05)], "packed")]
        ops += [("apply", 0, 10, False), ("mix", 256), ("apply", 10, n - 10, True)] + [("mix", 256)] * 4
        d.run(ops)
        d.finish()


@pytest.mark.parametrize("seed", range(20))
def test_call_sequences_property(seed):
    rng = random.Random(seed)
    fmt = (desc.FMT_STEREO, desc.FMT_STEREO, desc.FMT_MONO, rng.choice((desc.FMT_5POINT1, desc.FMT_6POINT1, desc.FMT_7POINT1)))[seed % 4]
    rate, slots, n = rng.choice((44100, 48000)), rng.randint(1, 3), rng.choice((24, 32, 48))
    with Batch(n, fmt, rate, slots) as b:
        d = Driver(b, fmt, rate, slots)
        d.run(batch_program(seed, n, slots))
        d.finish()


def test_group_setters_straddle_shards():
    """One group over three shards of one device: broadcast and per-instance setters (oalsfx_group_set_effect_props included)
    and partial applies whose ranges cross the shard boundaries, against one model per instance."""
    n = 30
    with Group(n, [0, 0, 0], desc.FMT_STEREO, 48000, 2) as g:
        bounds = [f for _, f, _ in g.shards][1:]
        assert len(g.shards) == 3 and all(0 < f < n for f in bounds)
        a, c = bounds[0] - 2, bounds[1] + 3   # ranges that straddle a boundary each, and one that spans a whole shard
        rng = random.Random(3)
        d = Driver(g, desc.FMT_STEREO, 48000, 2)
        ops = [("effect", 0, 0, [any_effect(rng, desc.EAX_REVERB) for _ in range(n)], "packed"), ("effect", 1, 0, [make_effect(desc.CHORUS)] * n, "zero"),
               ("apply", 0, n, False), ("mix", 256)]
        ops += [("send", 0, a, c - a, 0.5, 0.7, 0.9), ("send", -1, a + 1, 4, 0.8, 1.5, -0.2), ("apply", a, 5, False), ("mix", 256),
                ("apply", 0, n, False), ("mix", 441)]
        ops += [("props", 0, a, [any_effect(rng, desc.EAX_REVERB).props for _ in range(c - a)], "packed"),
                ("props", 1, bounds[0] - 1, [make_effect(desc.CHORUS, rate=2.5).props] * 3, "zero"),
                ("props", 1, bounds[1] - 1, [make_effect(desc.FLANGER).props] * 2, "wide"),
                ("send", 0, a, 3, 1.0, 1.0, 1.0), ("type", 1, c - 1, n - c + 1, desc.ECHO)]
        ops += [("apply", bounds[0] - 1, 2, False), ("mix", 256), ("apply", a, c - a, False), ("mix", 256)]
        ops += [("effect", 0, bounds[1] - 2, [make_effect(desc.REVERB)] * (n - bounds[1] + 2), "wide"), ("apply", 0, n, False)]
        ops += [("mix", 256)] * 4 + [("mix", 100)]
        d.run(ops)
        d.finish()


def test_cpp_api_and_api_array_sequences(tmp_path):
    """tests/cpp/api_sequences.cpp: oalsfxpp::Api and oalsfxpp::ApiArray, the public C++ surfaces over the same batch code, through
    the aux-to-unity sequence (set_effect_props on one instance, set_effect on another, a send left at 0.5 on a third)."""
    import os
    import subprocess
    from harness import ROOT
    from oalsfxpp_amd import lib
    exe, out = str(tmp_path / "api_sequences"), str(tmp_path / "out.f32")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "api_sequences.cpp"),
                    "-L", libdir, "-loalsfx_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape(4, -1)
    changes = [lambda m: m.set_effect_props(0, preset_effect(112).props), lambda m: m.set_effect_props(0, preset_effect(112).props),
               lambda m: m.set_effect(0, preset_effect(112)), lambda m: None]
    for k, change in enumerate(changes):   # Api; ApiArray instances 0, 1, 2
        m = OracleApi(desc.FMT_STEREO, 48000, 1)
        m.set_effect(0, make_effect(desc.EAX_REVERB))
        m.set_send_props(0, 0.5, 0.5, 0.5)
        m.apply_changes()
        outs = [m.mix(orc.synth(300 + k, j, 512).reshape(256, 2)) for j in range(3)]
        if k < 3:
            m.set_send_props(0, 1.0, 1.0, 1.0)
        change(m)
        m.apply_changes()
        outs += [m.mix(orc.synth(300 + k, j, 512).reshape(256, 2)) for j in range(3, 7)]
        ok, nbad = same_bits(got[k], np.concatenate(outs))
        assert ok, f"{('Api', 'ApiArray[0]', 'ApiArray[1]', 'ApiArray[2]')[k]}: {nbad} samples differ from the model"
