"""CPU: the oracle against the compiled reference on cases that are too many or too large to keep as full fixtures: all 113
presets, every channel format, low and high sampling rates, randomised properties, and the ring-light effects at the delays
where their kernels switch code paths (tests/ring_light_cases.py), where a uniform draw of the properties never lands.

What the reference computes for every case is kept in tests/golden/reference_digests.json (written by tests/golden/generate.py):
digests of each mix call's output, of the derived parameters and final state of each slot (the members the slot's effect type
uses), of its final delay rings and of the source's parameters and state.  Each digest is taken over a canonical form that
keeps exactly the distinctions the bit-exact comparison makes: NaNs are one value whatever their sign or payload, and a
structure's fields are compared by value (+0 and -0 alike, padding ignored) as `harness.struct_diff` does.  The ring-light edge
cases keep three digests each -- of these digests of the outputs, of the parameters and of the state and rings, mono and stereo runs
together -- one case per line ("name": "outputs parameters state") in tests/golden/ring_light_edge_digests.json.  Where the compiled
reference is present (oracle/_ref/libref.so) each case is also run on it, and its digests must still be the stored ones."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import ring_light_cases
from harness import OracleApi, make_effect, preset_effect
from oalsfxpp_amd import desc
from oalsfxpp_amd.workloads import FIELDS, random_effect
from oracle import oracle as orc

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")
EDGE_DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ring_light_edge_digests.json")
INPUT_SEED = 5


# ---- the cases: key -> [(fmt, rate, slots, effects, mixes)], one entry per run of a fresh Api; `mixes` are frame counts, or
# ("set", slot, effect): a property change applied in front of the next mix ----
def preset_runs(index):
    return [(desc.FMT_STEREO, 48000, 1, [(0, preset_effect(index))], [256] * 3)]


def format_runs(fmt):
    return [(fmt, 44100, 1, [(0, make_effect(t))], [200, 56]) for t in range(12)]


RATE_TYPES = (desc.EAX_REVERB, desc.REVERB, desc.CHORUS, desc.FLANGER, desc.ECHO, desc.DISTORTION, desc.RING_MODULATOR, desc.EQUALIZER,
              desc.COMPRESSOR)


def rate_runs(rate):
    return [(desc.FMT_STEREO, rate, 1, [(0, make_effect(t))], [256] * 3) for t in RATE_TYPES]


def random_runs(seed):
    rng = random.Random(seed)
    t = rng.choice(list(FIELDS))
    first = (desc.FMT_STEREO, 48000, 1, [(0, random_effect(rng, t))], [256] * 5)
    return [first, (desc.FMT_MONO, 48000, 1, [(0, random_effect(rng, desc.EAX_REVERB))], [256] * 4)]


def edge_runs(case):
    """A case of tests/ring_light_cases.py, mono and stereo (the GPU side compares the HIP path with the oracle on the same table)."""
    mixes = [c if isinstance(c, int) else ("set", 0, case.effect(**c)) for c in case.calls]
    return [(fmt, case.rate, 1, [(0, case.effect())], mixes) for fmt in (desc.FMT_STEREO, desc.FMT_MONO)]


EDGES = ring_light_cases.all_cases()
PRESETS = range(0, 113)
FORMATS = range(1, 8)
RATES = [8000, 11025, 22050, 32000, 96000, 192000]
SEEDS = range(24)


def all_cases():
    out = {}
    for i in PRESETS:
        out[f"preset[{i}]"] = preset_runs(i)
    for f in FORMATS:
        out[f"format[{f}]"] = format_runs(f)
    for r in RATES:
        out[f"rate[{r}]"] = rate_runs(r)
    for s in SEEDS:
        out[f"random[{s}]"] = random_runs(s)
    return out


# ---- canonical digests ----
def digest_floats(a):
    """Float32 words as `harness.same_bits` compares them: bit for bit, every NaN alike."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return hashlib.sha256(bits.tobytes()).hexdigest()[:16]


def _leaves(x):
    if isinstance(x, (C.Structure, C.Union)):
        for name, *_ in x._fields_:
            yield from _leaves(getattr(x, name))
    elif isinstance(x, C.Array):
        for v in x:
            yield from _leaves(v)
    elif isinstance(x, float):
        yield "nan" if x != x else x + 0.0   # (-0.0 + 0.0 is +0.0)
    else:
        yield x


def digest_struct(s):
    """A ctypes structure field by field, as `harness.struct_diff` compares two of them."""
    return hashlib.sha256(repr(list(_leaves(s))).encode()).hexdigest()[:16]


def _member(union, table, t):
    return digest_struct(getattr(union, table[t])) if t in table else None


# ---- one run on either side ----
def _drive(api, run):
    fmt, rate, slots, effects, mixes = run
    for s, e in effects:
        api.set_effect(s, e)
    api.apply_changes()
    outs = []
    k = 0
    for frames in mixes:
        if not isinstance(frames, int):
            api.set_effect(frames[1], frames[2])
            api.apply_changes()
            continue
        x = orc.synth(INPUT_SEED, k, frames * api.channels).reshape(frames, api.channels)
        outs.append(digest_floats(api.mix(x)))
        k += 1
    return outs


def reference_record(run):
    """What the compiled reference computes for one run (the digests stored in tests/golden/reference_digests.json)."""
    fmt, rate, slots = run[:3]
    ref = orc.Reference(fmt, rate, slots)
    rec = {"channels": ref.channels, "mix": _drive(ref, run), "slots": []}
    for s in range(slots):
        rp, rs = ref.dump_slot(s)
        rec["slots"].append({"type": rp.type, "params": _member(rp.u, desc.PARAMS_MEMBER, rp.type),
                             "state": _member(rs.u, desc.STATE_MEMBER, rp.type), "ring": digest_floats(ref.dump_rings(s, rp))})
    sp, ss = ref.dump_source()
    rec["source_params"], rec["source_state"] = digest_struct(sp), digest_struct(ss)
    return rec


def oracle_record(run, types):
    """The same digests of the oracle driven by the host update path; `types` are the reference's slot types, whose members
    of the parameter and state unions are compared."""
    fmt, rate, slots = run[:3]
    mine = OracleApi(fmt, rate, slots)
    rec = {"channels": mine.channels, "mix": _drive(mine, run), "slots": []}
    for s, t in zip(range(slots), types):
        rec["slots"].append({"type": t, "params": _member(mine.params[s].u, desc.PARAMS_MEMBER, t),
                             "state": _member(mine.oracle.state(s).u, desc.STATE_MEMBER, t), "ring": digest_floats(mine.oracle.ring(s))})
    rec["source_params"], rec["source_state"] = digest_struct(mine.source_params), digest_struct(mine.oracle.source_state())
    return rec


_stored = None


def stored(key):
    global _stored
    if _stored is None:
        with open(DIGESTS) as f:
            _stored = json.load(f)
    return _stored[key]


def compare(key, runs):
    expected = stored(key)
    assert len(expected) == len(runs), f"{key}: {len(expected)} runs stored, {len(runs)} defined"
    for i, (run, exp) in enumerate(zip(runs, expected)):
        where = f"{key} run {i}"
        if orc.have_reference():
            assert reference_record(run) == exp, f"{where}: the compiled reference no longer gives the stored digests (tests/golden/generate.py)"
        got = oracle_record(run, [s["type"] for s in exp["slots"]])
        assert got["channels"] == exp["channels"], where
        for k, (g, e) in enumerate(zip(got["mix"], exp["mix"])):
            assert g == e, f"{where}: mix {k} output differs from the reference's"
        assert len(got["mix"]) == len(exp["mix"]), where
        for s, (g, e) in enumerate(zip(got["slots"], exp["slots"])):
            assert g["params"] == e["params"], f"{where}: slot {s} derived parameters differ from the reference's"
            assert g["state"] == e["state"], f"{where}: slot {s} final state differs from the reference's"
            assert g["ring"] == e["ring"], f"{where}: slot {s} delay rings differ from the reference's"
        assert got["source_params"] == exp["source_params"], f"{where}: source parameters differ from the reference's"
        assert got["source_state"] == exp["source_state"], f"{where}: source state differs from the reference's"


@pytest.mark.parametrize("index", PRESETS)
def test_every_preset(index):
    compare(f"preset[{index}]", preset_runs(index))


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_every_effect(fmt):
    compare(f"format[{fmt}]", format_runs(fmt))


@pytest.mark.parametrize("rate", RATES)
def test_rates(rate):
    compare(f"rate[{rate}]", rate_runs(rate))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_properties(seed):
    compare(f"random[{seed}]", random_runs(seed))


# ---- the family edge[...]: the same records, condensed to three digests per case (mono and stereo run together) ----
PARTS = {"out": "outputs differ", "params": "derived parameters differ", "state": "final state or delay rings differ"}


def condensed(records):
    def h(x):
        return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:10]
    return {"out": h([[r["channels"], r["mix"]] for r in records]),
            "params": h([[[s["type"], s["params"]] for s in r["slots"]] + [r["source_params"]] for r in records]),
            "state": h([[[s["state"], s["ring"]] for s in r["slots"]] + [r["source_state"]] for r in records])}


_stored_edges = None


def compare_edge(key, case):
    global _stored_edges
    if _stored_edges is None:
        with open(EDGE_DIGESTS) as f:
            _stored_edges = json.load(f)
    expected, runs = dict(zip(PARTS, _stored_edges[case.name].split())), edge_runs(case)
    reference = [reference_record(run) for run in runs] if orc.have_reference() else None
    if reference:
        assert condensed(reference) == expected, f"{key}: the compiled reference no longer gives the stored digests (tests/golden/generate.py)"
    mine = [oracle_record(run, [case.type]) for run in runs]
    got = condensed(mine)
    for part, what in PARTS.items():
        assert got[part] == expected[part], f"{key}: {what} from the reference's" + _where(mine, reference)


def _where(mine, reference):
    """Which run (stereo, then mono) and which call or field differs: the stored digests are per case, so this takes the compiled
    reference (where it is not built the message says so)."""
    if not reference:
        return " (build oracle/_ref to see in which format and call)"
    out = []
    for fmt, m, r in zip(("stereo", "mono"), mine, reference):
        out += [f"{fmt} mix {k}" for k, (a, b) in enumerate(zip(m["mix"], r["mix"])) if a != b]
        out += [f"{fmt} slot {field}" for field in ("params", "state", "ring") if m["slots"][0][field] != r["slots"][0][field]]
        out += [f"{fmt} {field}" for field in ("source_params", "source_state") if m[field] != r[field]]
    return ": " + ", ".join(out[:8])


@pytest.mark.parametrize("name", list(EDGES))
def test_ring_light_edges(name):
    """The table states each case by the integers it is meant to hit; they are checked before the case is run."""
    ring_light_cases.check(EDGES[name])
    compare_edge(f"edge[{name}]", EDGES[name])
