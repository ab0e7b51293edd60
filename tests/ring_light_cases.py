"""The ring-light effects at the delays where their kernels switch code paths (csrc/hip/wave_effects_body.hpp): one table of named
cases for the CPU side (tests/test_oracle_vs_reference.py, family `edge[...]`: the oracle held to the reference) and the GPU side
(tests/test_gpu_ring_light_edges.py: the HIP path held to the oracle).

A case is (effect type, sampling rate, property overrides, calls) and the derived integers it is meant to hit -- tap1, tap2, delay,
depth, lfo_range, lfo_disp, step, as the host update path derives them (oalsfx_host_derive_slot).  `check` compares them, so that a
rounding in `delay * rate` cannot move a case off its edge unnoticed, and makes sure every property lies inside its legal range (the
normalised effect is the effect).  `calls` are frame counts, or a dict of property overrides applied in front of the next call.

What the edges are:
  * echo: the tile is walked in sub-blocks of min(64, tap2) samples; a tap shorter than its lane's position reads the tile being
    written instead of the ring; both taps >= 128 lets a tile request the next one's taps ahead.
  * chorus / flanger: per lane a delay d.  d == 0; every in-tile source the same d <= 16 (the chain path); anything else inside the
    tile (ballot and permute rounds); no source inside the tile (d >= 64); the request one tile ahead (delay - |depth| - 1 >= 128).
  * ring modulator: step forced to 1 at frequency 0; step == 2^24 at frequency == rate (the masked index stays put); the eight
    octants of the sinusoid carrier, where sinf changes branch or quadrant.
"""
import random

from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.workloads import FIELDS, make_effect

CALLS = (256, 1, 63, 65, 130, 256)      # whole tiles, one frame, ragged tiles below and above a tile, two tiles and a bit
MINMAX_CALLS = (256, 100, 1)
FRAC_ONE = 1 << 24


class Case:
    def __init__(self, name, effect_type, rate, props, expect, calls=CALLS, expect_changed=None):
        self.name, self.type, self.rate, self.props, self.expect, self.calls = name, effect_type, rate, dict(props), dict(expect), tuple(calls)
        self.expect_changed = dict(expect_changed or {})   # the derived integers behind every property change among the calls

    def effect(self, **changed):
        return make_effect(self.type, **dict(self.props, **changed))

    def frame_counts(self):
        return tuple(c for c in self.calls if isinstance(c, int))

    def __repr__(self):
        return f"Case({self.name})"


def derived(case, fmt=desc.FMT_STEREO, **changed):
    """The integers the kernels branch on, from the host update path."""
    e = case.effect(**changed)
    n = lib.effect_normalized(e)
    m = desc.PROPS_MEMBER[case.type]
    assert bytes(getattr(e.props, m)) == bytes(getattr(n.props, m)), f"{case.name}: a property lies outside its legal range"
    p = lib.derive_slot(fmt, case.rate, n)
    if case.type == desc.ECHO:
        return dict(tap1=p.u.echo.tap1, tap2=p.u.echo.tap2)
    if case.type in (desc.CHORUS, desc.FLANGER):
        q = p.u.moddelay
        return dict(delay=q.delay, depth=int(abs(q.depth)), lfo_range=q.lfo_range, lfo_disp=q.lfo_disp, ask=q.delay - int(abs(q.depth)) - 1)
    if case.type == desc.RING_MODULATOR:
        return dict(step=p.u.ringmod.step)
    return {}


def check(case):
    got = derived(case)
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.name}: {k} is {got[k]}, the case is meant to have {v}"
    for c in case.calls:
        if not isinstance(c, int):
            got = derived(case, **c)   # (the changed properties are legal too)
            assert case.expect_changed, f"{case.name}: a property change without an expectation"
            for k, v in case.expect_changed.items():
                assert got[k] == v, f"{case.name}: behind the change {k} is {got[k]}, the case is meant to have {v}"


def _seconds(samples, rate, most):
    """A property in seconds that the update path truncates to `samples` at `rate`: half a sample above, or the legal maximum."""
    return 0.0 if samples == 0 else min((samples + 0.5) / rate, most)


# ---- echo: tap1 = int(delay * rate) + 1, tap2 = tap1 + int(lr_delay * rate) ----
ECHO_TAPS = [(1, 2), (1, 63), (1, 64), (1, 65), (3, 5), (16, 17), (31, 33), (63, 63), (63, 64), (64, 64), (64, 128), (65, 127), (127, 128),
             (128, 128), (128, 129), (1, 128)]
ECHO_VARIANTS = [dict(feedback=f, damping=d, spread=s) for f, d, s in
                 [(1.0, 0.0, -1.0), (0.0, 0.99, 0.0), (1.0, 0.99, 1.0), (0.5, 0.0, 0.0), (1.0, 0.5, -1.0), (0.0, 0.0, 1.0)]]
GROUP_TAPS = [(2, 3), (9, 17), (33, 64), (140, 300)]   # echoes whose sub-blocks differ, for cooperative workgroups that share the minimum


def _echo(name, tap1, tap2, rate, variant):
    props = dict(delay=_seconds(tap1 - 1, rate, 0.207), lr_delay=_seconds(tap2 - tap1, rate, 0.404), **variant)
    return Case(name, desc.ECHO, rate, props, dict(tap1=tap1, tap2=tap2))


def echo_cases():
    out = []
    for i, (t1, t2) in enumerate(ECHO_TAPS):
        out.append(_echo(f"echo_{t1}_{t2}", t1, t2, 48000 if i % 2 == 0 else 8000, ECHO_VARIANTS[i % len(ECHO_VARIANTS)]))
    for i, (rate, t1, t2) in enumerate(((8000, 1657, 4889), (192000, 39745, 117313))):   # the longest taps there are
        out.append(Case(f"echo_max_{rate}", desc.ECHO, rate, dict(delay=0.207, lr_delay=0.404, **ECHO_VARIANTS[2 * i]), dict(tap1=t1, tap2=t2)))
    return out


def echo_group_cases():
    return [_echo(f"echo_group_{t2}", t1, t2, 48000, ECHO_VARIANTS[i]) for i, (t1, t2) in enumerate(GROUP_TAPS)]


# ---- chorus / flanger ----
MOD_MAX = {desc.CHORUS: 0.016, desc.FLANGER: 0.004}
MOD_NAME = {desc.CHORUS: "chorus", desc.FLANGER: "flanger"}
CONSTANT_DELAYS = [0, 1, 2, 3, 15, 16, 17, 32, 63, 64, 65, 127, 128, 129, 130]
MOVING_DELAYS = [1, 8, 16, 17, 40, 64, 129, 192]


def _lowest_rate(t, d):
    """The lowest of a few sampling rates at which a delay of d samples is legal (the shorter the LFO's period in samples, the more
    often a run wraps it: lfo_range = rate / 10 at the fastest LFO)."""
    for rate in (8000, 8200, 12100, 16200, 48200):
        if d == 0 or (d + 0.5) / rate <= MOD_MAX[t] or (d == 128 and rate == 8000 and t == desc.CHORUS):
            return rate
    raise ValueError((t, d))


def constant_delay_cases():
    """depth = 0: every lane of every tile has d == delay."""
    out = []
    for t in (desc.CHORUS, desc.FLANGER):
        for d in CONSTANT_DELAYS:
            rate = _lowest_rate(t, d) if t == desc.CHORUS else 48000
            for fb in (-1.0, 0.0, 1.0):
                props = dict(delay=_seconds(d, rate, MOD_MAX[t]), depth=0.0, feedback=fb, rate=1.1, phase=90, waveform=1)
                out.append(Case(f"{MOD_NAME[t]}_d{d}_fb{fb:+.0f}", t, rate, props, dict(delay=d, depth=0)))
    return out


def moving_delay_cases():
    """depth = 1: d sweeps 0 .. 2 * delay and crosses the regimes inside a call, the fastest LFO (10 Hz) at the lowest rate the delay
    allows.  Three rounds of CALLS (2313 frames): at 8 kHz (lfo_range 800) both taps cross the LFO's wrap more than once, inside a tile."""
    out = []
    for t in (desc.CHORUS, desc.FLANGER):
        for d in MOVING_DELAYS:
            rate = _lowest_rate(t, d)
            lfo_range = int(rate / 10.0 + 0.5)
            for w in (0, 1):
                for ph in (-180, 0, 90, 180):
                    props = dict(delay=_seconds(d, rate, MOD_MAX[t]), depth=1.0, feedback=(-0.9 if (w + ph // 90) % 2 else 0.9), rate=10.0, phase=ph, waveform=w)
                    disp = int(lfo_range * ((ph if ph >= 0 else 360 + ph) / 360.0))
                    out.append(Case(f"{MOD_NAME[t]}_sweep{d}_w{w}_ph{ph}", t, rate, props, dict(delay=d, depth=d, lfo_range=lfo_range, lfo_disp=disp), CALLS * 3))
        for d in (8, 64 if t == desc.CHORUS else 30):
            for w in (0, 1):   # rate 0: the LFO stands still -- the sinusoid at d == delay, the triangle at d == delay - depth == 0
                props = dict(delay=_seconds(d, 8000, MOD_MAX[t]), depth=1.0, feedback=0.7, rate=0.0, phase=90, waveform=w)
                out.append(Case(f"{MOD_NAME[t]}_still{d}_w{w}", t, 8000, props, dict(delay=d, depth=d, lfo_range=1, lfo_disp=0)))
    for ask, depth in ((127, 72), (128, 71), (129, 70)):
        # the request one tile ahead is taken from delay - int(|depth|) - 1 >= 128 on
        props = dict(delay=_seconds(200, 48000, 0.016), depth=(depth + 0.5) / 200.0, feedback=0.8, rate=10.0, phase=90, waveform=0)
        out.append(Case(f"chorus_ask{ask}", desc.CHORUS, 48000, props, dict(delay=200, depth=depth, ask=ask, lfo_range=4800), CALLS * 3))
    return out


# ---- ring modulator: step = int(frequency * 2^24 / rate), 1 where that is 0 ----
def ring_modulator_cases():
    out = []
    for w in (0, 1, 2):
        out.append(Case(f"ringmod_f0_w{w}", desc.RING_MODULATOR, 48000, dict(frequency=0.0, waveform=w), dict(step=1)))
        out.append(Case(f"ringmod_f8000_8k_w{w}", desc.RING_MODULATOR, 8000, dict(frequency=8000.0, waveform=w), dict(step=FRAC_ONE)))
        out.append(Case(f"ringmod_f8000_8M_w{w}", desc.RING_MODULATOR, 8000000, dict(frequency=8000.0, waveform=w), dict(step=16777)))
    for hp in (0.0, 24000.0):
        out.append(Case(f"ringmod_hp{hp:.0f}", desc.RING_MODULATOR, 8000, dict(frequency=440.0, high_pass_cutoff=hp, waveform=0), dict(step=922746)))
    # The octant boundaries of the sinusoid carrier, index k * 2^21.  At 16384 Hz step = frequency * 1024 exactly.  A first call of F
    # frames at step s parks the index at F * s = k * 2^21 - 512 (mod 2^24), a property change (frequency 0) sets step to 1 and keeps
    # the index, 1024 more frames walk across the boundary.  k = 1 .. 7: F = 2.  Index 2^24 - 512 (k = 0 and k = 8 are the same
    # boundary) would need a frequency above the legal 8000 Hz with two frames: four frames for k = 8, eight for k = 0.
    for k in range(9):
        frames = 2 if 1 <= k <= 7 else 4 if k == 8 else 8
        step = ((k * (1 << 21) - 512) % FRAC_ONE) // frames
        assert (step * frames) % FRAC_ONE == (k * (1 << 21) - 512) % FRAC_ONE
        out.append(Case(f"ringmod_octant{k}", desc.RING_MODULATOR, 16384, dict(frequency=step / 1024.0, waveform=0, high_pass_cutoff=100.0), dict(step=step),
                        (frames, dict(frequency=0.0), 1024), expect_changed=dict(step=1)))
    return out


# ---- every ring-light type, every property at either end of its range ----
MINMAX_TYPES = (desc.CHORUS, desc.FLANGER, desc.COMPRESSOR, desc.DEDICATED_DIALOG, desc.DEDICATED_LFE, desc.DISTORTION, desc.ECHO, desc.EQUALIZER,
                desc.RING_MODULATOR)


def minmax_cases():
    out = []
    for t in MINMAX_TYPES:
        for field, (lo, hi) in FIELDS[t].items():
            for end, v in (("min", lo), ("max", hi)):
                for rate in (8000, 192000):
                    out.append(Case(f"{desc.EFFECT_NAMES[t]}_{field}_{end}_{rate}", t, rate, {field: v}, {}, MINMAX_CALLS))
    return out


def all_cases():
    """Every case, by name."""
    out = {}
    for c in echo_cases() + echo_group_cases() + constant_delay_cases() + moving_delay_cases() + ring_modulator_cases() + minmax_cases():
        assert c.name not in out, c.name
        out[c.name] = c
    return out


# ---- placement on the device (csrc/hip/batch.cpp, wave_segments) ----
COOPERATIVE = (desc.DISTORTION, desc.ECHO, desc.EQUALIZER, desc.RING_MODULATOR)


def placements(cases):
    """Instance lists for up to six cases of one cooperative type, such that every case runs once inside a workgroup of four and once on
    a lone wavefront.  A single-slot grid takes the instances of such a type in instance order, whole workgroups of four first, and
    leaves `count & 3` at the end on lone wavefronts: a list is four cases and then up to three."""
    cases = list(cases)
    assert 1 <= len(cases) <= 6
    if len(cases) <= 3:
        return [(cases * 4)[:4] + cases]
    first = cases[:4] + (cases[4:] + cases)[:3]
    lone = [c for c in cases if c not in first[4:]]
    coop = (cases[4:] + [c for c in cases if c not in cases[4:]])[:4]
    return [first, coop + lone]


def batches(cases):
    """The cases as batches of one sampling rate and one call script each: [(rate, calls, [case per instance])].  Cooperative types go
    in sixes, each six twice (`placements`); the other types ride along once."""
    groups = {}
    for c in cases:
        groups.setdefault((c.rate, repr(c.calls)), []).append(c)
    out = []
    for (rate, _), members in groups.items():
        calls = members[0].calls
        lists = [[c for c in members if c.type not in COOPERATIVE]]
        for t in COOPERATIVE:
            mine = [c for c in members if c.type == t]
            for k in range(0, len(mine), 6):
                for j, pl in enumerate(placements(mine[k:k + 6])):
                    while len(lists) <= k // 6 * 2 + j:
                        lists.append([])
                    lists[k // 6 * 2 + j] += pl
        out += [(rate, calls, inst) for inst in lists if inst]
    return out


def shuffled(instances, seed):
    """The same instances with the types interleaved: the grid sorts by type and keeps the instance order inside a type."""
    rng = random.Random(seed)
    by_type = {}
    for c in instances:
        by_type.setdefault(c.type, []).append(c)
    order = [c.type for c in instances]
    rng.shuffle(order)
    its = {t: iter(v) for t, v in by_type.items()}
    return [next(its[t]) for t in order]
