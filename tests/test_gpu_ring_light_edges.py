"""GPU: the ring-light effect kernels (csrc/hip/wave_effects_body.hpp) against the CPU oracle on the cases of tests/ring_light_cases.py
-- delays of a few samples, where the echo's sub-blocks, the chorus's and flanger's five regimes and the ring modulator's carrier
switch code paths -- bit for bit: every output buffer, the slot state, the delay rings.  (The oracle itself is held to the reference on
the same table by tests/test_oracle_vs_reference.py, family edge[...].)

Where an instance runs matters as much as its properties.  A single-slot grid sorts the instances by effect type and keeps the instance
order inside a type (batch.cpp, wave_segments).  Of echoes, distortions, equalizers and ring modulators it makes cooperative workgroups
of four -- the first `count & ~3` instances of the type, four consecutive ones each, whose recurrences one wavefront runs for all four
-- and leaves the last `count & 3` on lone wavefronts; every other type has one wavefront per instance.  ring_light_cases.batches lays
the cases out accordingly: six cases of a cooperative type make two lists of seven (four, then three), the second one rotated, so that
every case runs once as one of four and once alone; `shuffled` then interleaves the types, which the sort undoes."""
import numpy as np
import pytest

import ring_light_cases as rl
from harness import OracleShadow, same_bits
from oalsfxpp_amd import desc
from oalsfxpp_amd.api import Batch
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FAMILIES = {
    "echo": lambda: rl.echo_cases() + rl.echo_group_cases(),
    "constant": rl.constant_delay_cases,
    "moving": rl.moving_delay_cases,
    "ringmod": rl.ring_modulator_cases,
    "minmax": rl.minmax_cases,
}


def run(fmt, rate, calls, instances, seed=0, slots=None):
    """One batch, instance i holding case instances[i] (or, with `slots`, instances[i][s] in slot s), taken through the calls with every
    instance followed by an oracle."""
    n = len(instances)
    per_slot = [[c] for c in instances] if slots is None else instances
    with Batch(n, fmt, rate, len(per_slot[0])) as b:
        for s in range(len(per_slot[0])):
            b.set_effect(s, [c[s].effect() for c in per_slot])
        b.apply_changes()
        shadows = [OracleShadow(b, i) for i in range(n)]
        names = ["+".join(c.name for c in cs) for cs in per_slot]
        k = 0
        for op in calls:
            if not isinstance(op, int):   # a property change of every instance
                for i, cs in enumerate(per_slot):
                    b.set_effect(0, cs[0].effect(**op), first=i, count=1)
                b.apply_changes()
                for sh in shadows:
                    sh.sync()
                continue
            x = np.stack([orc.synth(3000 + seed + i, k, op * b.channels).reshape(op, b.channels) for i in range(n)])
            y = b.mix(x)
            for i in range(n):
                ok, nbad = same_bits(y[i], shadows[i].mix(x[i]))
                assert ok, f"{names[i]} (instance {i} of {n}, {rate} Hz, format {fmt}), call {k} of {op} frames: {nbad} samples differ"
            k += 1
        for i in range(n):
            d = shadows[i].compare_state()
            assert not d, f"{names[i]} (instance {i} of {n}, {rate} Hz, format {fmt}): " + "; ".join(d[:6])


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO], ids=["mono", "stereo"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_edge_cases_in_workgroups_of_four_and_alone(family, fmt):
    for k, (rate, calls, instances) in enumerate(rl.batches(FAMILIES[family]())):
        run(fmt, rate, calls, rl.shuffled(instances, k), seed=100 * k)


@pytest.mark.parametrize("family", ["echo", "constant", "moving"])
def test_edge_cases_with_eight_channels(family):
    """7.1: the build of the kernel that takes the channel count at run time."""
    for k, (rate, calls, instances) in enumerate(rl.batches(FAMILIES[family]())):
        run(desc.FMT_7POINT1, rate, calls, rl.shuffled(instances, k), seed=100 * k)


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO], ids=["mono", "stereo"])
def test_echoes_of_a_workgroup_share_the_shortest_block(fmt):
    """The four echoes of a cooperative workgroup walk the tile in the same sub-blocks, the shortest of their own (EchoW::init): echoes
    with tap2 = 3, 17, 64 and 300 -- blocks of 3, 17, 64 and 64 -- as one workgroup, in each of the four orders, so that each of them
    is once in each place of its workgroup (instances 0..15: four whole workgroups, nothing left over).  Behind them, in a batch of
    their own, a workgroup whose shortest block is 17 and not anybody's in the first place, and three of the echoes alone."""
    g = rl.echo_group_cases()
    for c in g:
        rl.check(c)
    run(fmt, 48000, rl.CALLS, [g[(r + j) % 4] for r in range(4) for j in range(4)])
    run(fmt, 48000, rl.CALLS, [g[3], g[2], g[1], g[3], g[0], g[1], g[2]], seed=7)


@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO], ids=["mono", "stereo"])
def test_a_short_echo_into_a_short_flanger_and_back(fmt):
    """Two slots without a reverb are one fused launch: a wavefront walks its instance's slots in order, through the mix buffer (never
    a cooperative workgroup).  A short echo in front of a short flanger, then the same pairs in the other order."""
    echoes = [c for c in rl.echo_cases() if c.rate == 48000]
    flangers = [c for c in rl.constant_delay_cases() + rl.moving_delay_cases() if c.type == desc.FLANGER and c.rate == 48000 and c.calls == rl.CALLS and c.props["feedback"] != 0.0]   # (without feedback the effect's output is 0)
    picks = [flangers[(7 * i) % len(flangers)] for i in range(len(echoes))]
    run(fmt, 48000, rl.CALLS, [[e, f] for e, f in zip(echoes, picks)], slots=2)
    run(fmt, 48000, rl.CALLS, [[f, e] for e, f in zip(echoes, picks)], slots=2, seed=50)


TAIL = (256, 256, 128)   # behind a case's own calls, which end on 256 frames: four whole-tile calls in a row


def test_unwaited_calls():
    """The echo and the chorus / flanger cases, moving delays included, through mix_device calls in a row with nothing waited for in
    between -- a case's own six calls (three rounds of them for the moving delays) and then 256, 256 and 128 frames -- against the same
    oracles.  With the test switch of test_gpu_chained.test_ring_light_effects_alone_chain the whole-tile calls are chained launches: a
    call that is no whole number of tiles goes in stream order and ends the run, so of a case's own calls only a round's last and the
    next round's first hand an instance on from one launch to the next; the four whole-tile calls at the end are one run of four
    launches, three hand-overs per instance, for the short-block echoes in their cooperative workgroups and for the delays with a
    request one tile ahead alike.  Where chained launches are switched off in the environment the calls are compared all the same, in
    stream order; where they are on, every whole-tile call must have been one."""
    import os
    import test_gpu_chained as chained
    from oalsfxpp_amd import lib
    base = int(os.environ.get("OALSFX_DEBUG_FLAGS", "0"), 0)
    chaining = os.environ.get("OALSFX_RING_MEMORY", "uncached") == "uncached" and not base & 0x400
    cases = rl.echo_cases() + rl.echo_group_cases() + rl.constant_delay_cases() + rl.moving_delay_cases()
    lib.load().oalsfx_debug_set_flags(base | chained.CHAIN_ALWAYS | chained.CHAIN_RING_LIGHT)
    try:
        for k, (rate, calls, instances) in enumerate(rl.batches(cases)):
            instances = rl.shuffled(instances, k)
            script = list(calls) + list(TAIL)
            with Batch(len(instances), desc.FMT_STEREO, rate, 1) as b:
                b.set_effect(0, [c.effect() for c in instances])
                b.apply_changes()
                shadows = {i: OracleShadow(b, i) for i in range(len(instances))}
                warm = np.zeros((len(instances), 256, 2), dtype=np.float32)
                b.mix(warm)   # (the parameters are in place: a call that has something to upload goes in stream order)
                for sh in shadows.values():
                    sh.mix(warm[0])
                before = b.chained_calls
                chained.run_device_calls(b, script, shadows, 9000 + 100 * k, replicas=False)
                if chaining:
                    whole = sum(1 for c in script if c % 64 == 0)
                    assert b.chained_calls - before == whole, f"{rate} Hz, {len(instances)} instances: {b.chained_calls - before} of {whole} whole-tile calls were chained launches"
                for i, sh in shadows.items():
                    d = sh.compare_state()
                    assert not d, f"{instances[i].name} (instance {i}, {rate} Hz): " + "; ".join(d[:6])
    finally:
        lib.load().oalsfx_debug_set_flags(base)
