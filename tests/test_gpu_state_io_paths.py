"""GPU: snapshot / restore / reset on the paths tests/test_gpu_state_io.py leaves out -- every effect type, every place on the ring-line
grid, targets of another size and the shards of a group, the other entry points next to a state call, formats, rates and slot counts,
and damaged blobs.

The reference is a CPU oracle shadow that has followed its voice since creation and goes with it across the restore
(harness.OracleShadow.follow): outputs on every call, slot states, delay lines and send-filter histories at the end, all on bits.  Where
a twin exists (the source batch going on) it is compared as well, as a second, independent check."""
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

from harness import ROOT, ShadowArmy, make_effect, preset_effect, same_bits, steady_build
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import BatchError, Group
from oalsfxpp_amd.workloads import CONFIG3_CHAIN, random_effect
from test_gpu_state_io import Inputs, host, kinds_setup, make, run, same_view, snapshot

pytestmark = pytest.mark.gpu

E = make_effect
FRAMES = 256
ALL_TYPES = list(range(12))


def _torch():
    import torch
    return torch


def same_out_nan(a, b, label, rows_a=None, rows_b=None):
    """Rows equal on bits by harness.same_bits, the rule the oracle comparisons go by: where both sides hold a NaN its sign and payload
    do not count (random properties at low rates give voices that put out NaNs).  Not test_gpu_state_io.same_out, which has no such rule."""
    a = a if rows_a is None else a[rows_a]
    b = b if rows_b is None else b[rows_b]
    bad = [k for k in range(len(a)) if not same_bits(a[k], b[k])[0]]
    assert not bad, f"{label}: rows {bad[:8]} differ"


def ring_sizes(b, instances):
    return [[b.read_ring(i, s).size for s in range(b.effect_count)] for i in instances]


def step(b, inp, armies, frames=FRAMES, label="", twin=None):
    """One mix_device call of `frames` on b, every followed instance of every army against its oracle; returns (input, output)."""
    x = inp.make(frames)
    y = host(b, run(b, [x], frames))[0]
    for army in armies:
        bad = army.differing(y, army.mix(x[0]))
        assert not bad, f"{label}: instances (instance, samples) {bad[:6]} differ from the oracle; plan {b.plan(0)}, kernel {b.last_reverb_kernel}"
    return x, y


def no_state_diffs(army, label):
    d = army.compare_state()
    assert not d, f"{label}: device state differs from the oracle: " + "; ".join(f"instance {i}: {v[:3]}" for i, v in list(d.items())[:4])


def random_chain(seed, slots, types=ALL_TYPES):
    rng = random.Random(seed)
    return [preset_effect(rng.randrange(113)) if (t := rng.choice(types)) == desc.EAX_REVERB and rng.random() < 0.5 else random_effect(rng, t)
            for _ in range(slots)]


def set_chains(b, chains):
    for s in range(b.effect_count):
        b.set_effect(s, [c[s] for c in chains])


# ---- B1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD])
def test_every_effect_type_through_snapshot_and_restore(fmt):
    """Item 1 (effect types).  All 12 types with random properties, in counts that give whole cooperative workgroups of four and every
    remainder; six calls (one ragged), a snapshot, a restore into a fresh batch in a shuffled order -- the cooperative workgroups of the
    target are composed of other instances than the source's --, six more calls.  Every instance is followed by its oracle across
    the restore; the source going on is the twin."""
    counts = {desc.EQUALIZER: 9, desc.DISTORTION: 6, desc.RING_MODULATOR: 7, desc.COMPRESSOR: 5, desc.ECHO: 2, desc.CHORUS: 3, desc.FLANGER: 3,
              desc.DEDICATED_DIALOG: 2, desc.DEDICATED_LFE: 2, desc.REVERB: 3, desc.EAX_REVERB: 5, desc.NULL: 1}
    assert sorted(counts) == ALL_TYPES
    types = [t for t, c in counts.items() for _ in range(c)]
    random.Random(31 + fmt).shuffle(types)
    n = len(types)
    effects = [random_effect(random.Random(1000 * fmt + i), t) for i, t in enumerate(types)]
    a = make(n, lambda b: b.set_effect(0, effects), fmt=fmt)
    inp = Inputs(n, a.channels, seed=40 + fmt)
    army = ShadowArmy(a)
    for k, frames in enumerate([256, 256, 100, 256, 256, 256]):
        step(a, inp, [army], frames, f"source call {k}")
    blob = snapshot(a)
    perm = list(range(n))
    random.Random(77 + fmt).shuffle(perm)
    assert [types[i] for i in np.argsort(perm)] != types, "the shuffle left the type order as it was"
    b = make(n, lambda _: None, fmt=fmt)
    b.restore(perm, blob.data_ptr(), blob.numel())
    army.follow(b, perm)
    for i in (0, 1, n // 2, n - 1):
        same_view(a, i, b, perm[i], "right after the restore")
    torch = _torch()
    for k, frames in enumerate([256, 333, 256, 64, 256, 256]):
        x = inp.make(frames)
        xb = np.empty_like(x[0])
        xb[perm] = x[0]
        ya = host(a, run(a, [x], frames))[0]
        yb = host(b, run(b, [(xb, torch.from_numpy(xb).cuda())], frames))[0]
        bad = army.differing(yb, army.mix(xb))
        assert not bad, f"restored call {k}: {bad[:6]} differ from the oracle"
        same_out_nan(ya, yb[perm], f"restored call {k} against the source going on")
    no_state_diffs(army, "after the continuation")
    a.close(); b.close()


# ---- B2 -----------------------------------------------------------------------------------------------------------------------------
# 256-frame calls a restored batch may take until plan() shows every reverb proven steady again.  The proof is the device's own note of a
# call in which the instance was at rest, read back with the next call: one call on the believing builds is what it takes, and one is what
# every case here was seen to take on an MI355X; 8 leaves room for presets whose gains need more blocks to come to rest.
PROVEN_WITHIN = 8


def steady_picks(fmt):
    """Presets for every build of the steady-state kernel, as test_every_build_of_the_steady_kernel picks them, and short-tap ones."""
    def span(i):
        p = lib.derive_slot(fmt, 48000, lib.effect_normalized(preset_effect(i))).u.reverb
        taps = list(p.early_tap) + list(p.early_ap_off) + list(p.early_line_off) + [t - p.late_feed_tap for t in p.late_tap] + \
            list(p.late_ap_off) + list(p.late_line_off)
        return min(taps), p.mod_depth != 0.0
    spans = {i: span(i) for i in range(113)}
    plain = [i for i, (d, m) in spans.items() if d >= 128 and not m][:3]
    close = [i for i, (d, m) in spans.items() if 64 <= d < 128 and not m][:2]
    modulated = [i for i, (d, m) in spans.items() if d >= 64 and m][:2]
    short = [i for i, (d, m) in spans.items() if d < 64][:2]
    assert plain and close and modulated, (plain, close, modulated)
    return plain + close + modulated + short


def until_proven(b, inp, armies, label, limit=PROVEN_WITHIN):
    for calls in range(limit + 1):
        if b.plan(0)[1] == b.n:
            return calls
        step(b, inp, armies, FRAMES, f"{label}, call {calls} on the way to proven")
    raise AssertionError(f"{label}: not proven steady within {limit} calls of 256 frames: plan {b.plan(0)}")


@pytest.mark.parametrize("p_src", [0, 1, 31, 32, 37, 63])
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO])
def test_restore_across_grid_phases(fmt, p_src):
    """Item 2 (position on the ring-line grid).  EAX and plain reverbs of presets for every steady build, proven steady in the source,
    snapshotted p_src frames past a multiple of 64, and restored -- all of them, or every other one beside reverbs of the target's own
    -- into targets whose frames_total is 0, 5, 32 or 59 past a multiple of 64 and which held chorus, echo and Null there before.  The
    target at phase 5 has mixed 5 frames in all, fewer than the image's frames_since_start: started_at wraps.  Every instance against
    its oracle on every call (the restored ones followed from the source) and against the source going on; once proven again, within
    PROVEN_WITHIN calls (the count is printed), the steady build's CR is 2 exactly when some listed reverb is off the 32-frame grid,
    worked out here from the frames each voice was given."""
    picks = steady_picks(fmt)
    effects = [preset_effect(i) for i in picks] + [preset_effect(i, desc.REVERB) for i in picks[:3]]
    n = len(effects)
    a = make(n, lambda b: b.set_effect(0, effects), fmt=fmt)
    inp = Inputs(n, a.channels, seed=100 * fmt + p_src)
    src_army = ShadowArmy(a)
    warm = until_proven(a, inp, [src_army], "source")
    assert a.plan(0)[1] == n
    src_frames = warm * FRAMES
    if p_src:
        step(a, inp, [src_army], p_src, "source, ragged call")
        src_frames += p_src
    assert src_frames % 64 == p_src
    blob_all = snapshot(a)
    half = list(range(0, n, 2))
    blob_half = snapshot(a, half)
    # the continuation, once: inputs, the source's outputs, the oracle's outputs
    sizes = [FRAMES] * PROVEN_WITHIN + [480, 65, FRAMES, FRAMES, FRAMES]
    targets = []
    for phase in (0, 5, 32, 59):
        for restored in (list(range(n)), half):
            own = [i for i in range(n) if i not in restored]
            before = [E([desc.CHORUS, desc.ECHO, desc.NULL][i % 3]) if i in restored else preset_effect((11 * i + phase) % 113) for i in range(n)]
            t = make(n, lambda b: b.set_effect(0, before), fmt=fmt)
            own_army = [ShadowArmy(t, own)] if own else []
            tin = Inputs(n, t.channels, seed=7 * phase + len(restored))
            t_frames = 0
            for frames in ([5] if phase == 5 else [256, 256] + ([phase] if phase else [])):
                step(t, tin, own_army, frames, f"target phase {phase} before the restore")
                t_frames += frames
            assert t_frames % 64 == phase and (phase != 5 or t_frames < src_frames)
            had = ring_sizes(t, restored)
            blob = blob_all if len(restored) == n else blob_half
            t.restore(restored, blob.data_ptr(), blob.numel())
            assert ring_sizes(t, restored) == ring_sizes(a, restored) != had, "no delay-line slab changed hands"
            targets.append((phase, restored, own, t, own_army, tin, t_frames))
    torch = _torch()
    proven_after = {}
    since = 0   # frames since the snapshot
    for k, frames in enumerate(sizes):
        if k < PROVEN_WITHIN and all(k > proven_after.get(key, k) + 1 for key in range(len(targets))):
            continue    # (every target is proven again and has run twice on its proven build: on to the ragged calls)
        x = inp.make(frames)
        ya = host(a, run(a, [x], frames))[0]
        ref = src_army.mix(x[0])
        assert not src_army.differing(ya, ref), f"source continuation call {k}"
        for key, (phase, restored, own, t, own_army, tin, t_frames) in enumerate(targets):
            label = f"target phase {phase}, {len(restored)} restored, call {k} ({frames} frames)"
            was_proven = t.plan(0)[1] == n
            if was_proven and key not in proven_after:
                proven_after[key] = k
            xt = tin.make(frames)[0]
            xt[restored] = x[0][restored]
            yt = host(t, run(t, [(xt, torch.from_numpy(xt).cuda())], frames))[0]
            bad = [i for i in restored if not same_bits(yt[i], ref[i])[0]]
            assert not bad, f"{label}: restored instances {bad} differ from the oracle; plan {t.plan(0)}, kernel {t.last_reverb_kernel}"
            same_out_nan(ya, yt, label + " against the source going on", rows_a=restored, rows_b=restored)
            for army in own_army:
                bad = army.differing(yt, army.mix(xt))
                assert not bad, f"{label}: the target's own instances {bad} differ from the oracle"
            targets[key] = (phase, restored, own, t, own_army, tin, t_frames + frames)
            if was_proven and frames == FRAMES:
                off = (src_frames + since) % 32 != 0 or (bool(own) and t_frames % 32 != 0)
                build = steady_build(t.last_reverb_kernel)
                assert build["cr"] == (2 if off else 0), f"{label}: CR {build['cr']} with reverbs {'off' if off else 'on'} the grid ({t.last_reverb_kernel})"
        since += frames
    assert len(proven_after) == len(targets), f"targets {sorted(set(range(len(targets))) - set(proven_after))} were not proven again within {PROVEN_WITHIN} calls"
    print(f"p_src {p_src}: proven again after {sorted(proven_after.values())} calls of 256 frames (bound {PROVEN_WITHIN})")
    for phase, restored, own, t, own_army, tin, _ in targets:
        d = {}
        for i in restored:      # (only these: a shadow that read another voice's parameters would take them for an update of its own)
            src_army.shadows[i].follow(t, i)
            d.update({i: v for v in [src_army.shadows[i].compare_state()] if v})
        assert not d, f"target phase {phase}, {len(restored)} restored: state differs from the oracle: {list(d.items())[:2]}"
        for army in own_army:
            no_state_diffs(army, f"target phase {phase}, own instances")
        t.close()
    a.close()


# ---- B3 -----------------------------------------------------------------------------------------------------------------------------
def test_migration_into_a_warmed_batch_of_another_size():
    """Item 3 (targets of another size).  17 instances of a 96-instance batch, listed unsorted and with gaps, move onto 17 of a warmed
    40-instance batch, listed unsorted: onto other types, rings of other size classes and Null.  The 23 others keep matching their own
    oracles, the 17 match the oracles that came with them from the source."""
    slots = 2
    a = make(96, lambda b: set_chains(b, [random_chain(500 + i, slots) for i in range(96)]), slots=slots)
    t = make(40, lambda b: set_chains(b, [random_chain(900 + i, slots, ALL_TYPES + [desc.NULL] * 4) for i in range(40)]), slots=slots)
    rng = random.Random(5)
    src_list, tgt_list = rng.sample(range(96), 17), rng.sample(range(40), 17)
    assert src_list != sorted(src_list) and tgt_list != sorted(tgt_list)
    untouched = [i for i in range(40) if i not in tgt_list]
    moved, own, rest = ShadowArmy(a, src_list), ShadowArmy(t, untouched), ShadowArmy(t, tgt_list)
    ia, it = Inputs(96, a.channels, seed=50), Inputs(40, t.channels, seed=51)
    for k, frames in enumerate([256, 256, 200, 256]):
        step(a, ia, [moved], frames, f"source call {k}")
    for k, frames in enumerate([256, 100, 256]):
        step(t, it, [own, rest], frames, f"target call {k}")
    had, brings = ring_sizes(t, tgt_list), ring_sizes(a, src_list)
    types_had = [[t.get_effect(i, s).type for s in range(slots)] for i in tgt_list]
    types_new = [[a.get_effect(i, s).type for s in range(slots)] for i in src_list]
    pairs = [(h, w, th, tn) for hs, ws, ths, tns in zip(had, brings, types_had, types_new) for h, w, th, tn in zip(hs, ws, ths, tns)]
    assert any(th != tn for _, _, th, tn in pairs), "no target held another type"
    assert any(h and w and h != w for h, w, _, _ in pairs), "no target held a ring of another size class"
    assert any(th == desc.NULL and tn != desc.NULL for _, _, th, tn in pairs), "no target held Null"
    blob = snapshot(a, src_list)
    t.restore(tgt_list, blob.data_ptr(), blob.numel())
    assert ring_sizes(t, tgt_list) == brings
    moved.follow(t, tgt_list)
    for k, frames in enumerate([256, 256, 77, 256, 256, 256]):
        step(t, it, [own, moved], frames, f"after the migration, call {k}")
    no_state_diffs(own, "untouched instances")
    no_state_diffs(moved, "migrated instances")
    a.close(); t.close()


def test_migration_between_the_shards_of_a_group():
    """Item 3 (the shards of a group).  Seven instances of shard 0 move onto seven of shard 1 through Group.batch; Group.mix then goes
    on matching the oracle for every instance in the global numbering."""
    n, slots = 40, 2
    with Group(n, [0, 0], effect_count=slots) as g:
        chains = [random_chain(300 + i, slots) for i in range(n)]
        for s in range(slots):
            g.set_effect(s, [c[s] for c in chains])
        g.apply_changes()
        (_, f0, c0), (_, f1, c1) = g.shards
        assert (f0, c0, f1, c1) == (0, 20, 20, 20)
        b0, b1 = g.batch(0), g.batch(1)
        assert (b0.n, b1.n, b0.channels, b0.effect_count) == (20, 20, g.channels, slots)
        rng = random.Random(9)
        src_list, tgt_list = rng.sample(range(20), 7), rng.sample(range(20), 7)
        armies = [ShadowArmy(b0), ShadowArmy(b1, [i for i in range(20) if i not in tgt_list]), ShadowArmy(b0, src_list), ShadowArmy(b1, tgt_list)]
        first = [f0, f1, f0, f1]
        r = np.random.default_rng(60)

        def call(frames, using, label):
            x = r.uniform(-1, 1, (n, frames, g.channels)).astype(np.float32)
            y = g.mix(x)
            for k in using:
                army, f = armies[k], first[k]
                bad = army.differing(y[f: f + 20], army.mix(x[f: f + 20]))
                assert not bad, f"{label}: shard instances {bad[:6]} differ from the oracle"
        for k, frames in enumerate([256, 256, 130]):
            call(frames, [0, 1, 2, 3], f"call {k}")
        blob = snapshot(b0, src_list)
        had = ring_sizes(b1, tgt_list)
        b1.restore(tgt_list, blob.data_ptr(), blob.numel())
        assert ring_sizes(b1, tgt_list) == ring_sizes(b0, src_list) != had
        armies[2].follow(b1, tgt_list)
        first[2] = f1
        for k, frames in enumerate([256, 256, 99, 256]):
            call(frames, [0, 1, 2], f"after the move, call {k}")
        for army in armies[:3]:
            no_state_diffs(army, "group")
        b0.close(); b1.close()
        g.mix(np.zeros((n, 64, g.channels), np.float32))    # closing a view leaves the group's batches alive


def test_one_image_forked_to_eight_targets():
    """Item 3 (forks).  One voice's image restored eight times from one blob, the forks then fed different inputs: each matches an oracle
    that ran beside the voice from the start (the oracle has no copy) and went with its fork."""
    slots = 2
    a = make(4, lambda b: set_chains(b, [[preset_effect(20 + i), E(desc.ECHO)] for i in range(4)]), slots=slots)
    c = make(12, kinds_setup(12, slots), slots=slots)
    forks = [10, 3, 7, 0, 11, 5, 2, 8]
    army = ShadowArmy(a, [2] * 8)
    own = ShadowArmy(c, [i for i in range(12) if i not in forks])
    ia, ic = Inputs(4, a.channels, seed=70), Inputs(12, c.channels, seed=71)
    for k, frames in enumerate([256, 256, 45, 256]):
        step(a, ia, [army], frames, f"source call {k}")
    for k in range(2):
        step(c, ic, [own], FRAMES, f"target call {k}")
    blob = snapshot(a, [2])
    for i in forks:
        c.restore([i], blob.data_ptr(), blob.numel())
    army.follow(c, forks)
    for k, frames in enumerate([256, 256, 300, 256]):
        _, y = step(c, ic, [own, army], frames, f"forks, call {k}")
        assert len({y[i].tobytes() for i in forks}) == 8, "the forks were not told apart by their inputs"
    no_state_diffs(army, "forks")
    a.close(); c.close()


# ---- B5 (b), (c) ---------------------------------------------------------------------------------------------------------------------
def test_state_calls_between_chained_runs_and_long_host_calls():
    """Item 5 (state io between the other entry points): (c) on the batch's own stream with nothing synchronised between -- 8 chained
    mix_device calls, a snapshot, 8 more, a restore from that blob, the same 8 inputs again: the second and third groups of outputs are
    identical, the first two match the oracle, and chained_calls shows that the runs on both sides of the state calls chained; (b)
    mix() of 5000 frames (2048-frame chunks) before a snapshot and after the restore."""
    torch = _torch()
    n = 1024
    a = make(n, lambda b: b.set_effect(0, [preset_effect(i % 113) for i in range(n)]))
    inp = Inputs(n, a.channels, seed=80)
    followed = list(range(0, n, 64))
    army = ShadowArmy(a, followed)
    for _ in range(8):
        step(a, inp, [army], FRAMES, "warm-up")
    first, second = [inp.make() for _ in range(8)], [inp.make() for _ in range(8)]
    nbytes = a.snapshot_bytes()
    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c0 = a.chained_calls
    o1 = run(a, first)
    c1 = a.chained_calls
    a.snapshot(None, blob.data_ptr(), nbytes)
    o2 = run(a, second)
    c2 = a.chained_calls
    a.restore(None, blob.data_ptr(), nbytes)
    o3 = run(a, second)
    c3 = a.chained_calls
    y1, y2, y3 = host(a, o1), host(a, o2), host(a, o3)
    print("chained calls per run of 8:", c1 - c0, c2 - c1, c3 - c2)
    # (whole runs, as test_gpu_chained.py counts them: calls - 1 at the least; the call behind the restore has every instance's parameters
    # to upload and goes in stream order, chain_eligible, so that run is allowed one call more)
    assert c1 - c0 >= 7 and c2 - c1 >= 7 and c3 - c2 >= 6, f"a run beside the state calls did not chain as a whole: {c1 - c0}, {c2 - c1}, {c3 - c2} of 8 calls each"
    for k in range(8):
        assert not army.differing(y1[k], army.mix(first[k][0])), f"first run, call {k}"
    for k in range(8):
        assert not army.differing(y2[k], army.mix(second[k][0])), f"second run, call {k}"
        same_out_nan(y2[k], y3[k], f"the run behind the restore against the run behind the snapshot, call {k}")
    army.follow(a, followed)    # (the same instances, renumbered by the restore)
    no_state_diffs(army, "rolled back and run again")
    # (b)
    r = np.random.default_rng(81)
    x = r.uniform(-1, 1, (n, 5000, a.channels)).astype(np.float32)
    assert not army.differing(a.mix(x), army.mix(x)), "mix of 5000 frames"
    blob = snapshot(a)
    b = make(n, lambda _: None)
    b.restore(None, blob.data_ptr(), blob.numel())
    army.follow(b, followed)
    x = r.uniform(-1, 1, (n, 5000, a.channels)).astype(np.float32)
    ya, yb = a.mix(x), b.mix(x)
    assert not army.differing(yb, army.mix(x)), "mix of 5000 frames after the restore"
    same_out_nan(ya, yb, "5000 frames against the source going on")
    no_state_diffs(army, "after 5000 frames")
    a.close(); b.close()


# ---- B6 -----------------------------------------------------------------------------------------------------------------------------
FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_5POINT1_REAR, desc.FMT_6POINT1, desc.FMT_7POINT1]
CONTINUATIONS = [(f, 44100, 2) for f in FORMATS] + [(desc.FMT_STEREO, r, 2) for r in (8000, 11025, 96000, 192000)] + [(desc.FMT_STEREO, 48000, 4)]


@pytest.mark.parametrize("fmt, rate, slots", CONTINUATIONS)
def test_continuation_across_formats_rates_and_slot_counts(fmt, rate, slots):
    """Item 7 (formats, rates, slots).  Every channel format at 44.1 kHz with two slots, stereo from 8 to 192 kHz, and the four-slot chain
    chorus, flanger, echo, EAX reverb with send filters on some sends: a continuation in a fresh batch, oracle-followed."""
    n = 10
    if slots == 4:
        chains = [[random_effect(random.Random(10 * i + s), t) for s, t in enumerate(CONFIG3_CHAIN)] for i in range(n)]
    else:
        chains = [random_chain(700 + 13 * fmt + i + rate, slots) for i in range(n)]

    def setup(b):
        set_chains(b, chains)
        b.set_send_props(-1, 0.9, 0.5, 0.8, first=0, count=n // 2)
        b.set_send_props(slots - 1, 0.8, 0.6, 0.9, first=n // 4, count=n // 2)
        b.set_send_props(0, 0.7, 1.0, 0.4, first=n - 3, count=2)
    a = make(n, setup, fmt=fmt, slots=slots, rate=rate)
    army = ShadowArmy(a)
    inp = Inputs(n, a.channels, seed=90 + fmt + slots)
    for k, frames in enumerate([256, 256, 90, 256]):
        step(a, inp, [army], frames, f"source call {k}")
    blob = snapshot(a)
    b = make(n, lambda _: None, fmt=fmt, slots=slots, rate=rate)
    b.restore(None, blob.data_ptr(), blob.numel())
    army.follow(b, range(n))
    for k, frames in enumerate([256, 256, 123, 256]):
        x, yb = step(b, inp, [army], frames, f"restored call {k}")
        same_out_nan(host(a, run(a, [x], frames))[0], yb, f"restored call {k} against the source going on")
    no_state_diffs(army, "after the continuation")
    for i in (0, n - 1):
        same_view(a, i, b, i, "after the continuation")
    a.close(); b.close()


# ---- B7 -----------------------------------------------------------------------------------------------------------------------------
HEADER = "<IIiiiiQQQQQ"     # BlobHeader (hip/batch.cpp): magic, version, format, rate, slots, count, total, table, prefix, device stride, host stride
H_VERSION, H_COUNT, H_TOTAL, H_TABLE, H_PREFIX, H_DEVICE_STRIDE, H_HOST_STRIDE = 1, 5, 6, 7, 8, 9, 10
ENTRY_BYTES = 8 * (2 + desc.MAX_SLOTS)      # BlobEntry: host, device, ring[MAX_SLOTS]
EFFECT_BYTES, SEND_BYTES = C.sizeof(desc.Effect), C.sizeof(desc.SendProps)
BLOB_SLOT_AT = 2 * desc.MAX_SLOTS * EFFECT_BYTES + (2 + 2 * desc.MAX_SLOTS) * SEND_BYTES     # BlobHost::slot
LAYOUT, RECORDS = "layout is damaged", "records are damaged"


def damaged_blobs(good, n):
    """(what, blob bytes, bytes given, message) with one layout field changed each; only fields oalsfx_batch_restore checks on the host
    before anything is queued (hip/batch.cpp).  Device records, delay lines and effect properties are left alone: nothing validates them."""
    hdr = list(struct.unpack_from(HEADER, good))
    table, prefix, total = hdr[H_TABLE], hdr[H_PREFIX], hdr[H_TOTAL]
    out = []

    def header(what, field, value, message, given=None):
        h = list(hdr)
        h[field] = value
        blob = bytearray(good)
        struct.pack_into(HEADER, blob, 0, *h)
        out.append((what, blob, len(good) if given is None else given, message))

    def word(what, offset, fmt, value, message):
        blob = bytearray(good)
        struct.pack_into(fmt, blob, offset, value)
        out.append((what, blob, len(good), message))
    header("version", H_VERSION, 2, "version is not supported")
    header("count", H_COUNT, n - 1, "another number of instances")
    header("total_bytes above bytes", H_TOTAL, total + 256, "larger than the bytes")
    header("table_offset", H_TABLE, table + 256, LAYOUT)
    header("host_stride", H_HOST_STRIDE, hdr[H_HOST_STRIDE] + 256, LAYOUT)
    header("device_stride", H_DEVICE_STRIDE, hdr[H_DEVICE_STRIDE] - 256, LAYOUT)
    header("prefix_bytes above total_bytes", H_PREFIX, total + 256, LAYOUT)
    header("prefix_bytes inside the entry table", H_PREFIX, table + 16, LAYOUT)
    k = 3   # the entry that is damaged
    e_host, e_device, e_ring0 = struct.unpack_from("<QQQ", good, table + k * ENTRY_BYTES)
    assert e_ring0, "the damaged entry's slot holds a ring"
    for name, at, value in (("host", 0, e_host), ("device", 8, e_device), ("ring[0]", 16, e_ring0)):
        message = RECORDS if name == "ring[0]" else LAYOUT
        word(f"entry {name} out of range", table + k * ENTRY_BYTES + at, "<Q", total + 4096, message)
        word(f"entry {name} misaligned by 8", table + k * ENTRY_BYTES + at, "<Q", value + 8, message)
    word("entry host below the table", table + k * ENTRY_BYTES, "<Q", 0, LAYOUT)
    word("entry device inside the prefix", table + k * ENTRY_BYTES + 8, "<Q", e_host, LAYOUT)
    word("ring[0] == 0 for a slot with a ring", table + k * ENTRY_BYTES + 16, "<Q", 0, RECORDS)
    slot0 = e_host + BLOB_SLOT_AT
    s_type, s_floats = struct.unpack_from("<iI", good, slot0)
    assert s_type == desc.EAX_REVERB and s_floats == lib.load().oalsfx_host_ring_floats(desc.EAX_REVERB, 48000), "BlobHost layout as assumed"
    assert struct.unpack_from("<i", good, e_host)[0] == desc.EAX_REVERB
    word("BlobSlot.type out of range", slot0, "<i", 12, RECORDS)
    word("BlobSlot.type negative", slot0, "<i", -1, RECORDS)
    word("BlobSlot.type unequal to active.type", slot0, "<i", desc.REVERB, RECORDS)
    word("BlobSlot.ring_floats not the type's", slot0 + 4, "<I", s_floats - 64, RECORDS)
    word("BlobSlot.ring_floats zero", slot0 + 4, "<I", 0, RECORDS)
    return out


def test_damaged_blobs_are_refused_on_the_host():
    """Item 8 (damaged blobs).  One layout field of a good blob changed per case -- header fields, an entry's offsets (out of range,
    misaligned by 8, no ring where the slot has one), a slot record's type and ring size --: restore answers with the message it has
    for the case, and the target goes on like its twin."""
    torch = _torch()
    n = 16
    a = make(n, lambda b: b.set_effect(0, [preset_effect((3 * i) % 113) for i in range(n)]))
    inp = Inputs(n, a.channels, seed=110)
    host(a, run(a, [inp.make() for _ in range(3)]))
    good = snapshot(a).cpu().numpy().tobytes()
    target, twin = make(n, kinds_setup(n, 1)), make(n, kinds_setup(n, 1))
    warm = [inp.make() for _ in range(2)]
    host(target, run(target, warm)); host(twin, run(twin, warm))
    cases = damaged_blobs(good, n)
    assert len(cases) >= 20
    for what, blob, given, message in cases:
        dev = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
        with pytest.raises(BatchError, match=message):
            target.restore(None, dev.data_ptr(), given)
    xs = [inp.make() for _ in range(3)]
    yt, yw = host(target, run(target, xs)), host(twin, run(twin, xs))
    for k in range(3):
        same_out_nan(yt[k], yw[k], f"refused target, call {k}")
    for i in range(n):
        same_view(target, i, twin, i, "refused target")
    # and the undamaged blob is taken
    dev = torch.from_numpy(np.frombuffer(good, dtype=np.uint8).copy()).cuda()
    target.restore(None, dev.data_ptr(), len(good))
    for i in (0, 3, n - 1):
        same_view(a, i, target, i, "the good blob")
    for b in (a, target, twin):
        b.close()


# ---- B5 (a) --------------------------------------------------------------------------------------------------------------------------
def async_child(form, middle):
    """Runs in a process of its own (the pipeline form is cached per process): three mix_async calls from page-locked buffers, with no
    wait() a snapshot or a restore, three more, wait()."""
    torch = _torch()
    n = 256
    a, twin = make(n, kinds_setup(n, 1)), make(n, kinds_setup(n, 1))
    followed = list(range(0, n, 8))
    army = ShadowArmy(a, followed)
    army.sync()     # (descriptor read-backs wait for the batch: all of them before anything is in flight)
    r = np.random.default_rng(120)
    xs, ys = [a.pinned_array(FRAMES) for _ in range(6)], [a.pinned_array(FRAMES) for _ in range(6)]
    for x in xs:
        x[:] = r.uniform(-1, 1, x.shape).astype(np.float32)
    for x in xs[:3]:
        twin.mix(x)
    want = snapshot(twin)       # taken idle
    nbytes = want.numel()
    got = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(3):
        a.mix_async(xs[k], ys[k])
    if middle == "snapshot":
        a.snapshot(None, got.data_ptr(), nbytes)
    else:
        a.restore(None, want.data_ptr(), nbytes)    # the state the three calls in flight lead to: restored too early, they would run over it
    for k in range(3, 6):
        a.mix_async(xs[k], ys[k])
    a.wait()
    a.synchronize()
    assert a.host_pipeline()[0] == form, f"pipeline form {a.host_pipeline()[0]}, not {form}"
    for k in range(6):
        ref = np.stack(list(army.pool.map(lambda s: s.oracle.mix(xs[k][s.instance]), army.shadows)))
        bad = army.differing(ys[k], ref)
        assert not bad, f"{middle}, form {form}: call {k}: {bad[:6]} differ from the oracle"
    if middle == "snapshot":
        hdr = struct.unpack_from(HEADER, want[:256].cpu().numpy().tobytes())
        prefix, stride = hdr[H_PREFIX], hdr[H_DEVICE_STRIDE]
        for blob in (got, want):
            blob[prefix: prefix + n * stride].view(n, stride)[:, :4] = 0     # the slot state's update stamp
        torch.cuda.synchronize()
        assert torch.equal(got[prefix: prefix + n * stride], want[prefix: prefix + n * stride]), "device records differ from the idle twin's snapshot"
        assert torch.equal(got[prefix + n * stride:], want[prefix + n * stride:]), "delay lines differ from the idle twin's snapshot"
        c = make(n, lambda _: None)
        c.restore(None, got.data_ptr(), nbytes)
        for i in (0, 1, n - 1):
            same_view(c, i, twin, i, "restored from the snapshot taken between mix_async calls")
        c.close()
    else:
        army.follow(a, followed)
    no_state_diffs(army, f"{middle}, form {form}")
    a.close(); twin.close()
    print("async child ok")


@pytest.mark.parametrize("middle", ["snapshot", "restore"])
@pytest.mark.parametrize("form", [1, 3])
def test_state_calls_between_mix_async_calls(form, middle):
    """Item 5 (state io between the other entry points), (a): a snapshot, or a restore, between mix_async calls whose copies out are
    still pending, on three streams (form 3) and on one (form 1).  The blob equals an idle twin's snapshot after three synchronous
    calls -- device records with the update stamps masked, and delay lines --, all six outputs match the oracle, and so does the state
    at the end; the child asserts the pipeline form it ran in (host_pipeline)."""
    code = f"import test_gpu_state_io_paths as t; t.async_child({form}, {middle!r})"
    env = dict(os.environ, OALSFX_HOST_PIPELINE=str(form), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import torch\n" + code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "async child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- B4 -----------------------------------------------------------------------------------------------------------------------------
class PoolDevice:
    """The device side of tests/voice_pool.py's schedule: makes the calls and holds every result to what the pool expects."""

    def __init__(self, b):
        import voice_pool
        from oalsfxpp_amd.api import METER_DTYPE
        self.b, self.vp, self.dtype = b, voice_pool, METER_DTYPE
        self.vm, self.bm = np.zeros(voice_pool.N, METER_DTYPE), np.zeros(voice_pool.BUSES, METER_DTYPE)
        self.queued = []
        self.sizes_seen = set()

    def apply(self, started, routing):
        """reset, set_effect_at, set_send_props, apply_changes (and set_routing, and the records zeroed, unless the caller defers them)."""
        if started:
            voices = [v[0] for v in started]
            if routing is not None:     # (read-backs wait for the batch: none inside a run)
                self.sizes_seen.update(z for row in ring_sizes(self.b, voices) for z in row)
            self.b.reset(voices)
            if routing is not None:
                assert all(z == 0 for row in ring_sizes(self.b, voices) for z in row), "a reset voice kept a delay line"
            for s in range(self.vp.SLOTS):
                self.b.set_effect_at(s, voices, [v[1][s] for v in started])
            for i, _, direct, aux, _, _ in started:
                if direct:
                    self.b.set_send_props(-1, *direct, first=i, count=1)
                if aux:
                    self.b.set_send_props(*aux, first=i, count=1)
            self.b.apply_changes()
            for i, effects, *_ in started:
                assert [self.b.get_effect(i, s).type for s in range(self.vp.SLOTS)] == [e.type for e in effects]
            if routing is not None:
                for i in voices:
                    self.vm[i] = np.zeros((), self.dtype)
        if routing is not None:
            self.b.set_routing(*routing)

    def expect_records(self, label, want_v, want_b):
        import meter_ref
        assert meter_ref.same_records(self.vm, want_v), f"{label}: voice records: {meter_ref.first_difference(self.vm, want_v)}"
        assert meter_ref.same_records(self.bm, want_b), f"{label}: bus records: {meter_ref.first_difference(self.bm, want_b)}"

    def host_call(self, k, x, buses, want_v, want_b, threshold):
        from downmix_ref import same_bits as same
        got, _, _ = self.b.mix_downmix_meter(x, self.vp.BUSES, threshold, carry=True, voice_meters=self.vm, bus_meters=self.bm)
        assert same(got, buses), f"call {k} ({x.shape[1]} frames): the buses differ from the downmix of the oracles' outputs"
        self.expect_records(f"call {k} ({x.shape[1]} frames)", want_v, want_b)
        return self.vm

    def queue(self, x):
        torch = _torch()
        d = torch.from_numpy(x).cuda()
        o = torch.empty_like(d)
        self.b.mix_device(x.shape[1], d.data_ptr(), o.data_ptr())   # (own stream, nothing synchronised: a recycle may follow at once)
        self.queued.append((d, o))

    def finish_run(self, k, calls, threshold):
        from downmix_ref import same_bits as same
        torch = _torch()
        n, nb = self.vp.N, self.vp.BUSES
        self.b.synchronize()
        torch.cuda.synchronize()
        vm_t, bm_t = torch.from_numpy(self.vm.view(np.uint8).copy()).cuda(), torch.from_numpy(self.bm.view(np.uint8).copy()).cuda()
        for j, ((d, o), (x, y, buses, want_v, want_b, bus, gain, mid)) in enumerate(zip(self.queued, calls)):
            label = f"call {k + j} (mix_device, call {j} of its run)"
            got = o.cpu().numpy()
            bad = [i for i in range(n) if not same_bits(got[i], y[i])[0]]
            assert not bad, f"{label}: voices {bad[:8]} differ from their oracles (recycled inside the run: {mid})"
            if mid:     # the voices recycled in front of this call: their records start over, their routing is the new one
                vm_t.view(n, -1)[mid] = 0
            torch.cuda.synchronize()
            self.b.set_routing(bus, gain)
            out = torch.empty((nb,) + tuple(d.shape[1:]), dtype=torch.float32, device="cuda")
            self.b.downmix_device(x.shape[1], o.data_ptr(), nb, out.data_ptr())
            self.b.meter_device(n, x.shape[1], o.data_ptr(), vm_t.data_ptr(), threshold, carry=True)
            self.b.meter_device(nb, x.shape[1], out.data_ptr(), bm_t.data_ptr(), threshold, carry=True)
            self.b.synchronize()
            assert same(out.cpu().numpy(), buses), f"{label}: the buses differ from the downmix of the oracles' outputs"
            self.vm, self.bm = vm_t.cpu().numpy().view(self.dtype).copy(), bm_t.cpu().numpy().view(self.dtype).copy()
            self.expect_records(label, want_v, want_b)
        self.queued = []
        return self.vm


def test_voice_pool_life_cycle():
    """Item 4 (ring slab recycling) and the life cycle reset, bus downmix and meters were built for.  64 voices, stereo, two slots, 3
    buses, 80 calls (two of 441 frames and one of 2500 through mix_downmix_meter, so the 2048-frame chunks meet the meters): a seeded
    schedule (tests/voice_pool.py) starts voices -- reset, set_effect_at with any of the 12 types and EAX presets, set_send_props on some,
    apply_changes, set_routing --, feeds them noise for two to four calls and then silence, and the device's own quiet_run (carried;
    threshold 0.01) frees a voice at 512 frames; half the recycled voices come back with another type.  On every call: the voices
    against an OracleApi created afresh at each reset (directly in the mix_device stretch, calls 24-55, through buses and records
    elsewhere), the buses against downmix_ref of the oracles' outputs, voice and bus records against meter_ref with carry.
    The schedule's conditions are asserted from the schedule (voice_pool.conditions), and beforehand on the CPU
    (test_the_voice_pool_schedule_meets_its_conditions): starts per type [26, 43, 67, 39, 37, 45, 78, 53, 51, 49, 28, 41], 493 recycles
    (255 with another type), ring size classes released / retaken 1024: 107 / 103, 4096: 109 / 122, 32768: 153 / 148, 235520: 114 /
    119, and 76 recycles between two consecutive mix_device calls on the batch's stream with nothing synchronised between them.  (Such
    calls of 64 two-slot voices do not overlap on the device: the host chains two-slot steps from 4093 instances on, so chained_calls
    stays 0 here; the state calls inside runs that do chain are test_state_calls_between_chained_runs_and_long_host_calls.)"""
    import voice_pool
    b = make(voice_pool.N, lambda _: None, slots=voice_pool.SLOTS)
    pool, dev = voice_pool.VoicePool(), PoolDevice(b)
    counts = voice_pool.drive(pool, dev)
    print(counts, "; chained calls", b.chained_calls)
    classes = {voice_pool.ring_class(t) for t in range(12)} - {0}
    assert classes <= dev.sizes_seen, f"slabs given back at resets: {sorted(dev.sizes_seen)}, not every class of {sorted(classes)}"
    assert pool.recycles == 493 and pool.mid_run == 76, "the device's records led to another schedule than the one worked out on the CPU"
    b.close()
