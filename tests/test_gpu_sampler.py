"""GPU: the samplers (oalsfx_batch_set_samplers, _get_samplers, _sample_device, _play_downmix_meter and the ApiArray form;
include/oalsfx_hip.h, "samplers") against their NumPy restatement (tests/sampler_ref.py), and behind it against OracleApi, downmix_ref
and meter_ref.  Every comparison is on the bit patterns (NaNs by position) and on the exact integers; there is no tolerance anywhere.  No
test provokes a device fault: every refusal is decided on the host."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import meter_ref
import sampler_ref as ref
from downmix_ref import downmix
from harness import ROOT, OracleApi, ShadowArmy, preset_effect, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, SAMPLER_DTYPE, Batch, BatchError, Group
from oalsfxpp_amd.workloads import random_effect
from test_sampler_abi import random_records, rec

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = ref.ONE
FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_5POINT1_REAR, desc.FMT_6POINT1, desc.FMT_7POINT1]
FRAMES = [0, 1, 63, 64, 65, 256, 441, 2500]
GUARD = 64                      # floats in front of and behind a rendered buffer that must stay as they were
CHAIN_ALWAYS = 0x8000           # OALSFX_DEBUG_FLAGS: chained launches for short calls of small batches too


def _torch():
    import torch
    return torch


class Assets:
    """A pool of assets [(format, channels, PCM)] in device memory, each a tensor of its own, alive as long as this object."""

    def __init__(self, pool):
        torch = _torch()
        self.pool = pool
        self.tensors = [torch.from_numpy(np.ascontiguousarray(pcm)).cuda() for _, _, pcm in pool]
        torch.cuda.synchronize()

    def address(self, key):
        return self.tensors[key].data_ptr()

    def fill_in(self, records, keys):
        records["data"] = [self.address(k) for k in keys]
        return records


def playing(rng, n, channels, **kw):
    """n random playing records with their assets on the device: (records, the PCM of every record, Assets)."""
    records, pcm, keys, pool = random_records(rng, n, channels, **kw)
    assets = Assets(pool)
    return assets.fill_in(records, keys), pcm, assets


def device_render(b, frames, offset=0, stream=None):
    """One sample_device call into a buffer `offset` floats off its allocation; returns [n][frames][channels].  The floats around the
    buffer must be untouched."""
    torch = _torch()
    count = b.n * frames * b.channels
    buf = torch.full((GUARD + offset + count + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.sample_device(frames, buf.data_ptr() + 4 * (GUARD + offset), stream=stream)
    b.synchronize()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD + offset] == -7.5).all() and (host[GUARD + offset + count:] == -7.5).all(), "the render wrote outside its buffer"
    return host[GUARD + offset:GUARD + offset + count].reshape(b.n, frames, b.channels).copy()


def expect_output(got, want, label):
    ok, nbad = ref.same_floats(got, want)
    if not ok:
        rows = np.nonzero(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError(f"{label}: {nbad} samples differ, instances {rows[:8].tolist()}")


def expect_records(got, want, label):
    for field in SAMPLER_DTYPE.names:
        a, w = got[field], want[field]
        same = ref.same_floats(a, w)[0] if field == "gain" else bool((a == w).all())
        assert same, f"{label}: field {field} differs at instances {np.nonzero((a != w).reshape(len(got), -1).any(axis=1))[0][:8].tolist()}"


def run_calls(b, records, pcm, sizes, label, **kw):
    """set_samplers, then one render per size, each against the restatement, with get_samplers after every call."""
    b.set_samplers(records)
    expect_records(b.get_samplers(), records, f"{label}: as set")
    state = records
    for frames in sizes:
        want, state = ref.render(state, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        expect_output(got, want, f"{label}, {frames} frames")
        expect_records(b.get_samplers(), state, f"{label}, after {frames} frames")
    return state


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [1, 70])
def test_formats_layouts_and_frames(fmt, n):
    """Every PCM format x mono / wide asset x nearest / linear x looped / one-shot, taken in turn over the instances (n = 1: drawn), random
    steps with 4096 and 0 among them, random positions and gains; the calls continue one another."""
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(100 * fmt + n)
    with Batch(n, fmt, 48000, 1) as b:
        for trial in range(6 if n == 1 else 1):
            records, pcm, assets = playing(rng, n, ch, assets_per_format=1, cycle=n > 1, asset_frames=(1, 3000))
            if n > 1:
                combos = {(int(r["format"]), int(r["channels"]) == 1, int(r["flags"])) for r in records}
                assert len(combos) == 3 * (1 if ch == 1 else 2) * 4, combos
                assert (records["step"] == ONE).any() and (records["step"] == 0).any()
            run_calls(b, records, pcm, FRAMES, f"format {fmt}, n {n}, trial {trial}")


@pytest.mark.parametrize("fmt, sizes", [(desc.FMT_STEREO, FRAMES), (desc.FMT_7POINT1, [65, 256]), (desc.FMT_MONO, [441])])
def test_4096_instances_on_a_few_assets(fmt, sizes):
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(7 + fmt)
    with Batch(4096, fmt, 48000, 1) as b:
        records, pcm, assets = playing(rng, 4096, ch, assets_per_format=2, asset_frames=(200, 20000))
        assert len(set(records["data"].tolist())) <= 12           # many samplers on one asset
        after = run_calls(b, records, pcm, sizes, f"4096 instances, format {fmt}")
        if fmt == desc.FMT_STEREO:
            finished = (after["flags"] & ref.PLAYING) == 0
            assert finished.any() and not finished.all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_buffers_at_odd_float_offsets(fmt):
    """Destinations 4, 8, 12, ... bytes off the allocation: every store width is taken, and the output is the same whatever it is."""
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(50 + fmt)
    with Batch(70, fmt, 48000, 1) as b:
        records, pcm, assets = playing(rng, 70, ch, assets_per_format=1, cycle=True)
        records["flags"][::9] = 0               # some stopped rows: their zeros go through the same stores
        want, _ = ref.render(records, pcm, 300, ch)
        for offset in (0, 1, 2, 3, 4, 5, 6):
            b.set_samplers(records)
            expect_output(device_render(b, 300, offset=offset), want, f"format {fmt}, offset {offset}")


def test_special_values_at_known_places():
    torch = _torch()
    pcm = np.asarray([1.0, np.inf, 2.0, -0.0, -0.0, 1e-39, np.nan, 3e38, -3e38, 0.5], f32).reshape(-1, 1)
    asset = torch.from_numpy(pcm).cuda()
    cases = [rec(format=ref.PCM_F32, frames=10, flags=ref.PLAYING | ref.LINEAR),                      # Inf neighbour at m == 0: NaN
             rec(format=ref.PCM_F32, frames=10),                                                     # ... and without LINEAR: as stored
             rec(format=ref.PCM_F32, frames=10, flags=ref.PLAYING | ref.LINEAR, position=3 * ONE, step=ONE // 3),   # -0 + +0; denormals
             rec(format=ref.PCM_F32, frames=10, position=5 * ONE, step=0, gain=0.5),                  # a denormal that stays one
             rec(format=ref.PCM_F32, frames=10, gain=np.nan),
             rec(format=ref.PCM_F32, frames=10, gain=0.0, position=ONE),                              # 0 * Inf
             rec(format=ref.PCM_F32, frames=10, flags=ref.PLAYING | ref.LINEAR, position=7 * ONE, step=ONE // 2),   # 3e38 - -3e38 overflows
             rec(format=ref.PCM_F32, frames=10, gain=-1.0, position=3 * ONE),                          # -0 * -1 = +0
             rec(format=ref.PCM_F32, frames=10, flags=ref.LINEAR | ref.LOOP, gain=np.nan),             # stopped: +0.0f whatever the gain
             rec(format=ref.PCM_F32, frames=10, flags=ref.PLAYING | ref.LINEAR | ref.LOOP, loop_start=9, loop_end=10, position=9 * ONE + 1, step=5 * ONE + 7)]
    records = np.concatenate(cases)
    records["data"] = asset.data_ptr()
    with Batch(len(cases), desc.FMT_STEREO, 48000, 1) as b:
        after = run_calls(b, records, [pcm] * len(cases), [70, 3], "special values")
        out, _ = ref.render(records, [pcm] * len(cases), 12, 2)
        assert np.isnan(out[0, 0, 0]) and out[1, 1, 0] == np.inf and out[3, 0, 0] == f32(f32(1e-39) * f32(0.5)) != 0
        assert (after["flags"][:8] & ref.PLAYING).tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and after["flags"][9] & ref.PLAYING


def test_a_run_of_unsynchronised_calls():
    """Six renders of mixed sizes queued without a wait, set_samplers on a few voices between two pairs of them: outputs and records are
    the restatement's, voices that finish in mid-call are silent from that frame on and read back as finished, and records go to the
    device only in front of the renders that followed a set_samplers."""
    torch = _torch()
    n, ch = 130, 2
    rng = np.random.default_rng(31)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        records, pcm, assets = playing(rng, n, ch, asset_frames=(300, 2500))
        fresh, fresh_pcm = np.zeros(20, SAMPLER_DTYPE), [None] * 20           # twenty records on assets of the pool already on the device
        pool_keys = rng.integers(0, len(assets.pool), 20)
        for k, key in enumerate(pool_keys):
            fmt, width, data = assets.pool[key]
            fresh[k] = rec(format=fmt, channels=width, frames=data.shape[0], step=int(rng.integers(0, 3 * ONE)), position=int(rng.integers(0, data.shape[0])) * ONE,
                           flags=ref.PLAYING | (ref.LINEAR if k % 2 else 0), data=assets.address(key))[0]
            fresh[k]["gain"][:ch] = rng.uniform(-1, 1, ch)
            fresh_pcm[k] = data
        changes = {2: (list(range(5, 15)), fresh[:10], fresh_pcm[:10]), 4: ([0, 129, 64, 3, 77, 100, 101, 102, 9, 50], fresh[10:], fresh_pcm[10:])}
        sizes = [256, 64, 441, 1, 2500, 256]
        uploads = b.sampler_uploads()
        b.set_samplers(records)
        state, pcm = records.copy(), list(pcm)
        bufs, wants = [], []
        for k, frames in enumerate(sizes):
            if k in changes:
                voices, new, new_pcm = changes[k]
                b.set_samplers(new, instances=voices)
                state[voices] = new
                for v, p in zip(voices, new_pcm):
                    pcm[v] = p
            want, state = ref.render(state, pcm, frames, ch)
            buf = torch.empty((n, frames, ch), dtype=torch.float32, device="cuda")
            b.sample_device(frames, buf.data_ptr())
            bufs.append(buf)
            wants.append(want)
        assert b.sampler_uploads() - uploads == 3, "records went to the device in front of a render that followed no set_samplers"
        expect_records(b.get_samplers(), state, "after the run")            # (waits for the renders)
        b.synchronize()
        finished_in_mid_call = 0
        for k, (buf, want) in enumerate(zip(bufs, wants)):
            got = buf.cpu().numpy()
            expect_output(got, want, f"call {k} ({sizes[k]} frames)")
            silent_tail = (got[:, -1, :] == 0).all(axis=1) & (np.abs(got[:, 0, :]) > 0).any(axis=1)
            finished_in_mid_call += int(silent_tail.sum())
        finished = (state["flags"] & ref.PLAYING) == 0
        assert finished.any() and not finished.all() and finished_in_mid_call > 0
        assert (state["position"][finished] == state["frames"][finished].astype(np.uint64) * ONE).all()
        # nothing was set since: nothing goes to the device
        b.sample_device(64, bufs[0].data_ptr())
        b.synchronize()
        assert b.sampler_uploads() - uploads == 3
        # a caller's stream, then the batch's own again: the renders stay in order
        side = torch.cuda.Stream()
        a0, a1 = torch.empty((n, 100, ch), dtype=torch.float32, device="cuda"), torch.empty((n, 100, ch), dtype=torch.float32, device="cuda")
        _, state = ref.render(state, pcm, 64, ch)
        b.sample_device(100, a0.data_ptr(), stream=side.cuda_stream)
        b.sample_device(100, a1.data_ptr())
        w0, state = ref.render(state, pcm, 100, ch)
        w1, state = ref.render(state, pcm, 100, ch)
        expect_records(b.get_samplers(), state, "after renders on two streams")
        side.synchronize()
        b.synchronize()
        expect_output(a0.cpu().numpy(), w0, "on a caller's stream")
        expect_output(a1.cpu().numpy(), w1, "on the batch's stream behind it")


@pytest.fixture
def chain_small_batches():
    so = lib.load()
    base = int(os.environ.get("OALSFX_DEBUG_FLAGS", "0"), 0)
    so.oalsfx_debug_set_flags(base | CHAIN_ALWAYS)
    yield
    so.oalsfx_debug_set_flags(base)


def eleven_type_effects(n, slot):
    return [random_effect(random.Random(1000 * slot + i), (i + 3 * slot) % 12) if (i + 3 * slot) % 12 != desc.EAX_REVERB else preset_effect((7 * i) % 113)
            for i in range(n)]


@pytest.mark.parametrize("kind", ["proven reverbs", "eleven types", "two slots"])
def test_end_to_end_against_the_oracle(kind, chain_small_batches):
    """sample_device -> mix_device -> downmix_device -> meter_device with carry, all on the batch's stream, three buffers a round (the three
    mix_device calls of a round may overlap one another).  Expected: the restatement's render fed to one CPU oracle per voice that follows
    the batch's parameters, then downmix_ref and meter_ref; outputs, buses, records, and at the end effect state and delay lines."""
    torch = _torch()
    n, n_buses, frames, rounds, per_round = 72, 3, 256, 6, 3
    slots = 2 if kind == "two slots" else 1
    threshold = f32(0.02)
    rng = np.random.default_rng(len(kind))
    with Batch(n, desc.FMT_STEREO, 48000, slots) as b:
        if kind == "proven reverbs":
            b.set_effect(0, [preset_effect((5 * i) % 113) for i in range(n)])
        else:
            for s in range(slots):
                b.set_effect(s, eleven_type_effects(n, s))
        b.apply_changes()
        bus, gain = rng.integers(-1, n_buses, n), rng.uniform(0.2, 1, n).astype(f32)
        b.set_routing(bus, gain)
        army = ShadowArmy(b)
        army.sync()
        if kind == "proven reverbs":
            warm = np.zeros((n, 256, 2), f32)
            for _ in range(10):                # through the start-up cross-fade, until the device has proven every reverb steady
                b.mix(warm)
                army.mix(warm)
                if b.plan(0)[1] == n:
                    break
            assert b.plan(0)[1] == n, b.plan(0)
        records, pcm, assets = playing(rng, n, 2, asset_frames=(2000, 9000), max_step=2 * ONE)
        records["gain"] *= f32(0.25)
        b.set_samplers(records)
        state = records
        vm = torch.zeros(n * METER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        bm = torch.zeros(n_buses * METER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        want_v, want_b = np.zeros(n, METER_DTYPE), np.zeros(n_buses, METER_DTYPE)
        chained = b.chained_calls
        for r in range(rounds):
            xs = [torch.empty((n, frames, 2), dtype=torch.float32, device="cuda") for _ in range(per_round)]
            ys = [torch.empty_like(x) for x in xs]
            outs = [torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda") for _ in range(per_round)]
            torch.cuda.synchronize()
            for x in xs:
                b.sample_device(frames, x.data_ptr())
            for x, y in zip(xs, ys):
                b.mix_device(frames, x.data_ptr(), y.data_ptr())
            for y, out in zip(ys, outs):
                b.downmix_device(frames, y.data_ptr(), n_buses, out.data_ptr())
                b.meter_device(n, frames, y.data_ptr(), vm.data_ptr(), threshold, carry=True)
                b.meter_device(n_buses, frames, out.data_ptr(), bm.data_ptr(), threshold, carry=True)
            b.synchronize()
            for k in range(per_round):
                want_x, state = ref.render(state, pcm, frames, 2)
                expect_output(xs[k].cpu().numpy(), want_x, f"round {r}, buffer {k}: the render")
                want_y = army.mix(want_x)
                y = ys[k].cpu().numpy()
                assert not army.differing(y, want_y), f"round {r}, buffer {k}: outputs differ from the oracle's at {army.differing(y, want_y)[:6]}"
                want_buses = downmix(y, bus, gain, n_buses)
                ok, nbad = same_bits(outs[k].cpu().numpy(), want_buses)
                assert ok, f"round {r}, buffer {k}: {nbad} bus samples differ"
                want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            assert meter_ref.same_records(vm.cpu().numpy().view(METER_DTYPE), want_v), f"round {r}: voices' records"
            assert meter_ref.same_records(bm.cpu().numpy().view(METER_DTYPE), want_b), f"round {r}: buses' records"
        expect_records(b.get_samplers(), state, "the samplers at the end")
        if kind == "proven reverbs":
            assert b.chained_calls > chained, "no mix_device call overlapped its neighbour: the renders did not stand between chained calls"
        bad = army.compare_state()
        assert not bad, f"effect state or delay lines differ: {dict(list(bad.items())[:3])}"


def reverb_batch(n):
    b = Batch(n, desc.FMT_STEREO, 48000, 1)
    b.set_effect(0, [preset_effect((5 * i) % 113) for i in range(n)])
    b.apply_changes()
    return b


def test_play_downmix_meter():
    """Against a twin batch handed the restatement's render through mix_downmix_meter: buses and records are the twin's -- also for a
    call of more than one effect chunk --, either meter left out, carry from call to call; both left out: mix_downmix."""
    n, n_buses = 40, 4
    rng = np.random.default_rng(90)
    bus, gain = rng.integers(-1, n_buses, n), rng.uniform(-1, 1, n).astype(f32)
    threshold = f32(0.1)
    with reverb_batch(n) as b, reverb_batch(n) as twin:
        for t in (b, twin):
            t.set_routing(bus, gain)
        records, pcm, assets = playing(rng, n, 2, asset_frames=(3000, 12000), max_step=2 * ONE)
        b.set_samplers(records)
        state = records
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        for k, frames in enumerate([256, 2500, 100, 4096 + 37, 256, 1]):
            x, state = ref.render(state, pcm, frames, 2)
            if k == 2:      # the voices only, no carry
                got, gv, gb = b.play_downmix_meter(frames, n_buses, threshold, buses=False)
                want, wv, wb = twin.mix_downmix_meter(x, n_buses, threshold, buses=False)
            elif k == 3:    # the buses only
                got, gv, gb = b.play_downmix_meter(frames, n_buses, threshold, voices=False)
                want, wv, wb = twin.mix_downmix_meter(x, n_buses, threshold, voices=False)
            elif k == 4:    # neither: mix_downmix
                got, gv, gb = b.play_downmix_meter(frames, n_buses, threshold, voices=False, buses=False)
                want, wv, wb = twin.mix_downmix(x, n_buses), None, None
                assert gv is None and gb is None
            else:
                got, gv, gb = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
                want, wv, wb = twin.mix_downmix_meter(x, n_buses, threshold, carry=True, voice_meters=want_v, bus_meters=want_b)
                assert gv is vm and gb is bm
            assert got.tobytes() == want.tobytes(), f"call {k} ({frames} frames): the buses differ from mix_downmix_meter's"
            for g, w, what in ((gv, wv, "voices"), (gb, wb, "buses")):
                assert (g is None) == (w is None) and (g is None or g.tobytes() == w.tobytes()), f"call {k} ({frames} frames): the {what}' records differ"
            expect_records(b.get_samplers(), state, f"call {k}")
        assert np.abs(got).max() > 0
        b.play_downmix_meter(0, n_buses, threshold)         # no frames: succeeds, nothing moves
        expect_records(b.get_samplers(), state, "after a call of no frames")


def test_pool_life_cycle():
    """64 voices start one-shot assets through an effect each; a voice is freed once its sampler has finished and the device's carried
    quiet_run says its tail has died away, then reset and started again on another asset and another effect, against a fresh oracle.
    (An asset lasts 8 calls at most and the tails are short -- reverbs of 0.1 s, weak feedback --, so in 100 calls a voice comes round
    several times: at least as many recycles as voices.)"""
    n, n_buses, frames, calls, free_after = 64, 3, 256, 100, 512
    threshold = f32(0.01)
    rng = np.random.default_rng(2027)
    _, _, _, pool = random_records(rng, 1, 2, assets_per_format=3, asset_frames=(600, 2000))
    assets = Assets(pool)
    kinds = [desc.COMPRESSOR, desc.CHORUS, desc.EAX_REVERB, desc.NULL, desc.DISTORTION, desc.REVERB, desc.EQUALIZER, desc.FLANGER]

    def start(b, voices, state, pcm, oracles, generation):
        new = np.zeros(len(voices), SAMPLER_DTYPE)
        effects = []
        for k, i in enumerate(voices):
            key = int(rng.integers(len(pool)))
            fmt, width, data = pool[key]
            new[k] = rec(format=fmt, channels=width, frames=data.shape[0], step=int(rng.integers(ONE, 2 * ONE)), flags=ref.PLAYING | ref.LINEAR,
                         data=assets.address(key))[0]
            new[k]["gain"][:2] = rng.uniform(0.2, 0.6, 2)
            e = random_effect(random.Random(i + 100 * generation), kinds[(i + generation) % len(kinds)])
            if e.type in (desc.REVERB, desc.EAX_REVERB):
                e.props.reverb.decay_time = 0.1
            if e.type in (desc.CHORUS, desc.FLANGER):
                e.props.chorus.feedback = 0.25
            effects.append(e)
            state[i], pcm[i] = new[k], data
            oracles[i] = OracleApi(desc.FMT_STEREO, 48000, 1)
            oracles[i].set_effect(0, e)
            oracles[i].apply_changes()
        b.reset(voices)
        b.set_effect_at(0, voices, effects)
        b.apply_changes()
        b.set_samplers(new, instances=voices)

    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        bus, gain = rng.integers(0, n_buses, n), rng.uniform(0.2, 1, n).astype(f32)
        b.set_routing(bus, gain)
        state, pcm, oracles = np.zeros(n, SAMPLER_DTYPE), [None] * n, [None] * n
        start(b, list(range(n)), state, pcm, oracles, 0)
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        recycled, generation = 0, 0
        for k in range(calls):
            x, state = ref.render(state, pcm, frames, 2)
            y = np.stack([oracles[i].mix(x[i]) for i in range(n)])
            want_buses = downmix(y, bus, gain, n_buses)
            want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
            ok, nbad = same_bits(got, want_buses)
            assert ok, f"call {k}: {nbad} bus samples differ"
            assert meter_ref.same_records(vm, want_v) and meter_ref.same_records(bm, want_b), f"call {k}: records"
            now = b.get_samplers()
            expect_records(now, state, f"call {k}")
            due = [i for i in range(n) if not now["flags"][i] & ref.PLAYING and vm["quiet_run"][i] >= free_after]
            if due:
                generation += 1
                recycled += len(due)
                start(b, due, state, pcm, oracles, generation)
                vm[due] = np.zeros((), METER_DTYPE)
                want_v[due] = np.zeros((), METER_DTYPE)
        print("voices recycled:", recycled)
        assert recycled >= n, recycled


def test_refusals_leave_records_outputs_and_the_batch_alone():
    torch = _torch()
    hip = C.CDLL("libamdhip64.so")
    n, ch, frames = 8, 2, 32
    rng = np.random.default_rng(5)
    so = lib.load()
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        records, pcm, assets = playing(rng, n, ch)
        b.set_samplers(records)
        first = device_render(b, frames)
        want_first, state = ref.render(records, pcm, frames, ch)
        expect_output(first, want_first, "before the refusals")
        uploads = b.sampler_uploads()
        data = torch.full((1000,), 3, dtype=torch.int16, device="cuda")
        # the allocation the tensor lies in, as the runtime has it: the asset may end with it, and not one frame later
        base, size = C.c_void_p(0), C.c_size_t(0)
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(data.data_ptr())) == 0
        room = (base.value + size.value - data.data_ptr()) // 2      # S16 mono frames from the tensor to the allocation's end
        assert room >= 1000
        good = rec(data=data.data_ptr(), frames=room)
        idx = (C.c_int * 3)(1, 2, 3)

        def refused(message, record, instances=idx, count=1):
            arr = np.concatenate([record] * count)
            ok = so.oalsfx_batch_set_samplers(b._h, instances, count, C.c_void_p(arr.ctypes.data))
            assert not ok and message in b.error, (message, b.error)

        refused("one allocation", rec(data=data.data_ptr(), frames=room + 1))                           # one frame longer than its buffer
        refused("one allocation", rec(data=data.data_ptr(), frames=(room + 1) // 2 + 1, channels=2))
        refused("one allocation", rec(data=data.data_ptr() + 2, frames=room))                            # the right length from a later start
        host = np.zeros(1000, np.int16)
        refused("one allocation", rec(data=host.ctypes.data, frames=1000))                               # host memory
        refused("one allocation", rec(data=0x10000, frames=1000))                                        # no memory at all
        refused("Unknown sampler flags", rec(data=data.data_ptr(), flags=9))
        refused("Unknown sampler format", rec(data=data.data_ptr(), format=3))
        refused("reserved", rec(data=data.data_ptr(), reserved=1))
        refused("channel count", rec(data=data.data_ptr(), channels=3))
        refused("no data", rec(data=0))
        refused("frame count", rec(data=data.data_ptr(), frames=0))
        refused("frame count", rec(data=data.data_ptr(), frames=2 ** 31))
        refused("not aligned", rec(data=data.data_ptr() + 1))
        refused("loop region", rec(data=data.data_ptr(), flags=ref.PLAYING | ref.LOOP, loop_start=5, loop_end=5))
        refused("loop region", rec(data=data.data_ptr(), flags=ref.PLAYING | ref.LOOP, loop_start=5, loop_end=101))
        refused("past its end", rec(data=data.data_ptr(), position=100 * ONE))
        refused("past its end", rec(data=data.data_ptr(), flags=ref.PLAYING | ref.LOOP, loop_start=5, loop_end=50, position=50 * ONE))
        refused("Instance range", good, instances=(C.c_int * 1)(n))
        refused("Instance range", good, instances=(C.c_int * 1)(-1))
        refused("Instance range", good, instances=None, count=n + 1)
        refused("listed twice", good, instances=(C.c_int * 3)(1, 2, 1), count=3)
        arr = np.concatenate([good, rec(data=data.data_ptr(), frames=room + 1), good])                    # one bad record: none is taken
        assert not so.oalsfx_batch_set_samplers(b._h, idx, 3, C.c_void_p(arr.ctypes.data)) and "one allocation" in b.error
        out = torch.full((n * frames * ch,), -7.5, dtype=torch.float32, device="cuda")
        for args, message in (((-1, out.data_ptr()), "Frame count is negative"), ((frames, 0), "No destination"), ((frames, out.data_ptr() + 2), "4-byte aligned")):
            assert not so.oalsfx_batch_sample_device(b._h, args[0], C.c_void_p(args[1]), None) and message in b.error, (message, b.error)
        # frames * channels beyond 2^32 - 1: no int does that to a stereo batch, 2^30 frames do it to a quad one (decided before the
        # destination is looked at: no destination is given)
        with Batch(2, desc.FMT_QUAD, 48000, 1) as quad:
            assert not so.oalsfx_batch_sample_device(quad._h, 2 ** 30, C.c_void_p(0), None) and "Frame count is out of range" in quad.error, quad.error
        fp = C.POINTER(C.c_float)
        bus = np.zeros((1, frames, ch), f32)
        for args, message in (((frames, 0, bus.ctypes.data_as(fp), 0.5, 0), "Bus count"), ((frames, 1, None, 0.5, 0), "No destination"),
                              ((frames, 1, bus.ctypes.data_as(fp), -1.0, 0), "threshold"), ((frames, 1, bus.ctypes.data_as(fp), 0.5, 2), "Unknown meter flags"),
                              ((-1, 1, bus.ctypes.data_as(fp), 0.5, 0), "Frame count is negative")):
            assert not so.oalsfx_batch_play_downmix_meter(b._h, *args, None, None) and message in b.error, (message, b.error)
        with pytest.raises(BatchError, match="one allocation"):
            b.set_samplers(rec(data=data.data_ptr(), frames=room + 1), instances=[0])
        b.synchronize()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.5).all(), "a refused call wrote to its destination"
        assert b.sampler_uploads() == uploads
        expect_records(b.get_samplers(), state, "the records after the refusals")
        # a following good call works: the asset that ends with its allocation is taken (and played where the tensor is)
        last = rec(data=data.data_ptr(), frames=room, position=5 * ONE + 100, flags=ref.PLAYING | ref.LINEAR)
        b.set_samplers(last, instances=[3])
        state[3] = last[0]
        pcm[3] = np.zeros((room, 1), np.int16)
        pcm[3][:1000] = 3
        want, state = ref.render(state, pcm, frames, ch)
        expect_output(device_render(b, frames), want, "after the refusals")
        expect_records(b.get_samplers(), state, "the records after the good call")


def test_api_array_samplers(tmp_path):
    """tests/cpp/api_array_samplers.cpp: ApiArray::play_to_buses_metered against mix_to_buses_metered on a second array fed the render
    the program computes itself in the order the C header states."""
    exe = str(tmp_path / "api_array_samplers")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_samplers.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout


# ---- the records of tests/test_sampler_extremes.py: the whole 64-bit range, tile edges, loop extremes, idle fields ----
EXTREME_FAMILIES = ["high positions", "large steps", "loop extremes", "exact endings", "addresses", "idle fields"]
EXTREME_FORMATS = [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_7POINT1]     # both tile lengths, the three store widths


class Placed:
    """The assets of any number of cases in device memory, each distinct array put there once and kept as long as this object."""

    def __init__(self):
        self.tensors = {}

    def fill_in(self, records, assets):
        torch = _torch()
        records = records.copy()
        for r, pcm in enumerate(assets):
            if id(pcm) not in self.tensors:
                self.tensors[id(pcm)] = (pcm, torch.from_numpy(np.ascontiguousarray(pcm)).cuda())
            records["data"][r] = self.tensors[id(pcm)][1].data_ptr()
        torch.cuda.synchronize()
        return records


def expect_same_bytes(got, want, label):
    """Whole records on their 80 bytes: a NaN in a gain the batch has no channel for must come back as the NaN it was."""
    expect_records(got, want, label)
    rows = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not rows, f"{label}: records differ in their bytes at instances {rows[:8]}"


@pytest.mark.parametrize("fmt", EXTREME_FORMATS)
@pytest.mark.parametrize("family", EXTREME_FAMILIES)
def test_extreme_records(family, fmt):
    """Every case of the family: its own calls, then calls of 1, 63, 512 and 513 frames that continue them, against the restatement (which
    the scalar model has vouched for on these very records); the records after every call, at the end on their 80 bytes."""
    import test_sampler_extremes as extremes
    ch = desc.FORMAT_CHANNELS[fmt]
    placed = Placed()
    for label, records, pcm, sizes in extremes.cases(family, ch):
        records = placed.fill_in(records, pcm)
        with Batch(len(records), fmt, 48000, 1) as b:
            after = run_calls(b, records, pcm, sizes + extremes.SPLIT, label)
            expect_same_bytes(b.get_samplers(), after, label)


@pytest.mark.parametrize("fmt", [desc.FMT_STEREO, desc.FMT_7POINT1])
def test_assets_at_every_address_their_element_size_allows(fmt):
    """One allocation per format, the asset 1, 3 and 5 elements into it -- 16-bit stereo at 2 mod 4 bytes, 8-bit at an odd address, fp32
    of 8 channels at 4 mod 16 --, mono and wide, LINEAR and nearest: the output is the aligned placement's, bit for bit.  Every asset
    lies inside its allocation with room behind it."""
    import test_sampler_extremes as extremes
    torch = _torch()
    hip = C.CDLL("libamdhip64.so")
    ch = desc.FORMAT_CHANNELS[fmt]
    records, pcm = extremes.addresses(ch)
    distinct = {id(p): p for p in pcm}
    slack = max(extremes.ADDRESS_OFFSETS) + 64          # elements: more than a frame of any asset behind the farthest placement
    room = {k: torch.zeros(p.size + slack, dtype=getattr(torch, p.dtype.name), device="cuda") for k, p in distinct.items()}
    with Batch(len(records), fmt, 48000, 1) as b:
        outputs = {}
        for offset in [0] + extremes.ADDRESS_OFFSETS:
            placed = records.copy()
            for k, p in distinct.items():
                room[k].zero_()
                room[k][offset:offset + p.size] = torch.from_numpy(p.reshape(-1)).cuda()
                address, nbytes = room[k].data_ptr() + offset * p.itemsize, p.size * p.itemsize
                base, size = C.c_void_p(0), C.c_size_t(0)
                assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(address)) == 0
                assert base.value <= room[k].data_ptr() and address + nbytes + p.shape[1] * p.itemsize <= room[k].data_ptr() + room[k].numel() * p.itemsize <= base.value + size.value
                assert address % p.itemsize == 0 and (offset == 0 or address % (4 * p.itemsize) != 0)
                placed["data"][[r for r, q in enumerate(pcm) if q is p]] = address
            torch.cuda.synchronize()
            b.set_samplers(placed)
            want, after = ref.render(placed, pcm, 300, ch)
            outputs[offset] = device_render(b, 300)
            expect_output(outputs[offset], want, f"format {fmt}, assets {offset} elements in")
            expect_records(b.get_samplers(), after, f"format {fmt}, assets {offset} elements in")
            assert same_bits(outputs[offset], outputs[0])[0], f"format {fmt}: {offset} elements in differs from the aligned placement"
        assert np.abs(outputs[0]).max() > 0


@pytest.mark.parametrize("fmt", EXTREME_FORMATS)
def test_idle_fields_come_back_as_they_were(fmt):
    """gain[C:] holds a NaN with a payload, -0.0, a denormal and Inf, loop_start and loop_end of the one-shots random values: after
    set_samplers, three renders and get_samplers the records are the restatement's on all 80 bytes."""
    import test_sampler_extremes as extremes
    ch = desc.FORMAT_CHANNELS[fmt]
    records, pcm = extremes.idle_fields(ch)
    records = Placed().fill_in(records, pcm)
    with Batch(len(records), fmt, 48000, 1) as b:
        b.set_samplers(records)
        assert b.get_samplers().tobytes() == records.tobytes()
        state = records
        for frames in (64, 256, 441):
            _, state = ref.render(state, pcm, frames, ch)
            device_render(b, frames)
        got = b.get_samplers()
        expect_same_bytes(got, state, f"format {fmt}")
        assert got["gain"].view(np.uint32)[:, ch:].tobytes() == records["gain"].view(np.uint32)[:, ch:].tobytes()
        assert ch == 8 or np.isnan(got["gain"][:, ch:]).any()
        assert got["position"].tobytes() != records["position"].tobytes()


def test_state_calls_leave_the_samplers_alone():
    """24 stereo voices, reverbs and choruses, playing into their effects.  reset of half the voices, snapshot of all, two more renders,
    restore of the snapshot: after each the records are the restatement's, which knows none of the three calls, and so is the render that
    follows -- a restore rewinds no position.  (The effects' outputs: tests/test_gpu_state_io_paths.py.)"""
    torch = _torch()
    n, ch, frames = 24, 2, 256
    rng = np.random.default_rng(77)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect(0, [preset_effect(3 * i) if i % 2 else random_effect(random.Random(i), desc.CHORUS) for i in range(n)])
        b.apply_changes()
        records, pcm, assets = playing(rng, n, ch, asset_frames=(4000, 9000), max_step=2 * ONE)
        b.set_samplers(records)
        state = [records]
        y = torch.empty((n, frames, ch), dtype=torch.float32, device="cuda")

        def render(label):
            want, state[0] = ref.render(state[0], pcm, frames, ch)
            got = device_render(b, frames)
            expect_output(got, want, label)
            x = torch.from_numpy(got).cuda()
            b.mix_device(frames, x.data_ptr(), y.data_ptr())          # the effects take the render in: they have state to reset and to carry
            b.synchronize()
            expect_records(b.get_samplers(), state[0], label)

        render("first render")
        render("second render")
        b.reset(list(range(0, n, 2)))
        expect_records(b.get_samplers(), state[0], "after reset")
        render("the render after reset")
        nbytes = b.snapshot_bytes()
        blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        b.snapshot(None, blob.data_ptr(), nbytes)
        b.synchronize()
        expect_records(b.get_samplers(), state[0], "after snapshot")
        at_snapshot = state[0].copy()
        render("first render after snapshot")
        render("second render after snapshot")
        b.restore(None, blob.data_ptr(), nbytes)
        b.synchronize()
        expect_records(b.get_samplers(), state[0], "after restore")
        assert (state[0]["position"] != at_snapshot["position"]).any()
        render("the render after restore")
        assert (state[0]["flags"] & ref.PLAYING).any() and float(np.abs(y.cpu().numpy()).max()) > 0


def test_samplers_on_the_shards_of_a_group():
    """A group offers no samplers of its own; oalsfx_group_batch gives each shard's batch to set them on.  Two shards on one device, other
    records on each: a shard's render is the restatement's for its own records and leaves the other shard's as they were."""
    n = 24
    rng = np.random.default_rng(88)
    with Group(n, [0, 0], desc.FMT_STEREO, 48000, 1) as g:
        views = [g.batch(0), g.batch(1)]
        assert [v.n for v in views] == [12, 12]
        sets = [playing(rng, 12, 2, asset_frames=(300, 3000)) for _ in views]
        assert sets[0][0].tobytes() != sets[1][0].tobytes()
        for v, (records, pcm, assets) in zip(views, sets):
            v.set_samplers(records)
        for v, (records, pcm, assets) in zip(views, sets):
            expect_records(v.get_samplers(), records, "as set")
        state = [s[0] for s in sets]
        for k, frames in ((0, 300), (1, 513), (1, 64), (0, 1)):
            want, state[k] = ref.render(state[k], sets[k][1], frames, 2)
            expect_output(device_render(views[k], frames), want, f"shard {k}, {frames} frames")
            for j, v in enumerate(views):
                expect_records(v.get_samplers(), state[j], f"shard {j} after shard {k} rendered {frames} frames")
        g.mix(np.zeros((n, 64, 2), f32))                  # the group's own calls go on working beside them
        for j, v in enumerate(views):
            expect_records(v.get_samplers(), state[j], f"shard {j} after a group call")
            v.close()
