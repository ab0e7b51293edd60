"""GPU: the resamplers (oalsfx_batch_set_fir_table, _set_resamplers, and the renders of _sample_device and _play_downmix_meter while an
instance names a table; include/oalsfx_hip.h, "resamplers") against their restatement (tests/resample_ref.py).  Every comparison is on
the bit patterns (NaNs by position) and on the exact integers, outputs and both records; there is no tolerance anywhere.  No test
provokes a device fault: every refusal is decided on the host, and every asset of the named rows lies inside a larger allocation, so
that a tap read outside an asset would show as a wrong value and not as a fault."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meter_ref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from downmix_ref import downmix
from harness import ROOT, same_bits
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.api import METER_DTYPE, Batch, BatchError
from test_gpu_sampler import Assets, device_render, expect_output, expect_records
from test_gpu_voice import expect_envelopes
from test_sampler_abi import rec
from test_voice_abi import env

pytestmark = pytest.mark.gpu
f32 = np.float32
ONE = sref.ONE
CALLS = cases.CALLS
FORMAT = {1: desc.FMT_MONO, 2: desc.FMT_STEREO, 4: desc.FMT_QUAD, 6: desc.FMT_5POINT1, 7: desc.FMT_6POINT1, 8: desc.FMT_7POINT1}
GUARD_FRAMES = 8


def _torch():
    import torch
    return torch


class Guarded:
    """Assets in device memory, each inside an allocation of its own with GUARD_FRAMES frames in front of it and behind it that hold NaN
    (fp32) or the largest value (integers): a tap read outside the asset shows in the output."""

    def __init__(self):
        self.kept = {}

    def address(self, pcm):
        torch = _torch()
        if id(pcm) not in self.kept:
            fill = np.nan if pcm.dtype == np.float32 else np.iinfo(pcm.dtype).max
            guard = np.full((GUARD_FRAMES, pcm.shape[1]), fill, pcm.dtype)
            whole = torch.from_numpy(np.concatenate([guard, pcm, guard])).cuda()
            self.kept[id(pcm)] = (pcm, whole)
        return self.kept[id(pcm)][1].data_ptr() + GUARD_FRAMES * pcm.shape[1] * pcm.dtype.itemsize

    def fill_in(self, records, pcm):
        records = records.copy()
        records["data"] = [self.address(p) for p in pcm]
        _torch().cuda.synchronize()
        return records


def set_tables(b, tables):
    for t, coef in tables.items():
        b.set_fir_table(t, coef)
        assert b.get_fir_table(t) == (coef.shape[1], coef.shape[0].bit_length() - 1)


def run_calls(b, records, envelopes, resamplers, tables, pcm, sizes, label, names=None, **kw):
    """set_samplers, set_envelopes and set_resamplers, then one render per size, each against the restatement, with both records and the
    resamplers read back after every call.  Returns (the outputs side by side, the records, the envelopes)."""
    b.set_samplers(records)
    b.set_envelopes(envelopes)
    b.set_resamplers(resamplers)
    assert (b.get_resamplers() == resamplers).all()
    state, env_state, outs = records, envelopes, []
    for frames in sizes:
        want, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, frames, b.channels)
        got = device_render(b, frames, **kw)
        assert b.last_render_kernel() == ("k_fir_rows" if (resamplers != ref.NONE).any() else "k_voice_rows" if (envelopes["flags"] & vref.ACTIVE).any() else "k_sampler_rows")
        if names:
            bad = [names[r] for r in range(len(names)) if not sref.same_floats(got[r], want[r])[0]]
            assert not bad, f"{label}, {frames} frames: the outputs of {bad[:6]} differ"
        expect_output(got, want, f"{label}, {frames} frames")
        expect_records(b.get_samplers(), state, f"{label}, after {frames} frames")
        expect_envelopes(b.get_envelopes(), env_state, f"{label}, after {frames} frames")
        assert (b.get_resamplers() == resamplers).all()
        outs.append(got)
    return np.concatenate(outs, axis=1), state, env_state


@pytest.mark.parametrize("fmt", [sref.PCM_U8, sref.PCM_S16, sref.PCM_F32])
@pytest.mark.parametrize("taps", [4, 8])
def test_the_rows_the_contract_names(taps, fmt):
    """resample_cases.named_rows, one row each: mono output, a mono and a wide asset under stereo, a wide asset under 7.1; four renders
    and one of their sum."""
    tables = cases.tables()
    placed = Guarded()
    for channels, width in ((1, 1), (2, 1), (2, 2), (8, 8)):
        names, records, resamplers, pcm = cases.named_rows(taps, fmt, width, channels)
        records = placed.fill_in(records, pcm)
        envelopes = np.zeros(len(records), vref.DTYPE)
        label = f"T = {taps}, PCM format {fmt}, {width} of {channels} channels"
        with Batch(len(records), FORMAT[channels], 48000, 1) as b:
            set_tables(b, tables)
            parts, after, _ = run_calls(b, records, envelopes, resamplers, tables, pcm, CALLS, label, names)
            whole, after_whole, _ = run_calls(b, records, envelopes, resamplers, tables, pcm, [sum(CALLS)], label + ", one render", names, offset=1)
            assert same_bits(parts, whole)[0] and after.tobytes() == after_whole.tobytes(), f"{label}: four renders and one differ"
        row = dict(zip(names, range(len(names))))
        assert not after["flags"][row["a one-shot that ends in mid-call"]] & sref.PLAYING and after["flags"][row["the last H frames of a one-shot"]] & sref.PLAYING
        if fmt == sref.PCM_F32:
            hit = parts[row["NaN and Inf samples under a zero coefficient"]]
            assert np.isnan(hit).any() and not np.isnan(hit).all(), "0 * Inf is NaN, not skipped"
            assert not np.isnan(np.delete(parts, [row[k] for k in row if k.startswith(("NaN", "denormal samples"))], axis=0)).any(), "a guard frame was read"
            quiet = parts[row["denormal products"]]
            assert (quiet != 0).any() and np.abs(quiet).max() < np.finfo(f32).tiny


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("fmt", [desc.FMT_MONO, desc.FMT_STEREO, desc.FMT_QUAD, desc.FMT_5POINT1, desc.FMT_6POINT1, desc.FMT_7POINT1])
def test_seventy_voices_in_four_renders_and_in_one(fmt, offset):
    """70 instances -- a partial last workgroup --, every PCM format x mono / wide asset x looped / one-shot taken in turn; a third of the
    rows each at 4 taps, at 8 taps and without a table; every second row under a random envelope (delay, ramp, STOP, glide).  Renders of
    441, 256, 1 and 63 frames, then the same records again in one render of 761.  The destination 0, 1 and 2 floats off its allocation:
    every store width runs."""
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(2000 * fmt + offset)
    records, envelopes, resamplers, pcm, keys, pool = cases.random_rows(rng, 70, ch, True, asset_frames=(1, 3000))
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    tables = cases.tables()
    kinds = [int((resamplers == ref.NONE).sum()), int(np.isin(resamplers, (0, 2, 4, 6)).sum()), int(np.isin(resamplers, (1, 3, 5, 7)).sum())]
    active = (envelopes["flags"] & vref.ACTIVE) != 0
    assert min(kinds) >= 20 and 25 <= active.sum() <= 35 and (active & (resamplers != ref.NONE)).sum() >= 10, (kinds, active.sum())
    assert len({(int(r["format"]), int(r["channels"]) == 1, int(r["flags"]) & sref.LOOP, int(t) % 2) for r, t in zip(records, resamplers) if t != ref.NONE}) == 3 * (1 if ch == 1 else 2) * 2 * 2
    with Batch(70, fmt, 48000, 1) as b:
        set_tables(b, tables)
        parts, after, env_after = run_calls(b, records, envelopes, resamplers, tables, pcm, CALLS, f"format {fmt}, offset {offset}", offset=offset)
        whole, after_whole, env_whole = run_calls(b, records, envelopes, resamplers, tables, pcm, [sum(CALLS)], f"format {fmt}, offset {offset}, one render", offset=offset)
        assert same_bits(parts, whole)[0], "four renders and one differ"
        expect_records(after, after_whole, "four renders and one")
        expect_envelopes(env_after, env_whole, "four renders and one")
        assert np.abs(whole).max() > 0 and (env_whole["sub"] != 0).any()


@pytest.mark.parametrize("enveloped", [False, True])
@pytest.mark.parametrize("fmt", [desc.FMT_STEREO, desc.FMT_7POINT1])
def test_rows_without_a_table_are_the_old_kernels_rows(fmt, enveloped):
    """The same 41 records on two batches; on one, a 42nd instance names a table, so that k_fir_rows renders them all; on the other
    k_voice_rows (envelopes) or k_sampler_rows (none) does.  The 41 rows' outputs and records are the same on their bits."""
    ch = desc.FORMAT_CHANNELS[fmt]
    rng = np.random.default_rng(70 + fmt + enveloped)
    records, envelopes, _, pcm, keys, pool = cases.random_rows(rng, 42, ch, enveloped, asset_frames=(1, 2000))
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    if enveloped:
        assert (envelopes["flags"][:41] & vref.ACTIVE).any()
    resamplers = np.full(42, ref.NONE)
    resamplers[41] = 1
    with Batch(42, fmt, 48000, 1) as b, Batch(42, fmt, 48000, 1) as old:
        b.set_fir_table(1, cases.tables()[1])
        for batch in (b, old):
            batch.set_samplers(records)
            batch.set_envelopes(envelopes)
        b.set_resamplers(resamplers)
        for frames in CALLS + (700,):
            got, theirs = device_render(b, frames), device_render(old, frames)
            assert b.last_render_kernel() == "k_fir_rows" and old.last_render_kernel() == ("k_voice_rows" if enveloped else "k_sampler_rows")
            assert same_bits(got[:41], theirs[:41])[0], f"{frames} frames"
            assert b.get_samplers()[:41].tobytes() == old.get_samplers()[:41].tobytes() and b.get_envelopes()[:41].tobytes() == old.get_envelopes()[:41].tobytes()
        assert np.abs(got[:41]).max() > 0


def test_the_launch_follows_the_resamplers():
    rng = np.random.default_rng(4)
    records, envelopes, _, pcm, keys, pool = cases.random_rows(rng, 20, 2, True)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    tables = {0: ref.cubic(8), 1: ref.sinc(8, 6, 0.5)}
    none = np.full(20, ref.NONE)
    with Batch(20, desc.FMT_STEREO, 48000, 1) as b:
        assert (b.get_resamplers() == ref.NONE).all() and b.get_fir_table(0) == (0, 0)
        b.set_samplers(records)
        want, state = sref.render(records, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "before any resampler")
        assert b.last_render_kernel() == "k_sampler_rows" and b.resampler_uploads() == 0
        b.set_envelopes(envelopes)
        want, state, env_state = vref.render(state, envelopes, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "envelopes, no resampler")
        assert b.last_render_kernel() == "k_voice_rows" and b.resampler_uploads() == 0
        set_tables(b, tables)
        expect_output(device_render(b, 1), vref.render(state, env_state, pcm, 1, 2)[0], "tables that no instance names")
        _, state, env_state = vref.render(state, env_state, pcm, 1, 2)
        assert b.last_render_kernel() == "k_voice_rows" and b.resampler_uploads() == 0
        b.set_resamplers([1], instances=[4])
        resamplers = none.copy()
        resamplers[4] = 1
        want, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "one resampler")
        assert b.last_render_kernel() == "k_fir_rows" and b.resampler_uploads() == 1
        want, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, 7, 2)
        expect_output(device_render(b, 7), want, "a second render")
        assert b.resampler_uploads() == 1, "a render after which nothing was set put resamplers on the device"
        b.set_resamplers([1], instances=[4])                   # the same again: nothing has changed, nothing goes up
        b.set_resamplers([ref.NONE], instances=[4])
        want, state, env_state = vref.render(state, env_state, pcm, 100, 2)
        expect_output(device_render(b, 100), want, "the resampler cleared")
        assert b.last_render_kernel() == "k_voice_rows" and (b.get_resamplers() == ref.NONE).all()
        b.set_envelopes(np.zeros(20, vref.DTYPE))
        b.set_resamplers(np.where(np.arange(20) % 2, 0, 1))
        resamplers = np.where(np.arange(20) % 2, 0, 1)
        state = b.get_samplers()
        want, state, _ = ref.render(state, np.zeros(20, vref.DTYPE), resamplers, tables, pcm, 300, 2)
        expect_output(device_render(b, 300), want, "every instance, no envelope")
        assert b.last_render_kernel() == "k_fir_rows"
        expect_records(b.get_samplers(), state, "every instance, no envelope")
        b.set_resamplers(none)
        device_render(b, 5)
        assert b.last_render_kernel() == "k_sampler_rows"
        b.set_fir_table(0, None)                                # nobody names them: they can go
        b.set_fir_table(1, None)
        assert b.get_fir_table(1) == (0, 0)


def test_refusals_leave_resamplers_and_tables_alone():
    so = lib.load()
    rng = np.random.default_rng(9)
    records, envelopes, _, pcm, keys, pool = cases.random_rows(rng, 8, 2, False)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    tables = {0: ref.cubic(5), 3: ref.sinc(8, 2, 1.0)}
    resamplers = np.asarray([0, 3, ref.NONE, 0, 3, ref.NONE, 0, 3])
    good = np.zeros((4, 4), f32)
    with Batch(8, desc.FMT_STEREO, 48000, 1) as b:
        b.set_samplers(records)
        set_tables(b, tables)
        b.set_resamplers(resamplers)

        def table_refused(message, table, taps, bits, coef):
            ptr = C.c_void_p(coef.ctypes.data) if coef is not None else C.c_void_p(0)
            assert not so.oalsfx_batch_set_fir_table(b._h, table, taps, bits, ptr) and message in b.error, (message, b.error)

        table_refused("FIR table index out of range.", 8, 4, 2, good)
        table_refused("FIR table index out of range.", -1, 4, 2, good)
        table_refused("Unknown FIR tap count.", 1, 5, 2, good)
        table_refused("Unknown FIR tap count.", 1, 0, 2, good)
        table_refused("FIR phase bits out of range.", 1, 4, 13, good)
        table_refused("Null FIR coefficients.", 1, 4, 2, None)
        bad = good.copy()
        bad[3, 3] = np.inf
        table_refused("Non-finite FIR coefficient.", 1, 4, 2, bad)
        table_refused("Non-finite FIR coefficient.", 0, 4, 5, np.full((32, 4), np.nan, f32))
        table_refused("The FIR table is still named by an instance.", 0, 0, 0, None)
        table_refused("The FIR table is still named by an instance.", 0, 4, 4, np.zeros((16, 4), f32))
        table_refused("The FIR table is still named by an instance.", 3, 4, 2, good)
        with pytest.raises(BatchError, match="still named"):
            b.set_fir_table(3, None)

        def refused(message, values, instances):
            idx = (C.c_int * len(instances))(*instances)
            assert not so.oalsfx_batch_set_resamplers(b._h, idx, len(instances), (C.c_int * len(values))(*values)) and message in b.error, (message, b.error)

        refused("Unknown resampler.", [8], [2])
        refused("Unknown resampler.", [-2], [2])
        refused("The resampler names a table that has not been set.", [1], [2])
        refused("The resampler names a table that has not been set.", [3, 0, 7], [2, 5, 6])       # one bad index: none is taken
        refused("Instance range", [0], [8])
        refused("listed twice", [0, 0], [1, 1])
        with pytest.raises(BatchError, match="has not been set"):
            b.set_resamplers([2], instances=[2])
        assert b.resampler_uploads() == 0 and (b.get_resamplers() == resamplers).all()
        assert b.get_fir_table(0) == (4, 5) and b.get_fir_table(3) == (8, 2) and b.get_fir_table(1) == (0, 0)
        none = np.zeros(8, vref.DTYPE)
        want, state, _ = ref.render(records, none, resamplers, tables, pcm, 300, 2)
        expect_output(device_render(b, 300), want, "after the refusals")
        expect_records(b.get_samplers(), state, "after the refusals")
        assert b.resampler_uploads() == 1


def test_replacing_a_table_takes_effect_at_the_next_render():
    rng = np.random.default_rng(11)
    records, envelopes, _, pcm, keys, pool = cases.random_rows(rng, 12, 2, False)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    torch = _torch()
    first, second = ref.sinc(8, 6, 1.0), ref.sinc(8, 6, 0.4)
    resamplers = np.full(12, 2)
    none = np.zeros(12, vref.DTYPE)
    with Batch(12, desc.FMT_STEREO, 48000, 1) as b:
        b.set_samplers(records)
        b.set_fir_table(2, first)
        b.set_resamplers(resamplers)
        # a render queued and not waited for, then the replacement: the render has the old coefficients, the next one the new ones
        buf = torch.empty((12, 2000, 2), dtype=torch.float32, device="cuda")
        b.sample_device(2000, buf.data_ptr())
        b.set_fir_table(2, second)
        want, state, _ = ref.render(records, none, resamplers, {2: first}, pcm, 2000, 2)
        torch.cuda.synchronize()
        expect_output(buf.cpu().numpy(), want, "the render queued in front of the replacement")
        stale = ref.render(state, none, resamplers, {2: first}, pcm, 500, 2)[0]
        want, state, _ = ref.render(state, none, resamplers, {2: second}, pcm, 500, 2)
        got = device_render(b, 500)
        expect_output(got, want, "the render behind the replacement")
        assert not same_bits(want, stale)[0], "the two tables must differ in what they render"
        expect_records(b.get_samplers(), state, "behind the replacement")
        assert b.get_fir_table(2) == (8, 6) and b.resampler_uploads() == 1


def three_rounds_of_records(n=200, frames=64, counts=(3, 200, 65)):
    """What test_three_records_set_and_rendered_three_times_without_a_wait sets and expects: per round (the rows, their sampler records
    with `data` still the asset's key, their envelopes, their resamplers), and `expected(records per round with their addresses)` ->
    (the outputs per round, the records, the envelopes and the resamplers behind the last).  No envelope glides: set_envelopes reads
    the samplers back, and waits, where a glide is set while a render with a glide is queued.  One 4-tap table, number 0; every round's
    resamplers differ from what their rows had, so that each round has resamplers to put on the device."""
    rng = np.random.default_rng(36)
    records, envelopes, _, pcm, keys, pool = cases.random_rows(rng, 3 * n, 2, True, calls=(frames,) * 3)
    envelopes["flags"] &= ~np.uint32(vref.GLIDE)
    rows = [np.sort(rng.choice(n, count, replace=False)) for count in counts]
    held = np.full(n, ref.NONE)
    rounds = []
    for k, at in enumerate(rows):
        # (the table for every row that has none, and none for one in three of the others)
        resamplers = np.where(held[at] == ref.NONE, 0, np.where(at % 3 == 0, ref.NONE, 0))
        assert (resamplers != held[at]).sum() > (0, 64, 0)[k]
        held[at] = resamplers
        block = k * n + np.arange(len(at))
        rounds.append((at, records[block], envelopes[block], resamplers, [pcm[r] for r in block], [keys[r] for r in block]))

    def expected(placed):
        state, env_state, res, assets = np.zeros(n, sref.DTYPE), np.zeros(n, vref.DTYPE), np.full(n, ref.NONE), [None] * n
        outs = []
        for (at, _, env_k, res_k, pcm_k, _), rec_k in zip(rounds, placed):
            state[at], env_state[at], res[at] = rec_k, env_k, res_k
            for r, p in zip(at, pcm_k):
                assets[r] = p
            out, state, env_state = ref.render(state, env_state, res, {0: ref.cubic(8)}, assets, frames, 2)
            outs.append(out)
        return outs, state, env_state, res
    return rounds, pool, expected


def test_three_records_set_and_rendered_three_times_without_a_wait():
    """Samplers, envelopes and resamplers go to the device by the same route (record_table.hpp, batch.cpp: records_upload), one launch each
    in front of the render.  200 stereo voices, renders of 64 frames, nothing waited for in between: 3 rows of each record set and a
    render on the batch's stream; all 200 rows set and a render on a caller's stream -- each page-locked buffer, made for 64 rows, is
    outgrown while the launch that read it may still be in flight --; 65 rows set and a render on the batch's stream again.  Then the
    three read-backs.  Outputs and records are the restatement's on their bits, and every record's uploads are three more."""
    torch = _torch()
    n, frames = 200, 64
    rounds, pool, expected = three_rounds_of_records(n, frames)
    assets = Assets(pool)
    placed = [assets.fill_in(rec_k.copy(), keys_k) for _, rec_k, _, _, _, keys_k in rounds]
    want, state, env_state, res = expected(placed)
    bufs = [torch.full((n, frames, 2), -7.5, dtype=torch.float32, device="cuda") for _ in rounds]
    caller = torch.cuda.Stream()
    torch.cuda.synchronize()
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_fir_table(0, ref.cubic(8))
        before = (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads())
        for k, ((at, _, env_k, res_k, _, _), rec_k) in enumerate(zip(rounds, placed)):
            b.set_samplers(rec_k, instances=at)
            b.set_envelopes(env_k, instances=at)
            b.set_resamplers(res_k, instances=at)
            b.sample_device(frames, bufs[k].data_ptr(), stream=caller.cuda_stream if k == 1 else None)
            assert b.last_render_kernel() == "k_fir_rows"
        got_records, got_envelopes, got_resamplers = b.get_samplers(), b.get_envelopes(), b.get_resamplers()
        assert (b.sampler_uploads(), b.envelope_uploads(), b.resampler_uploads()) == tuple(c + 3 for c in before)
        b.synchronize()
        torch.cuda.synchronize()
        for k, buf in enumerate(bufs):
            expect_output(buf.cpu().numpy(), want[k], f"render {k + 1}")
        expect_records(got_records, state, "behind the three renders")
        expect_envelopes(got_envelopes, env_state, "behind the three renders")
        assert (got_resamplers == res).all()
        assert all(np.abs(w).max() > 0 for w in want) and (env_state["ramp_done"] != 0).any()


def test_play_downmix_meter_with_tables():
    """48 voices into 4 buses, calls of 256 frames with carried meters; the voices' outputs are those of a twin batch fed the
    restatement's render; buses and meters are downmix_ref's and meter_ref's over them."""
    n, n_buses, frames = 48, 4, 256
    threshold = f32(1e-4)
    rng = np.random.default_rng(65)
    records, envelopes, resamplers, pcm, keys, pool = cases.random_rows(rng, n, 2, True, asset_frames=(500, 3000), max_step=3 * ONE)
    assets = Assets(pool)
    records = assets.fill_in(records, keys)
    resamplers = np.where(np.isin(resamplers, (cases.TINY, cases.TINY + 1)), 0, resamplers)        # (audible rows for the meters)
    tables = cases.tables()
    bus, gain = rng.integers(0, n_buses, n), rng.uniform(0.2, 1, n).astype(f32)
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b, Batch(n, desc.FMT_STEREO, 48000, 1) as twin:
        b.set_routing(bus, gain)
        set_tables(b, tables)
        b.set_samplers(records)
        b.set_envelopes(envelopes)
        b.set_resamplers(resamplers)
        state, env_state = records, envelopes
        vm, bm, want_v, want_b = (np.zeros(k, METER_DTYPE) for k in (n, n_buses, n, n_buses))
        for k in range(4):
            x, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, frames, 2)
            y = twin.mix(x)
            want_buses = downmix(y, bus, gain, n_buses)
            want_v, want_b = meter_ref.meter(y, threshold, want_v), meter_ref.meter(want_buses, threshold, want_b)
            got, _, _ = b.play_downmix_meter(frames, n_buses, threshold, carry=True, voice_meters=vm, bus_meters=bm)
            assert b.last_render_kernel() == "k_fir_rows"
            ok, nbad = same_bits(got, want_buses)
            assert ok, f"call {k}: {nbad} bus samples differ"
            assert meter_ref.same_records(vm, want_v) and meter_ref.same_records(bm, want_b), f"call {k}: the meters' records"
            expect_records(b.get_samplers(), state, f"call {k}")
            expect_envelopes(b.get_envelopes(), env_state, f"call {k}")
        assert np.abs(got).max() > 0


def test_api_array_resamplers(tmp_path):
    """tests/cpp/api_array_resamplers.cpp: ApiArray::set_fir_table / set_resampler / get_resampler, one round trip through a render."""
    exe = str(tmp_path / "api_array_resamplers")
    libdir = os.path.dirname(lib.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "cpp", "api_array_resamplers.cpp"), "-L", libdir, "-loalsfx_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr + r.stdout
