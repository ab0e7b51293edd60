"""CPU: the host model of the whole voice stack (tests/stack_model.py), which tests/test_gpu_voice_stack.py replays on a GPU.  Three
things are checked here, without one: the generated sequences meet their conditions and hold every stretch; the real kernel bodies,
built for the host (tests/cpp/program_rows_host.cpp through tests/test_program_host.py: a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer where a host compiler has their runtime, run directly), leave every render of a sequence the way the model
says, from the states the sequence reaches and not only from fresh ones; and the comparison helpers report a changed history, a changed
queue head and a changed sign bit on a zero."""
import numpy as np
import pytest

import biquad_ref as bref
import program_cases as gcases
import stack_model as sm
import voice_ref as vref
from test_program_host import program, run        # noqa: F401 (the fixture that builds the host program)

f32 = np.float32


def script(seed, n, channels, lanes_max, **kw):
    pool = sm.pool_for(seed, channels)
    return sm.build(seed, n, channels, lanes_max, pool, [0x10000 * (k + 1) for k in range(len(pool))], **kw)


@pytest.mark.parametrize("channels, n, lanes_max, seed", sm.SHAPES)
def test_the_generator_meets_its_conditions(channels, n, lanes_max, seed):
    s = script(seed, n, channels, lanes_max)
    missing = [what for what, there in sm.present(s.ops).items() if not there]
    unmet = [what for what, met in sm.conditions(s.ops).items() if not met]
    print(sm.summary(s.ops))
    assert not missing and not unmet, (missing, unmet, len(s.ops))
    # under every one of the seven kernels some render goes to the caller's stream
    assert {op["kernel"] for op in s.ops if op["kind"] == "render" and op["side"]} == set(sm.KERNELS)
    assert max(op["lanes"] for op in s.ops) == lanes_max and all(len(op["want"]) == n for op in s.ops if op["kind"] in ("render", "play"))


@pytest.mark.parametrize("seed", [21, 22])
def test_the_short_sequences_hold_their_stretches(seed):
    """The two sequences tests/test_gpu_voice_stack.py interleaves on one stream."""
    s = script(seed, 5, 2, 3, only=sm.SHORT)
    found = sm.present(s.ops)
    assert 25 <= len(s.ops) <= 45 and all(found[what] for what in (sm.STRETCHES[3], sm.STRETCHES[5], sm.STRETCHES[6], sm.STRETCHES[7], "streams alternate"))
    assert not any(np.isnan(op["want"]).any() for op in s.ops if op["kind"] in ("render", "play"))


def hosted():
    return script(21, 5, 2, 3, only=sm.HOSTED)


def expectation(op):
    """What the kernels must leave behind a render, from the model: (out, records, envelopes, filters, queues)."""
    before, after = op["before"], op["after"]
    taken = [[len(b) - len(a) for b, a in zip(lb, la)] for lb, la in zip(before["prog"], after["prog"])]
    return op["want"], after["rec"], gcases.first_segments(after["prog"]), after["filt"], sm.queue_rows(after["prog"], taken)


def differences(got, want, filtered=True):
    """{what: where} for everything in which what the kernels left differs from the expectation, on bit patterns and bytes."""
    out, rec, envelopes, filt, queues = got
    w_out, w_rec, w_env, w_filt, w_queues = want
    rec = rec.copy()
    rec["data"] = w_rec["data"]                             # (the host program's own addresses)
    found = {"outputs": sm.bits_differ(out, w_out), "records": sm.records_differ(rec, w_rec), "envelopes": sm.records_differ(envelopes, w_env),
             "filters": sm.records_differ(filt, w_filt) if filtered else [], "queues": sm.queues_differ(queues, w_queues)}
    return {what: where for what, where in found.items() if where}


def test_the_kernels_follow_the_model_on_the_host(program, tmp_path):
    """Every render of one sequence of 5 instances, up to 3 lanes: the model's state in front of it handed to the host build of
    k_program_biquad_rows (a filter ACTIVE) or k_program_rows (none), one call; outputs, both records, filters and queues behind it
    against the model's.  A pending LOAD is the model's to resolve: the kernels never see the bit."""
    s = hosted()
    renders = [op for op in s.ops if op["kind"] in ("render", "play")]
    assert 20 <= len(renders) <= 32 and {op["kernel"] for op in renders} == set(sm.KERNELS)
    assert any(op["queued"] and any(len(b) > len(a) for lb, la in zip(op["before"]["prog"], op["after"]["prog"]) for b, a in zip(lb, la)) for op in renders)
    for k, op in enumerate(renders):
        before = op["before"]
        filtered = bool((before["filt"]["flags"] & bref.ACTIVE).any())
        assert filtered == op["filters_active"] and not (before["filt"]["flags"] & bref.LOAD).any()
        got = run(program, tmp_path, before["rec"], before["prog"], before["res"], before["filt"] if filtered else None, before["tables"], before["pcm"], s.channels,
                  [op["frames"]], offset=op["offset"])[0]
        bad = differences(got, expectation(op), filtered)
        assert not bad, f"render {k} ({op['frames']} frames, {op['lanes']} lanes, {op['kernel']} on the device): {bad}"


def test_the_comparison_reports_what_it_must():
    """One thing changed in a copy of the model's expectation, three times: the comparison says so each time, and says nothing of the
    expectation against itself."""
    s = hosted()
    renders = [op for op in s.ops if op["kind"] in ("render", "play")]
    copy = lambda: tuple(np.array(x, copy=True) for x in want)
    want = expectation(next(o for o in renders if o["filters_active"] and any(len(p) > 1 for lane in o["after"]["prog"] for p in lane)))
    assert differences(copy(), want) == {}

    changed = copy()
    k, i = np.argwhere(changed[3]["flags"] & bref.ACTIVE)[0]
    changed[3]["y"][k, i, 0, 1] = np.nextafter(changed[3]["y"][k, i, 0, 1], f32(9))
    assert differences(changed, want) == {"filters": [(int(k), int(i))]}

    changed = copy()
    k, i = np.argwhere(changed[4]["count"] > 0)[0]
    changed[4]["head"][k, i] += 1
    assert differences(changed, want) == {"queues": [(int(k), int(i))]}

    want = expectation(next(o for o in renders if (o["want"].view(np.uint32) == 0).any()))
    changed = copy()
    at = tuple(np.argwhere(changed[0].view(np.uint32) == 0)[0])
    changed[0][at] = f32(-0.0)
    assert changed[0][at] == want[0][at] and differences(changed, want) == {"outputs": [tuple(int(x) for x in at)]}
    # ... and a NaN stands for a NaN at its place only
    changed = copy()
    changed[0][at] = np.nan
    assert differences(changed, want) == {"outputs": [tuple(int(x) for x in at)]} and differences(changed, changed) == {}
