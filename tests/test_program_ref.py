"""CPU: what the restatement of the envelope programs (tests/program_ref.py) promises by itself, before any kernel is compared with it: a
program in one render equals split renders with the next segment set at each boundary, and any split of the calls gives the same bits,
records and queues."""
import numpy as np
import pytest

import polyphony_cases as pcases
import program_cases as gcases
import program_ref as gref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref

f32 = np.float32
FRAMES = sum(gcases.CALLS)


def voices():
    names, records, programs, resamplers, pcm, which = gcases.named_programs(2)
    return [(what, records[k][i], programs[k][i], resamplers[k][i], pcm[k][i]) for what, (k, i) in which.items()]


@pytest.mark.parametrize("what, record, program, table, asset", voices(), ids=[v[0] for v in voices()])
def test_a_program_is_the_split_render_with_a_set_at_each_boundary(what, record, program, table, asset):
    coef = cases.tables()[int(table)] if int(table) != ref.NONE else None
    whole, after, left = gref.render_voice(record, program, coef, asset, FRAMES, 2)
    # by hand: render up to each boundary with the plain voice, then put the next segment in place
    at = gref.boundaries(program, FRAMES)
    state, current, t, parts = record, program[0], 0, []
    for j, b in enumerate(at):
        if b > t:
            o, state, current = ref.render_one(state, current, coef, asset, b - t, 2)
            parts.append(o)
            t = b
        assert gref.complete(current), what
        current = program[j + 1]
    if FRAMES > t:
        o, state, current = ref.render_one(state, current, coef, asset, FRAMES - t, 2)
        parts.append(o)
    assert sref.same_floats(whole, np.concatenate(parts))[0], what
    assert state.tobytes() == after.tobytes() and np.asarray(current).tobytes() == left[0].tobytes()
    assert len(left) == len(program) - len(at)


@pytest.mark.parametrize("seed", range(4))
def test_any_split_of_the_calls_gives_the_same_bits_records_and_queues(seed):
    rng = np.random.default_rng(100 + seed)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 5, 3, 2, True, calls=gcases.CALLS, asset_frames=(1, 200))
    programs = gcases.random_programs(rng, envelopes, 2, share=0.7)
    tables = cases.tables()
    whole, after, left, _ = gref.render(records, programs, resamplers, None, tables, pcm, 300, 2)
    cuts = sorted(set(int(c) for c in rng.integers(0, 301, 6)) | {0, 300})
    state, p_state, parts = records, programs, []
    for a, b in zip(cuts, cuts[1:]):
        o, state, p_state, _ = gref.render(state, p_state, resamplers, None, tables, pcm, b - a, 2)
        parts.append(o)
    assert sref.same_floats(whole, np.concatenate(parts, axis=1))[0] and state.tobytes() == after.tobytes()
    assert all(np.asarray(a).tobytes() == np.asarray(c).tobytes() for la, lc in zip(p_state, left) for a, c in zip(la, lc))


def test_an_empty_queue_is_the_plain_voice():
    rng = np.random.default_rng(9)
    records, envelopes, resamplers, pcm, _, _ = pcases.random_voices(rng, 6, 2, 2, True, calls=(30, 30, 40), asset_frames=(1, 200))
    import polyphony_ref as pref
    want, after, env_after = pref.render(records, envelopes, resamplers, cases.tables(), pcm, 100, 2)
    programs = [[[envelopes[k][i]] for i in range(6)] for k in range(2)]
    got, after1, left, _ = gref.render(records, programs, resamplers, None, cases.tables(), pcm, 100, 2)
    assert sref.same_floats(got, want)[0] and after.tobytes() == after1.tobytes()
    assert all(left[k][i].tobytes() == env_after[k][i].tobytes() for k in range(2) for i in range(6))
