"""CPU controls for OracleShadow.follow / ShadowArmy.follow (tests/harness.py), on the oracle alone.

`Voices` plays the device's part: one oracle per instance that runs on undisturbed, behind the read-back calls of a `Batch`.  Its
`restore_from` does what oalsfx_batch_restore does as far as a shadow can see: the voice's state and rings continue in another instance
of another batch, and its parameters come back derived anew under another update_seq.  A shadow that followed the voice correctly
matches it bit for bit afterwards; the wrong expectations (one frame short before the switch, the restore taken for a restart, a shadow
that is not reset when its voice is) must be caught by the very comparisons the GPU tests use."""

import numpy as np
import pytest

from harness import OracleShadow, ShadowArmy, make_effect, noise, preset_effect, same_bits
from oalsfxpp_amd import desc, lib
from oracle import oracle as orc

FMT, RATE = desc.FMT_STEREO, 48000


class Voices:
    """The read-back side of a `Batch` over CPU oracles."""

    def __init__(self, n, slots, first_seq=1):
        self.n, self.effect_count, self.channels = n, slots, desc.FORMAT_CHANNELS[FMT]
        self.voice = [orc.Oracle(self.channels, slots) for _ in range(n)]
        self.effects = [[lib.effect_defaults(desc.NULL) for _ in range(slots)] for _ in range(n)]
        self.own_seq = [[0] * slots for _ in range(n)]    # the numbering the voice's oracle counts in
        self.shown_seq = [[first_seq] * slots for _ in range(n)]  # the numbering read_slot shows
        self.sends = [None] * n
        for i in range(n):
            for s in range(slots):
                self._set(i, s, self.effects[i][s], True)

    def _params(self, i, s):
        return lib.derive_slot(FMT, RATE, lib.effect_normalized(self.effects[i][s]))

    def _set(self, i, s, effect, restart):
        self.effects[i][s] = effect
        p = self._params(i, s)
        self.own_seq[i][s] += 1
        self.shown_seq[i][s] += 1
        p.update_seq = self.own_seq[i][s]
        self.voice[i].set_slot(s, p, restart)
        ones = desc.SendProps(1.0, 1.0, 1.0)
        self.sends[i] = lib.derive_source(FMT, RATE, ones, [ones] * self.effect_count, [e.type for e in self.effects[i]])
        self.voice[i].set_source(self.sends[i])

    def set_effect(self, i, s, effect):
        self._set(i, s, effect, effect.type != self.effects[i][s].type)

    def restore_from(self, i, other, j):
        """Instance j of `other` continues here as instance i: same state and rings, parameters under this batch's next update_seq."""
        self.voice[i] = other.voice[j]
        self.effects[i] = list(other.effects[j])
        self.own_seq[i] = list(other.own_seq[j])
        self.sends[i] = other.sends[j]
        for s in range(self.effect_count):
            self.shown_seq[i][s] += 1

    def mix(self, x):
        return np.stack([v.mix(x[i]) for i, v in enumerate(self.voice)])

    def read_slot(self, i, s):
        p = self._params(i, s)
        p.update_seq = self.shown_seq[i][s]
        return p, self.voice[i].state(s)

    def read_ring(self, i, s):
        return self.voice[i].ring(s)

    def read_source(self, i):
        return desc.SourceParams.from_buffer_copy(bytes(self.sends[i])), self.voice[i].source_state()


def x_for(n, call, frames=256):
    return np.stack([noise(100 * call + i, frames, 2) for i in range(n)])


def source_and_target():
    a, b = Voices(3, 2), Voices(5, 2, first_seq=40)
    for i in range(3):
        a.set_effect(i, 0, preset_effect(7 + 30 * i))
        a.set_effect(i, 1, make_effect([desc.CHORUS, desc.ECHO, desc.EQUALIZER][i]))
    for i in range(5):
        b.set_effect(i, 0, make_effect(desc.FLANGER))
    return a, b


@pytest.mark.parametrize("inside_cross_fade", [False, True])
def test_a_shadow_that_follows_its_voice_matches_it(inside_cross_fade):
    a, b = source_and_target()
    army = ShadowArmy(a, [2, 0])
    for k in range(4):
        assert not army.differing(a.mix(x_for(3, k)), army.mix(x_for(3, k)))
    if inside_cross_fade:
        # new taps 64 frames before the switch: the cross-fade (OALSFX_RV_FADE_SAMPLES) is in flight, and folding the renumbered
        # parameters in a second time would start it over
        for i in (0, 2):
            a.set_effect(i, 0, preset_effect(50 + i))
        x = x_for(3, 9, 64)
        assert not army.differing(a.mix(x), army.mix(x))
    b.restore_from(4, a, 2)
    b.restore_from(1, a, 0)
    army.follow(b, [4, 1])
    for k in range(4, 8):
        x = x_for(5, k, 100 if k == 5 else 256)
        assert not army.differing(b.mix(x), army.mix(x)), f"call {k}"
    assert army.compare_state() == {}
    # an update in the target afterwards is an update for the oracle too
    b.set_effect(4, 0, preset_effect(3))
    x = x_for(5, 8)
    assert not army.differing(b.mix(x), army.mix(x))
    assert army.compare_state() == {}


def test_one_frame_short_before_the_switch_is_caught():
    a, b = source_and_target()
    shadow = OracleShadow(a, 1)
    for k in range(3):
        x = x_for(3, k)
        assert same_bits(a.mix(x)[1], shadow.mix(x[1]))[0]
    x = x_for(3, 3)
    a.mix(x)
    shadow.mix(x[1][:255])   # the voice got 256 frames
    b.restore_from(2, a, 1)
    shadow.follow(b, 2)
    x = x_for(5, 4)
    assert not same_bits(b.mix(x)[2], shadow.mix(x[2]))[0], "a shadow one frame behind its voice went unnoticed in the output"
    assert shadow.compare_state(), "a shadow one frame behind its voice went unnoticed in the state"


def test_a_restore_taken_for_a_restart_is_caught():
    a, b = source_and_target()
    shadow = OracleShadow(a, 0)
    for k in range(3):
        x = x_for(3, k)
        assert same_bits(a.mix(x)[0], shadow.mix(x[0]))[0]
    b.restore_from(3, a, 0)
    shadow.follow(b, 3, restart=True)
    x = x_for(5, 3)
    assert not same_bits(b.mix(x)[3], shadow.mix(x[3]))[0], "a shadow that restarted at the restore went unnoticed in the output"
    assert shadow.compare_state(), "a shadow that restarted at the restore went unnoticed in the state"


def test_a_shadow_not_reset_with_its_voice_is_caught():
    """The voice pool's control: a recycled voice is a fresh Api.  A shadow that keeps its oracle across the recycle differs even
    when the voice comes back with the type it had."""
    a, _ = source_and_target()
    kept, fresh = OracleShadow(a, 0), OracleShadow(a, 0)
    for k in range(3):
        x = x_for(3, k)
        y = a.mix(x)
        assert same_bits(y[0], kept.mix(x[0]))[0] and same_bits(y[0], fresh.mix(x[0]))[0]
    for s in range(2):              # reset and started again with what it held
        effect = a.effects[0][s]
        a.set_effect(0, s, lib.effect_defaults(desc.NULL))
        a.set_effect(0, s, effect)
    fresh = OracleShadow(a, 0)
    kept.seq = [None] * 2           # (it sees the new parameters, but takes them for an update: the type is the one it knows)
    x = x_for(3, 3)
    y = a.mix(x)
    assert same_bits(y[0], fresh.mix(x[0]))[0]
    assert not same_bits(y[0], kept.mix(x[0]))[0], "a shadow that kept its state across a recycle went unnoticed"


def test_the_voice_pool_schedule_meets_its_conditions():
    """tests/voice_pool.py on the oracle, downmix_ref and meter_ref alone: the seed, threshold and free-after count the GPU test runs with
    give a schedule that starts every type at least three times, recycles at least 40 voices because of quiet_run, releases and retakes
    every ring size class at least twice and recycles inside a run of unsynchronised mix_device calls."""
    import voice_pool
    print(voice_pool.drive(voice_pool.VoicePool()))


def test_a_voice_pool_whose_shadows_are_not_reset_is_caught():
    """The same schedule with the wrong expectation -- a recycled voice's oracle keeps its state -- gives other records (and so another
    schedule): the comparison the GPU test makes on every call would fail."""
    import voice_pool
    right, wrong = voice_pool.VoicePool(), voice_pool.VoicePool(reset_shadows=False)
    voice_pool.drive(right)
    try:
        voice_pool.drive(wrong)
    except AssertionError:
        pass
    assert not voice_pool.meter_ref.same_records(right.want_v, wrong.want_v) or right.recycles != wrong.recycles
