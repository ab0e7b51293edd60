"""The voice-pool life cycle that reset, bus downmix and level meters were built for, as a seeded schedule with its expectation.

`VoicePool` holds the host side and the reference side, and no device: which voices start with what, what they are fed, and what a
fresh `OracleApi` per started voice, `downmix_ref` and `meter_ref` (with carry) make of it.  The one input it takes from outside is the
voices' meter records after each call -- the device's in tests/test_gpu_state_io_paths.py, its own expectation in the CPU test
(tests/test_oracle_follow.py) that checks the schedule's conditions beforehand -- because what frees a voice is the answer to "has the
tail died": a carried quiet_run of FREE_AFTER frames or more."""
import random
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import meter_ref
from downmix_ref import downmix
from harness import OracleApi, noise, preset_effect
from oalsfxpp_amd import desc, lib
from oalsfxpp_amd.workloads import random_effect

N, SLOTS, BUSES, RATE, FMT = 64, 2, 3, 48000, desc.FMT_STEREO
CALLS = 80
FRAMES = {17: 441, 61: 2500, 70: 441}       # the calls that are not 256 frames
DEVICE_STRETCH = range(24, 56)              # calls made as mix_device + downmix_device + meter_device, in runs of RUN unsynchronised calls
RUN = 4
# chosen on the CPU (test_the_voice_pool_schedule_meets_its_conditions prints the counts they give)
SEED, THRESHOLD, FREE_AFTER = 2026, 0.01, 512


def frames_of(k):
    return FRAMES.get(k, 256)


def ring_class(effect_type):
    return lib.load().oalsfx_host_ring_floats(effect_type, RATE)


class VoicePool:
    def __init__(self, seed=SEED, threshold=THRESHOLD, free_after=FREE_AFTER, reset_shadows=True):
        self.rng = random.Random(seed)
        self.threshold, self.free_after = np.float32(threshold), free_after
        self.reset_shadows = reset_shadows      # False: the wrong expectation (a recycled voice's oracle keeps its state), for the control
        self.api = [None] * N
        self.types = [[desc.NULL] * SLOTS for _ in range(N)]
        self.feed = [0] * N                     # calls of noise left
        self.bus, self.gain = [-1] * N, [np.float32(1.0)] * N
        self.want_v, self.want_b = np.zeros(N, meter_ref.DTYPE), np.zeros(BUSES, meter_ref.DTYPE)
        self.starts, self.released, self.retaken = Counter(), Counter(), Counter()
        self.recycles = self.other_type = self.mid_run = 0
        self.pool = ThreadPoolExecutor(max_workers=16)

    # ---- the schedule ----
    def due(self, records):
        """Voices the records free: running, fed out, and quiet for free_after frames or more."""
        return [i for i in range(N) if self.api[i] is not None and self.feed[i] == 0 and int(records["quiet_run"][i]) >= self.free_after]

    def start(self, voices, recycled):
        """Draws what `voices` start with and starts their oracles afresh; returns [(voice, effects, direct send or None, aux send or None,
        bus, gain)] for the device side: reset, set_effect_at, set_send_props, apply_changes, set_routing."""
        out = []
        for i in voices:
            rng = self.rng
            if recycled:
                self.recycles += 1
                for t in self.types[i]:
                    if ring_class(t):
                        self.released[ring_class(t)] += 1
            t0 = self.types[i][0]
            if not recycled or rng.random() < 0.5:
                t0 = rng.choice([t for t in range(12) if t != t0])
                self.other_type += recycled
            types = [t0, rng.choice([desc.NULL, desc.NULL, desc.ECHO, desc.CHORUS, desc.FLANGER, desc.EQUALIZER, desc.EAX_REVERB])]
            effects = [preset_effect(rng.randrange(113)) if t == desc.EAX_REVERB and rng.random() < 0.6 else random_effect(rng, t) for t in types]
            for e in effects:   # tails that die within the run
                if e.type in (desc.REVERB, desc.EAX_REVERB):
                    e.props.reverb.decay_time = min(e.props.reverb.decay_time, rng.uniform(0.1, 0.6))
                if e.type == desc.ECHO:
                    e.props.echo.feedback = min(e.props.echo.feedback, 0.4)
                if e.type in (desc.CHORUS, desc.FLANGER):
                    e.props.chorus.feedback = max(-0.5, min(0.5, e.props.chorus.feedback))
            direct = (rng.uniform(0.3, 1.0), rng.uniform(0.2, 1.0), 1.0) if rng.random() < 0.3 else None
            aux = (rng.randrange(SLOTS), rng.uniform(0.3, 1.0), 1.0, rng.uniform(0.2, 1.0)) if rng.random() < 0.3 else None
            self.types[i] = types
            self.starts[t0] += 1
            if recycled:
                for t in types:
                    if ring_class(t):
                        self.retaken[ring_class(t)] += 1
            self.feed[i] = rng.randint(2, 4)
            self.bus[i], self.gain[i] = rng.randrange(-1, BUSES), np.float32(rng.uniform(0.2, 1.0))
            if self.reset_shadows or self.api[i] is None:
                self.api[i] = OracleApi(FMT, RATE, SLOTS)
            else:
                self.api[i].set_send_props(-1, 1.0, 1.0, 1.0)
                for s in range(SLOTS):
                    self.api[i].set_send_props(s, 1.0, 1.0, 1.0)
            api = self.api[i]
            for s, e in enumerate(effects):
                api.set_effect(s, e)
            if direct:
                api.set_send_props(-1, *direct)
            if aux:
                api.set_send_props(*aux)
            api.apply_changes()
            self.want_v[i] = np.zeros((), meter_ref.DTYPE)
            out.append((i, effects, direct, aux, self.bus[i], self.gain[i]))
        return out

    def input(self, k):
        x = np.zeros((N, frames_of(k), 2), np.float32)
        for i in range(N):
            if self.api[i] is not None and self.feed[i] > 0:
                x[i] = noise(1000 * k + i, frames_of(k), 2) * np.float32(0.5)
        return x

    def fed(self):
        self.feed = [max(0, f - 1) for f in self.feed]

    # ---- the expectation ----
    def expect(self, x):
        """The voices' outputs, the buses and both sets of records (carried) for input x; advances the oracles."""
        y = np.stack(list(self.pool.map(lambda i: self.api[i].mix(x[i]), range(N))))
        buses = downmix(y, self.bus, self.gain, BUSES)
        self.want_v = meter_ref.meter(y, self.threshold, self.want_v)
        self.want_b = meter_ref.meter(buses, self.threshold, self.want_b)
        return y, buses

    def conditions(self):
        """The schedule's conditions, from the schedule itself."""
        classes = sorted({ring_class(t) for t in range(12)} - {0})
        assert all(self.starts[t] >= 3 for t in range(12)), f"a type was started fewer than three times: {dict(self.starts)}"
        assert self.recycles >= 40, f"{self.recycles} recycles"
        assert all(self.released[c] >= 2 and self.retaken[c] >= 2 for c in classes), f"released {dict(self.released)}, retaken {dict(self.retaken)}"
        assert self.other_type >= self.recycles // 4, f"{self.other_type} of {self.recycles} recycled voices came back with another type"
        return (f"starts per type {[self.starts[t] for t in range(12)]}, {self.recycles} recycles ({self.other_type} with another type, "
                f"{self.mid_run} inside a run), released {dict(sorted(self.released.items()))}, retaken {dict(sorted(self.retaken.items()))}")


def drive(pool, dev=None):
    """The 80 calls.  `dev` (tests/test_gpu_state_io_paths.py: PoolDevice) makes every call on the device, compares what it gets with what
    it is handed, and returns the device's voice records, which free the voices; without one the expectation's own records do."""
    records = pool.want_v
    k = 0
    while k < CALLS:
        if k in DEVICE_STRETCH and (k - DEVICE_STRETCH[0]) % RUN == 0:
            # a run of RUN mix_device calls with nothing synchronised between them; every other voice that is due is recycled only
            # between the run's second and third call (the pool acts on the records it read last)
            due = pool.due(records)
            now, later = due[::2], due[1::2]
            started = pool.start(now, True)
            if dev:
                dev.apply(started, routing=(list(pool.bus), list(pool.gain)))
            calls = []
            for j in range(RUN):
                mid = pool.start(later, True) if j == 2 else []
                pool.mid_run += len(mid)
                if dev and mid:
                    dev.apply(mid, routing=None)
                x = pool.input(k + j)
                pool.fed()
                y, buses = pool.expect(x)
                calls.append((x, y, buses, pool.want_v.copy(), pool.want_b.copy(), list(pool.bus), list(pool.gain), [m[0] for m in mid]))
                if dev:
                    dev.queue(x)
            if dev:
                records = dev.finish_run(k, calls, pool.threshold)
            else:
                records = pool.want_v
            k += RUN
            continue
        started = pool.start(range(N) if k == 0 else pool.due(records), k > 0)
        x = pool.input(k)
        pool.fed()
        y, buses = pool.expect(x)
        if dev:
            dev.apply(started, routing=(list(pool.bus), list(pool.gain)))
            records = dev.host_call(k, x, buses, pool.want_v, pool.want_b, pool.threshold)
        else:
            records = pool.want_v
        k += 1
    assert pool.mid_run >= 1, "no recycle landed between two calls of a run of mix_device calls"
    return pool.conditions()
