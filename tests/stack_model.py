"""The host model of the whole voice stack for call-sequence tests (tests/test_stack_model.py on the CPU, tests/test_gpu_voice_stack.py on
a GPU): five record tables -- samplers, envelopes with their programs, resamplers, voice filters -- behind one set/get path, the FIR
tables, the polyphony, and the bookkeeping of include/oalsfx_hip.h and DESIGN.md 4 that decides what a render launches and uploads.
StackScript records a list of calls (`ops`), each with what it must give; a render's output and the state behind it come from
program_ref.render and from nothing else.  Every refusal is the host's; nothing here is out of the device's bounds.

What the model keeps for lanes x n voices, lane-major as the batch does: rec (sampler records), prog (a list of envelope records per
voice, the current segment first), res (table indices), filt (the filter the next render finds: flags without LOAD, and the histories a
pending LOAD will have put in place by then) with load_pending (the rows whose LOAD has not gone up yet), tables, lanes, pcm.  The
bookkeeping: horizon (frames), dirty (per table, the rows set since the last render), uploads (per table), given (the voices whose queue
was filled since a set call last emptied it) and queues_made (the queues' table exists)."""
import numpy as np

import biquad_cases as bcases
import biquad_ref as bref
import program_cases as gcases
import program_ref as gref
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from test_sampler_abi import rec
from test_voice_abi import env

f32 = np.float32
ONE = sref.ONE
TABLES = ("samplers", "envelopes", "resamplers", "filters", "programs")
KERNELS = ("k_program_biquad_rows", "k_program_rows", "k_biquad_rows", "k_mix_rows", "k_fir_rows", "k_voice_rows", "k_sampler_rows")
PROGRAM_KERNELS = KERNELS[:2]
SETS = ("set_samplers", "set_envelopes", "set_env_programs", "set_resamplers", "set_filters")
GETS = ("get_samplers", "get_envelopes", "get_env_programs", "get_filters", "get_resamplers")
KINDS = SETS + GETS + ("set_fir_table", "set_polyphony", "render", "play")
SIZES = (1, 63, 64, 65, 129, 7, 30, 100, 200, 257)       # what the filler draws from; 300 is kept for the scratch's growth
SPARE = 7                                                   # the table no voice ever names: cleared and set again in mid-sequence
GLIDE_TO = 200 * ONE
STRETCHES = ("the ladder, down and up, under one continuing sound", "horizon to the frame", "horizon to the frame, a play doing part",
             "a coefficient change on a sounding voice, not waited for", "LOAD pending, then set without LOAD, then render",
             "a program replaced in mid-program", "a program replaced in mid-program, read back before the render",
             "a plain set on a voice with a pending queue", "polyphony up and down with rows pending in every table",
             "a lane kept busy by a filter alone", "scratch growth under load", "streams alternate", "a FIR table replaced behind a render",
             "an unnamed table cleared and set", "a refused call per table with rows pending", "a glide checked against the device's step")
MESSAGES = {"twice": "An instance is listed twice as {} target.", "glides": "A program's segment glides.", "inactive": "A program's segment is not active.",
            "unset": "The resampler names a table that has not been set.", "unknown": "Unknown resampler.", "coefficient": "Non-finite voice filter coefficient.",
            "dropped": "A lane that would be dropped is still in use.", "named": "The FIR table is still named by an instance."}
TARGET = {"samplers": "a sampler", "envelopes": "an envelope", "programs": "an envelope", "resamplers": "a resampler", "filters": "a voice filter"}


def left_when_set(program):
    """The frames a program of two or more has left when it is set: 1 + what its segments but the last still take."""
    return 1 + sum(int(e["delay"]) + int(e["ramp_frames"]) - int(e["ramp_done"]) for e in program[:-1])


class StackScript:
    def __init__(self, seed, n, channels, lanes_max, pool, addresses):
        self.rng = np.random.default_rng(seed)
        self.n, self.channels, self.lanes_max, self.pool, self.addresses = n, channels, lanes_max, pool, addresses
        self.base = 2 if lanes_max > 2 else 1              # the polyphony between the stretches
        self.lanes = 1
        self.rec = np.zeros((1, n), sref.DTYPE)
        self.prog = [[[np.zeros(1, vref.DTYPE)[0]] for _ in range(n)]]
        self.res = np.full((1, n), ref.NONE)
        self.filt = np.zeros((1, n), bref.DTYPE)
        self.pcm = [[pool[0][2]] * n]
        self.tables = dict(cases.tables())                 # (the test sets these on the batch before the first op)
        self.load_pending = set()
        self.given, self.queues_made, self.horizon = set(), False, 0
        self.dirty = {t: set() for t in TABLES}
        self.uploads = dict.fromkeys(TABLES, 0)
        self.step_before = self.rec["step"].copy()
        self.in_flight = False                             # a render has been queued and nothing has waited since
        self.most_frames = 0
        self.length_set = {}                               # the length every voice's program had when it was set
        self.forms = {}
        self.ops = []

    # ---- what the model knows of its state ----
    def voices(self):
        return [(k, i) for k in range(self.lanes) for i in range(self.n)]

    def envelopes(self):
        return gcases.first_segments(self.prog)

    def filters_active(self):
        return bool((self.filt["flags"] & bref.ACTIVE).any())

    def queued(self):
        return [(k, i) for k, i in self.voices() if len(self.prog[k][i]) > 1]

    def kernel(self):
        """The ladder of sampler_queue."""
        if self.horizon > 0:
            return KERNELS[0] if self.filters_active() else KERNELS[1]
        if self.filters_active():
            return "k_biquad_rows"
        if self.lanes >= 2:
            return "k_mix_rows"
        if (self.res != ref.NONE).any():
            return "k_fir_rows"
        return "k_voice_rows" if (self.envelopes()["flags"] & vref.ACTIVE).any() else "k_sampler_rows"

    def snapshot(self):
        return dict(lanes=self.lanes, rec=self.rec.copy(), prog=[[list(p) for p in lane] for lane in self.prog], res=self.res.copy(), filt=self.filt.copy(),
                    tables=dict(self.tables), pcm=[list(lane) for lane in self.pcm])

    def add(self, kind, **fields):
        op = dict(kind=kind, refused=None, lanes=self.lanes, horizon=self.horizon, in_flight=self.in_flight, filters_active=self.filters_active(),
                  queued=len(self.queued()), pending={t: frozenset(rows) for t, rows in self.dirty.items()})
        op.update(fields)
        self.ops.append(op)
        return op

    def targets(self, lane, rows):
        rows = list(range(self.n)) if rows is None else [int(r) for r in rows]
        return rows, [(lane, i) for i in rows]

    def lane_form(self, lane, kind, every):
        """Whether the call names its lane: always above lane 0; at lane 0, where both forms address the same voices, taken in turn for
        the sets and for the gets, on subsets and on all instances."""
        if lane:
            return True
        key = (kind[:3], every)
        self.forms[key] = not self.forms.get(key, True)
        return self.forms[key]

    # ---- the set calls ----
    def set_samplers(self, lane, rows, records, pcm):
        every = rows is None
        rows, voices = self.targets(lane, rows)
        refused = MESSAGES["twice"].format(TARGET["samplers"]) if len(set(rows)) < len(rows) else None
        for (k, i), r in zip(voices, records):
            e = self.prog[k][i][0]
            if not refused and int(e["flags"]) & vref.GLIDE:
                refused = vref.check(e, int(r["step"]))
        op = self.add("set_samplers", lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=np.array(records, sref.DTYPE), refused=refused)
        if refused:
            return op
        for (k, i), r, p in zip(voices, records, pcm):
            self.rec[k][i], self.pcm[k][i] = r, p
        self.dirty["samplers"] |= set(voices)
        return op

    def set_env_programs(self, lane, rows, programs, plain=False):
        """plain: the call is set_envelopes, every program one record."""
        every = rows is None
        rows, voices = self.targets(lane, rows)
        refused = MESSAGES["twice"].format(TARGET["envelopes"]) if len(set(rows)) < len(rows) else None
        for (k, i), p in zip(voices, programs):
            for e in p:
                if refused:
                    break
                if len(p) >= 2 and int(e["flags"]) & vref.GLIDE:
                    refused = MESSAGES["glides"]
                elif vref.check(e, int(self.rec[k][i]["step"])):
                    refused = vref.check(e, int(self.rec[k][i]["step"]))
                elif len(p) >= 2 and not int(e["flags"]) & vref.ACTIVE:
                    refused = MESSAGES["inactive"]
        mid = [v for v in voices if len(self.prog[v[0]][v[1]]) > 1 and v in self.taken_from()]
        op = self.add("set_envelopes" if plain else "set_env_programs", lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every),
                      data=[np.array(p, vref.DTYPE) for p in programs], refused=refused, mid_program=bool(mid) and not refused,
                      empties=[v for v in voices if len(self.prog[v[0]][v[1]]) > 1 and not refused and all(len(p) == 1 for p in programs)],
                      steps_before=[int(self.step_before[k][i]) for k, i in voices], steps_now=[int(self.rec[k][i]["step"]) for k, i in voices],
                      tabled=[int(self.res[k][i]) != ref.NONE for k, i in voices])
        if refused:
            return op
        for (k, i), p in zip(voices, programs):
            self.prog[k][i] = [np.array(e, vref.DTYPE).reshape(()).copy() for e in p]
            self.length_set[(k, i)] = len(p)
            self.dirty["envelopes"].add((k, i))
            if len(p) >= 2:
                self.queues_made = True
                self.given.add((k, i))
                self.dirty["programs"].add((k, i))
                self.horizon = max(self.horizon, left_when_set(p))
            elif self.queues_made and (k, i) in self.given:
                self.given.discard((k, i))
                self.dirty["programs"].add((k, i))
        return op

    def taken_from(self):
        """The voices whose queue the renders have taken a segment from since their program was set."""
        return {v for v, length in self.length_set.items() if v[0] < self.lanes and len(self.prog[v[0]][v[1]]) < length}

    def set_envelopes(self, lane, rows, envelopes):
        return self.set_env_programs(lane, rows, [[e] for e in envelopes], plain=True)

    def set_resamplers(self, lane, rows, tables):
        every = rows is None
        rows, voices = self.targets(lane, rows)
        tables = [int(t) for t in tables]
        refused = MESSAGES["twice"].format(TARGET["resamplers"]) if len(set(rows)) < len(rows) else None
        for t in tables:
            if not refused and not ref.NONE <= t < ref.FIR_TABLES:
                refused = MESSAGES["unknown"]
            elif not refused and t != ref.NONE and t not in self.tables:
                refused = MESSAGES["unset"]
        op = self.add("set_resamplers", lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=np.asarray(tables), refused=refused)
        if refused:
            return op
        for (k, i), t in zip(voices, tables):
            if int(self.res[k][i]) != t:
                self.res[k][i] = t
                self.dirty["resamplers"].add((k, i))
        return op

    def set_filters(self, lane, rows, filters):
        every = rows is None
        rows, voices = self.targets(lane, rows)
        filters = np.array(filters, bref.DTYPE)
        refused = MESSAGES["twice"].format(TARGET["filters"]) if len(set(rows)) < len(rows) else None
        if not refused and not np.isfinite(bref.coefficients(filters)).all():
            refused = MESSAGES["coefficient"]
        loads = bool((filters["flags"] & bref.LOAD).any())
        op = self.add("set_filters", lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=filters, refused=refused, loads=loads,
                      were_active=[bool(self.filt[k][i]["flags"] & bref.ACTIVE) for k, i in voices], were_loading=[v in self.load_pending for v in voices])
        if refused:
            return op
        bcases.set_model(self.filt, filters, lane, rows)
        for v, f in zip(voices, filters):
            if f["flags"] & bref.LOAD:
                self.load_pending.add(v)
        self.dirty["filters"] |= set(voices)
        return op

    def set_fir_table(self, table, coef):
        named = int((self.res == table).sum())
        shape = lambda c: None if c is None else np.shape(c)
        same_shape = coef is not None and shape(self.tables.get(table)) == shape(coef)
        refused = MESSAGES["named"] if named and not same_shape else None
        op = self.add("set_fir_table", table=table, data=None if coef is None else np.array(coef, f32), refused=refused, named=named, same_shape=same_shape)
        if refused:
            return op
        self.in_flight = False                              # (a set-up call: it waits for the renders queued so far)
        if coef is None:
            self.tables.pop(table, None)
        else:
            self.tables[table] = np.array(coef, f32)
        return op

    def busy(self, k, i):
        return [what for what, there in (("sampler", int(self.rec[k][i]["flags"]) & sref.PLAYING), ("envelope", int(self.prog[k][i][0]["flags"]) & vref.ACTIVE),
                                         ("resampler", int(self.res[k][i]) != ref.NONE), ("filter", int(self.filt[k][i]["flags"]) & bref.ACTIVE)) if there]

    def set_polyphony(self, lanes):
        busy = sorted({what for k in range(lanes, self.lanes) for i in range(self.n) for what in self.busy(k, i)})
        refused = MESSAGES["dropped"] if busy else None
        ringing = [(k, i) for k, i in self.voices() if self.busy(k, i) == ["filter"]]
        op = self.add("set_polyphony", to=lanes, refused=refused, busy=busy, ringing=len(ringing), taken=len(self.taken_from() & set(self.queued())))
        if refused or lanes == self.lanes:
            return op
        self.in_flight = False
        keep = min(lanes, self.lanes)
        grown = lambda a, fill: np.concatenate([a[:keep], np.full((lanes - keep, self.n), fill, a.dtype)]) if lanes > keep else a[:keep].copy()
        self.rec, self.res, self.filt = grown(self.rec, np.zeros(1, sref.DTYPE)[0]), grown(self.res, ref.NONE), grown(self.filt, np.zeros(1, bref.DTYPE)[0])
        self.step_before = grown(self.step_before, 0)
        self.prog = self.prog[:keep] + [[[np.zeros(1, vref.DTYPE)[0]] for _ in range(self.n)] for _ in range(lanes - keep)]
        self.pcm = self.pcm[:keep] + [[self.pool[0][2]] * self.n for _ in range(lanes - keep)]
        self.given = {v for v in self.given if v[0] < lanes}
        self.length_set = {v: length for v, length in self.length_set.items() if v[0] < lanes}
        # the whole tables went to the device: no row is pending any more, a LOAD has been carried out, and no counter has moved
        self.load_pending = set()
        self.dirty = {t: set() for t in TABLES}
        self.lanes = lanes
        return op

    # ---- renders ----
    def render(self, frames, side=False, wait=True, offset=0, play=False):
        op = self.add("play" if play else "render", frames=frames, side=side and not play, wait=wait or play, offset=0 if play else offset, kernel=self.kernel(),
                      uploaded={t: len(rows) for t, rows in self.dirty.items()}, before=self.snapshot(), most_before=self.most_frames)
        for t in TABLES:
            self.uploads[t] += 1 if self.dirty[t] else 0
            self.dirty[t] = set()
        self.load_pending = set()
        self.step_before = self.rec["step"].copy()
        filters = self.filt if self.filters_active() else None
        want, self.rec, self.prog, after = gref.render(self.rec, self.prog, self.res, filters, self.tables, self.pcm, frames, self.channels)
        if filters is not None:
            self.filt = after
        op.update(want=want, uploads=dict(self.uploads), after=self.snapshot())
        self.horizon = max(0, self.horizon - frames)
        self.most_frames = max(self.most_frames, frames)
        self.in_flight = not (wait or play)
        return op

    def play(self, frames):
        return self.render(frames, play=True)

    def get(self, what, lane=0, rows=None):
        every = rows is None
        rows, voices = self.targets(lane, rows)
        if what == "env_programs":
            want = [np.array(self.prog[k][i], vref.DTYPE) for k, i in voices]
        else:
            source = dict(samplers=self.rec, envelopes=self.envelopes(), filters=self.filt, resamplers=self.res)[what]
            want = source[lane][rows].copy()
        op = self.add("get_" + what, lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "get", every), want=want)
        self.in_flight = False
        return op


# ---- what the sequences are made of ----
class Maker:
    """Draws records for a StackScript and strings its stretches together."""

    def __init__(self, s):
        self.s, self.rng = s, s.rng
        self.sizes = list(SIZES)

    # -- records --
    def fresh(self, looped=None, step=None, key=None, playing=True):
        """A record on one of the pool's assets, with the asset: looped over the whole asset, or a one-shot."""
        s, rng = self.s, self.rng
        key = int(rng.integers(len(s.pool))) if key is None else key
        fmt, width, data = s.pool[key]
        frames = data.shape[0]
        looped = bool(rng.random() < 0.7) if looped is None else looped
        flags = (sref.PLAYING if playing else 0) | (sref.LOOP if looped else 0) | (sref.LINEAR if rng.random() < 0.5 else 0)
        start, end = 0, frames if looped else 0
        if looped and key != self.f32_key() and rng.random() < 0.3:        # a loop shorter than the taps, with a lead-in
            start = int(rng.integers(0, frames))
            end = min(frames, start + int(rng.integers(1, 4)))
        r = rec(format=fmt, channels=width, frames=frames, flags=flags, loop_start=start, loop_end=end, step=int(rng.integers(ONE // 4, 2 * ONE)) if step is None else step,
                position=int(rng.integers(0, (end if looped else frames) * ONE)), data=s.addresses[key])
        r["gain"][0, :] = 0
        r["gain"][0, :s.channels] = rng.uniform(0.2, 1, s.channels) * rng.choice([-1.0, 1.0], s.channels)
        return r[0], data

    def f32_key(self):
        """The longest fp32 asset of the pool."""
        return max((k for k, (fmt, _, _) in enumerate(self.s.pool) if fmt == sref.PCM_F32), key=lambda k: self.s.pool[k][2].shape[0])

    def segment(self, ramp, delay=0, flags=vref.ACTIVE):
        e = gcases.segment(self.rng, self.s.channels, ramp, delay=delay, flags=flags)
        for name in ("gain_from", "gain_to"):               # (away from zero: a programmed voice is heard)
            e[name][:self.s.channels] = np.where(np.abs(e[name][:self.s.channels]) < 0.2, f32(0.5), e[name][:self.s.channels])
        if ramp:
            e["gain_step"][:self.s.channels] = ((e["gain_to"][:self.s.channels] - e["gain_from"][:self.s.channels]) / f32(ramp)).astype(f32)
        return e

    def program(self, ramps, delays=None):
        delays = delays or [0] * len(ramps)
        return [self.segment(r, delay=d) for r, d in zip(ramps, delays)]

    def envelope(self):
        """A plain envelope: a fade out with STOP, a delayed fade in, a hold, or none."""
        rng, ch = self.rng, self.s.channels
        kind = int(rng.integers(4))
        if kind == 3:
            return np.zeros(1, vref.DTYPE)[0]
        e = env(flags=vref.ACTIVE | (vref.STOP if kind == 0 else 0), delay=int(rng.integers(0, 90)) if kind == 1 else 0)
        vref.ramp(e[0], rng.uniform(0.5, 1, ch) * (kind != 1), rng.uniform(0.5, 1, ch) * (kind != 0), int(rng.integers(0, 300)))
        return e[0]

    def filter(self, active=True, load=False):
        rng = self.rng
        coef = bcases.low_pass(rng.uniform(0.05, 0.45), rng.uniform(0.5, 1.5)) if rng.random() < 0.7 else bcases.band_pass(rng.uniform(0.05, 0.4), rng.uniform(0.4, 1.5))
        f = bcases.filt(coef, (bref.ACTIVE if active else 0) | (bref.LOAD if load else 0))[0]
        if load:
            f["x"], f["y"] = rng.uniform(-0.5, 0.5, (8, 2)).astype(f32), rng.uniform(-0.5, 0.5, (8, 2)).astype(f32)
        return f

    # -- rows: (lane 0, instance 0) is the continuing sound, which only the stretches touch --
    def lane(self):
        return int(self.rng.integers(self.s.lanes))

    def rows(self, lane, most=3):
        first = 1 if lane == 0 else 0
        count = int(self.rng.integers(1, min(most, self.s.n - first) + 1))
        return sorted(int(r) for r in self.rng.choice(np.arange(first, self.s.n), size=count, replace=False))

    def row(self, lane):
        return self.rows(lane, 1)[0]

    def size(self):
        return int(self.rng.choice(self.sizes))

    def render(self, frames=None, wait=None, side=None):
        rng = self.rng
        return self.s.render(self.size() if frames is None else frames, side=bool(rng.integers(2)) if side is None else side,
                             wait=bool(rng.random() < 0.4) if wait is None else wait, offset=int(rng.integers(3)))

    def voices_on(self, lane):
        new = [self.fresh() for _ in range(self.s.n)]
        self.s.set_samplers(lane, None, [r for r, _ in new], [p for _, p in new])

    def quiet(self, lane):
        """Everything that keeps a lane busy cleared, on all its instances; a table in which the lane is idle is left alone."""
        s, n = self.s, self.s.n
        busy = {what for i in range(n) for what in s.busy(lane, i)}
        if "sampler" in busy:
            s.set_samplers(lane, None, np.concatenate([rec(flags=0, data=0)] * n), [s.pool[0][2]] * n)
        if "envelope" in busy or any(len(p) > 1 for p in s.prog[lane]):
            s.set_envelopes(lane, None, np.zeros(n, vref.DTYPE))
        if "resampler" in busy:
            s.set_resamplers(lane, None, [ref.NONE] * n)
        if "filter" in busy:
            s.set_filters(lane, None, np.zeros(n, bref.DTYPE))

    def to_lanes(self, lanes):
        s = self.s
        if lanes > s.lanes:
            first = s.lanes
            s.set_polyphony(lanes)
            for k in range(first, lanes):
                self.voices_on(k)
        elif lanes < s.lanes:
            for k in range(lanes, s.lanes):
                self.quiet(k)
            s.set_polyphony(lanes)
            assert not s.ops[-1]["refused"]

    def start(self):
        """The continuing sound at (lane 0, instance 0): a looping fp32 asset; the other voices of lane 0; then the base polyphony."""
        s = self.s
        new = [self.fresh(looped=True, key=self.f32_key(), step=ONE + 17)] + [self.fresh() for _ in range(s.n - 1)]
        s.set_samplers(0, None, [r for r, _ in new], [p for _, p in new])
        self.to_lanes(s.base)

    def filler(self, count):
        s, rng = self.s, self.rng
        for _ in range(count):
            kind, lane = int(rng.integers(12)), self.lane()
            rows = self.rows(lane)
            if kind == 0:
                new = [self.fresh() for _ in rows]
                for r in rows:                              # (a glide's envelope would hold the row's step where it has room: none is left here)
                    assert not int(s.prog[lane][r][0]["flags"]) & vref.GLIDE
                s.set_samplers(lane, rows, [r for r, _ in new], [p for _, p in new])
            elif kind == 1:
                s.set_envelopes(lane, rows, [self.envelope() for _ in rows])
            elif kind == 2:
                s.set_env_programs(lane, rows, [self.program([int(x) for x in rng.integers(0, 60, int(rng.integers(1, 5)))]) for _ in rows])
            elif kind == 3:
                s.set_resamplers(lane, rows, [int(rng.choice([ref.NONE, 0, 1, 2, 3, 6])) for _ in rows])
            elif kind == 4:
                s.set_filters(lane, rows, [self.filter(active=bool(rng.integers(2)), load=bool(rng.integers(2))) for _ in rows])
            elif kind in (5, 6, 7):
                self.render()
            elif kind == 8:
                s.play(self.size())
            else:
                what = ("samplers", "envelopes", "env_programs", "filters", "resamplers")[int(rng.integers(5))]
                s.get(what, lane, self.rows(lane, s.n) if rng.integers(2) else None)

    # -- the stretches --
    def ladder(self):
        s, rng, n = self.s, self.rng, self.s.n
        sizes = iter([63, 64, 65, 129, 1, 257, 7, 64, 65, 63, 30, 129])
        rung = lambda kernel, **kw: (self.render(next(sizes), **kw), self.expect(kernel))
        self.to_lanes(max(2, s.lanes))
        top = s.lanes - 1
        # down: the filtered programs, the horizon runs out, the filters go, the lanes go, the resamplers go, the envelopes go
        v = self.row(top)
        s.set_filters(0, [0], [self.filter(load=True)])
        s.set_env_programs(top, [v], [self.program([60, 40])])
        rung("k_program_biquad_rows", side=True, wait=False)
        self.burn()
        rung("k_biquad_rows", side=True, wait=False)
        for k in range(s.lanes):
            if (s.filt[k]["flags"] & bref.ACTIVE).any():
                cleared = s.filt[k].copy()
                cleared["flags"] = 0
                s.set_filters(k, None, cleared)
        rung("k_mix_rows", side=True)
        self.to_lanes(1)
        if not (s.res != ref.NONE).any():
            s.set_resamplers(0, [self.row(0)], [1])
        rung("k_fir_rows", side=True, wait=False)
        s.set_resamplers(0, None, [ref.NONE] * n)
        if not (s.envelopes()["flags"] & vref.ACTIVE).any():
            s.set_envelopes(0, [self.row(0)], [self.segment(150, delay=10)])
        rung("k_voice_rows", side=True, wait=False)
        s.set_envelopes(0, None, np.zeros(n, vref.DTYPE))
        rung("k_sampler_rows", side=True)
        # up, in another order: the lanes, a filter, a program, and the filter gone from under the program
        s.set_envelopes(0, [self.row(0)], [self.segment(90)])
        rung("k_voice_rows", wait=False)
        s.set_resamplers(0, [0], [0])
        rung("k_fir_rows", wait=False)
        self.to_lanes(2)
        rung("k_mix_rows", wait=False)
        w = self.row(1)
        s.set_filters(1, [w], [self.filter(load=True)])
        rung("k_biquad_rows", side=True, wait=False)
        s.set_env_programs(0, [self.row(0)], [self.program([40, 60, 20])])
        rung("k_program_biquad_rows", wait=False)
        s.set_filters(1, [w], [self.filter(active=False)])
        rung("k_program_rows", side=True)
        self.to_lanes(s.base)

    def burn(self):
        """Renders until no queue can hold a segment any more."""
        while self.s.horizon > 0:
            self.render(min(self.s.horizon, 200), wait=False)
            assert self.s.ops[-1]["kernel"] in PROGRAM_KERNELS

    def expect(self, kernel):
        assert self.s.ops[-1]["kernel"] == kernel, (self.s.ops[-1]["kernel"], kernel)

    def horizon_to_the_frame(self):
        s = self.s
        for with_play in (False, True):
            lane = self.lane()
            self.burn()
            h = 90
            s.set_env_programs(lane, [self.row(lane)], [self.program([h - 41, 40, 25])])
            assert s.horizon == h
            a = int(self.rng.integers(20, 60))
            if with_play:
                s.play(a)
            else:
                self.render(a, wait=False, side=True)
            self.render(h - 1 - a, wait=False)
            self.render(1, wait=False, side=with_play)
            assert s.ops[-1]["kernel"] in PROGRAM_KERNELS and s.horizon == 0
            self.render(int(self.rng.integers(2, 40)))
            assert s.ops[-1]["kernel"] not in PROGRAM_KERNELS

    def coefficient_change(self):
        s = self.s
        rows = [0] + self.rows(0, 2)
        s.set_filters(0, rows, [self.filter(load=True) for _ in rows])
        self.render(wait=False)
        s.set_filters(0, rows[:2], [self.filter() for _ in rows[:2]])
        self.render(wait=False, side=True)
        s.get("filters", 0, None)

    def load_then_plain(self):
        s = self.s
        lane = 0
        rows = self.rows(lane, 3)
        s.set_filters(lane, rows, [self.filter(load=True) for _ in rows])
        s.set_filters(lane, rows[:1], [self.filter()])
        self.render()
        s.get("filters", lane, rows)

    def program_replaced(self):
        s = self.s
        lane = self.lane()
        v = self.row(lane)
        s.set_env_programs(lane, [v], [self.program([10, 280, 20])])
        for read_back in (False, True):
            self.render(int(self.rng.integers(12, 40)))
            assert len(s.prog[lane][v]) == 2
            self.render(wait=False, frames=int(self.rng.integers(5, 60)), side=read_back)
            s.set_env_programs(lane, [v], [self.program([10, 280, 20])])
            assert s.ops[-1]["mid_program"] and s.ops[-1]["in_flight"]
            if read_back:
                s.get("env_programs", lane, None)
        self.render(30, wait=False)

    def plain_set_on_a_queue(self):
        s = self.s
        lane = self.lane()
        v = self.row(lane)
        s.set_env_programs(lane, [v], [self.program([200, 50, 10])])
        self.render(wait=False, frames=int(self.rng.integers(5, 60)))
        s.set_envelopes(lane, [v], [self.segment(120)])
        assert s.ops[-1]["empties"] == [(lane, v)] and s.ops[-1]["in_flight"]
        before = s.uploads["programs"]
        self.render(wait=False)
        assert s.uploads["programs"] == before + 1
        s.get("env_programs", lane, [v])
        s.get("envelopes", lane, None)

    def polyphony_up_and_down(self):
        s = self.s
        low = min(s.lanes, s.lanes_max - 1)
        self.to_lanes(low)
        a, b, c = (int(x) for x in self.rng.choice(np.arange(1, s.n), 3, replace=False))
        # a voice in mid-program and a voice that has stopped and rings out of its filter
        s.set_env_programs(0, [a], [self.program([10, 250, 30])])
        s.set_samplers(0, [b], [self.fresh(playing=False)[0]], [s.pool[0][2]])
        s.set_envelopes(0, [b], np.zeros(1, vref.DTYPE))
        s.set_resamplers(0, [b], [ref.NONE])
        s.set_filters(0, [b], [self.filter(load=True)])
        self.render(int(self.rng.integers(12, 40)), wait=False)
        # rows pending in every table
        r, p = self.fresh()
        s.set_samplers(0, [c], [r], [p])
        s.set_env_programs(0, [c], [self.program([30, 60])])
        s.set_resamplers(0, [c], [3 if int(s.res[0][c]) != 3 else 2])
        s.set_filters(0, [c], [self.filter(load=True)])
        assert all(s.dirty[t] for t in TABLES)
        counted = dict(s.uploads)
        s.set_polyphony(s.lanes_max)
        self.render(64, wait=False, side=True)
        assert s.uploads == counted
        # the new lane kept busy by a filter alone
        top = s.lanes_max - 1
        s.set_filters(top, [a], [self.filter(load=True)])
        self.render(63, wait=False)
        s.set_filters(0, [b], [self.filter()])             # (a row pending when the refusal and the call that is taken come)
        s.set_polyphony(low)
        assert s.ops[-1]["refused"] and s.ops[-1]["busy"] == ["filter"]
        s.set_filters(top, [a], [self.filter(active=False)])
        s.set_polyphony(low)
        assert not s.ops[-1]["refused"]
        self.render()
        self.to_lanes(s.base)

    def scratch_growth(self):
        s = self.s
        if not s.filters_active():
            s.set_filters(0, [0], [self.filter(load=True)])
        side = bool(self.rng.integers(2))
        self.render(wait=False, side=side)
        self.render(300, wait=False, side=not side)         # (no other render of a sequence has more than 257 frames)
        assert s.ops[-1]["most_before"] < 300

    def streams_alternate(self):
        s = self.s
        lane = self.lane()
        s.set_env_programs(lane, [self.row(lane)], [self.program([120, 120, 9])])
        s.set_filters(0, [0], [self.filter()])
        side = bool(self.rng.integers(2))
        for k in range(4):
            self.render(int(self.rng.choice([1, 63, 64, 65])), wait=k == 3, side=side ^ bool(k % 2))
            assert s.ops[-1]["queued"] and s.ops[-1]["filters_active"]

    def fir_table_replaced(self):
        s = self.s
        s.set_resamplers(0, [0], [0])
        self.render(wait=False, side=bool(self.rng.integers(2)))
        s.set_fir_table(0, ref.sinc(4, 12, float(self.rng.uniform(0.6, 0.95))))
        assert s.ops[-1]["named"] and s.ops[-1]["same_shape"] and s.ops[-1]["in_flight"]
        self.render()

    def refusals(self):
        s, rng = self.s, self.rng
        lane = self.lane()
        first = 1 if lane == 0 else 0
        a, b = (int(x) for x in rng.choice(np.arange(first, s.n), 2, replace=False))
        r, p = self.fresh()
        assert not int(s.prog[lane][a][0]["flags"]) & vref.GLIDE
        s.set_samplers(lane, [a], [r], [p])
        s.set_samplers(lane, [b, b], [r, r], [p, p])
        s.set_envelopes(lane, [a], [self.segment(70, delay=5)])
        step = int(s.rec[lane][b]["step"])
        away = env(flags=vref.ACTIVE | vref.GLIDE, glide_frames=100, glide_slope=-((step << 16) // 100) - 1, step_to=0)[0]
        s.set_envelopes(lane, [b], [away])
        assert s.ops[-1]["refused"] == "leaves the range"
        s.set_env_programs(lane, [a], [self.program([40, 30])])
        gliding = env(flags=vref.ACTIVE | vref.GLIDE)[0]
        vref.glide(gliding, step, step, 10)
        s.set_env_programs(lane, [b], [[gliding, self.segment(5)]])
        s.set_resamplers(lane, [a], [2 if int(s.res[lane][a]) != 2 else 3])
        s.set_fir_table(SPARE, None)
        s.set_resamplers(lane, [b], [SPARE])
        s.set_fir_table(SPARE, cases.tables()[SPARE])
        s.set_filters(lane, [a], [self.filter(load=True)])
        bad = self.filter()
        bad["a1"] = np.inf
        s.set_filters(lane, [b], [bad])
        assert [op["refused"] is not None for op in s.ops[-12:]] == [False, True, False, True, False, True, False, False, True, False, False, True]
        self.render(wait=False)
        s.get("resamplers", lane, None)

    def glide_on_the_devices_step(self):
        s = self.s
        self.to_lanes(max(2, s.lanes))
        lane, v = 1, self.row(1)
        s.set_envelopes(lane, [v], np.zeros(1, vref.DTYPE))
        r, p = self.fresh(looped=True, step=ONE, key=self.f32_key())
        s.set_samplers(lane, [v], [r], [p])
        s.set_resamplers(lane, [v], [1])
        e = env(flags=vref.ACTIVE | vref.GLIDE, sub=12345)[0]
        vref.glide(e, ONE, GLIDE_TO, 100)
        assert s.set_envelopes(lane, [v], [e])["refused"] is None
        self.render(150, wait=False)
        assert int(s.rec[lane][v]["step"]) == GLIDE_TO and int(s.step_before[lane][v]) == ONE
        down = env(flags=vref.ACTIVE | vref.GLIDE, glide_frames=100, glide_slope=-(((150 * ONE) << 16) // 100), step_to=50 * ONE)[0]
        assert vref.check(down, ONE) == "leaves the range" and s.set_envelopes(lane, [v], [down])["refused"] is None
        self.render(120, wait=False)
        s.get("samplers", lane, [v])
        s.set_envelopes(lane, [v], [self.segment(20)])      # (the glide is over: the row's step is anybody's to set again)
        self.to_lanes(s.base)

    def stretches(self):
        return [self.ladder, self.horizon_to_the_frame, self.coefficient_change, self.load_then_plain, self.program_replaced, self.plain_set_on_a_queue,
                self.polyphony_up_and_down, self.scratch_growth, self.streams_alternate, self.fir_table_replaced, self.refusals, self.glide_on_the_devices_step]


def pool_for(seed, channels):
    """The assets of a sequence: one of every PCM format, mono and `channels` wide, of 1 to 500 frames."""
    import polyphony_cases as pcases
    return pcases.random_voices(np.random.default_rng(seed), 1, 1, channels, True, asset_frames=(1, 500))[-1]


SHAPES = [(2, 9, 4, 11), (6, 5, 3, 12), (8, 4, 2, 13), (7, 4, 2, 14)]                  # (channels, n, lanes up to, seed) of the whole sequences
SHORT = ("coefficient_change", "program_replaced", "streams_alternate", "plain_set_on_a_queue")     # the stretches of a sequence of some thirty calls
HOSTED = ("ladder", "program_replaced", "polyphony_up_and_down", "coefficient_change")             # ... of the one the host build of the kernels runs


def build(seed, n, channels, lanes_max, pool, addresses, only=None, filler=(0, 1)):
    """A whole sequence: the start, the stretches (`only`: the names of the Maker's methods to keep) in an order the seed chooses with
    filler between them, and a last render."""
    s = StackScript(seed, n, channels, lanes_max, pool, addresses)
    m = Maker(s)
    m.start()
    blocks = [b for b in m.stretches() if only is None or b.__name__ in only]
    for k in s.rng.permutation(len(blocks)):
        m.filler(int(s.rng.integers(filler[0], filler[1] + 1)))
        blocks[k]()
    m.filler(1)
    m.render(wait=False)
    return s


# ---- what a sequence holds, looked up in the calls themselves ----
def present(ops):
    found = dict.fromkeys(STRETCHES, False)
    kinds = [op["kind"] for op in ops]
    renders = [k for k, kind in enumerate(kinds) if kind in ("render", "play")]
    taken = lambda op, kind: op["kind"] == kind and not op["refused"]
    after = lambda k: next((j for j in renders if j > k), None)
    before = lambda k: max((j for j in renders if j < k), default=None)
    sounding = lambda op: bool(op["want"][0].any())                       # (instance 0 carries the continuing sound)

    # the ladder: the kernels of consecutive renders, repeats taken once, go down all seven rungs... and come up again to the first
    run = []
    for j in renders:
        if not run or run[-1][0] != ops[j]["kernel"]:
            run.append((ops[j]["kernel"], j))
    names = [kernel for kernel, _ in run]
    down = [KERNELS[0]] + list(KERNELS[2:])
    for at in range(len(names) - len(down) + 1):
        if names[at:at + len(down)] == down:
            rest = names[at + len(down):]
            up = [rest.index(k) if k in rest else None for k in ("k_voice_rows", "k_fir_rows", "k_mix_rows", "k_biquad_rows", KERNELS[0], KERNELS[1])]
            last = run[at + len(down) + up[-1]][1] if None not in up else None
            if None not in up and up == sorted(up) and all(sounding(ops[j]) for j in renders if run[at][1] <= j <= last) and set(names) == set(KERNELS):
                found[STRETCHES[0]] = True

    for at, j in enumerate(renders):
        op = ops[j]
        # the horizon: ... two renders that leave 1, a render of 1 frame that still walks the queues, the plain kernel behind it
        if at >= 2 and at + 1 < len(renders) and op["frames"] == 1 and op["horizon"] == 1 and op["kernel"] in PROGRAM_KERNELS and kinds[j] == "render":
            a, b, c = ops[renders[at - 2]], ops[renders[at - 1]], ops[renders[at + 1]]
            set_at = max((k for k in range(renders[at - 2]) if taken(ops[k], "set_env_programs")), default=None)
            whole = set_at is not None and before(renders[at - 2]) in (None, *[r for r in renders if r < set_at])
            if whole and a["kernel"] in PROGRAM_KERNELS and b["kernel"] in PROGRAM_KERNELS and a["horizon"] - a["frames"] - b["frames"] == 1 and c["kernel"] not in PROGRAM_KERNELS:
                found[STRETCHES[2 if "play" in (a["kind"], b["kind"]) else 1]] = True
        # the scratch grows under a render in flight, on the other stream
        if at >= 1 and kinds[j] == "render" and op["filters_active"] and op["frames"] > op["most_before"] and op["in_flight"]:
            prev = ops[renders[at - 1]]
            if renders[at - 1] == j - 1 and prev["kind"] == "render" and prev["filters_active"] and not prev["wait"] and prev["side"] != op["side"]:
                found["scratch growth under load"] = True
        # three renders in a row that alternate between the streams, none waited for
        if at + 2 < len(renders) and renders[at + 2] == j + 2:
            three = [ops[j], ops[j + 1], ops[j + 2]]
            if all(o["kind"] == "render" and o["queued"] and o["filters_active"] for o in three) and not three[0]["wait"] and not three[1]["wait"] \
                    and three[0]["side"] != three[1]["side"] != three[2]["side"]:
                found["streams alternate"] = True

    for k, op in enumerate(ops):
        nxt, prv = after(k), before(k)
        if taken(op, "set_filters") and not op["loads"] and op["rows"] is not None and op["in_flight"] and prv == k - 1 and nxt == k + 1 and all(op["were_active"]):
            if not ops[nxt]["wait"] and kinds[nxt] == "render" and kinds[nxt + 1] == "get_filters" and (op["data"]["flags"] & bref.ACTIVE).all():
                found["a coefficient change on a sounding voice, not waited for"] = True
        if taken(op, "set_filters") and not op["loads"] and any(op["were_loading"]) and nxt is not None:
            if any(kinds[j] == "get_filters" and ops[j]["lane"] == op["lane"] for j in range(nxt + 1, len(ops))):
                found["LOAD pending, then set without LOAD, then render"] = True
        if taken(op, "set_env_programs") and op["mid_program"] and op["in_flight"] and nxt is not None:
            read = any(kinds[j] == "get_env_programs" and ops[j]["lane"] == op["lane"] for j in range(k + 1, nxt))
            found[STRETCHES[6 if read else 5]] = True
        if taken(op, "set_envelopes") and op["empties"] and op["in_flight"] and nxt is not None and prv is not None:
            if ops[nxt]["uploads"]["programs"] == ops[prv]["uploads"]["programs"] + 1 and ops[nxt]["uploaded"]["programs"] >= len(op["empties"]):
                found["a plain set on a voice with a pending queue"] = True
        if taken(op, "set_polyphony") and op["to"] > op["lanes"] and all(op["pending"][t] for t in TABLES) and op["taken"] and op["ringing"] and nxt is not None and prv is not None:
            down_at = next((j for j in range(k + 1, len(ops)) if taken(ops[j], "set_polyphony") and ops[j]["to"] < ops[j]["lanes"]), None)
            if ops[nxt]["uploads"] == ops[prv]["uploads"] and down_at is not None and ops[down_at]["taken"] and ops[down_at]["ringing"] and any(ops[down_at]["pending"].values()):
                found["polyphony up and down with rows pending in every table"] = True
        if op["kind"] == "set_polyphony" and op["refused"] == MESSAGES["dropped"] and op["busy"] == ["filter"]:
            found["a lane kept busy by a filter alone"] = True
        if taken(op, "set_fir_table") and op["same_shape"] and op["named"] and op["in_flight"] and prv is not None and nxt is not None:
            old, new = ops[prv]["before"]["tables"][op["table"]], ops[nxt]["before"]["tables"][op["table"]]
            if old.shape == new.shape and old.tobytes() != new.tobytes() and sounding(ops[prv]) and sounding(ops[nxt]):
                found["a FIR table replaced behind a render"] = True
        if taken(op, "set_fir_table") and op["data"] is None and not op["named"]:
            if any(taken(ops[j], "set_fir_table") and ops[j]["table"] == op["table"] and ops[j]["data"] is not None for j in range(k + 1, len(ops))):
                found["an unnamed table cleared and set"] = True
        if taken(op, "set_envelopes") and len(op["data"]) == 1 and int(op["data"][0][0]["flags"]) & vref.GLIDE and prv == k - 1 and not ops[prv]["wait"]:
            e, old, new = op["data"][0][0], op["steps_before"][0], op["steps_now"][0]
            if old != new and vref.check(e, old) == "leaves the range" and vref.check(e, new) is None and op["lanes"] >= 2 and op["lane"] >= 1 and op["tabled"][0]:
                found["a glide checked against the device's step"] = True
    table_of = dict(zip(SETS, ("samplers", "envelopes", "programs", "resamplers", "filters")))
    refused = {table_of[op["kind"]] for op in ops if op["kind"] in SETS and op["refused"] and op["pending"][table_of[op["kind"]]]}
    found["a refused call per table with rows pending"] = refused == set(TABLES)
    return found


def conditions(ops):
    """What every generated sequence must meet, as {what: whether it does}; tests/test_stack_model.py asserts them on the CPU."""
    renders = [op for op in ops if op["kind"] == "render"]
    sizes = {op["frames"] for op in ops if op["kind"] in ("render", "play")}
    sided = {op["kernel"] for op in renders if op["side"]}
    outs = [op["want"] for op in ops if op["kind"] in ("render", "play")]
    return {"between 70 and 140 ops": 70 <= len(ops) <= 140,
            "a third of the renders not waited for": 3 * sum(not op["wait"] for op in renders) >= len(renders),
            "the caller's stream under four kernels or more": len(sided) >= 4,
            "every op kind": {op["kind"] for op in ops} == set(KINDS),
            "both lane forms, subsets and all instances": all({(bool(op["lane_form"]), op["rows"] is None) for op in ops if op["kind"] in group} == {(a, b) for a in (False, True) for b in (False, True)}
                                                              for group in (SETS, GETS)),
            "sizes between 1 and 300": min(sizes) >= 1 and max(sizes) <= 300,
            "sizes 1, 63, 64, 65 and 64 k + 1": {1, 63, 64, 65} <= sizes and any(x > 65 and x % 64 == 1 for x in sizes),
            "every offset": {op["offset"] for op in renders} == {0, 1, 2},
            "no NaN in the reference": not any(np.isnan(o).any() for o in outs),
            "nine renders in ten are heard": 10 * sum(bool(np.abs(o).max() > 0) for o in outs) >= 9 * len(outs)}


def summary(ops):
    renders = [op for op in ops if op["kind"] == "render"]
    return dict(ops=len(ops), renders=len(renders), not_waited=sum(not op["wait"] for op in renders), plays=sum(op["kind"] == "play" for op in ops),
                kernels=sorted({op["kernel"] for op in ops if op["kind"] in ("render", "play")}, key=KERNELS.index),
                stretches=[what for what, there in present(ops).items() if there])


# ---- comparisons on bit patterns, shared by the CPU and the GPU test ----
QUEUE = np.dtype([("head", np.uint32), ("count", np.uint32), ("reserved", np.uint32, (2,)), ("queue", vref.DTYPE, (gref.PROGRAM_MAX - 1,))])


def queue_rows(programs, taken=None):
    """The queues' rows [lanes][n] as the kernels keep them for `programs`; taken [lanes][n]: how many segments the device has taken
    already (the head; the entries in front of it stay where they were and are not looked at here)."""
    rows = np.zeros((len(programs), len(programs[0])), QUEUE)
    for k, lane in enumerate(programs):
        for i, p in enumerate(lane):
            head = 0 if taken is None else int(taken[k][i])
            rows[k][i]["head"], rows[k][i]["count"] = head, len(p) - 1
            for j, e in enumerate(p[1:]):
                rows[k][i]["queue"][head + j] = e
    return rows


def bits_differ(got, want):
    """Where two float arrays differ on their bit patterns (NaNs by position): the indices, so -0.0 against +0.0 differs."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    if got.shape != want.shape:
        return [("shape", got.shape, want.shape)]
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    return [tuple(int(x) for x in at) for at in np.argwhere(differ)[:8]]


def records_differ(got, want):
    """Where two record arrays of one dtype differ on their bytes: the indices of the records."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", got.shape, want.shape)]
    size = got.dtype.itemsize
    a, w = (np.frombuffer(x.tobytes(), np.uint8).reshape(-1, size) for x in (got, want))
    return [tuple(int(x) for x in np.unravel_index(r, got.shape)) for r in np.nonzero((a != w).any(axis=1))[0][:8]]


def queues_differ(got, want):
    """Queue rows against queue rows: head, count and the `count` entries from the head on."""
    bad = []
    for at in np.ndindex(got.shape):
        g, w = got[at], want[at]
        live = lambda q: q["queue"][int(q["head"]):int(q["head"]) + int(q["count"])].tobytes()
        if int(g["head"]) != int(w["head"]) or int(g["count"]) != int(w["count"]) or live(g) != live(w):
            bad.append(tuple(int(x) for x in at))
    return bad[:8]
