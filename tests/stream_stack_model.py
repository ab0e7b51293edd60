"""The host model of the whole voice stack as it stands now, for call-sequence tests (tests/test_stream_stack_model.py on the CPU,
tests/test_gpu_stream_stack.py on a GPU): stack_model's five record tables and, on top of them, the filter sweeps, the filter programs
and the sampler streams, with the bookkeeping of include/oalsfx_hip.h and DESIGN.md 4 that decides which of the thirteen kernels of
sampler_queue a render launches, what it uploads first and which calls wait.  StreamScript records a list of calls (`ops`), each with
what it must give; a render's output and the state behind it come from stream_ref.render and from nothing else (a sweep is a filter
program of one).  Every refusal is the host's; nothing here is out of the device's bounds, and check_bounds() walks the ops to say so.

What the model keeps per voice (lane, instance) beyond stack_model's: streams (the current record and the ring's waiting entries, as the
device has them behind every render so far), queued (the entries put into the ring since the stream was last set), taken (the device's
count, which the model knows because it renders), host_taken (the host's last reading of it), fprog (the filter program, the current
sweep first), sweep_set and fp_set (the rows a set call has left something in).  Per batch: made (the rings' table exists), ahead (a render
has walked the rings since the last reading), the three horizons, and the lanes.  The number of open rings is by the host's reading:
queued != host_taken.

Where the header leaves a behaviour open the model follows batch.cpp: a refused set_polyphony and a refused GLIDE envelope have read
the taken counts back before they refuse, so rings that were dry are closed behind them; sweep_horizon runs only under a render that
looks at the sweeps, so it can outlive a batch whose filters were all switched off; the first stream, envelope program and filter
program of two or more on a batch each wait for the batch's stream once."""
import numpy as np

import biquad_ref as bref
import filter_program_ref as fref
import resample_ref as ref
import sampler_ref as sref
import stack_model as sm
import stream_ref as stref
import sweep_ref as wref
import voice_ref as vref
from stack_model import MESSAGES, SIZES, bits_differ, records_differ      # noqa: F401 (shared with the tests)
from test_sampler_abi import rec
from test_voice_abi import env

f32 = np.float32
ONE = sref.ONE
RING = stref.QUEUE
TABLES = sm.TABLES + ("sweeps", "filter_programs")
STREAM_KERNELS = ("k_stream_filter_rows", "k_stream_rows")
KERNELS = STREAM_KERNELS + ("k_filter_program_env_rows", "k_filter_program_rows", "k_sweep_program_rows", "k_sweep_rows") + sm.KERNELS
SETS = sm.SETS + ("set_streams", "append_streams", "set_sweeps", "set_filter_programs")
GETS = sm.GETS + ("get_streams", "get_stream_state", "get_sweeps", "get_filter_programs")
KINDS = SETS + GETS + ("set_polyphony", "render", "play")
FULL, GLIDING, STREAMS_GLIDE = "The stream queue is full.", "The gliding voice streams.", "The streaming voice's envelope glides."
TWICE = {"set_streams": "a stream", "append_streams": "a stream", "set_sweeps": "a filter sweep", "set_filter_programs": "a filter program"}
STRETCHES = ("an append with room by the stale count", "an append that needs a read-back", "an append to a truly full ring",
             "a set over a half-played ring", "set, then append, with no render in between", "an append after reset was consumed",
             "a plain set over an open ring", "underrun and restart without a state call", "the kernel name through a stream's life",
             "a ring carrying 17 entries", "set_polyphony while busy", "the glide pair", "takes inside tiles that also switch segments",
             "a play with open rings", "the filter programs' horizon to the frame", "the filter programs' horizon to the frame, under envelope programs",
             "a filter program replaced in mid-program", "a filter program replaced in mid-program, read back before the render",
             "a sweep set on a sounding voice", "set_filters on a swept and programmed voice with rows pending", "a refused call per new table with rows pending")
NO_SWEEP = np.zeros(1, wref.DTYPE)[0]


def idle():
    return np.zeros(1, sref.DTYPE)


class StreamScript(sm.StackScript):
    def __init__(self, seed, n, channels, lanes_max, pool, addresses):
        super().__init__(seed, n, channels, lanes_max, pool, addresses)
        self.base = 2 if lanes_max > 2 else 1
        self.dirty = {t: set() for t in TABLES}
        self.uploads = dict.fromkeys(TABLES, 0)
        self.assets = {(int(a), int(p.shape[0])): p for a, (_, _, p) in zip(addresses, pool)}
        self.streams = [[idle() for _ in range(n)]]
        self.ring_queued, self.taken, self.host_taken = (np.zeros((1, n), np.int64) for _ in range(3))
        self.fprog = [[[NO_SWEEP.copy()] for _ in range(n)]]
        self.sweep_set, self.fp_set = np.zeros((1, n), bool), np.zeros((1, n), bool)
        self.made = self.fp_made = self.ahead = False
        self.sweep_horizon = self.fp_horizon = 0
        self.ring_dirty, self.reset_rows = set(), set()
        self.kind_forms = {}
        self.fp_taken = {}                                  # per voice: the filter segments taken since its program was set
        self.history = {}                                   # per voice, since its stream was last set: S(et) R(ender) A(ppend) B (read back)
        self.dry_renders = {}                               # per voice: the renders in a row it began at its end with an empty ring

    # ---- what the model knows of its state ----
    def open_rings(self):
        return int((self.ring_queued != self.host_taken).sum()) if self.made else 0

    def device_open(self):
        return sum(len(s) > 1 for lane in self.streams for s in lane)

    def kernel(self):
        """The ladder of sampler_queue, all thirteen rungs."""
        rings, biquads = self.open_rings() > 0, self.filters_active()
        queues = self.queues_made if rings else self.horizon > 0
        swept = biquads and (rings or self.sweep_horizon > 0)
        filter_queues = biquads and (self.fp_made if rings else self.fp_horizon > 0)
        if rings:
            return STREAM_KERNELS[0] if biquads else STREAM_KERNELS[1]
        if filter_queues:
            return "k_filter_program_env_rows" if queues else "k_filter_program_rows"
        if swept:
            return "k_sweep_program_rows" if queues else "k_sweep_rows"
        return super().kernel()

    def walks(self):
        """(whether the next render looks at the envelope queues, at the sweeps, at the filter queues): what its horizons run under."""
        rings, biquads = self.open_rings() > 0, self.filters_active()
        return (self.queues_made if rings else self.horizon > 0, biquads and (rings or self.sweep_horizon > 0),
                biquads and (self.fp_made if rings else self.fp_horizon > 0))

    def snapshot(self):
        return dict(lanes=self.lanes, streams=[[s.copy() for s in lane] for lane in self.streams], taken=self.taken.copy(), queued=self.ring_queued.copy(),
                    prog=[[list(p) for p in lane] for lane in self.prog], res=self.res.copy(), filt=self.filt.copy(),
                    fprog=[[[s.copy() for s in p] for p in lane] for lane in self.fprog], tables=dict(self.tables), rec=self.rec.copy())

    def add(self, kind, **fields):
        if "lane_form" in fields:
            # whether the call names its lane: always above lane 0; at lane 0, where both forms address the same voices, taken in turn for
            # every call kind by itself, on subsets and on all instances
            key = (kind, fields["rows"] is None)
            self.kind_forms[key] = not self.kind_forms.get(key, True)
            fields["lane_form"] = bool(fields["lane"]) or self.kind_forms[key]
        op = super().add(kind, waits=False, open=self.open_rings(), device_open=self.device_open(), ahead=self.ahead, horizons=(self.horizon, self.sweep_horizon, self.fp_horizon),
                         reset_rows=frozenset(self.reset_rows), ring_pending=frozenset(self.ring_dirty))
        op.update(fields)
        return op

    def waited(self, op):
        op["waits"] = True
        self.in_flight = False

    def read_taken(self, op):
        """stream_taken_read_back: nothing where no render has walked the rings since the last reading."""
        if not (self.made and self.ahead):
            return
        before = self.open_rings()
        self.host_taken = self.taken.copy()
        self.ahead = False
        for v, h in self.history.items():
            self.history[v] = h + "B"
        op["read_back"], op["closed_by_read"] = True, before - self.open_rings()
        self.waited(op)

    def sync(self, k, i):
        self.rec[k][i] = self.streams[k][i][0]

    def glides(self, k, i):
        return int(self.prog[k][i][0]["flags"]) & (vref.ACTIVE | vref.GLIDE) == vref.ACTIVE | vref.GLIDE

    # ---- the streams' calls ----
    def set_streams(self, lane, rows, streams, plain=False):
        """plain: the call is set_samplers, every stream one record."""
        every = rows is None
        rows, voices = self.targets(lane, rows)
        kind = "set_samplers" if plain else "set_streams"
        streams = [np.array(s, sref.DTYPE).reshape(-1) for s in streams]
        refused = MESSAGES["twice"].format("a sampler" if plain else "a stream") if len(set(rows)) < len(rows) else None
        for (k, i), s in zip(voices, streams):
            if not refused and len(s) > 1 and self.glides(k, i):
                refused = STREAMS_GLIDE
        for (k, i), s in zip(voices, streams):
            e = self.prog[k][i][0]
            if not refused and int(e["flags"]) & vref.GLIDE:
                refused = vref.check(e, int(s[0]["step"]))
        half = [v for v in voices if len(self.streams[v[0]][v[1]]) > 1 and self.taken[v] > 0 and self.history.get(v, "").count("R")]
        op = self.add(kind, lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=np.concatenate(streams) if plain else streams,
                      refused=refused, half_played=half, over_open=[v for v in voices if self.made and self.ring_queued[v] != self.host_taken[v]])
        if refused:
            return op
        if any(len(s) > 1 for s in streams) and not self.made:
            self.made = True
            self.waited(op)                                 # (the rings' table is made: the batch's stream is waited for once)
        for v, s in zip(voices, streams):
            k, i = v
            self.streams[k][i] = s.copy()
            self.sync(k, i)
            self.dirty["samplers"].add(v)
            self.history[v], self.dry_renders[v] = "S", 0
            if len(s) == 1 and not (self.made and (self.ring_queued[v] or self.host_taken[v])):
                self.taken[v] = 0
                continue
            self.ring_queued[v], self.taken[v], self.host_taken[v] = len(s) - 1, 0, 0
            self.ring_dirty.add(v)
            self.reset_rows.add(v)
        return op

    def set_samplers(self, lane, rows, records, pcm=None):
        return self.set_streams(lane, rows, [np.array(r, sref.DTYPE).reshape(1) for r in records], plain=True)

    def append_streams(self, lane, rows, entries):
        every = rows is None
        rows, voices = self.targets(lane, rows)
        entries = [np.array(e, sref.DTYPE).reshape(-1) for e in entries]
        refused = MESSAGES["twice"].format("a stream") if len(set(rows)) < len(rows) else None
        for (k, i), e in zip(voices, entries):
            if not refused and len(e) and self.glides(k, i):
                refused = STREAMS_GLIDE
        waiting = lambda v: int(self.ring_queued[v] - self.host_taken[v])
        op = self.add("append_streams", lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=entries, refused=refused, read_back=False,
                      stale=[int(self.taken[v] - self.host_taken[v]) for v in voices], room_by_host=[RING - waiting(v) for v in voices],
                      room=[RING - int(self.ring_queued[v] - self.taken[v]) for v in voices], histories=[self.history.get(v, "") for v in voices],
                      dry=[self.dry_renders.get(v, 0) for v in voices], asked=[len(e) for e in entries])
        if refused or not any(len(e) for e in entries):
            return op
        if not self.made:
            self.made = True
            self.waited(op)
        short = lambda: any(len(e) > RING - waiting(v) for v, e in zip(voices, entries))
        if short():
            self.read_taken(op)
            if short():
                op["refused"] = FULL
                return op
        for v, e in zip(voices, entries):
            if len(e):
                k, i = v
                self.streams[k][i] = stref.append(self.streams[k][i], e)
                self.ring_queued[v] += len(e)
                self.ring_dirty.add(v)
                self.history[v] = self.history.get(v, "") + "A"
        op["queued_after"] = [int(self.ring_queued[v]) for v in voices]
        return op

    # ---- the envelopes: a GLIDE is refused on a voice whose ring may hold an entry ----
    def set_env_programs(self, lane, rows, programs, plain=False):
        _, voices = self.targets(lane, rows)
        fields = {}
        if len(set(voices)) == len(voices):
            for v, p in zip(voices, programs):
                glides = len(p) == 1 and int(p[0]["flags"]) & (vref.ACTIVE | vref.GLIDE) == vref.ACTIVE | vref.GLIDE
                if glides and self.made and self.ring_queued[v] != self.host_taken[v]:
                    probe = {}
                    self.read_taken(probe)
                    fields.update(probe, glide_on_open=True, dry_on_device=len(self.streams[v[0]][v[1]]) == 1)
                    if self.ring_queued[v] != self.host_taken[v]:
                        op = self.add("set_envelopes" if plain else "set_env_programs", lane=lane, rows=rows, lane_form=self.lane_form(lane, "set", rows is None),
                                      data=[np.array(q, vref.DTYPE) for q in programs], refused=GLIDING, mid_program=False, empties=[], **fields)
                        return op
                    break
        first = not self.queues_made
        op = super().set_env_programs(lane, rows, programs, plain)
        op.update(fields)
        if fields.get("waits") or (first and self.queues_made):
            self.waited(op)
        return op

    # ---- the filters, their sweeps and programs ----
    def set_filters(self, lane, rows, filters):
        _, voices = self.targets(lane, rows)
        swept = [v for v in voices if wref.under_way(self.fprog[v[0]][v[1]][0]) or len(self.fprog[v[0]][v[1]]) > 1]
        op = super().set_filters(lane, rows, filters)
        op["cancels"] = [] if op["refused"] else swept
        if op["refused"]:
            return op
        for v in voices:
            self.empty_filter_queue(v)
            if self.sweep_set[v]:
                self.sweep_set[v] = False
                self.dirty["sweeps"].add(v)
            self.fprog[v[0]][v[1]] = [NO_SWEEP.copy()]
        return op

    def empty_filter_queue(self, v):
        if self.fp_made and self.fp_set[v]:
            self.fp_set[v] = False
            self.dirty["filter_programs"].add(v)

    def set_filter_programs(self, lane, rows, programs, plain=False):
        """plain: the call is set_sweeps, every program one record."""
        every = rows is None
        rows, voices = self.targets(lane, rows)
        kind = "set_sweeps" if plain else "set_filter_programs"
        refused = MESSAGES["twice"].format(TWICE[kind]) if len(set(rows)) < len(rows) else None
        if not refused and not all(1 <= len(p) <= fref.MAX for p in programs):
            refused = fref.MESSAGES["length"]
        for (k, i), p in zip(voices, programs):
            for j, s in enumerate(p):
                if refused:
                    break
                refused = wref.check(s)
                if not refused and len(p) >= 2 and not int(s["flags"]) & wref.ACTIVE:
                    refused = fref.MESSAGES["active"]
                elif not refused and j >= 1 and int(s["done"]):
                    refused = fref.MESSAGES["started"]
                elif not refused and int(s["flags"]) & wref.ACTIVE and not int(self.filt[k][i]["flags"]) & bref.ACTIVE:
                    refused = wref.MESSAGES["filter"]
        mid = [v for v in voices if len(self.fprog[v[0]][v[1]]) > 1 and self.fp_taken.get(v)]
        op = self.add(kind, lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "set", every), data=[np.array(p, wref.DTYPE) for p in programs],
                      refused=refused, mid_program=bool(mid) and not refused,
                      sounding=[bool(int(self.rec[k][i]["flags"]) & sref.PLAYING and int(self.filt[k][i]["flags"]) & bref.ACTIVE) for k, i in voices])
        if refused:
            return op
        if any(len(p) >= 2 for p in programs) and not self.fp_made:
            self.fp_made = True
            self.waited(op)
        for v, p in zip(voices, programs):
            p = [np.array(s, wref.DTYPE).reshape(()).copy() for s in p]
            self.fp_taken[v] = 0
            if len(p) == 1:
                self.empty_filter_queue(v)
                something = bool(p[0].tobytes().strip(b"\0"))
                if not something and not self.sweep_set[v]:
                    continue
                self.sweep_set[v] = something
                self.dirty["sweeps"].add(v)
                self.fprog[v[0]][v[1]] = p
                if int(p[0]["flags"]) & wref.ACTIVE:
                    self.sweep_horizon = max(self.sweep_horizon, int(p[0]["frames"]) - int(p[0]["done"]))
                continue
            self.sweep_set[v] = self.fp_set[v] = True
            self.dirty["sweeps"].add(v)
            self.dirty["filter_programs"].add(v)
            self.fprog[v[0]][v[1]] = p
            in_front = sum(int(s["frames"]) - int(s["done"]) for s in p[:-1])
            self.fp_horizon = max(self.fp_horizon, 1 + in_front)
            self.sweep_horizon = max(self.sweep_horizon, in_front + int(p[-1]["frames"]) - int(p[-1]["done"]))
        return op

    def set_sweeps(self, lane, rows, sweeps):
        return self.set_filter_programs(lane, rows, [[s] for s in sweeps], plain=True)

    # ---- the polyphony ----
    def busy(self, k, i):
        return super().busy(k, i) + (["ring"] if self.made and self.ring_queued[k][i] != self.host_taken[k][i] else [])

    def set_polyphony(self, lanes):
        probe = {}
        if lanes != self.lanes:
            self.read_taken(probe)                          # (a set-up call reads everything back before it refuses anything)
        was, resets, flight = self.lanes, frozenset(self.reset_rows), self.in_flight or bool(probe)
        op = super().set_polyphony(lanes)
        op.update(probe, resets_pending=len(resets), was_in_flight=flight, kept_taken=int(self.taken[:min(lanes, was)].sum()))
        if lanes != was:
            self.waited(op)
        if op["refused"] or lanes == was:
            return op
        keep = min(lanes, was)
        grown = lambda a, fill: np.concatenate([a[:keep], np.full((lanes - keep, self.n), fill, a.dtype)])
        self.ring_queued, self.taken, self.host_taken = grown(self.ring_queued, 0), grown(self.taken, 0), grown(self.host_taken, 0)
        self.sweep_set, self.fp_set = grown(self.sweep_set, False), grown(self.fp_set, False)
        self.streams = self.streams[:keep] + [[idle() for _ in range(self.n)] for _ in range(lanes - keep)]
        self.fprog = self.fprog[:keep] + [[[NO_SWEEP.copy()] for _ in range(self.n)] for _ in range(lanes - keep)]
        self.history = {v: h for v, h in self.history.items() if v[0] < lanes}
        self.fp_taken = {v: t for v, t in self.fp_taken.items() if v[0] < lanes}
        self.dirty = {t: set() for t in TABLES}
        self.ring_dirty, self.reset_rows = set(), set()
        return op

    # ---- renders ----
    def render(self, frames, side=False, wait=True, offset=0, play=False):
        walks = self.walks()
        op = self.add("play" if play else "render", frames=frames, side=side and not play, wait=wait or play, offset=0 if play else offset, kernel=self.kernel(),
                      uploaded={t: len(rows) for t, rows in self.dirty.items()}, before=self.snapshot(), most_before=self.most_frames, walks=walks)
        for t in TABLES:
            self.uploads[t] += 1 if self.dirty[t] else 0
            self.dirty[t] = set()
        self.load_pending, self.ring_dirty, self.reset_rows = set(), set(), set()
        self.step_before = self.rec["step"].copy()
        takes, switches, f_switches = {}, {}, {}
        for v in self.voices():
            k, i = v
            s, p, fp = self.streams[k][i], self.prog[k][i], self.fprog[k][i]
            self.dry_renders[v] = self.dry_renders.get(v, 0) + 1 if len(s) == 1 and stref.at_end(s[0]) else 0
            if len(s) > 1:
                coef = self.tables[int(self.res[k][i])] if int(self.res[k][i]) != ref.NONE else None
                takes[v] = stref.render_voice(s, 0, p, coef, self.assets, frames, self.channels)[4]
            if len(p) > 1:
                switches[v] = [int(x) for x in np.cumsum([int(e["delay"]) + int(e["ramp_frames"]) - int(e["ramp_done"]) for e in p[:-1]]) if x < frames]
            if len(fp) > 1 and int(self.filt[k][i]["flags"]) & bref.ACTIVE:
                f_switches[v] = [int(x) for x in np.cumsum([int(e["frames"]) - int(e["done"]) for e in fp[:-1]]) if x < frames]
        want, self.streams, taken, self.prog, self.filt, self.fprog = stref.render(self.streams, self.taken, self.prog, self.res, self.tables, self.assets, frames,
                                                                                  self.channels, filters=self.filt, filter_programs=self.fprog)
        self.streams = [[np.array(s, sref.DTYPE) for s in lane] for lane in self.streams]
        self.prog = [[list(p) for p in lane] for lane in self.prog]
        assert all(int(taken[v]) - int(self.taken[v]) == len(t) for v, t in takes.items())
        for v, p in f_switches.items():
            self.fp_taken[v] = self.fp_taken.get(v, 0) + len(p)
        self.taken = taken.astype(np.int64)
        for k, i in self.voices():
            self.sync(k, i)
        rings = op["kernel"] in STREAM_KERNELS
        for v in self.history:
            self.history[v] += "R"
        op.update(want=want, uploads=dict(self.uploads), after=self.snapshot(), takes=takes, switches=switches, filter_switches=f_switches)
        if walks[1] or walks[2]:
            self.sweep_horizon = max(0, self.sweep_horizon - frames)
        self.fp_horizon = max(0, self.fp_horizon - frames)
        self.horizon = max(0, self.horizon - frames)
        self.ahead = self.ahead or rings
        self.most_frames = max(self.most_frames, frames)
        self.in_flight = not (wait or play)
        op["waits"] = not self.in_flight
        return op

    def get(self, what, lane=0, rows=None):
        if what in sm.TABLES or what == "env_programs":
            op = super().get(what, lane, rows)
            op["waits"] = True
            return op
        every = rows is None
        rows, voices = self.targets(lane, rows)
        op = self.add("get_" + what, lane=lane, rows=None if every else rows, lane_form=self.lane_form(lane, "get", every))
        if what in ("streams", "stream_state"):
            self.read_taken(op)
        self.waited(op)
        if what == "streams":
            op["want"] = [self.streams[k][i].copy() for k, i in voices]
        elif what == "stream_state":
            op["want"] = (np.array([self.taken[v] for v in voices], np.uint32), np.array([self.ring_queued[v] - self.taken[v] for v in voices], np.uint32))
        elif what == "sweeps":
            op["want"] = np.array([self.fprog[k][i][0] for k, i in voices], wref.DTYPE)
        else:
            op["want"] = [np.array(self.fprog[k][i], wref.DTYPE) for k, i in voices]
        return op


# ---- what the sequences are made of ----
class Maker(sm.Maker):
    """Draws records for a StreamScript and strings its stretches together."""

    def __init__(self, s):
        super().__init__(s)
        self.long_key = max(range(len(s.pool)), key=lambda k: s.pool[k][2].shape[0])
        assert s.pool[self.long_key][2].shape[0] >= 250

    # -- records --
    def chunks(self, lengths, step=ONE, key=None, linear=False):
        """A one-shot over the first sum(lengths) frames of one of the pool's assets, cut into chunks of `lengths` frames: at step ONE
        from position 0 the takes fall on the running sums of the lengths."""
        s, rng = self.s, self.rng
        total = sum(lengths)
        fits = [k for k in range(len(s.pool)) if s.pool[k][2].shape[0] >= total]
        key = int(rng.choice(fits)) if key is None else key
        fmt, width, data = s.pool[key]
        r = rec(format=fmt, channels=width, frames=total, flags=sref.PLAYING | (sref.LINEAR if linear else 0), step=step, position=0, data=s.addresses[key])
        r["gain"][0, :] = 0
        r["gain"][0, :s.channels] = rng.uniform(0.3, 1, s.channels) * rng.choice([-1.0, 1.0], s.channels)
        out = stref.chunks(r[0], list(lengths))
        first = 0
        for c, n in zip(out, lengths):
            s.assets[stref.asset_key(c)] = data[first:first + n]
            first += n
        return out

    def one_shot(self):
        return self.fresh(looped=False)[0]

    def sweep(self, voice, frames, done=0):
        """A sweep from the coefficients the voice's filter has to a fresh stable design."""
        k, i = voice
        to = bref.coefficients(self.filter())
        return wref.make(bref.coefficients(self.s.filt[k][i]), to, frames, done)[0]

    def filter_program(self, voice, lengths):
        k, i = voice
        nodes = [np.asarray(bref.coefficients(self.s.filt[k][i]), f32)] + [np.asarray(bref.coefficients(self.filter()), f32) for _ in lengths]
        return fref.chain(nodes, list(lengths))

    def render(self, frames=None, wait=None, side=None):
        rng = self.rng
        return self.s.render(self.size() if frames is None else frames, side=bool(rng.integers(2)) if side is None else side,
                             wait=bool(rng.random() < 0.1) if wait is None else wait, offset=int(rng.integers(3)))

    def rows(self, lane, most=3):
        count = int(self.rng.integers(1, min(most, self.s.n) + 1))
        return sorted(int(r) for r in self.rng.choice(np.arange(self.s.n), size=count, replace=False))

    def pick(self, count, lane=0):
        return [(lane, int(i)) for i in self.rng.choice(np.arange(self.s.n), count, replace=False)]

    def plain(self, voices, playing=True):
        """Plain records on the voices, one call per lane: their rings are empty and closed by the host's count at once."""
        for lane in sorted({k for k, _ in voices}):
            rows = sorted(i for k, i in voices if k == lane)
            new = [self.fresh(looped=True)[0] if playing else rec(flags=0, data=0)[0] for _ in rows]
            self.s.set_samplers(lane, rows, new)

    def quiet(self, lane):
        s = self.s
        self.plain([(lane, i) for i in range(s.n) if s.made and s.ring_queued[lane][i] != s.host_taken[lane][i]], playing=False)
        super().quiet(lane)

    def entries(self, lengths, **kw):
        return self.chunks(lengths, **kw) if len(lengths) else np.zeros(0, sref.DTYPE)

    def no_glide(self, voices, glides_only=False):
        """No envelope on the voices: the takes of a stretch fall where its chunks end (glides_only: but for a GLIDE, the envelopes stay)."""
        for k, i in voices:
            p = self.s.prog[k][i]
            if int(p[0]["flags"]) & vref.GLIDE or not glides_only and (len(p) > 1 or int(p[0]["flags"])):
                self.s.set_envelopes(k, [i], np.zeros(1, vref.DTYPE))

    def minus_zero(self):
        """A voice under an envelope that holds the gain 0: its frames are zeros with the signs of its samples."""
        s = self.s
        self.calm(filters=True)
        v, = self.pick(1)
        e = env(flags=vref.ACTIVE)[0]
        vref.ramp(e, np.zeros(s.channels), np.zeros(s.channels), 0)
        s.set_samplers(0, [v[1]], [self.fresh(looped=True, key=self.f32_key())[0]])
        s.set_envelopes(0, [v[1]], [e])
        self.render(64, wait=False)

    def calm(self, filters=False):
        """No ring open by the host's count, no horizon left; filters: no filter ACTIVE either."""
        s = self.s
        self.plain([v for v in s.voices() if s.made and s.ring_queued[v] != s.host_taken[v]])
        if filters:
            for k in range(s.lanes):
                if (s.filt[k]["flags"] & bref.ACTIVE).any():
                    s.set_filters(k, None, np.zeros(s.n, bref.DTYPE))
        self.burn()
        assert s.open_rings() == 0 and (s.horizon, s.sweep_horizon, s.fp_horizon) == (0, 0, 0)

    def burn(self):
        s = self.s
        while max(s.horizon, s.fp_horizon, s.sweep_horizon if s.filters_active() else 0) > 0:
            self.render(min(max(s.horizon, s.fp_horizon, s.sweep_horizon), 257), wait=False)
        if s.sweep_horizon:                                 # (no filter is ACTIVE: the sweeps' horizon runs only under one)
            s.set_filters(0, [0], [self.filter(load=True)])
            while s.sweep_horizon:
                self.render(min(s.sweep_horizon, 257), wait=False)
            s.set_filters(0, [0], np.zeros(1, bref.DTYPE))

    def filler(self, count):
        s, rng = self.s, self.rng
        for _ in range(count):
            kind, lane = int(rng.integers(20)), self.lane()
            rows = self.rows(lane)
            voices = [(lane, r) for r in rows]
            every = rng.random() < 0.2
            if every:
                rows, voices = list(range(s.n)), [(lane, r) for r in range(s.n)]
            where = None if every else rows
            filtered = all(int(s.filt[v]["flags"]) & bref.ACTIVE for v in voices)
            if kind == 0:
                self.no_glide(voices, True)
                s.set_samplers(lane, where, [self.fresh()[0] for _ in rows])
            elif kind in (1, 2):
                self.no_glide(voices, True)
                s.set_streams(lane, where, [self.chunks([int(x) for x in rng.integers(1, 50, int(rng.integers(2, 6)))], step=int(rng.integers(ONE // 2, 2 * ONE)),
                                                        linear=bool(rng.integers(2))) for _ in rows])
            elif kind in (3, 4):
                self.no_glide(voices, True)
                room = min(RING - int(s.ring_queued[v] - s.host_taken[v]) for v in voices) if s.made else RING
                if room:
                    s.append_streams(lane, where, [self.entries([int(x) for x in rng.integers(1, 50, int(rng.integers(0 if len(rows) > 1 else 1, min(room, 3) + 1)))])
                                                   for _ in rows])
            elif kind == 5:
                s.set_envelopes(lane, where, [self.envelope() for _ in rows])
            elif kind == 6:
                s.set_env_programs(lane, where, [self.program([int(x) for x in rng.integers(0, 60, int(rng.integers(1, 5)))]) for _ in rows])
            elif kind == 7:
                s.set_resamplers(lane, where, [int(rng.choice([ref.NONE, 0, 1, 2, 3, 6])) for _ in rows])
            elif kind == 8:
                s.set_filters(lane, where, [self.filter(active=bool(rng.integers(4)), load=bool(rng.integers(2))) for _ in rows])
            elif kind == 9 and filtered:
                s.set_sweeps(lane, where, [self.sweep(v, int(rng.integers(1, 200))) for v in voices])
            elif kind == 10 and filtered:
                s.set_filter_programs(lane, where, [self.filter_program(v, [int(x) for x in rng.integers(1, 90, int(rng.integers(1, 5)))]) for v in voices])
            elif kind == 11:
                s.play(self.size())
            elif kind == 12:
                what = ("samplers", "envelopes", "env_programs", "filters", "resamplers", "streams", "stream_state", "sweeps", "filter_programs")[int(rng.integers(9))]
                s.get(what, lane, where)
            else:
                self.render()

    # -- the streams' stretches --
    def appends(self):
        """A stale count with room; a read-back that finds exactly the room there is; a truly full ring; set then append; the reset
        consumed; a set over a half-played ring."""
        s = self.s
        v, w, u = self.pick(3)
        self.no_glide([v, w, u])
        s.set_streams(0, [v[1]], [self.chunks([30, 30, 150])])
        self.render(40, wait=False)
        s.append_streams(0, [v[1]], [self.chunks([20, 20])])
        assert not s.ops[-1]["read_back"] and s.ops[-1]["stale"] == [1]
        self.render(63, wait=False, side=True)
        # full by the host's count, three taken on the device; a second ring that the read-back shows dry
        s.set_streams(0, [v[1], w[1]], [self.chunks([10] * (1 + RING)), self.chunks([10, 10])])
        s.append_streams(0, [w[1]], [self.chunks([5])])    # set, then append: one row carries both
        self.render(35, wait=False)
        s.append_streams(0, [v[1]], [self.chunks([10, 10, 10])])
        op = s.ops[-1]
        assert not op["refused"] and op["read_back"] and op["closed_by_read"] >= 1 and op["room_by_host"] == [0] and op["room"] == [3]
        self.render(1, wait=False, side=True)
        assert s.ops[-1]["open"] == op["open"] - op["closed_by_read"]
        # truly full now, by the host's count and by the device's: refused whole, the voice with room untouched
        s.append_streams(0, [v[1], u[1]], [self.chunks([10]), self.chunks([10])])
        assert s.ops[-1]["refused"] == FULL and s.ops[-1]["room"][0] == 0 and s.ops[-1]["room"][1] >= 1
        # set, render, append, render: no read-back, the second upload does not zero the count again
        s.set_streams(0, [u[1]], [self.chunks([15, 15, 15])])
        self.render(20, wait=False)
        s.append_streams(0, [u[1]], [self.chunks([15, 15])])
        self.render(30, wait=False, side=True)
        assert s.history[u] == "SRAR" and s.taken[u] == 3
        # a set over the ring the device is half-way through
        s.set_streams(0, [v[1]], [self.chunks([25, 25, 25])])
        assert s.ops[-1]["half_played"] == [v] and s.ops[-1]["in_flight"]
        self.render(60, wait=False)
        assert s.taken[v] == 2

    def plain_set_and_restart(self):
        s = self.s
        v, w = self.pick(2)
        self.no_glide([v, w])
        s.set_streams(0, [v[1], w[1]], [self.chunks([40, 40, 40]), self.chunks([12, 12])])
        self.render(30, wait=False)
        s.set_samplers(0, [v[1]], [self.chunks([50])[0]])
        assert s.ops[-1]["over_open"] == [v] and s.ops[-1]["in_flight"]
        self.render(64, wait=False, side=True)              # (w is dry for the whole of this render)
        s.append_streams(0, [v[1], w[1]], [self.chunks([20]), self.chunks([33, 9])])
        assert s.ops[-1]["dry"][1] >= 1 and not s.ops[-1]["read_back"]
        self.render(65, wait=False)
        assert s.ops[-1]["takes"][w][0] == 0

    def life(self):
        """The kernel through a stream's life, under a filter and without one."""
        s = self.s
        for filtered in (True, False):
            self.calm(filters=True)
            v, = self.pick(1)
            self.no_glide([v])
            if filtered:
                s.set_filters(0, [v[1]], [self.filter(load=True)])
            name = STREAM_KERNELS[0 if filtered else 1]
            s.set_streams(0, [v[1]], [self.chunks([20, 20, 20])])
            for k, frames in enumerate((30, 64, 7)):        # dry from the second on: the host cannot know
                self.render(frames, wait=False, side=bool(k % 2) ^ filtered)
                self.expect(name)
            s.get("stream_state", 0, None if filtered else [v[1]])
            assert s.ops[-1]["closed_by_read"] == 1
            self.render(30, wait=False, side=True)
            assert s.ops[-1]["kernel"] not in STREAM_KERNELS
            s.append_streams(0, [v[1]], [self.chunks([9, 9])])
            self.render(30, wait=False, side=filtered)
            self.expect(name)
            self.render(63, wait=False, side=not filtered)
            self.expect(name)

    def seventeen(self):
        s = self.s
        self.calm(filters=True)                             # (k_stream_rows: the host build of that kernel replays these renders)
        v, = self.pick(1)
        self.no_glide([v])
        s.set_streams(0, [v[1]], [self.chunks([10] * (1 + RING))])
        for count in (RING, 4):
            self.render(45, wait=False)
            self.render(45, wait=False, side=True)
            s.set_resamplers(0, [v[1]], [int(self.rng.choice([ref.NONE, 1]))])
            s.append_streams(0, [v[1]], [self.chunks([10] * count)])
            assert not s.ops[-1]["refused"]
        self.render(45, wait=False)
        assert s.ring_queued[v] >= 17 and s.taken[v] >= 17

    def polyphony_while_busy(self):
        s = self.s
        low = s.lanes_max - 1
        self.to_lanes(low)
        a, b, c = self.pick(3)
        self.no_glide([a, b])
        s.set_streams(0, [a[1]], [self.chunks([10, 10, 10, 200])])
        self.render(25, wait=False)
        s.set_streams(0, [b[1]], [self.chunks([30, 30])])
        s.set_polyphony(low + 1)
        assert s.ops[-1]["resets_pending"] and s.ops[-1]["was_in_flight"] and s.ops[-1]["kept_taken"] >= 2
        s.set_streams(low, [c[1]], [self.chunks([10, 10, 10])])
        self.render(15, wait=False, side=True)
        s.set_streams(0, [b[1]], [self.chunks([40, 10])])   # (a row that carries `reset` when the refusal and the call that is taken come)
        s.set_polyphony(low)
        assert s.ops[-1]["refused"] == MESSAGES["dropped"] and "ring" in s.ops[-1]["busy"]
        self.render(40, wait=False)
        s.set_polyphony(low)
        assert not s.ops[-1]["refused"] and s.ops[-1]["resets_pending"] == 0
        s.get("stream_state", 0, None)
        assert s.ops[-1]["want"][0][a[1]] >= 3
        s.set_streams(0, [b[1]], [self.chunks([40, 10])])
        s.set_polyphony(low + 1)
        s.get("stream_state", low, None)
        s.set_polyphony(low)
        self.to_lanes(s.base)

    def glide_pair(self):
        s = self.s
        g, h = self.pick(2)
        self.no_glide([g, h])
        s.set_streams(0, [g[1], h[1]], [self.chunks([10, 10]), self.chunks([10, 200, 10])])
        self.render(30, wait=False)
        step = int(s.rec[g]["step"])
        e = env(flags=vref.ACTIVE | vref.GLIDE)[0]
        vref.glide(e, step, step, 10)
        s.set_envelopes(0, [g[1]], [e])
        assert not s.ops[-1]["refused"] and s.ops[-1]["glide_on_open"] and s.ops[-1]["dry_on_device"] and s.ops[-1]["read_back"]
        s.set_streams(0, [g[1]], [self.chunks([10, 10], step=step)])
        s.append_streams(0, [g[1]], [self.chunks([10], step=step)])
        assert [op["refused"] for op in s.ops[-2:]] == [STREAMS_GLIDE] * 2
        s.set_envelopes(0, [h[1]], [e])
        assert s.ops[-1]["refused"] == GLIDING
        self.render(30, wait=False)
        s.set_envelopes(0, [g[1]], np.zeros(1, vref.DTYPE))

    def takes_and_switches(self):
        """Takes at 70 and 129 (a render's last frame) under an envelope program that switches at 75; a take at 110 under a filter program
        that switches at 100; a dry voice appended to between the renders, taken at frame 0 of the next: on alternating streams."""
        s = self.s
        a, b, c = self.pick(3)
        self.no_glide([a, b, c])
        s.set_streams(0, [a[1], b[1], c[1]], [self.chunks([70, 59, 40, 60]), self.chunks([110, 50, 60]), self.chunks([20, 20])])
        s.set_resamplers(0, [a[1], b[1], c[1]], [ref.NONE] * 3)
        s.set_env_programs(0, [a[1], b[1], c[1]], [self.program([75, 30, 150]), self.program([0]), self.program([0])])
        s.set_filters(0, [b[1]], [self.filter(load=True)])
        s.set_filter_programs(0, [b[1]], [self.filter_program(b, [100, 60, 90])])
        self.render(129, wait=False, side=False)
        op = s.ops[-1]
        assert op["takes"][a] == [70, 129] and op["switches"][a] == [75, 105] and op["takes"][b] == [110] and op["filter_switches"][b] == [100]
        s.append_streams(0, [c[1]], [self.chunks([30, 30])])
        self.render(64, wait=False, side=True)
        assert s.ops[-1]["takes"][c][0] == 0
        self.render(65, wait=False, side=False)

    def play_with_rings(self):
        s = self.s
        v, = self.pick(1)
        self.no_glide([v])
        s.set_streams(0, [v[1]], [self.chunks([10, 10, 10, 100])])
        s.play(64)
        assert s.ops[-1]["kernel"] in STREAM_KERNELS and len(s.ops[-1]["takes"][v]) == 3

    # -- the sweeps' and the filter programs' --
    def horizons(self):
        s = self.s
        for programmed in (False, True):
            self.calm(filters=True)
            self.plain(s.voices())                          # (whole assets and no FIR table: the filter programs' host build replays these renders)
            for k in range(s.lanes):
                s.set_resamplers(k, None, [ref.NONE] * s.n)
            v, w = self.pick(2)
            s.set_filters(0, [v[1]], [self.filter(load=True)])
            if programmed:
                s.set_env_programs(0, [w[1]], [self.program([290, 10])])
            s.set_filter_programs(0, [v[1]], [self.filter_program(v, [50, 40, 60])])
            assert (s.fp_horizon, s.sweep_horizon) == (91, 150)
            names = ("k_filter_program_env_rows", "k_sweep_program_rows") if programmed else ("k_filter_program_rows", "k_sweep_rows")
            a = int(self.rng.integers(20, 60))
            for frames, name in ((a, names[0]), (90 - a, names[0]), (1, names[0]), (1, names[1]), (57, names[1]), (1, names[1]),
                                 (30, "k_program_biquad_rows" if programmed else "k_biquad_rows")):
                self.render(frames, wait=False, side=bool(frames % 2))
                self.expect(name)

    def filter_program_replaced(self):
        s = self.s
        self.calm()
        v, = self.pick(1)
        s.set_filters(0, [v[1]], [self.filter(load=True)])
        s.set_filter_programs(0, [v[1]], [self.filter_program(v, [10, 280, 20])])
        for read_back in (False, True):
            self.render(int(self.rng.integers(12, 40)), wait=False)
            self.render(wait=False, frames=int(self.rng.integers(5, 60)), side=read_back)
            s.set_filter_programs(0, [v[1]], [self.filter_program(v, [10, 280, 20])])
            assert s.ops[-1]["mid_program"] and s.ops[-1]["in_flight"]
            if read_back:
                s.get("filter_programs", 0, None)
        self.render(30, wait=False)

    def sweep_on_a_sounding_voice(self):
        s = self.s
        self.calm()
        v, = self.pick(1)
        self.no_glide([v])
        s.set_samplers(0, [v[1]], [self.fresh(looped=True)[0]])
        s.set_filters(0, [v[1]], [self.filter(load=True)])
        self.render(wait=False)
        s.set_sweeps(0, [v[1]], [self.sweep(v, 100)])
        assert s.ops[-1]["sounding"] == [True] and s.ops[-1]["in_flight"]
        self.render(63, wait=False, side=True)
        self.render(64, wait=False)
        s.get("sweeps", 0, [v[1]])

    def cancel_and_refusals(self):
        s = self.s
        self.calm()
        x, y, z = self.pick(3)
        s.set_filters(0, [x[1], y[1]], [self.filter(load=True), self.filter(load=True)])
        s.set_filters(0, [z[1]], [self.filter(active=False)])
        s.set_filter_programs(0, [x[1]], [self.filter_program(x, [30, 60])])
        self.render(20, wait=False)
        s.set_filter_programs(0, [y[1]], [self.filter_program(y, [40, 40])])
        s.set_filters(0, [x[1]], [self.filter()])
        assert s.ops[-1]["cancels"] == [x] and y in s.ops[-1]["pending"]["filter_programs"] and y in s.ops[-1]["pending"]["sweeps"]
        self.render(30, wait=False, side=True)
        s.set_sweeps(0, [y[1]], [self.sweep(y, 50)])
        s.set_filter_programs(0, [x[1]], [self.filter_program(x, [20, 20])])
        s.set_sweeps(0, [z[1]], [self.sweep(z, 50)])
        bad = self.sweep(x, 50)
        bad["to"][3] = np.inf
        s.set_sweeps(0, [x[1]], [bad])
        s.set_filter_programs(0, [x[1]], [self.filter_program(x, [5] * 9)])
        assert [op["refused"] for op in s.ops[-3:]] == [wref.MESSAGES["filter"], wref.MESSAGES["finite"], fref.MESSAGES["length"]]
        before = dict(s.uploads)
        self.render(30, wait=False)
        assert s.uploads["sweeps"] == before["sweeps"] + 1 and s.uploads["filter_programs"] == before["filter_programs"] + 1
        s.get("filters", 0, None)

    def forms(self):
        """Every set call and every get call in both lane forms, on a subset and on all instances: at lane 0, where the two forms address
        the same voices, four calls of every kind."""
        s, rng = self.s, self.rng
        self.no_glide([(0, i) for i in range(s.n)])
        for every in (False, True, False, True):
            rows = list(range(s.n)) if every else self.rows(0, s.n - 1)
            where, voices = None if every else rows, [(0, i) for i in rows]
            s.set_filters(0, where, [self.filter(load=True) for _ in rows])
            s.set_sweeps(0, where, [self.sweep(v, int(rng.integers(20, 120))) for v in voices])
            s.set_filter_programs(0, where, [self.filter_program(v, [int(x) for x in rng.integers(10, 70, 3)]) for v in voices])
            s.set_samplers(0, where, [self.fresh()[0] for _ in rows])
            s.set_streams(0, where, [self.chunks([int(x) for x in rng.integers(5, 40, 3)]) for _ in rows])
            s.append_streams(0, where, [self.chunks([int(x) for x in rng.integers(5, 40, 2)]) for _ in rows])
            s.set_envelopes(0, where, [self.envelope() for _ in rows])
            s.set_env_programs(0, where, [self.program([int(x) for x in rng.integers(5, 60, 3)]) for _ in rows])
            s.set_resamplers(0, where, [int(rng.choice([ref.NONE, 0, 1, 2, 3, 6])) for _ in rows])
            assert not any(op["refused"] for op in s.ops[-9:])
            self.render(wait=False)
            self.render(wait=False)
        for every in (False, True, False, True):
            for what in ("samplers", "envelopes", "env_programs", "filters", "resamplers", "streams", "stream_state", "sweeps", "filter_programs"):
                s.get(what, 0, None if every else self.rows(0, s.n - 1))
            self.render(wait=False)
            self.render(wait=False)

    def old_ladder(self):
        self.calm(filters=True)
        self.s.set_envelopes(0, None, np.zeros(self.s.n, vref.DTYPE))
        self.s.set_resamplers(0, None, [ref.NONE] * self.s.n)
        self.plain(self.s.voices())
        if self.s.lanes_max >= 2:
            self.ladder()
        else:
            raise AssertionError("the ladder needs two lanes")

    def stretches(self):
        return [self.appends, self.plain_set_and_restart, self.life, self.seventeen, self.polyphony_while_busy, self.glide_pair, self.takes_and_switches,
                self.play_with_rings, self.forms, self.minus_zero, self.horizons, self.filter_program_replaced, self.sweep_on_a_sounding_voice, self.cancel_and_refusals, self.old_ladder]


# (channels, instances, lanes up to, seed) of the whole sequences.  Mono is rendered at one lane throughout -- the store sink, where a lone
# voice's -0.0f must survive --; its second lane exists only inside the polyphony stretch and the old ladder's k_mix_rows rung.
SHAPES = [(2, 9, 4, 31), (6, 5, 3, 32), (8, 4, 2, 33), (7, 4, 2, 34), (1, 3, 2, 35)]
SHORT = ("appends", "plain_set_and_restart", "glide_pair", "sweep_on_a_sounding_voice")


def build(seed, n, channels, lanes_max, pool, addresses, only=None, filler=(1, 3)):
    s = StreamScript(seed, n, channels, lanes_max, pool, addresses)
    m = Maker(s)
    m.plain(s.voices())
    m.to_lanes(s.base)
    blocks = [b for b in m.stretches() if only is None or b.__name__ in only]
    for k in s.rng.permutation(len(blocks)):
        m.filler(int(s.rng.integers(filler[0], filler[1] + 1)))
        blocks[k]()
    m.filler(2)
    m.render(wait=False)
    return s


pool_for = sm.pool_for


# ---- what a sequence holds, looked up in the calls themselves ----
def unwaited(ops):
    """The indices of the renders that nothing waits for before the next call has been made: not waited for themselves, and the call
    behind them neither reads anything back nor waits otherwise."""
    return [k for k, op in enumerate(ops) if op["kind"] == "render" and not op["wait"] and k + 1 < len(ops) and not ops[k + 1]["waits"]]


def present(ops):
    found = dict.fromkeys(STRETCHES, False)
    renders = [k for k, op in enumerate(ops) if op["kind"] in ("render", "play")]
    after = lambda k: next((j for j in renders if j > k), None)
    before = lambda k: max((j for j in renders if j < k), default=None)
    ok = lambda op, kind: op["kind"] == kind and not op["refused"]
    voices_of = lambda op: [(op["lane"], i) for i in (op["rows"] if op["rows"] is not None else range(len(op["data"])))]
    lively = set(unwaited(ops))
    life, names = [], set()
    for k, op in enumerate(ops):
        nxt, prv = after(k), before(k)
        streams_next = nxt is not None and ops[nxt]["kernel"] in STREAM_KERNELS
        if ok(op, "append_streams") and any(op["asked"]):
            asked = [(v, a, j) for j, (v, a) in enumerate(zip(voices_of(op), op["asked"])) if a]
            if op["in_flight"] and not op["read_back"] and any(op["stale"][j] > 0 for _, _, j in asked) and streams_next:
                found[STRETCHES[0]] = True
            # (the rings the read-back showed dry are closed: the count of open rings that chooses the next render's kernel has fallen by them)
            if op["read_back"] and any(op["room_by_host"][j] < a == op["room"][j] for _, a, j in asked) and op["closed_by_read"] >= 1 and streams_next and \
                    nxt == k + 1 and ops[nxt]["open"] == op["open"] - op["closed_by_read"]:
                found[STRETCHES[1]] = True
            if any(op["histories"][j] == "S" for _, _, j in asked) and nxt is not None and all(o["kind"] != "render" for o in ops[k:nxt]):
                found[STRETCHES[4]] = True
            if any(op["histories"][j] == "SR" and len(ops[prv]["takes"].get(v, ())) >= 1 for v, _, j in asked) and nxt is not None:
                if any(len(ops[nxt]["takes"].get(v, ())) >= 1 and "B" not in op["histories"][j] for v, _, j in asked):
                    found[STRETCHES[5]] = True
            if any(op["dry"][j] >= 1 and not op["read_back"] and ops[nxt]["takes"].get(v, [None])[0] == 0 for v, _, j in asked if nxt is not None):
                found[STRETCHES[7]] = True
            if any(q >= 17 for q in op["queued_after"]):
                found[STRETCHES[9]] = True
        if op["kind"] == "append_streams" and op["refused"] == FULL and any(r >= a > 0 for r, a in zip(op["room"], op["asked"])) and \
                any(r < a for r, a in zip(op["room"], op["asked"])):
            found[STRETCHES[2]] = True
        if ok(op, "set_streams") and op["half_played"] and op["in_flight"] and nxt is not None and not op["waits"]:
            v = op["half_played"][0]
            if int(ops[nxt]["before"]["taken"][v]) == 0 and len(ops[nxt]["takes"].get(v, ())) >= 1:
                found[STRETCHES[3]] = True
        if ok(op, "set_samplers") and op["over_open"] and op["in_flight"]:
            if any(ok(o, "append_streams") and set(voices_of(o)) & set(op["over_open"]) for o in ops[k + 1:]):
                found[STRETCHES[6]] = True
        # the kernel through a stream's life: rings that are dry on the device and open by the host's count, a state call that closes
        # them, the ladder's rung, an append, the rings' kernel again -- under either of the two, on each of the two HIP streams
        if op["kind"] == "render" and op["kernel"] in STREAM_KERNELS and op["device_open"] == 0 and op["uploaded"]["samplers"] == 0 and not op["ring_pending"]:
            life = [("dry", op["kernel"])]
        elif op["kind"] == "get_stream_state" and life and life[-1][0] == "dry" and op.get("closed_by_read") and ops[k]["open"] == op["closed_by_read"]:
            life.append(("closed", life[-1][1]))
        elif op["kind"] == "render" and life and life[-1][0] == "closed":
            life = [("rung", life[-1][1])] if op["kernel"] not in STREAM_KERNELS and k in lively else []
        elif ok(op, "append_streams") and life and life[-1][0] == "rung":
            life.append(("appended", life[-1][1]))
        elif op["kind"] == "render" and life and life[-1][0] == "appended":
            if op["kernel"] == life[-1][1]:
                names.add(op["kernel"])
            life = []
        elif op["kind"] in ("render", "play") or op.get("read_back"):
            life = []
        if op["kind"] == "set_polyphony":
            if not op["refused"] and op["to"] > op["lanes"] and op["resets_pending"] and op["was_in_flight"] and op["kept_taken"]:
                rest = ops[k + 1:]
                refused = next((j for j, o in enumerate(rest) if o["kind"] == "set_polyphony" and o["refused"] == MESSAGES["dropped"] and "ring" in o["busy"]), None)
                if refused is not None and any(ok(o, "set_polyphony") and o["to"] == rest[refused]["to"] for o in rest[refused + 1:]):
                    found[STRETCHES[10]] = True
        if op["kind"] == "set_envelopes" and op.get("glide_on_open") and not op["refused"] and op["dry_on_device"] and op["read_back"]:
            g = voices_of(op)[0]
            later = [o for o in ops[k + 1:k + 4] if o["refused"] == STREAMS_GLIDE and voices_of(o) == [g]]
            if {o["kind"] for o in later} == {"set_streams", "append_streams"} and any(o["kind"] == "set_envelopes" and o["refused"] == GLIDING for o in ops):
                found[STRETCHES[11]] = True
        if op["kind"] == "render" and k in lively and nxt is not None and nxt in lively and ops[nxt]["side"] != op["side"]:
            tile = lambda t: t // 64
            env_hit = any(tile(t) == tile(x) and t < op["frames"] for v, ts in op["takes"].items() for t in ts for x in op["switches"].get(v, ()))
            fp_hit = any(tile(t) == tile(x) and t < op["frames"] for v, ts in op["takes"].items() for t in ts for x in op["filter_switches"].get(v, ()))
            last = any(op["frames"] in ts for ts in op["takes"].values())
            first = any(ts[:1] == [0] and len(op["after"]["streams"][v[0]][v[1]]) == 1 for v, ts in ops[nxt]["takes"].items())
            if env_hit and fp_hit and last and first:
                found[STRETCHES[12]] = True
        if op["kind"] == "play" and op["kernel"] in STREAM_KERNELS and any(op["takes"].values()):
            found[STRETCHES[13]] = True
        if ok(op, "set_filter_programs") and op["mid_program"] and op["in_flight"] and nxt is not None:
            read = any(o["kind"] == "get_filter_programs" and o["lane"] == op["lane"] for o in ops[k + 1:nxt])
            found[STRETCHES[17 if read else 16]] = True
        if ok(op, "set_sweeps") and all(op["sounding"]) and op["in_flight"] and prv == k - 1 and prv in lively and op["open"] == 0:
            found[STRETCHES[18]] = True
        if ok(op, "set_filters") and op.get("cancels") and nxt is not None:
            others = lambda t: op["pending"][t] - set(op["cancels"])
            if others("sweeps") and others("filter_programs") and ops[nxt]["uploaded"]["sweeps"] > len(op["cancels"]) - 1 and ops[nxt]["uploaded"]["filter_programs"]:
                found[STRETCHES[19]] = True
    found[STRETCHES[8]] = names == set(STREAM_KERNELS) and all({ops[j]["side"] for j in renders if ops[j]["kind"] == "render" and ops[j]["kernel"] == name} == {False, True}
                                                               for name in STREAM_KERNELS)
    # the horizons: fp_horizon - 1 frames in renders, one frame, one more; then the sweeps' in the same way
    for at in range(len(renders) - 6):
        seven = [ops[j] for j in renders[at:at + 7]]
        fp, sw = seven[0]["horizons"][2], seven[0]["horizons"][1]
        if all(o["open"] == 0 and o["kind"] == "render" for o in seven) and fp > 1 and seven[0]["frames"] + seven[1]["frames"] == fp - 1 and seven[2]["frames"] == 1 and \
                seven[3]["frames"] == 1 and sum(o["frames"] for o in seven[:5]) == sw - 1 and seven[5]["frames"] == 1:
            for env_too, names7 in ((False, ["k_filter_program_rows"] * 3 + ["k_sweep_rows"] * 3 + ["k_biquad_rows"]),
                                    (True, ["k_filter_program_env_rows"] * 3 + ["k_sweep_program_rows"] * 3 + ["k_program_biquad_rows"])):
                if [o["kernel"] for o in seven] == names7:
                    found[STRETCHES[15 if env_too else 14]] = True
    wanted = {"set_sweeps": {wref.MESSAGES["filter"], wref.MESSAGES["finite"]}, "set_filter_programs": {fref.MESSAGES["length"]}}
    table_of = {"set_sweeps": "sweeps", "set_filter_programs": "filter_programs"}
    got = {kind: {op["refused"] for op in ops if op["kind"] == kind and op["refused"] and op["pending"][table_of[kind]]} for kind in wanted}
    found[STRETCHES[20]] = all(wanted[kind] <= got[kind] for kind in wanted)
    return found


def check_bounds(ops):
    """Walks every op: no ring ever holds more than RING entries on the device, no position is at or past its end in a PLAYING record that is
    not at its end by the contract, no program is longer than its maximum.  Returns the number of (voice, render) pairs looked at."""
    looked = 0
    for op in ops:
        if op["kind"] in ("set_streams", "append_streams") and not op["refused"]:
            assert all(len(s) <= (1 + RING if op["kind"] == "set_streams" else RING) for s in op["data"])
        if op["kind"] in ("set_env_programs", "set_filter_programs") and not op["refused"]:
            assert all(1 <= len(p) <= 8 for p in op["data"])
        if op["kind"] not in ("render", "play"):
            continue
        assert 1 <= op["frames"] <= 300
        for state in (op["before"], op["after"]):
            for k in range(state["lanes"]):
                for i in range(len(state["streams"][k])):
                    s, looked = state["streams"][k][i], looked + 1
                    waiting = int(state["queued"][k][i]) - int(state["taken"][k][i])
                    assert 0 <= waiting <= RING and (waiting == len(s) - 1 or len(s) == 1 and int(state["queued"][k][i]) == 0), (k, i, waiting, len(s))
                    for r in s:
                        if int(r["flags"]) & sref.PLAYING:
                            end = int(r["loop_end"] if int(r["flags"]) & sref.LOOP else r["frames"]) << sref.FRAC_BITS
                            assert int(r["position"]) < end and int(r["frames"]) >= 1 and int(r["data"]) != 0
                        else:
                            assert int(r["position"]) <= int(r["frames"]) << sref.FRAC_BITS
                    assert 1 <= len(state["prog"][k][i]) <= 8 and 1 <= len(state["fprog"][k][i]) <= fref.MAX
                    for e in state["fprog"][k][i]:
                        assert int(e["done"]) <= int(e["frames"]) <= wref.MAX_FRAMES
    return looked


def forms_missing(ops):
    """{call kind: the (names its lane, all instances) combinations in which no call of that kind was taken}, for every set and get call."""
    missing = {}
    for kind in SETS + GETS:
        used = {(bool(op["lane_form"]), op["rows"] is None) for op in ops if op["kind"] == kind and not op["refused"]}
        if len(used) < 4:
            missing[kind] = sorted({(a, b) for a in (False, True) for b in (False, True)} - used)
    return missing


def conditions(ops):
    """What every generated sequence must meet, as {what: whether it does}; tests/test_stream_stack_model.py asserts them on the CPU."""
    renders = [k for k, op in enumerate(ops) if op["kind"] == "render"]
    lively = set(unwaited(ops))
    takes = lambda k: sum(len(t) for t in ops[k]["takes"].values())
    previous = {k: renders[at - 1] for at, k in enumerate(renders) if at}
    sizes = {op["frames"] for op in ops if op["kind"] in ("render", "play")}
    outs = [op["want"] for op in ops if op["kind"] in ("render", "play")]
    both = lambda a, b: {(x, y) for x in a for y in b}
    return {"three renders in four are not waited for": 4 * len(lively) >= 3 * len(renders),
            "20 entries taken in renders not waited for": sum(takes(k) for k in lively) >= 20,
            "5 of them behind a render not waited for either": sum(takes(k) for k in lively if previous.get(k) in lively) >= 5,
            "all thirteen kernels": {ops[k]["kernel"] for k in renders} | {op["kernel"] for op in ops if op["kind"] == "play"} == set(KERNELS),
            "both stream kernels on both HIP streams": {(ops[k]["kernel"], ops[k]["side"]) for k in renders if ops[k]["kernel"] in STREAM_KERNELS} == both(STREAM_KERNELS, (False, True)),
            "every op kind": {op["kind"] for op in ops} == set(KINDS),
            "every call kind in both lane forms, on subsets and on all instances": not forms_missing(ops),
            "sizes between 1 and 300": min(sizes) >= 1 and max(sizes) <= 300,
            "sizes 1, 63, 64, 65 and 64 k + 1": {1, 63, 64, 65} <= sizes and any(x > 65 and x % 64 == 1 for x in sizes),
            "every offset": {ops[k]["offset"] for k in renders} == {0, 1, 2},
            "no NaN in the reference": not any(np.isnan(o).any() for o in outs),
            "nine renders in ten are heard": 10 * sum(bool(np.abs(o).max() > 0) for o in outs) >= 9 * len(outs)}


def summary(ops):
    renders = [k for k, op in enumerate(ops) if op["kind"] == "render"]
    lively = unwaited(ops)
    return dict(ops=len(ops), renders=len(renders), not_waited=len(lively), share=round(len(lively) / len(renders), 2), plays=sum(op["kind"] == "play" for op in ops),
                takes_not_waited=sum(len(t) for k in lively for t in ops[k]["takes"].values()), takes=sum(len(t) for k in renders for t in ops[k]["takes"].values()))
