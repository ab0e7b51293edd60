"""CPU: the sampler streams at the ends of their 64-bit range -- takes at positions past 2^32, excesses of up to 2^32 - 6 units that skip
whole entries, land in loops of one frame and hand their rest on, takes on and beside the 64-frame tile edges at those values,
envelopes at their bounds across a take, entries that differ from the current record in every field -- as case families that
tests/test_gpu_stream_extremes.py plays on the device.  Here: an independent frame-at-a-time model (tests/stream_model.py) agrees with
the restatement (tests/stream_ref.py) on every family, bit for bit and byte for byte; every family reaches what it claims to reach, by
the model's trace; chunks of a long asset play the whole asset's bits by sampler_ref alone; the sanitized host build of the kernel plays
every family; and value-only wrong forms of the restatement are caught by the family aimed at them and not by the committed cases -- no
GPU needed."""
import functools
import os

import numpy as np
import pytest

import resample_cases as cases
import resample_ref as ref
import sampler_model
import sampler_ref as sref
import stream_cases as scases
import stream_model as model
import stream_ref as stref
import test_sampler_extremes as sx
import test_stream_ref as tsr
import voice_ref as vref
from program_cases import segment
from test_sampler_abi import rec
from test_stream_host import compare, program, run          # (program: the host build, made once for this module as well)
from test_voice_abi import env

f32 = np.float32
ONE, H, N, TWO32 = sref.ONE, sx.H, sx.N, 1 << 32
PLAY, LOOP, LIN = sref.PLAYING, sref.LOOP, sref.LINEAR
LARGE_STEPS, IDLE_GAINS = sx.LARGE_STEPS, sx.IDLE_GAINS
LONG = H + 100                  # frames of a long first chunk: its end E0 lies 100 frames past 2^32
E0 = LONG * ONE
SPLIT = [1, 63, 65]             # the calls that follow a case's own, continuing it: on and beside the streams' 64-frame tile
TILE = stref.TILE
GRID_FRAMES = [63, 64, 65, 128]
STEPS = [ONE + 7, ONE // 2, 1] + LARGE_STEPS
MODES = {"nearest": (0, ref.NONE), "LINEAR": (LIN, ref.NONE), "4 taps": (0, cases.FINE), "8 taps": (0, cases.FINE + 1)}
L16, L8, LF, W16, S8 = range(5)                      # the pool: long 16-bit, 8-bit and fp32, small 16-bit of the batch's width, small 8-bit mono
FMT = [sref.PCM_S16, sref.PCM_U8, sref.PCM_F32, sref.PCM_S16, sref.PCM_U8]
NO_ENV = [np.zeros(1, vref.DTYPE)[0]]


def pool_of(channels):
    """test_sampler_extremes' long assets a batch of `channels` channels can play -- the 16-bit one stereo for a stereo batch and mono
    otherwise: the same memory --, and two of its small ones."""
    small = sx.small_assets(channels)
    return [pcm for _, pcm in sx.long_pool(channels)] + [small["s16 wide"][1], small["u8"][1]]


def chunk(pool, key, first, frames, **fields):
    """A playing one-shot over the frames [first, first + frames) of pool[key] (the placeholder of stream_cases in `data`)."""
    pcm = pool[key]
    assert 0 <= first and first + frames <= pcm.shape[0]
    base = dict(data=(key << 32) | (first * pcm.shape[1] * pcm.dtype.itemsize), format=FMT[key], channels=pcm.shape[1], frames=frames)
    return rec(**dict(base, **fields))[0]


def gains(rng, channels, idle=0):
    """Random gains for the batch's channels; behind them IDLE_GAINS from its entry `idle` on, which no render reads."""
    g = np.zeros(sref.MAX_CHANNELS, f32)
    g[:channels] = rng.uniform(-1.0, 1.0, channels).astype(f32)
    g.view(np.uint32)[channels:] = np.resize(np.roll(IDLE_GAINS, -idle), sref.MAX_CHANNELS - channels)
    return g


class Case:
    """One batch's worth of voices: names [n], streams [n] (placeholders), programs [n], resamplers [n], the calls, the appends
    {index of the call they follow: [(instance, entries)]}, and the pool the placeholders name."""

    def __init__(self, label, pool, voices, calls, appends=None):
        self.label, self.pool, self.calls, self.appends = label, pool, list(calls), appends or {}
        self.names = [v[0] for v in voices]
        self.streams = [np.array(v[1], dtype=sref.DTYPE) for v in voices]
        self.programs = [list(v[2]) for v in voices]
        self.resamplers = np.asarray([v[3] for v in voices])
        assert 1 <= len(voices) <= 16 and sum(self.calls) + sum(SPLIT) <= 1500
        for s, p in zip(self.streams, self.programs):
            assert 1 <= len(s) <= 1 + stref.QUEUE and not host_refuses(s, p[0], pool), self.label

    def placed(self, bases=None):
        """(streams [1][n] with addresses, the assets' table, the appends with addresses)."""
        bases = scases.fake_bases(self.pool) if bases is None else bases
        streams, assets = scases.resolve_streams([self.streams], self.pool, bases)
        appends = {c: [(0, i, scases.resolve(e, self.pool, bases, assets)) for i, e in v] for c, v in self.appends.items()}
        return streams, assets, appends


def host_refuses(stream, envelope, pool):
    """What oalsfx_batch_set_streams would refuse in a voice's records (batch.cpp: sampler_ok, stream_records_ok), or None."""
    for j, r in enumerate(stream):
        flags, frames = int(r["flags"]), int(r["frames"])
        if flags & ~(PLAY | LOOP | LIN) or int(r["reserved"]):
            return "flags"
        if j and not flags & PLAY:
            return "a queued sampler is not playing"
        if not flags & PLAY:
            continue
        end = frames * ONE
        if flags & LOOP:
            if not int(r["loop_start"]) < int(r["loop_end"]) <= frames:
                return "loop region"
            end = int(r["loop_end"]) * ONE
        if not 0 < frames < 1 << 31 or int(r["position"]) >= end:
            return "frames or position"
        pcm = pool[int(r["data"]) >> 32]
        width = pcm.shape[1] * pcm.dtype.itemsize
        offset = int(r["data"]) & 0xFFFFFFFF
        if offset % width or offset // width + frames > pcm.shape[0] or int(r["channels"]) != pcm.shape[1]:
            return "outside the asset"
    if len(stream) > 1 and int(envelope["flags"]) & (vref.ACTIVE | vref.GLIDE) == vref.ACTIVE | vref.GLIDE:
        return "glides"
    return None


def cut_long(pool, key, lengths_behind, step, flags, back, gain):
    """A long asset as consecutive chunks: the first LONG frames, then `lengths_behind`, then the rest; the voice stands `back` units in
    front of the first chunk's end."""
    n = pool[key].shape[0]
    lengths = [LONG] + list(lengths_behind)
    lengths.append(n - sum(lengths))
    assert lengths[-1] > 0 and 0 < back <= E0
    return stref.chunks(chunk(pool, key, 0, n, step=step, flags=PLAY | flags, position=E0 - back, gain=gain), lengths)


def back_for(step, frames=10, rest=3):
    """So that the one-shot's first frame at or past E0 is frame `frames`, `rest` units short of a whole number of steps (large steps: the
    second frame)."""
    return (frames - 1) * step + min(rest, step) if step < 1 << 20 else 5


# ---- the families: each a function of the batch's channel count that returns Cases ----
def takes_past(channels):
    pool, rng = pool_of(channels), np.random.default_rng(100 + channels)
    out = []
    for label, modes in (("nearest and LINEAR", ("nearest", "LINEAR")), ("through tables", ("4 taps", "8 taps"))):
        voices = []
        for s, step in enumerate(STEPS):
            for m, mode in enumerate(modes):
                lin, table = MODES[mode]
                stream = cut_long(pool, (s + m) % 3, [1, 1, 1], step, lin, back_for(step), gains(rng, channels))
                voices.append((f"{mode}, step {step}", stream, NO_ENV, table))
        if label.startswith("nearest"):
            s = ONE + 7
            for k, (what, back) in enumerate((("E - P a multiple of the step", 9 * s), ("... one unit more", 9 * s + 1), ("... one unit less", 9 * s - 1))):
                voices.append((what, cut_long(pool, k, [1, 1, 1], s, LIN if k == 1 else 0, back, gains(rng, channels)), NO_ENV, ref.NONE))
        out.append(Case(label, pool, voices, [7, 5, 64]))
    return out


def shorts(pool, rng, count, channels, longest=40, positions=False):
    """`count` entries over the small 16-bit asset, each 1 .. `longest` frames, far shorter than any excess of a large step."""
    out, first = [], 0
    for k in range(count):
        frames = int(rng.integers(1, longest + 1))
        position = int(rng.integers(0, frames * ONE)) if positions else 0
        out.append(chunk(pool, W16, first, frames, step=ONE + 11 * k, position=position, gain=gains(rng, channels, k)))
        first += frames
    return out


def room(entries):
    """The units a chain takes off an excess in passing over `entries` whole."""
    return sum(int(e["frames"]) * ONE - int(e["position"]) for e in entries)


def skips(channels):
    pool, rng = pool_of(channels), np.random.default_rng(200 + channels)
    first = lambda key, step, position=E0 - 5: chunk(pool, key, 0, LONG, step=step, position=position, gain=gains(rng, channels))
    voices = []
    for k in list(range(1, 8)) + [8, 8, 8]:
        step = LARGE_STEPS[len(voices) % 3]
        voices.append((f"a ring of {k} skipped whole, step {step}", [first(len(voices) % 3, step)] + shorts(pool, rng, k, channels, positions=k % 2 == 0), NO_ENV, ref.NONE))
    out = [Case("whole rings", pool, voices, [3, 5, 64])]
    voices = []
    whole = lambda key, position, **kw: chunk(pool, key, 0, pool[key].shape[0], position=position, gain=gains(rng, channels), **kw)
    for k, (step, position) in enumerate(zip(LARGE_STEPS[::-1], (100 * ONE, (H // 2 + 50) * ONE, (H - 2000) * ONE))):
        ring = shorts(pool, rng, 3, channels, longest=3) + [whole((k + 1) % 3, position + 9, step=ONE + 3, flags=PLAY | (LIN if k == 1 else 0))]
        voices.append((f"lands in a long entry past 2^32, step {step}", [first(k, step)] + ring, NO_ENV, ref.NONE))
    for k, step in enumerate(LARGE_STEPS):
        ring = shorts(pool, rng, 3, channels, positions=True)
        ring.append(chunk(pool, S8, 100, 200, step=ONE + 3, position=7 * ONE + 5, flags=PLAY | LIN, gain=gains(rng, channels)))
        # one step from P runs over E0 by exactly what the three entries take off it
        voices.append((f"lands on an entry's end, step {step}", [first(k, step, E0 - step + room(ring[:3]))] + ring, NO_ENV, ref.NONE))
    voices.append(("two steps from 2^32 and more in front of the end", [first(L8, LARGE_STEPS[1], 50 * ONE)] + shorts(pool, rng, 2, channels), NO_ENV, ref.NONE))
    refill = len(voices)
    voices.append(("dry with an excess left over, refilled behind the first call", [first(LF, LARGE_STEPS[2])] + shorts(pool, rng, 2, channels), NO_ENV, ref.NONE))
    appended = [chunk(pool, S8, 300, 300, step=ONE + 5, position=77, gain=gains(rng, channels)), chunk(pool, W16, 1000, 50, gain=gains(rng, channels))]
    out.append(Case("landings", pool, voices, [3, 5, 64], {0: [(refill, np.array(appended, dtype=sref.DTYPE))]}))
    return out


REFILLED = ("an excess that skips entries", "landings")        # the case with the append, for the device's unwaited test


def into_loops(channels):
    pool, rng = pool_of(channels), np.random.default_rng(300 + channels)
    voices = []

    def add(what, key, step, entry_fields, behind=0, lin=0):
        n = pool[key].shape[0]
        entry_fields = dict(dict(step=ONE + 3, flags=PLAY | LOOP | lin), **entry_fields(n))
        ring = [chunk(pool, key, 0, n, gain=gains(rng, channels), **entry_fields)] + shorts(pool, rng, behind, channels)
        voices.append((f"{what}{', LINEAR' if lin else ''}, step {step}", [chunk(pool, (key + 1) % 3, 0, LONG, step=step, position=E0 - 5, gain=gains(rng, channels))] + ring, NO_ENV, ref.NONE))

    big = LARGE_STEPS[2]
    for lin in (0, LIN):
        add("a loop of one frame", L8 if lin else LF, big, lambda n: dict(loop_start=H + 7, loop_end=H + 8, position=(H + 7) * ONE + 4095), lin=lin, behind=1 if lin else 0)
        for step in LARGE_STEPS[1:]:
            add("a loop of three frames", L16 if lin else L8, step, lambda n: dict(loop_start=n - 3, loop_end=n, position=(n - 3) * ONE + 5), lin=lin)
        add("a loop of the whole asset", LF if lin else L16, big, lambda n: dict(loop_start=0, loop_end=n, position=(n - 10) * ONE + 1), lin=lin)
    add("a position in front of loop_start", L8, big, lambda n: dict(loop_start=H + 7, loop_end=H + 10, position=50 * ONE), lin=LIN, behind=2)
    add("a position in front of loop_start, no wrap", LF, LARGE_STEPS[0], lambda n: dict(loop_start=H + 7, loop_end=H + 10, position=(H - 3000) * ONE), behind=1)
    add("step 0 in the loop's place", L16, big, lambda n: dict(step=0, flags=PLAY, position=100 * ONE + 5), behind=1)
    add("step 0 in the loop's place", LF, LARGE_STEPS[1], lambda n: dict(step=0, flags=PLAY, position=(H // 2 + 60) * ONE + 2000), behind=1, lin=LIN)
    # (the second case: every take at t == F of a call of one frame, so that the entry's position is read back as the take left it)
    return [Case("", pool, voices, [3, 5, 64]), Case("taken on a render's last frame", pool, voices, [1, 2])]


def on_the_grid(channels, frames):
    """The voices of "takes past 2^32" placed against a first call of `frames` frames: the first frame an entry plays is frame frames - 1,
    frames (taken in the first call, at t == F, and played as frame 0 of the next) and frames + 1; and three takes inside one tile."""
    pool, rng = pool_of(channels), np.random.default_rng(400 + channels + frames)
    voices = []
    modes = list(MODES)
    for a, at in enumerate((frames - 1, frames, frames + 1)):
        for s, step in enumerate((ONE + 7, ONE // 2, LARGE_STEPS[0])):
            lin, table = MODES[modes[(a + s + frames) % 4]]
            back = (at * step, at * step - 1, (at - 1) * step + 1)[(a + s) % 3]            # excess 0, 1 and step - 1
            voices.append((f"a take at frame {at}, step {step}, {modes[(a + s + frames) % 4]}", cut_long(pool, (a + s) % 3, [1, 1], step, lin, back, gains(rng, channels)), NO_ENV, table))
    at = frames // TILE * TILE + 3
    voices.append((f"takes at {at}, {at + 2} and {at + 5}", cut_long(pool, frames % 3, [2, 3], ONE + 7, 0, at * (ONE + 7) - 9, gains(rng, channels)), NO_ENV, ref.NONE))
    return [Case(f"F {frames}", pool, voices, [frames])]


def under_envelopes(channels):
    pool, rng = pool_of(channels), np.random.default_rng(500 + channels)
    s = ONE + 7
    voice = lambda key, step=s, lin=0, behind=(1, 1), **kw: cut_long(pool, key, list(behind), step, lin, back_for(step, **kw), gains(rng, channels))
    seg = lambda ramp, **kw: segment(rng, channels, ramp, **kw)

    def ramping(done):
        e = vref.ramp(env()[0], rng.uniform(-1, 1, channels).astype(f32), rng.uniform(-1, 1, channels).astype(f32), vref.MAX_RAMP)
        e["ramp_done"] = done
        return [e]

    voices = [
        ("the longest delay less 7 in front of ten frames", voice(L16), [env(delay=2 ** 32 - 8)[0]], ref.NONE),
        ("a delay of 5 in front of ten frames", voice(L8, lin=LIN), [env(delay=5)[0]], ref.NONE),
        ("a ramp of 2^24 frames, 40 from its end", voice(LF), ramping(vref.MAX_RAMP - 40), ref.NONE),
        ("a ramp of 2^24 frames, 5000 from its end, 8 taps", voice(L16), ramping(vref.MAX_RAMP - 5000), cases.FINE + 1),
        ("a ramp of 2^24 frames under a step of 2^32 - 1", voice(L8, step=LARGE_STEPS[2]), ramping(vref.MAX_RAMP - 3), ref.NONE)]
    for R in (9, 10, 11):           # the take's frame is 10
        voices.append((f"STOP completes at frame {R}, the take's frame is 10", voice(R % 3, lin=LIN if R == 10 else 0, behind=(3, 1)), [seg(R, flags=vref.ACTIVE | vref.STOP)], ref.NONE))
    voices += [
        ("a segment switch on the take's frame, past 2^32", voice(LF), [seg(10), seg(30), seg(200)], ref.NONE),
        ("a segment switch on the take's frame, step 2^32 - 1, LINEAR", cut_long(pool, L16, [1], LARGE_STEPS[2], LIN, 5, gains(rng, channels)), [seg(1), seg(0), seg(90)], ref.NONE),
        ("a queued delay across the take, 4 taps", voice(L8), [seg(4), seg(20, delay=3), seg(100)], cases.FINE)]
    return [Case("", pool, voices, [7, 5, 64])]


def whole_fields(channels):
    """Every entry differs from the record in front of it in format, channels (where the batch is wider than mono), gains, LINEAR and
    step; the gains the batch has no channel for are IDLE_GAINS, in another order in every record."""
    pool, rng = pool_of(channels), np.random.default_rng(600 + channels)
    g = lambda k: gains(rng, channels, k)
    s = ONE + 7
    voices = [
        ("long 16-bit, then 8-bit LINEAR, fp32, wide 16-bit",
         [chunk(pool, L16, 0, LONG, step=s, position=E0 - 3 * s, gain=g(0)), chunk(pool, L8, H + 9, 2, step=ONE // 2, flags=PLAY | LIN, gain=g(1)),
          chunk(pool, LF, 77, 5, step=3 * ONE + 1, position=9, gain=g(2)), chunk(pool, W16, 10, 400, step=ONE - 1, flags=PLAY | LIN, gain=g(3))], NO_ENV, ref.NONE),
        ("wide 16-bit, then long fp32 past 2^32, 8-bit",
         [chunk(pool, W16, 4000, 1000, step=5 * ONE, position=990 * ONE, flags=PLAY | LIN, gain=g(1)), chunk(pool, LF, 0, LONG, step=ONE // 3, position=E0 - 5 * (ONE // 3), gain=g(2)),
          chunk(pool, S8, 0, 300, step=2 * ONE + 1, flags=PLAY | LIN, gain=g(3))], NO_ENV, ref.NONE),
        ("a step of 2^32 - 1 into an entry unlike it in everything",
         [chunk(pool, LF, 0, LONG, step=LARGE_STEPS[2], position=E0 - 5, flags=PLAY | LIN, gain=g(2)),
          chunk(pool, L8, 0, pool[L8].shape[0], step=ONE + 1, position=(N - H - 50) * ONE + 123, gain=g(0)), chunk(pool, W16, 0, 9, flags=PLAY | LIN, gain=g(1))], NO_ENV, ref.NONE),
        ("under an envelope, 4 taps",
         [chunk(pool, L8, 0, LONG, step=s, position=E0 - 4 * s + 1, gain=g(3)), chunk(pool, W16, 50, 30, step=ONE + 500, flags=PLAY | LIN, gain=g(0)),
          chunk(pool, LF, 5, 700, step=777, gain=g(1))], [segment(rng, channels, 300)], cases.FINE)]
    return [Case("", pool, voices, [7, 5, 64])]


# name -> [builder(channels) -> [Case]]
FAMILIES = {
    "takes past 2^32": [takes_past],
    "an excess that skips entries": [skips],
    "an excess into a loop": [into_loops],
    "ends on the grid at large values": [functools.partial(on_the_grid, frames=F) for F in GRID_FRAMES],
    "under envelopes at their bounds": [under_envelopes],
    "fields a take must carry whole": [whole_fields],
}


@functools.lru_cache(maxsize=None)
def _cases(name, channels):
    out = []
    for builder in FAMILIES[name]:
        for case in builder(channels):
            case.label = f"{name} {case.label}".strip() + f", {channels} channels"
            out.append(case)
    return out


def cases_of(name, channels):
    """The family's cases for a batch of `channels` channels (built once and never changed: everything that plays them copies)."""
    return _cases(name, channels)


def case_named(name, label, channels):
    return next(c for c in cases_of(name, channels) if c.label.startswith(f"{name} {label}"))


# ---- playing a case: one voice after the other, through the model or the restatement ----
def play(case, render_voice, calls=None, channels=2, wrong=None, traces=None):
    """Every call of `calls` (the case's own and SPLIT) for every voice, the appends behind the calls they follow: [(out [n][frames]
    [channels], streams, taken, programs, takes [n])] per call.  render_voice: stream_model's or stream_ref's."""
    streams, assets, appends = case.placed()
    streams, programs, taken = list(streams[0]), [list(p) for p in case.programs], [0] * len(case.names)
    tables, results = cases.tables(), []
    at = 0                  # frames before this call: the traces count frames from the first call's start
    for c, frames in enumerate(case.calls + SPLIT if calls is None else calls):
        outs, takes = [], []
        for i in range(len(streams)):
            coef = tables[int(case.resamplers[i])] if int(case.resamplers[i]) != ref.NONE else None
            extra = {} if wrong is None else dict(wrong=wrong)
            if traces is not None:
                extra["trace"] = notes = []
            o, streams[i], taken[i], programs[i], t = render_voice(streams[i], taken[i], programs[i], coef, assets, frames, channels, **extra)
            if traces is not None:
                traces[i] += [dict(note, frame=note["frame"] + at, call=c) for note in notes]
            outs.append(o)
            takes.append(t)
        results.append((np.stack(outs), [s.copy() for s in streams], list(taken), [np.array(p).copy() for p in programs], takes))
        for _, i, entries in appends.get(c, ()) if calls is None else ():
            streams[i] = stref.append(streams[i], entries)
            assert streams[i] is not None
        at += frames
    sampler_model._converted.clear()            # (the model's float copies of the chunks: a long one is megabytes)
    return results


def same_results(a, b):
    """Outputs on their bits (NaNs by position); records, rings, taken counts, programs and the frames of the takes exactly."""
    return (sref.same_floats(a[0], b[0])[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2] == b[2] and
            all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3])) and a[4] == b[4])


def differing(a, b):
    return [i for i in range(len(a[2])) if not (sref.same_floats(a[0][i], b[0][i])[0] and a[1][i].tobytes() == b[1][i].tobytes() and a[2][i] == b[2][i] and
                                                 a[3][i].tobytes() == b[3][i].tobytes() and a[4][i] == b[4][i])]


@functools.lru_cache(maxsize=None)
def restated(name, channels):
    """The restatement's results for every case of the family, computed once: [results per call] per case."""
    return [play(case, stref.render_voice, channels=channels) for case in cases_of(name, channels)]


@functools.lru_cache(maxsize=None)
def traced(name, channels=2):
    """The model's traces for every case of the family: ([traces per voice] per case, [results] per case)."""
    all_traces, all_results = [], []
    for case in cases_of(name, channels):
        traces = [[] for _ in case.names]
        all_results.append(play(case, model.render_voice, channels=channels, traces=traces))
        all_traces.append(traces)
    return all_traces, all_results


# ---- model against restatement ----
@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_model_and_restatement_agree(name, channels):
    """Every case's own calls, then the calls of SPLIT continuing them: outputs on their bits, the current record and the ring on their
    bytes, taken, the envelope program and the frames of the takes after every call; and the restatement's one render of the calls' sum
    gives what its calls gave (a case with an append: up to the append)."""
    for case, want in zip(cases_of(name, channels), restated(name, channels)):
        got = play(case, model.render_voice, channels=channels) if channels != 2 else traced(name)[1][cases_of(name, 2).index(case)]
        for c, (g, w) in enumerate(zip(got, want)):
            assert same_results(g, w), f"{case.label}, call {c}: model and restatement differ for the voices {[case.names[i] for i in differing(g, w)]}"
        upto = 1 + min(case.appends) if case.appends else len(want)
        frames = (case.calls + SPLIT)[:upto]
        whole, = play(case, stref.render_voice, calls=[sum(frames)], channels=channels)
        assert sref.same_floats(whole[0], np.concatenate([w[0] for w in want[:upto]], axis=1))[0], f"{case.label}: one render differs from the split"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(whole[1], want[upto - 1][1])) and whole[2] == want[upto - 1][2], case.label
        assert whole[4] == [sum(([t + sum(frames[:c]) for t in want[c][4][i]] for c in range(upto)), []) for i in range(len(case.names))], case.label


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_model_and_restatement_agree_on_the_random_streams(channels):
    rng = np.random.default_rng(70 + channels)
    calls = (70, 130, 3, 97)
    streams, programs, resamplers, pool = scases.random_streams(rng, 10, 2, channels, calls)
    streams, assets = scases.resolve_streams(streams, pool, scases.fake_bases(pool))
    tables, taken_all = cases.tables(), 0
    for k in range(2):
        for i in range(10):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            a = b = (None, streams[k][i], 0, programs[k][i], None)
            for frames in calls:
                a = stref.render_voice(a[1], a[2], a[3], coef, assets, frames, channels)
                b = model.render_voice(b[1], b[2], b[3], coef, assets, frames, channels)
                assert sref.same_floats(a[0], b[0])[0] and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes() and a[4] == b[4], (k, i, frames)
            taken_all += a[2]
    assert taken_all > 10
    sampler_model._converted.clear()


def test_the_model_computes_the_values_worked_out_by_hand():
    """Three chunks of a ramp at step 2.5 frames: q = 0, 2.5, 5 | 7.5 -> chunk two (frames 4 .. 5) was skipped whole at over = 3.5 - 2 = 1.5
    ... worked through by hand: the frames read are 0, 2, (4 is the end: over 1 into [4, 6)) 5, then 7.5 is 1.5 past the end of [4, 6) at
    6, so [6, 10) starts at 1.5: 7, then 10: dry."""
    ramp = np.arange(10.0, dtype=f32).reshape(-1, 1)
    first = rec(data=0x1000, format=sref.PCM_F32, frames=10, step=5 * ONE // 2)[0]
    chunks = stref.chunks(first, [4, 2, 4])
    assets = {stref.asset_key(c): ramp[a:b] for c, (a, b) in zip(chunks, ((0, 4), (4, 6), (6, 10)))}
    trace = []
    out, after, taken, _, takes = model.render_voice(chunks, 0, NO_ENV, None, assets, 6, 1, trace=trace)
    assert out[:, 0].tolist() == [0.0, 2.0, 5.0, 7.0, 0.0, 0.0] and takes == [2, 3] and taken == 2
    assert [(n["over"], n["start"], n["ended"]) for n in trace] == [(ONE, ONE, False), (3 * ONE // 2, 3 * ONE // 2, False)]
    assert len(after) == 1 and int(after[0]["position"]) == 4 * ONE and not int(after[0]["flags"]) & PLAY
    # the same with a one-frame chunk in the middle that the excess passes over: [0, 4), [4, 5), [5, 10) at step 3.5: 0, 3.5 -> 3, then 7:
    # 3 past 4; [4, 5) takes 1 off, ended; [5, 10) starts at 2: 7, then 10.5: dry with 0.5 left over, which is lost
    first["step"] = 7 * ONE // 2
    chunks = stref.chunks(first, [4, 1, 5])
    assets = {stref.asset_key(c): ramp[a:b] for c, (a, b) in zip(chunks, ((0, 4), (4, 5), (5, 10)))}
    trace = []
    out, after, taken, _, takes = model.render_voice(chunks, 0, NO_ENV, None, assets, 5, 1, trace=trace)
    assert out[:, 0].tolist() == [0.0, 3.0, 7.0, 0.0, 0.0] and takes == [2, 2]
    assert [(n["hop"], n["over"], n["ended"]) for n in trace] == [(0, 3 * ONE, True), (1, 2 * ONE, False)]


# ---- the families reach what they claim: by the model's trace ----
def takes_of(name, channels=2):
    """[(case, voice name, the voice's stream as set, its trace)] over the family."""
    traces, _ = traced(name, channels)
    return [(case, case.names[i], case.streams[i], traces[k][i]) for k, case in enumerate(cases_of(name, channels)) for i in range(len(case.names))]


def test_takes_past_2_to_the_32_are():
    rows = takes_of("takes past 2^32")
    assert len(rows) == 27
    for case, name, stream, trace in rows:
        assert trace and trace[0]["end"] == E0 > TWO32 and trace[0]["q"] >= E0, name          # every voice's first take is from a position past 2^32
        assert int(stream[0]["frames"]) > H and [int(f) for f in stream["frames"][1:4]] == [1, 1, 1]
    seen = {(name.split(",")[0], int(stream[0]["step"])) for _, name, stream, _ in rows}
    assert {(mode, step) for mode in MODES for step in STEPS} <= seen
    # the moderate steps take at frame 10 (step 1: there the chunk of one frame lasts 4096 frames), the large ones at frame 1 and chain on
    for case, name, stream, trace in rows:
        step = int(stream[0]["step"])
        if step in LARGE_STEPS:
            assert trace[0]["frame"] == 1 and trace[0]["over"] == step - 5 and [n["hop"] for n in trace[:4]] == [0, 1, 2, 3], name
        elif "E - P" not in name and "one unit" not in name:
            assert trace[0]["frame"] == 10 and trace[0]["over"] == step - min(3, step), name
    exact = {name: trace for _, name, _, trace in rows if "E - P" in name or "one unit" in name}
    assert [exact[k][0]["over"] for k in ("E - P a multiple of the step", "... one unit more", "... one unit less")] == [0, ONE + 6, 1]
    assert [exact[k][0]["frame"] for k in ("E - P a multiple of the step", "... one unit more", "... one unit less")] == [9, 10, 9]
    # the seam's taps: a table reads the long chunk's last frames, at indices >= 2^20
    assert all(int(stream[0]["position"]) >> 12 >= H for _, _, stream, _ in rows)


def test_an_excess_skips_entries_and_lands():
    rows = takes_of("an excess that skips entries")
    by = {name: (stream, trace) for _, name, stream, trace in rows}
    traces, results = traced("an excess that skips entries")
    final = {case.names[i]: (results[k][-1][1][i], results[k][-1][2][i]) for k, case in enumerate(cases_of("an excess that skips entries", 2)) for i in range(len(case.names))}
    chains = {}
    for name, (stream, trace) in by.items():
        if name.startswith("a ring of"):
            k = len(stream) - 1
            chain = [n for n in trace if n["frame"] == 1]
            assert [n["hop"] for n in chain] == list(range(k)) and all(n["ended"] for n in chain), name          # every entry taken in frame 1, and ended
            assert all(n["over"] > 20 * (int(e["frames"]) << 12) for n, e in zip(chain, stream[1:])), name         # ... each far shorter than the excess
            after, taken = final[name]
            assert taken == k and len(after) == 1 and int(after[0]["flags"]) & PLAY == 0, name
            assert int(after[0]["position"]) == int(stream[-1]["frames"]) << 12 and after[0]["data"] != 0, name  # dry at E' of the last entry
            chains[k] = chains.get(k, 0) + 1
    assert sorted(chains) == list(range(1, 9)) and chains[8] == 3
    assert max(n["over"] for _, t in by.values() for n in t) == TWO32 - 6 and sum(n["over"] > 1 << 31 for _, t in by.values() for n in t) > 20
    for step in LARGE_STEPS:
        stream, trace = by[f"lands in a long entry past 2^32, step {step}"]
        assert [n["ended"] for n in trace[:4]] == [True, True, True, False] and trace[3]["frame"] == 1
        assert TWO32 <= trace[3]["start"] < int(stream[4]["frames"]) << 12 and int(stream[4]["position"]) < TWO32          # the take itself forms a position past 2^32
        stream, trace = by[f"lands on an entry's end, step {step}"]
        assert [n["ended"] for n in trace[:4]] == [True, True, True, False] and [n["frame"] for n in trace[:4]] == [1] * 4
        assert trace[2]["start"] == int(stream[3]["frames"]) << 12 and trace[3]["over"] == 0 and trace[3]["start"] == int(stream[4]["position"])
    stream, trace = by["dry with an excess left over, refilled behind the first call"]
    assert [(n["frame"], n["call"], n["ended"]) for n in trace[:2]] == [(1, 0, True), (1, 0, True)] and trace[1]["start"] - (int(stream[2]["frames"]) << 12) > 1 << 31
    assert (trace[2]["frame"], trace[2]["call"], trace[2]["over"], trace[2]["start"]) == (3, 1, 0, 77)            # frame 0 of the call behind the append


def test_an_excess_wraps_loops_many_times():
    first, last = cases_of("an excess into a loop", 2)
    rows = [r for r in takes_of("an excess into a loop") if r[0] is first]
    traces, results = traced("an excess into a loop")
    assert last.calls[0] == 1 and all(t[0]["frame"] == 1 and t[0]["call"] == 0 for t in traces[1])           # taken at t == F
    after = {name: results[0][-1][1][i] for i, (_, name, _, _) in enumerate(rows)}
    wraps = {name: trace[0]["wraps"] for _, name, _, trace in rows}
    lengths = {name: int(stream[1]["loop_end"]) - int(stream[1]["loop_start"]) for _, name, stream, _ in rows if int(stream[1]["flags"]) & LOOP}
    assert {1, 3, N} <= set(lengths.values()) and all(len(trace) == 1 and trace[0]["frame"] == 1 for _, _, _, trace in rows)
    one = [n for n in lengths if lengths[n] == 1]
    # (an excess is below 2^32 and a position inside a loop of one frame below its end: 2^20 wraps is the most there is)
    assert len(one) == 2 and all(wraps[n] == 1 << 20 for n in one)
    assert all(wraps[n] > 1 << 17 for n in lengths if lengths[n] == 3 and "front" not in n) and sum(lengths[n] == 3 for n in lengths) >= 5
    assert all(wraps[n] == 1 for n in lengths if lengths[n] >= N) and sum(lengths[n] >= N for n in lengths) == 2
    front = [(name, stream, trace) for _, name, stream, trace in rows if "front" in name]
    assert all(int(s[1]["position"]) < int(s[1]["loop_start"]) << 12 for _, s, _ in front) and sorted(t[0]["wraps"] > 0 for _, _, t in front) == [False, True]
    flags = {int(stream[1]["flags"]) & LIN for _, _, stream, _ in rows if int(stream[1]["flags"]) & LOOP}
    assert flags == {0, LIN}
    # an entry behind a loop, and behind a step of 0, stays; the step-0 entry stands where the excess put it, past 2^32
    held = [name for _, name, stream, _ in rows if len(stream) > 2]
    assert len(held) >= 5 and all(len(after[n]) == len(s) - 1 for _, n, s, _ in rows)
    for _, name, stream, trace in rows:
        if "step 0" in name:
            assert trace[0]["start"] == int(after[name][0]["position"]) and int(after[name][0]["flags"]) & PLAY and (trace[0]["start"] >= TWO32 or "LINEAR" in name)


def test_ends_fall_on_the_grid():
    """A take at frame F - 1, at F (in the first call, at t == F) and at F + 1 for every F of GRID_FRAMES, which lie on and beside the
    64-frame tile; excesses 0, 1 and step - 1; three takes inside one tile."""
    traces, _ = traced("ends on the grid at large values")
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE} <= set(GRID_FRAMES)
    for case, per_voice in zip(cases_of("ends on the grid at large values", 2), traces):
        frames = case.calls[0]
        firsts = {}
        for name, stream, trace in zip(case.names, case.streams, per_voice):
            if name.startswith("a take at"):
                at, step = int(name.split()[4].rstrip(",")), int(stream[0]["step"])
                assert trace[0]["frame"] == at and trace[0]["call"] == (0 if at <= frames else 1) and trace[0]["q"] >= E0 > TWO32, (case.label, name)
                firsts.setdefault(at, set()).add(trace[0]["over"] if trace[0]["over"] < 2 else "step - 1" if trace[0]["over"] == step - 1 else None)
            else:
                at = frames // TILE * TILE + 3
                assert [n["frame"] for n in trace[:3]] == [at, at + 2, at + 5] and at // TILE == (at + 5) // TILE, (case.label, name)
        assert sorted(firsts) == [frames - 1, frames, frames + 1] and all(v == {0, 1, "step - 1"} for v in firsts.values()), (case.label, firsts)
        assert {int(s[0]["step"]) for s in case.streams} == {ONE + 7, ONE // 2, LARGE_STEPS[0]} and len(set(case.resamplers.tolist())) == 3


def test_envelopes_meet_takes_at_their_bounds():
    rows = takes_of("under envelopes at their bounds")
    _, results = traced("under envelopes at their bounds")
    case = cases_of("under envelopes at their bounds", 2)[0]
    by = {name: (i, stream, trace) for i, (_, name, stream, trace) in enumerate(rows)}
    total = sum(case.calls + SPLIT)
    last = results[0][-1]
    i, stream, trace = by["the longest delay less 7 in front of ten frames"]
    assert not trace and int(case.programs[i][0]["delay"]) + 10 > TWO32 and int(last[3][i][0]["delay"]) == 2 ** 32 - 8 - total
    assert not np.concatenate([r[0][i] for r in results[0]]).any()
    assert by["a delay of 5 in front of ten frames"][2][0]["frame"] == 15
    for name, done in (("a ramp of 2^24 frames, 40 from its end", 40), ("a ramp of 2^24 frames, 5000 from its end, 8 taps", 5000)):
        i, stream, trace = by[name]
        assert int(case.programs[i][0]["ramp_frames"]) == 1 << 24 and trace[0]["frame"] == 10 and len(trace) >= 2
        assert int(last[3][i][0]["ramp_done"]) == min(1 << 24, (1 << 24) - done + total)
    assert by["a ramp of 2^24 frames under a step of 2^32 - 1"][2][0]["over"] == TWO32 - 6
    # STOP one frame before the take's frame: nothing taken, the record one step short of its end; on it: taken, and the entry never
    # plays; one frame behind: the entry plays one frame
    kinds = []
    for R in (9, 10, 11):
        i, stream, trace = by[f"STOP completes at frame {R}, the take's frame is 10"]
        after = last[1][i]
        out = np.concatenate([r[0][i] for r in results[0]])
        kinds.append((len(trace), bool(out[10].any()), int(after[0]["position"]) == (E0 - back_for(ONE + 7) + 9 * (ONE + 7) if R == 9 else int(stream[1]["position"]) + (R - 10) * (ONE + 7) + ONE + 4)))
        assert not int(after[0]["flags"]) & PLAY and not out[R:].any() and out[R - 1].any()
    assert kinds == [(0, False, True), (1, False, True), (1, True, True)]
    i, stream, trace = by["a segment switch on the take's frame, past 2^32"]
    assert trace[0]["frame"] == 10 and trace[0]["q"] > TWO32 and int(case.programs[i][0]["ramp_frames"]) == 10
    i, stream, trace = by["a segment switch on the take's frame, step 2^32 - 1, LINEAR"]
    assert trace[0]["frame"] == 1 and int(case.programs[i][0]["ramp_frames"]) == 1 and len(last[3][i]) == 1


def test_whole_fields_differ_in_every_field():
    for channels in (1, 2, 6):
        case, = cases_of("fields a take must carry whole", channels)
        results = restated("fields a take must carry whole", channels)[0]
        for i, stream in enumerate(case.placed()[0][0]):
            for a, b in zip(stream[:-1], stream[1:]):
                differ = [f for f in ("format", "step", "gain", "frames", "data") if a[f].tobytes() == b[f].tobytes()]
                assert not differ and (a["flags"] ^ b["flags"]) & LIN, (case.names[i], differ)
            assert channels == 1 or len({int(r["channels"]) for r in stream}) == 2, case.names[i]
            idle = stream["gain"].view(np.uint32)[:, channels:]
            assert set(idle.reshape(-1).tolist()) == set(IDLE_GAINS.tolist()) and len({row.tobytes() for row in idle}) == len(stream)
            # after every call the current record is an entry as set, but for position and flags
            for r in results:
                current = r[1][i][0]
                source = stream[r[2][i]]
                assert [f for f in sref.DTYPE.names if current[f].tobytes() != source[f].tobytes()] in ([], ["position"], ["position", "flags"], ["flags"])
            assert results[-1][2][i] >= 2


def test_the_device_tests_play_every_family():
    """tests/test_gpu_stream_extremes.py plays the families by name: one taken out there shows here."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_stream_extremes.py")).read()
    for name in FAMILIES:
        assert f'"{name}"' in text, name
    assert "mark.skip" not in text and "xfail" not in text and '"k_stream_rows"' in text and '"k_stream_filter_rows"' in text


# ---- the chunks property at the extremes, no stream code in the oracle ----
@pytest.mark.parametrize("step", [1] + LARGE_STEPS)
def test_chunks_play_the_whole_long_asset(step):
    """The nearest-sample voices of "takes past 2^32" are consecutive chunks of one long asset: sampler_ref.render_one of the whole asset
    from the same position gives the stream's bits over all the calls, and the same final position in the asset."""
    case = case_named("takes past 2^32", "nearest and LINEAR", 2)
    results = restated("takes past 2^32", 2)[0]
    rows = [i for i, s in enumerate(case.streams) if int(s[0]["step"]) == step and not int(s[0]["flags"]) & LIN and int(case.resamplers[i]) == ref.NONE]
    assert rows
    for i in rows:
        stream = case.streams[i]
        key = int(stream[0]["data"]) >> 32
        pcm = case.pool[key]
        whole = chunk(case.pool, key, 0, pcm.shape[0], step=step, position=int(stream[0]["position"]), gain=stream[0]["gain"])
        assert sum(int(f) for f in stream["frames"]) == pcm.shape[0] and not stream["position"][1:].any()
        want, after = sref.render_one(whole, pcm, sum(case.calls + SPLIT), 2)
        got = np.concatenate([r[0][i] for r in results])
        assert sref.same_floats(got, want)[0], case.names[i]
        current = results[-1][1][i][0]
        first = (int(current["data"]) - scases.fake_bases(case.pool)[key]) // (pcm.shape[1] * pcm.dtype.itemsize)
        assert first * ONE + int(current["position"]) == int(after["position"]) and int(current["flags"]) == int(after["flags"]), case.names[i]
        if not int(after["flags"]) & PLAY:
            assert results[-1][2][i] == len(stream) - 1


# ---- the sanitized host build of the kernel ----
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_host_build_plays_every_family(program, tmp_path, name):
    """tests/cpp/stream_rows_host.cpp, the kernel's own text compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer
    where the compiler has them, run as a program of its own: every case of the family, stereo, every chunk's PCM a heap block of exactly
    its size, against the restatement after every call."""
    for case in cases_of(name, 2):
        streams, assets, appends = case.placed()
        calls = case.calls + SPLIT
        args = (streams, [case.programs], [case.resamplers], cases.tables(), assets, 2)
        out, taken = compare(run(program, tmp_path, *args, calls, appends), *args, calls, appends)
        assert taken.sum() >= len(case.names) // 2, case.label


# ---- controls: restatements with one number wrong ----
def caught_by_family(wrong, name, channels=2):
    for case, right in zip(cases_of(name, channels), restated(name, channels)):
        other = play(case, stref.render_voice, channels=channels, wrong=wrong)
        if any(differing(a, b) for a, b in zip(other, right)):
            return True
    return False


@functools.lru_cache(maxsize=None)
def old_random():
    out = []
    for channels in (1, 2, 6):
        rng = np.random.default_rng(5200 + channels)
        streams, programs, resamplers, pool = scases.random_streams(rng, 12, 3, channels, (70, 200, 3, 330))
        streams, assets = scases.resolve_streams(streams, pool, scases.fake_bases(pool))
        out.append((channels, streams, programs, resamplers, assets))
    return out


def caught_by_the_old_cases(wrong):
    """stream_cases.named_streams in its committed calls, and random_streams as tests/test_stream_host.py draws them."""
    right, other = tsr.run_named([(c,) for c in scases.CALLS]), tsr.run_named([(c,) for c in scases.CALLS], wrong)
    if not sref.same_floats(right[0], other[0])[0] or not tsr.same_state(right, other):
        return True
    for channels, streams, programs, resamplers, assets in old_random():
        taken = np.zeros((3, 12), np.uint32)
        a = b = (None, streams, taken, programs)
        for frames in (70, 200, 3, 330):
            a = stref.render(a[1], a[2], a[3], resamplers, cases.tables(), assets, frames, channels)
            b = stref.render(b[1], b[2], b[3], resamplers, cases.tables(), assets, frames, channels, wrong)
            if not sref.same_floats(a[0], b[0])[0] or not tsr.same_state(a, b):
                return True
    return False


# wrong -> the family aimed at it: the forms the committed cases let pass
CONTROLS = {
    "over in 16 bits": "takes past 2^32",
    "start in 32 bits": "an excess that skips entries",
    "one subtraction": "an excess into a loop",
}
# The other four forms of stream_ref.VALUE_WRONG are no evidence of a gap.  Three are caught by the committed cases already: the named
# voice "chains through one-frame chunks shorter than a step" and the random streams' one-frame chunks show a chain that drops the
# excess and an entry that hands its whole start on, and "a STOP fade that completes inside the second chunk" shows a STOP that takes.
# "distance in 32 bits" changes no value anywhere: a truncated E - P gives an n that is too small, never too large; the span is cut short
# of the end, the record is seen not to have reached it, and the next span forms n again -- a split of the render, which the contract's
# invariance makes invisible.  wrong -> (the family that shows it, or None; whether the old cases show it)
DROPPED = {
    "chain drops": ("an excess that skips entries", True),
    "whole start": ("an excess that skips entries", True),
    "stop takes": ("under envelopes at their bounds", True),
    "distance in 32 bits": (None, False),
}


def test_the_lists_of_wrong_forms_are_complete():
    assert sorted(list(CONTROLS) + list(DROPPED)) == sorted(stref.VALUE_WRONG)


@pytest.mark.parametrize("wrong", list(CONTROLS))
def test_a_wrong_form_is_caught_by_its_family_and_not_by_the_old_cases(wrong):
    """The excess kept in 16 bits; the entry's position and the excess added in 32 bits; an entry's loop wrapped by one subtraction.  Each
    differs from the restatement on the family aimed at it, and each gives the committed named voices and the random streams bit for bit
    and byte for byte -- their steps are at most four frames, so no excess reaches 2^16 units, no position plus an excess reaches 2^32,
    and no excess runs past a queued loop's end by more than the loop's length: those gaps were real."""
    assert caught_by_family(wrong, CONTROLS[wrong]), f"{CONTROLS[wrong]} does not show '{wrong}'"
    assert not caught_by_the_old_cases(wrong), f"the old cases catch '{wrong}'"


@pytest.mark.parametrize("wrong", list(DROPPED))
def test_the_dropped_forms_are_dropped_for_their_reasons(wrong):
    """What DROPPED says of each: three forms show on their family and on the committed cases alike; a truncated distance shows nowhere,
    although "an excess that skips entries" holds a voice whose E - P is 2^32 and more."""
    family, old = DROPPED[wrong]
    assert caught_by_the_old_cases(wrong) == old
    if family is not None:
        assert caught_by_family(wrong, family)
    else:
        far = [s for c in cases_of("an excess that skips entries", 2) for s in c.streams if (int(s[0]["frames"]) << 12) - int(s[0]["position"]) >= TWO32]
        assert far and not any(caught_by_family(wrong, name) for name in FAMILIES)
