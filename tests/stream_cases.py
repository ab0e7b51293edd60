"""The voices the sampler streams' contract names one by one (include/oalsfx_hip.h, "sampler streams"), and seeded random streams, for
the restatement's own tests (tests/test_stream_ref.py), the host build of the kernel (tests/test_stream_host.py) and the device
(tests/test_gpu_streams.py).  Everything is data for stream_ref.

A record names its asset by address, and a chunk's address lies inside its asset, so the cases are built with a placeholder in `data`:
the asset's number in the pool in the high 32 bits, the chunk's byte offset in the low ones.  resolve() puts the real addresses in --
the device's, or made-up ones where nothing reads them -- and fills the {(address, frames): PCM} table stream_ref.render looks the assets up in."""
import numpy as np

import polyphony_cases as pcases
import resample_cases as cases
import resample_ref as ref
import sampler_ref as sref
import stream_ref as stref
import voice_ref as vref
from program_cases import segment
from test_sampler_abi import rec
from test_voice_abi import env

f32 = np.float32
ONE = sref.ONE
PLAYING, LOOP, LINEAR = sref.PLAYING, sref.LOOP, sref.LINEAR
CALLS = (1, 63, 64, 65, 256, 7, 200)     # the calls end at 1, 64, 128, 193, 449, 456 and 656
ENDS = tuple(int(v) for v in np.cumsum(CALLS))
LANES, INSTANCES = 2, 6


def width_of(record):
    return np.dtype(sref.PCM_DTYPE[int(record["format"])]).itemsize * int(record["channels"])


def fake_bases(pool):
    """Addresses nothing reads, far enough apart and aligned for every format."""
    return [0x40000000 + 0x1000000 * k for k in range(len(pool))]


def resolve(records, pool, bases, assets):
    """A copy of `records` (an array of sampler_ref.DTYPE) with the placeholders replaced by addresses; a PLAYING record's PCM goes into
    `assets` under its address."""
    out = np.array(records, dtype=sref.DTYPE).copy()
    for r in out.reshape(-1):
        if not int(r["flags"]) & PLAYING:
            r["data"] = 0
            continue
        key, offset = int(r["data"]) >> 32, int(r["data"]) & 0xFFFFFFFF
        first = offset // width_of(r)
        pcm = pool[key][first:first + int(r["frames"])]
        assert offset % width_of(r) == 0 and pcm.shape == (int(r["frames"]), int(r["channels"]))
        r["data"] = bases[key] + offset
        assets[stref.asset_key(r)] = pcm
    return out


def resolve_streams(streams, pool, bases):
    """streams [lanes][n] of placeholder records -> (the same with addresses, the assets' table)."""
    assets = {}
    return [[resolve(s, pool, bases, assets) for s in lane] for lane in streams], assets


def whole(pool, key, fmt, **fields):
    """A playing one-shot over the whole of pool[key], at its own rate unless told otherwise."""
    pcm = pool[key]
    return rec(**dict(dict(data=key << 32, format=fmt, channels=pcm.shape[1], frames=pcm.shape[0], step=ONE, flags=PLAYING), **fields))[0]


def cut(pool, key, fmt, lengths, **fields):
    return stref.chunks(whole(pool, key, fmt, **fields), lengths)


def named_streams(channels=2, seed=31):
    """(names [lanes][n], streams [lanes][n] with placeholders, programs [lanes][n], resamplers [lanes][n], pool, appends: {index of the
    call they follow: [(lane, instance, entries)]})."""
    rng = np.random.default_rng(seed)
    pool = []

    def asset(fmt, width, frames):
        pool.append(cases.asset(rng, fmt, width, frames))
        return len(pool) - 1

    gains = lambda: rng.uniform(-1, 1, sref.MAX_CHANNELS).astype(f32)
    S16, U8, F32 = sref.PCM_S16, sref.PCM_U8, sref.PCM_F32
    idle = [np.zeros(1, sref.DTYPE)[0]]
    none = [env()[0]]
    s = lambda ramp, **kw: segment(rng, channels, ramp, **kw)
    a = [asset(S16, 1, 600), asset(U8, channels, 400), asset(F32, channels, 300), asset(S16, 1, 50), asset(S16, 1, 80), asset(S16, 1, 12), asset(S16, 1, 90),
         asset(F32, 1, 260), asset(S16, channels, 260), asset(U8, 1, 180), asset(F32, channels, 225), asset(S16, channels, 120), asset(U8, 1, 41)]
    loop = whole(pool, a[4], S16, flags=PLAYING | LOOP | LINEAR, loop_start=10, loop_end=70, step=ONE + 9, gain=gains())
    voices = [
        # lane 0
        [("takes at 64, 128, 129, 130, 131, 168 and 512: on calls' last frames, on tile boundaries, three in a tile", cut(pool, a[0], S16, [64, 64, 1, 1, 1, 37, 344, 88], gain=gains()), none, ref.NONE),
         ("pitched, nearest, wide U8: step 5000 from position 123", cut(pool, a[1], U8, [50, 3, 97, 1, 149, 100], step=5000, position=123, gain=gains()), none, ref.NONE),
         ("LINEAR across the seams, wide F32", cut(pool, a[2], F32, [100, 100, 100], step=3000, flags=PLAYING | LINEAR, gain=gains()), none, ref.NONE),
         ("an intro, its loop, and an entry held behind the loop", [whole(pool, a[3], S16, step=ONE + 5, gain=gains()), loop, whole(pool, a[3], S16)], none, ref.NONE),
         ("chains through one-frame chunks shorter than a step, then dry", cut(pool, a[5], S16, [5] + [1] * 7, step=3 * ONE + 77, gain=gains()), none, ref.NONE),
         ("an idle voice that is appended to", idle, none, ref.NONE)],
        # lane 1
        [("under a gain ramp", cut(pool, a[7], F32, [100, 60, 100], gain=gains()), [s(300)], ref.NONE),
         ("under a delay", cut(pool, a[8], S16, [30, 30, 200], step=2 * ONE, gain=gains()), [s(40, delay=70)], ref.NONE),
         ("a STOP fade that completes inside the second chunk", cut(pool, a[9], U8, [60, 60, 60], gain=gains()), [s(100, flags=vref.ACTIVE | vref.STOP)], ref.NONE),
         ("an envelope program whose switches fall in the tile of a take", cut(pool, a[10], F32, [75, 100, 50], gain=gains()), [s(70), s(10), s(200)], ref.NONE),
         ("an 8-tap table over the seams", cut(pool, a[11], S16, [40, 40, 40], step=3500, gain=gains()), none, cases.FINE + 1),
         ("a 4-tap table, pitched down, a one-frame chunk", cut(pool, a[12], U8, [20, 1, 20], step=1000, gain=gains()), none, cases.FINE)],
    ]
    names = [[v[0] for v in lane] for lane in voices]
    streams = [[np.array(v[1], dtype=sref.DTYPE) for v in lane] for lane in voices]
    programs = [[list(v[2]) for v in lane] for lane in voices]
    resamplers = np.asarray([[v[3] for v in lane] for lane in voices])
    appends = {
        0: [(0, 5, cut(pool, a[6], S16, [45, 45], step=ONE + 1000, position=77, gain=gains()))],         # the idle voice starts at frame 1
        4: [(0, 4, cut(pool, a[6], S16, [30, 60], step=ONE // 2, gain=gains())),                          # restart behind an underrun
            (0, 5, cut(pool, a[3], S16, [50], gain=gains()))],
    }
    return names, streams, programs, resamplers, pool, appends


def random_streams(rng, n, lanes, channels, calls, share=0.7):
    """n * lanes voices of polyphony_cases.random_voices' kinds; about `share` of the one-shots are cut into 2 .. 8 random chunks (ones
    of a single frame among them), and some loops get a one-shot intro in front.  A streaming voice's envelope does not GLIDE.  Returns
    (streams [lanes][n] with placeholders, envelopes as programs of one [lanes][n], resamplers [lanes][n], pool)."""
    records, envelopes, resamplers, _, keys, pool = pcases.random_voices(rng, n, lanes, channels, True, calls=calls, asset_frames=(1, 300))
    pcm = [p for _, _, p in pool]
    streams = [[None] * n for _ in range(lanes)]
    programs = [[None] * n for _ in range(lanes)]
    for k in range(lanes):
        for i in range(n):
            r, e = records[k][i].copy(), envelopes[k][i].copy()
            r["data"] = keys[k][i] << 32
            frames = int(r["frames"])
            stream = [r]
            if not int(r["flags"]) & LOOP and int(r["flags"]) & PLAYING and frames >= 2 and rng.random() < share:
                r["position"] = min(int(r["position"]), ONE - 1)
                pieces = int(rng.integers(2, min(8, frames) + 1))
                at = np.sort(rng.choice(np.arange(1, frames), pieces - 1, replace=False))
                stream = list(stref.chunks(r, np.diff(np.concatenate([[0], at, [frames]])).tolist()))
            elif int(r["flags"]) & LOOP and rng.random() < 0.5 and int(r["flags"]) & PLAYING:      # (a queued record must be PLAYING)
                intro = r.copy()
                intro["flags"] = PLAYING | (int(r["flags"]) & LINEAR)
                intro["position"] = 0
                intro["step"] = max(int(r["step"]), 1)
                stream = [intro, r]
            if len(stream) > 1:
                e["flags"] = int(e["flags"]) & ~vref.GLIDE
                if e["flags"] & vref.ACTIVE == 0:
                    e["flags"] = 0
            streams[k][i] = np.array(stream, dtype=sref.DTYPE)
            programs[k][i] = [e]
    return streams, programs, resamplers, pcm


def streams_of(rng, records, keys, share=0.8, frames_used=150):
    """records [lanes][n] of some other case, keys[k][i] their assets' numbers in its pool -> streams [lanes][n] with placeholders: about
    `share` of the PLAYING voices play the first `frames_used` frames of their asset as a one-shot (a loop is dropped) cut into 2 .. 8
    random chunks, from a position inside the first; the other voices are a stream of one."""
    lanes, n = records.shape
    streams = [[None] * n for _ in range(lanes)]
    for k in range(lanes):
        for i in range(n):
            r = records[k][i].copy()
            r["data"] = int(keys[k][i]) << 32
            flags = int(r["flags"])
            stream = [r]
            if flags & PLAYING and int(r["frames"]) >= 2 and rng.random() < share:
                r["flags"], r["loop_start"], r["loop_end"] = flags & ~LOOP, 0, 0
                r["frames"] = frames = min(int(r["frames"]), frames_used)
                r["position"] = int(r["position"]) % ONE
                pieces = int(rng.integers(2, min(8, frames) + 1))
                at = np.sort(rng.choice(np.arange(1, frames), pieces - 1, replace=False))
                stream = list(stref.chunks(r, np.diff(np.concatenate([[0], at, [frames]])).tolist()))
            streams[k][i] = np.array(stream, dtype=sref.DTYPE)
    return streams


def firsts(streams):
    return np.array([[s[0] for s in lane] for lane in streams], dtype=sref.DTYPE)
