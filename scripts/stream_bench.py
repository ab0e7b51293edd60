"""Sampler streams (oalsfx_batch_set_streams): what k_stream_rows and k_stream_filter_rows cost beside the kernels the commit in front of
the streams launches for the same voices.

    python scripts/stream_bench.py [--pairs 5] [--repeats 8] [--json out.json]

Shape: 4096 instances x 256 frames x stereo, mono 16-bit assets, nearest sample, steps near 1.0.  A stream is used up by the frames
rendered, so every timed render is preceded by a set call that puts the variant's records back and by a render of ONE frame that carries
the upload of those rows to the device (both outside the events); the render between the two HIP events is then ONE sample_device call
of 256 frames.  Chunk lengths below count from the timed render's first frame; the first chunk is one frame longer for the frame in
front.  A voice plays a one-shot long enough not to end (or, for the takes, chunks that add up to more than the render).

  unfiltered, one lane
  (s)   k_sampler_rows          every voice a plain one-shot: the baseline.
  (p)   k_program_rows          the same voices under an envelope program of two long segments: the sibling that walks a queue.
  (r0)  k_stream_rows           every voice a stream of two chunks whose first outlasts the render: the ring walked, no take.
  (r1)  k_stream_rows           chunks (100, long): one take inside the render, in mid-tile.
  (r8)  k_stream_rows           eight chunks of 30 frames and a long one: eight takes inside the render.
  unfiltered, four lanes
  (m)   k_mix_rows, K = 4       four plain voices per instance: the baseline at K = 4.
  (m0)  k_stream_rows, K = 4    the same with lane 0 a stream of two chunks, no take.
  filtered, one lane, every voice under an ACTIVE low-pass
  (b)   k_biquad_rows           plain voices: the baseline.
  (f)   k_filter_program_env_rows   the same under an envelope program and a filter program of two long segments each.
  (f0)  k_stream_filter_rows    streams of two chunks, no take.
  (f1)  k_stream_filter_rows    chunks (100, long): one take in mid-tile.

The sides are taken in turn `pairs` times in one process, so that a drift of the box hits all alike; per pair the ratio of the medians
against the group's baseline -- (s), (m) or (b) --, and over the pairs the ratios' median, minimum and maximum.  The ratios are findings,
not pass marks.  The spread of each baseline -- (max - min) / median over all its samples -- is printed beside them.

Run the timing as one step under a time limit:

    timeout -k 10 900 python scripts/stream_bench.py --json streams.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import ENVELOPE_DTYPE, SAMPLER_DTYPE, SWEEP_DTYPE, Batch  # noqa: E402
from polyphony_bench import ASSET_FRAMES, ASSETS, FRAMES, N  # noqa: E402
from sweep_bench import filters  # noqa: E402

ONE = 1 << desc.SAMPLER_FRAC_BITS
LONG = 1 << 24
# variant: (kernel, lanes, filtered, chunk lengths of lane 0's stream or None, envelope / filter programs, its baseline)
VARIANTS = {
    "s": ("k_sampler_rows", 1, False, None, False, None), "p": ("k_program_rows", 1, False, None, True, "s"),
    "r0": ("k_stream_rows", 1, False, (ASSET_FRAMES // 2, ASSET_FRAMES // 2), False, "s"), "r1": ("k_stream_rows", 1, False, (101, ASSET_FRAMES - 101), False, "s"),
    "r8": ("k_stream_rows", 1, False, (31,) + (30,) * 7 + (ASSET_FRAMES - 241,), False, "s"),
    "m": ("k_mix_rows", 4, False, None, False, None), "m0": ("k_stream_rows", 4, False, (ASSET_FRAMES // 2, ASSET_FRAMES // 2), False, "m"),
    "b": ("k_biquad_rows", 1, True, None, False, None), "f": ("k_filter_program_env_rows", 1, True, None, True, "b"),
    "f0": ("k_stream_filter_rows", 1, True, (ASSET_FRAMES // 2, ASSET_FRAMES // 2), False, "b"), "f1": ("k_stream_filter_rows", 1, True, (101, ASSET_FRAMES - 101), False, "b"),
}


def one_shots(lanes, s16, rng):
    """records [lanes][N]: one-shots from frame 0 at steps within 64 of 1.0, nearest sample, which 257 frames do not use up."""
    r = np.zeros((lanes, N), SAMPLER_DTYPE)
    r["frames"] = ASSET_FRAMES
    r["step"] = rng.integers(ONE - 64, ONE + 65, (lanes, N))
    r["flags"] = desc.SAMPLER_PLAYING
    r["gain"][:, :, :2] = rng.uniform(0.2, 1.0, (lanes, N, 2))
    r["format"], r["channels"] = desc.PCM_S16, 1
    r["data"] = s16.data_ptr() + rng.integers(0, ASSETS, (lanes, N)) * (ASSET_FRAMES * 2)
    return r


def chunked(records, lengths):
    """[N][len(lengths)] records: every voice's asset cut into consecutive chunks of `lengths` frames (oalsfx_host_stream_chunks' arithmetic
    for chunks of unequal length)."""
    out = np.zeros((N, len(lengths)), SAMPLER_DTYPE)
    first = 0
    for j, frames in enumerate(lengths):
        out[:, j] = records
        out[:, j]["data"] = records["data"] + first * 2
        out[:, j]["frames"] = frames
        first += frames
    return out


def two_long(dtype, **fields):
    """[N][2] ACTIVE records of a program whose first segment outlasts every render."""
    out = np.zeros((N, 2), dtype)
    for k, v in fields.items():
        out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated rounds (at least five)")
    ap.add_argument("--repeats", type=int, default=8, help="timed renders per variant per round")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated rounds")
    assert ASSET_FRAMES > 2 * (FRAMES + 1) + 241, "the chunks must outlast a render"
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    low = filters(rng)
    envelopes = two_long(ENVELOPE_DTYPE, flags=desc.ENV_ACTIVE, ramp_frames=LONG, gain_from=1.0, gain_to=1.0)
    sweeps = two_long(SWEEP_DTYPE, flags=desc.SWEEP_ACTIVE, frames=LONG)
    for k in ("from", "to"):
        for j, name in enumerate(("b0", "b1", "b2", "a1", "a2")):
            sweeps[k][:, :, j] = low[name][:, None]
    dst = torch.empty((N, FRAMES, 2), dtype=torch.float32, device="cuda")
    batches, records = {}, {}
    try:
        for v, (_, lanes, filtered, lengths, programs, _) in VARIANTS.items():
            b = batches[v] = Batch(N, desc.FMT_STEREO, 48000, 1)
            b.set_polyphony(lanes)
            records[v] = one_shots(lanes, s16, np.random.default_rng(1))
            if filtered:
                b.set_filters(low)

        def render(v):
            """One timed render of variant v, its records put back first; returns microseconds."""
            kernel, lanes, filtered, lengths, programs, _ = VARIANTS[v]
            b = batches[v]
            for k in range(lanes):
                if lengths and k == 0:
                    b.set_streams(list(chunked(records[v][0], lengths)))
                else:
                    b.set_samplers(records[v][k], lane=k)
            if programs:
                b.set_env_programs(envelopes)
                if filtered:
                    b.set_filter_programs(list(sweeps))
            b.sample_device(1, dst.data_ptr(), stream=stream.cuda_stream)     # (the upload, and one frame)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            b.sample_device(FRAMES, dst.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            stream.synchronize()
            assert b.last_render_kernel() == kernel, (v, b.last_render_kernel())
            return e0.elapsed_time(e1) * 1e3

        for v in VARIANTS:
            for _ in range(3):
                render(v)
        # what a render leaves: the takes the variants' names promise
        taken = {v: int(batches[v].get_stream_state(instances=[0])[0][0]) for v in VARIANTS}
        assert taken == {"s": 0, "p": 0, "r0": 0, "r1": 1, "r8": 8, "m": 0, "m0": 0, "b": 0, "f": 0, "f0": 0, "f1": 1}, taken
        us = {v: [] for v in VARIANTS}
        ratios = {v: [] for v, spec in VARIANTS.items() if spec[5]}
        for _ in range(args.pairs):
            got = {v: [render(v) for _ in range(args.repeats)] for v in VARIANTS}
            for v, spec in VARIANTS.items():
                us[v].extend(got[v])
                if spec[5]:
                    ratios[v].append(statistics.median(got[v]) / statistics.median(got[spec[5]]))
    finally:
        for b in batches.values():
            b.synchronize()
            b.close()
    summary = lambda x: {"median": round(statistics.median(x), 2), "min": round(min(x), 2), "max": round(max(x), 2),
                         "spread": round((max(x) - min(x)) / statistics.median(x), 4)}
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2", "calls_per_event_pair": 1,
              "variants": {v: {"kernel": spec[0], "lanes": spec[1], "filtered": spec[2], "chunks": spec[3], "baseline": spec[5]} for v, spec in VARIANTS.items()},
              "us": {v: summary(us[v]) for v in VARIANTS},
              "over_baseline": {v: {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3), "pairs": args.pairs} for v, r in ratios.items()}}
    for v, spec in VARIANTS.items():
        if spec[5]:
            o = result["over_baseline"][v]
            print(f"({v:3s}) {spec[0]:26s} {result['us'][v]['median']:8.2f} us, over ({spec[5]}) {o['median']} ({o['min']} - {o['max']})")
        else:
            print(f"({v:3s}) {spec[0]:26s} {result['us'][v]['median']:8.2f} us (spread {result['us'][v]['spread']})")
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
