"""Filter programs (oalsfx_batch_set_filter_programs): what k_filter_program_rows costs beside k_sweep_rows on the same voices.

    python scripts/filter_program_bench.py [--pairs 5] [--repeats 8] [--json out.json]

Shape: 4096 instances x 256 frames x stereo, one lane, mono 16-bit assets, looped, LINEAR set, steps near 1.0 (polyphony_bench.voices),
every voice under an ACTIVE low-pass.  A program is used up by the frames rendered, so every timed render is preceded by a set call that
puts the variant's records back and by a render of ONE frame that carries the upload of those rows to the device (both outside the
events: the first timed attempt had the upload of 4096 queue rows, 2.4 MB out of page-locked host memory, inside them, and measured
that); the render between the two HIP events is then ONE sample_device call of 256 frames.  The segment lengths below count from the
timed render's first frame; the first segment is one frame longer for the frame in front.

  (a) baseline   every voice on one sweep of 2^24 frames: k_sweep_rows, what the commit in front of the filter programs launches.
  (b) no switch  every voice on a program of two segments whose first is 2^24 frames long: k_filter_program_rows, the queue walked, no
                 segment taken inside the render.
  (c) one        every voice on (128, 2^24): one switch inside the render, on a tile boundary.
  (c_mid)        every voice on (100, 2^24): one switch inside the render, in mid-tile.
  (d) seven      every voice on eight segments of 30 frames: seven switches inside the render, up to three in one tile, and 16 frames
                 of `to` behind the program's end.

The sides are taken in turn `pairs` times in one process, so that a drift of the box hits all alike; per pair the ratio of the medians,
and over the pairs the ratios' median, minimum and maximum.  The ratios are findings, not pass marks.  The spread of (a) -- (max - min) /
median over all its samples -- is printed beside them.

Run the timing as one step under a time limit:

    timeout -k 10 600 python scripts/filter_program_bench.py --json filter_programs.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import SWEEP_DTYPE, Batch, voice_filter  # noqa: E402
from polyphony_bench import ASSET_FRAMES, ASSETS, FRAMES, N, voices  # noqa: E402
from sweep_bench import filters  # noqa: E402

LONG = 1 << 24
COEFFICIENTS = ("b0", "b1", "b2", "a1", "a2")
SHAPES = {"a": (LONG,), "b": (LONG, LONG), "c": (129, LONG), "c_mid": (101, LONG), "d": (31,) + (30,) * 7}
KERNEL = {"a": "k_sweep_rows", "b": "k_filter_program_rows", "c": "k_filter_program_rows", "c_mid": "k_filter_program_rows", "d": "k_filter_program_rows"}


def programs(rng, low, shape):
    """[N][len(shape)] sweeps: for every voice a continuous chain from its filter `low` through low-passes further up and down."""
    out = np.zeros((N, len(shape)), SWEEP_DTYPE)
    for i in range(N):
        at = np.asarray([low[i][k] for k in COEFFICIENTS], np.float32)
        for j, frames in enumerate(shape):
            to = voice_filter(desc.VF_LOW_PASS, 1.0, rng.uniform(0.05, 0.4), rng.uniform(0.5, 1.5))[0]
            to = np.asarray([to[k] for k in COEFFICIENTS], np.float32)
            out[i][j]["flags"], out[i][j]["frames"] = desc.SWEEP_ACTIVE, frames
            out[i][j]["from"], out[i][j]["to"], out[i][j]["step"] = at, to, (to - at) / np.float32(frames)
            at = to
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated rounds (at least five)")
    ap.add_argument("--repeats", type=int, default=8, help="timed renders per variant per round")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("filter_program_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated rounds")
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    records, low = voices(1, s16, rng, False), filters(rng)
    dst = torch.empty((len(SHAPES), N, FRAMES, 2), dtype=torch.float32, device="cuda")
    batches, rows = {}, {}
    try:
        for v, shape in SHAPES.items():
            b = batches[v] = Batch(N, desc.FMT_STEREO, 48000, 1)
            b.set_samplers(records[0])
            b.set_filters(low)
            rows[v] = programs(np.random.default_rng(1), low, shape)

        def render(v):
            """One timed render of variant v, its records put back first; returns microseconds."""
            b = batches[v]
            if len(SHAPES[v]) == 1:
                b.set_sweeps(np.ascontiguousarray(rows[v][:, 0]))
            else:
                b.set_filter_programs(rows[v])
            b.sample_device(1, dst[list(SHAPES).index(v)].data_ptr(), stream=stream.cuda_stream)     # (the upload, and one frame)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            b.sample_device(FRAMES, dst[list(SHAPES).index(v)].data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            stream.synchronize()
            assert b.last_render_kernel() == KERNEL[v], (v, b.last_render_kernel())
            return e0.elapsed_time(e1) * 1e3

        for v in SHAPES:
            for _ in range(3):
                render(v)
        # what a render leaves: (c) and (d) have walked their queues
        left = {v: len(batches[v].get_filter_programs(instances=[0])[0]) for v in SHAPES}
        assert left == {"a": 1, "b": 2, "c": 1, "c_mid": 1, "d": 1}, left
        us = {v: [] for v in SHAPES}
        ratios = {v: [] for v in SHAPES if v != "a"}
        for _ in range(args.pairs):
            got = {v: [render(v) for _ in range(args.repeats)] for v in SHAPES}
            for v in SHAPES:
                us[v].extend(got[v])
                if v != "a":
                    ratios[v].append(statistics.median(got[v]) / statistics.median(got["a"]))
    finally:
        for b in batches.values():
            b.synchronize()
            b.close()
    summary = lambda x: {"median": round(statistics.median(x), 2), "min": round(min(x), 2), "max": round(max(x), 2),
                         "spread": round((max(x) - min(x)) / statistics.median(x), 4)}
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2, one lane, every voice filtered", "calls_per_event_pair": 1,
              "segments": {v: [int(f) for f in s] for v, s in SHAPES.items()}, "us": {v: summary(us[v]) for v in SHAPES},
              "over_baseline": {v: {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3), "pairs": args.pairs} for v, r in ratios.items()}}
    print(f"(a) k_sweep_rows, one sweep per voice {result['us']['a']['median']:8.2f} us (spread {result['us']['a']['spread']})")
    for v, what in (("b", "no switch"), ("c", "one switch, frame 128"), ("c_mid", "one switch, frame 100"), ("d", "seven switches")):
        o = result["over_baseline"][v]
        print(f"({v}) k_filter_program_rows, {what:22s} {result['us'][v]['median']:8.2f} us, ratio {o['median']} ({o['min']} - {o['max']})")
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
