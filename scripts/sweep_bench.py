"""Voice filter sweeps (oalsfx_batch_set_sweeps): what k_sweep_rows costs beside k_biquad_rows on the same voices.

    python scripts/sweep_bench.py [--pairs 5] [--repeats 6] [--json out.json]

Shape: 4096 instances x 256 frames x stereo, one lane, mono 16-bit assets, looped, LINEAR set, steps near 1.0 (polyphony_bench.voices),
every voice under an ACTIVE low-pass.  Every run is sample_device alone on one stream between two HIP events, 6 calls per event pair
divided by 6.

  (a) baseline   no sweep is set: the batch launches k_biquad_rows, what the commit in front of the sweeps launches for these voices.
  (b) none       a twin batch on which one voice's sweep was set and cancelled again: the batch still expects a sweep, so k_sweep_rows,
                 and every voice's stage looks at its sweep record (three words) and runs the plain stage.
  (c) one in 64  a twin on which every 64th voice sweeps.
  (d) all        a twin on which every voice sweeps.

The sweeps are 2^24 frames long, so that none completes during the measurement.  The sides are taken in turn `pairs` times in one
process, so that a drift of the box hits all alike; per pair the ratio of the medians, and over the pairs the ratios' median, minimum
and maximum.  The ratios are findings, not pass marks.  The spread of (a) -- (max - min) / median over all its samples -- is printed
beside them.

Run the timing as one step under a time limit:

    timeout -k 10 600 python scripts/sweep_bench.py --json sweeps.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import FILTER_DTYPE, SWEEP_DTYPE, Batch, voice_filter  # noqa: E402
from polyphony_bench import ASSET_FRAMES, ASSETS, FRAMES, N, timed, voices  # noqa: E402

PER = 6
LONG = 1 << 24
VARIANTS = {"a": 0, "b": N, "c": 64, "d": 1}     # every how-manieth voice sweeps (0: none; N: voice 0 alone, cancelled again)


def filters(rng):
    out = np.zeros(N, FILTER_DTYPE)
    for i in range(N):
        out[i] = voice_filter(desc.VF_LOW_PASS, 1.0, rng.uniform(0.01, 0.2), rng.uniform(0.5, 1.5))[0]
    out["flags"] = desc.VF_ACTIVE | desc.VF_LOAD
    return out


def sweeps(rng, low, every):
    """Sweeps of LONG frames from the filters `low` to low-passes an octave or so up, for every `every`-th voice."""
    out = np.zeros(N, SWEEP_DTYPE)
    for i in range(0, N, every):
        to = voice_filter(desc.VF_LOW_PASS, 1.0, rng.uniform(0.2, 0.4), rng.uniform(0.5, 1.5))[0]
        a = np.asarray([low[i][k] for k in ("b0", "b1", "b2", "a1", "a2")], np.float32)
        b = np.asarray([to[k] for k in ("b0", "b1", "b2", "a1", "a2")], np.float32)
        out[i]["flags"], out[i]["frames"] = desc.SWEEP_ACTIVE, LONG
        out[i]["from"], out[i]["to"], out[i]["step"] = a, b, (b - a) / np.float32(LONG)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated rounds (at least five)")
    ap.add_argument("--repeats", type=int, default=6, help="event pairs per variant per round")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated rounds")
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    records, low = voices(1, s16, rng, False), filters(rng)
    dst = torch.empty((len(VARIANTS), N, FRAMES, 2), dtype=torch.float32, device="cuda")
    batches = {}
    try:
        for v, every in VARIANTS.items():
            b = batches[v] = Batch(N, desc.FMT_STEREO, 48000, 1)
            b.set_samplers(records[0])
            b.set_filters(low)
            if every:
                b.set_sweeps(sweeps(np.random.default_rng(1), low, every))
            if v == "b":
                b.set_sweeps(np.zeros(1, SWEEP_DTYPE), instances=[0])
        call = lambda v: batches[v].sample_device(FRAMES, dst[list(VARIANTS).index(v)].data_ptr(), stream=stream.cuda_stream)
        for v in VARIANTS:
            timed(stream, lambda: call(v), PER, 2)
        assert batches["a"].last_render_kernel() == "k_biquad_rows", batches["a"].last_render_kernel()
        assert all(batches[v].last_render_kernel() == "k_sweep_rows" for v in "bcd"), [batches[v].last_render_kernel() for v in "bcd"]
        us = {v: [] for v in VARIANTS}
        ratios = {v: [] for v in "bcd"}
        for _ in range(args.pairs):
            got = {v: timed(stream, lambda: call(v), PER, args.repeats) for v in VARIANTS}
            for v in VARIANTS:
                us[v].extend(got[v])
                if v != "a":
                    ratios[v].append(statistics.median(got[v]) / statistics.median(got["a"]))
        done = batches["d"].get_sweeps(instances=[0])[0]
        assert done["flags"] & desc.SWEEP_ACTIVE and done["done"] < LONG, "a sweep ran out during the measurement"
    finally:
        for b in batches.values():
            b.synchronize()
            b.close()
    summary = lambda x: {"median": round(statistics.median(x), 2), "min": round(min(x), 2), "max": round(max(x), 2),
                         "spread": round((max(x) - min(x)) / statistics.median(x), 4)}
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2, one lane, every voice filtered", "calls_per_event_pair": PER,
              "us": {v: summary(us[v]) for v in VARIANTS},
              "over_baseline": {v: {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3), "pairs": args.pairs} for v, r in ratios.items()}}
    print(f"(a) k_biquad_rows {result['us']['a']['median']:8.2f} us (spread {result['us']['a']['spread']})")
    for v, what in (("b", "no voice sweeps"), ("c", "one voice in 64"), ("d", "every voice")):
        o = result["over_baseline"][v]
        print(f"({v}) k_sweep_rows, {what:16s} {result['us'][v]['median']:8.2f} us, ratio {o['median']} ({o['min']} - {o['max']})")
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
