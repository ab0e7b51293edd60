"""Voice filters (oalsfx_batch_set_filters): what k_biquad_rows costs beside the render of the same voices without a filter.

    python scripts/biquad_bench.py [--pairs 5] [--repeats 6] [--per 10] [--json out.json]

Shape: 4096 instances x 256 frames x stereo, mono 16-bit assets, looped, LINEAR set, steps near 1.0 (4096 +- 64), every lane playing.
Every run is sample_device alone on one stream between two HIP events, `per` calls per event pair divided by `per`.

  unfiltered  a batch in which no filter is ACTIVE: it launches what the commit in front of the voice filters launched for these voices
              (k_sampler_rows or k_fir_rows at K = 1, k_mix_rows at K >= 2; those files' gfx950 code is unchanged).
  filtered    a twin batch with the same voices and ACTIVE low-passes on a share of them: k_biquad_rows.  "none": one voice of the whole
              batch is filtered, so that the kernel is k_biquad_rows and every other voice takes its unfiltered path.

Cases: K = 1, 4 and 16; none, one voice in four (every fourth instance at K = 1, lane k of instance i where (k + i) % 4 == 0 else)
and all voices filtered; without a table and through an 8-tap table of 12 phase bits.  The two sides of a case are taken in turn `pairs`
times in one process, so that a drift of the box hits both alike; per pair the ratio of the medians, and over the pairs the ratios'
median, minimum and maximum.  There is no pass mark: the figure is what the feature costs.

Run it as one step under a time limit:

    timeout -k 10 600 python scripts/biquad_bench.py --json biquad.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import FILTER_DTYPE, Batch, fir_sinc, rcp_q_from_bandwidth, voice_filter  # noqa: E402
from polyphony_bench import ASSET_FRAMES, ASSETS, FRAMES, N, timed, voices  # noqa: E402


def filters(lanes, share):
    """[lanes][N] of FILTER_DTYPE: low-passes at a tenth of the sampling rate on `share` of the voices."""
    f = np.zeros((lanes, N), FILTER_DTYPE)
    f[:] = voice_filter(desc.VF_LOW_PASS, 1.0, 0.1, rcp_q_from_bandwidth(0.1, 1.0))[0]
    k, i = np.arange(lanes)[:, None], np.arange(N)[None, :]
    on = {"none": (k == 0) & (i == 0), "one in four": (k + i) % 4 == 0, "all": (k + i) >= 0}[share]
    f["flags"] = np.where(on, desc.VF_ACTIVE | desc.VF_LOAD, desc.VF_LOAD)
    return f


def bench_case(stream, lanes, tabled, share, s16, rng, pairs, repeats, per):
    records = voices(lanes, s16, rng, False)
    table = fir_sinc(8, 12, 0.9) if tabled else None
    rows = filters(lanes, share)
    with Batch(N, desc.FMT_STEREO, 48000, 1) as plain, Batch(N, desc.FMT_STEREO, 48000, 1) as b:
        for batch in (plain, b):
            batch.set_polyphony(lanes)
            if tabled:
                batch.set_fir_table(0, table)
            for k in range(lanes):
                batch.set_samplers(records[k], lane=k)
                if tabled:
                    batch.set_resamplers(np.zeros(N, np.int64), lane=k)
        for k in range(lanes):
            b.set_filters(rows[k], lane=k)
        dst = torch.empty((2, N, FRAMES, 2), dtype=torch.float32, device="cuda")
        unfiltered = lambda: plain.sample_device(FRAMES, dst[0].data_ptr(), stream=stream.cuda_stream)
        filtered = lambda: b.sample_device(FRAMES, dst[1].data_ptr(), stream=stream.cuda_stream)
        for _ in range(3):
            unfiltered()
            filtered()
        stream.synchronize()
        former = plain.last_render_kernel()
        assert b.last_render_kernel() == "k_biquad_rows" and former == ("k_mix_rows" if lanes >= 2 else "k_fir_rows" if tabled else "k_sampler_rows"), (b.last_render_kernel(), former)
        ours, theirs, ratios = [], [], []
        for _ in range(pairs):
            a, t = timed(stream, filtered, per, repeats), timed(stream, unfiltered, per, repeats)
            ours.extend(a)
            theirs.extend(t)
            ratios.append(statistics.median(a) / statistics.median(t))
        b.synchronize()
        plain.synchronize()
    return {"lanes": lanes, "table": "T8_bits12" if tabled else "none", "filtered": share, "unfiltered_kernel": former,
            "filtered_us": {"median": round(statistics.median(ours), 2), "min": round(min(ours), 2), "max": round(max(ours), 2)},
            "unfiltered_us": {"median": round(statistics.median(theirs), 2), "min": round(min(theirs), 2), "max": round(max(theirs), 2)},
            "filtered_over_unfiltered": {"median": round(statistics.median(ratios), 3), "min": round(min(ratios), 3), "max": round(max(ratios), 3), "pairs": pairs}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated pairs per case (at least five)")
    ap.add_argument("--repeats", type=int, default=6, help="event pairs per side per pair")
    ap.add_argument("--per", type=int, default=10, help="calls per event pair")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("biquad_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated pairs")
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    cases = [(lanes, tabled, share) for tabled in (False, True) for lanes in (1, 4, 16) for share in ("none", "one in four", "all")]
    rows = []
    for lanes, tabled, share in cases:
        rows.append(bench_case(stream, lanes, tabled, share, s16, rng, args.pairs, args.repeats, args.per))
        r = rows[-1]
        print(f"K = {lanes:2d}  {r['table']:9s}  {share:11s}  {r['filtered_us']['median']:8.2f} us against {r['unfiltered_us']['median']:8.2f} ({r['unfiltered_kernel']})  "
              f"ratio {r['filtered_over_unfiltered']['median']} ({r['filtered_over_unfiltered']['min']} - {r['filtered_over_unfiltered']['max']})", flush=True)
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2", "empty_event_pair_us": round(statistics.median(timed(stream, lambda: None, 1, 30)), 2), "cases": rows}
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
