"""Envelope programs (oalsfx_batch_set_env_programs): what k_program_rows costs beside the render of the same voices without a program.

    python scripts/program_bench.py [--pairs 5] [--repeats 6] [--json out.json]
    python scripts/program_bench.py --baseline-only [--json out.json]
    python scripts/program_bench.py --only b --lanes 4 [--calls 60]

Shape: 4096 instances x 256 frames x stereo, mono 16-bit assets, looped, LINEAR set, steps near 1.0 (4096 +- 64), every lane playing
under an ACTIVE envelope whose gains ramp (polyphony_bench.voices).  Every run is sample_device alone on one stream between two HIP
events, 6 calls per event pair divided by 6.

  (a) baseline   every voice has one envelope segment, set with oalsfx_batch_set_envelopes, and no batch call of this feature is made:
                 the batch launches what the commit in front of the envelope programs launches for these voices (k_voice_rows at K = 1,
                 k_mix_rows at K >= 2).
  (b) pending    a twin batch, every voice with a program of two segments whose first is 2^24 frames long: the queues are pending in
                 every call and no boundary falls inside one.  k_program_rows.
  (c) switching  a twin batch, every voice with a program of eight segments: the first ends at a frame of the voice's own inside the first
                 call (1 + (37 * voice) mod 255), the next six are 256 frames long, so that every call of seven has one boundary per voice,
                 each voice's at another frame.  The programs are set again in front of every event pair and the first call, which also
                 carries the upload, is made outside the timed region: six timed calls, one boundary per voice in each.

Cases: K = 1, 4 and 16.  The sides of a case are taken in turn `pairs` times in one process, so that a drift of the box hits all alike;
per pair the ratio of the medians, and over the pairs the ratios' median, minimum and maximum.  (b)/(a) and (c)/(a) are findings, not
pass marks.  The spread of (a) -- (max - min) / median over all its samples -- is printed beside them: (a) on two builds is the same
within it or is not.

--baseline-only measures (a) alone and calls nothing the parent commit lacks: copied into a checkout of the parent's scripts/ and run
there on the same machine, the file gives the parent's figure and run-to-run spread for (a).

--only a|b|c runs `calls` calls of one variant at one K and times nothing: the run to collect counters in, by itself, e.g.

    timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR -d out -- \\
        python scripts/program_bench.py --only c --lanes 4

Run the timing as one step under a time limit:

    timeout -k 10 600 python scripts/program_bench.py --json programs.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import ENVELOPE_DTYPE, Batch  # noqa: E402
from polyphony_bench import ASSET_FRAMES, ASSETS, FRAMES, N, timed, voices  # noqa: E402

PER = 6                # timed calls per event pair: the boundaries a program of eight has left behind the untimed first call
LONG = 1 << 24         # the longest ramp a record holds


def segments(rng, shape, ramp):
    """Envelope records of `shape`, ACTIVE, gains ramping between random levels over `ramp` frames (an array or a number)."""
    e = np.zeros(shape, ENVELOPE_DTYPE)
    e["flags"] = desc.ENV_ACTIVE
    e["ramp_frames"] = ramp
    a, b = rng.uniform(0.2, 1.0, shape + (2,)).astype(np.float32), rng.uniform(0.2, 1.0, shape + (2,)).astype(np.float32)
    e["gain_from"][..., :2], e["gain_to"][..., :2] = a, b
    frames = np.maximum(e["ramp_frames"], 1).astype(np.float32)[..., None]
    e["gain_step"][..., :2] = (b - a) / frames
    return e


def programs_switching(rng, lanes):
    """[lanes][N][8]: one boundary per voice in each of seven calls of FRAMES frames, at a frame of the voice's own."""
    voice = np.arange(lanes)[:, None] * N + np.arange(N)[None, :]
    p = segments(rng, (lanes, N, 8), FRAMES)
    p["ramp_frames"][:, :, 0] = 1 + (37 * voice) % (FRAMES - 1)
    p["gain_step"][:, :, 0, :2] = (p["gain_to"][:, :, 0, :2] - p["gain_from"][:, :, 0, :2]) / p["ramp_frames"][:, :, 0, None].astype(np.float32)
    p["ramp_frames"][:, :, 7] = LONG
    return p


class Case:
    def __init__(self, stream, lanes, s16, rng, variants):
        self.stream, self.lanes = stream, lanes
        records = voices(lanes, s16, rng, False)
        self.plain_envelopes = segments(rng, (lanes, N), LONG)
        self.switching = programs_switching(rng, lanes) if "c" in variants else None
        self.batches = {v: Batch(N, desc.FMT_STEREO, 48000, 1) for v in variants}
        self.dst = torch.empty((len(variants), N, FRAMES, 2), dtype=torch.float32, device="cuda")
        for b in self.batches.values():
            b.set_polyphony(lanes)
            for k in range(lanes):
                b.set_samplers(records[k], lane=k)
        self.arm("a")
        self.arm("b")

    def arm(self, v):
        b = self.batches.get(v)
        if b is None:
            return
        for k in range(self.lanes):
            if v == "a":
                b.set_envelopes(self.plain_envelopes[k], lane=k)
            elif v == "b":
                pending = segments(np.random.default_rng(k), (N, 2), LONG)
                b.set_env_programs(pending, lane=k)
            else:
                b.set_env_programs(self.switching[k], lane=k)

    def call(self, v):
        at = list(self.batches).index(v)
        self.batches[v].sample_device(FRAMES, self.dst[at].data_ptr(), stream=self.stream.cuda_stream)

    def sample(self, v, repeats):
        """`repeats` event pairs of PER calls of variant v, in microseconds per call."""
        out = []
        for _ in range(repeats):
            if v == "c":
                self.arm("c")
                self.call("c")        # the upload and the first boundary, outside the timed region
                self.stream.synchronize()
            out.extend(timed(self.stream, lambda: self.call(v), PER, 1))
        return out

    def kernel(self, v):
        return self.batches[v].last_render_kernel()

    def close(self):
        for b in self.batches.values():
            b.synchronize()
            b.close()


def summary(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
            "spread": round((max(us) - min(us)) / statistics.median(us), 4)}


def bench_case(stream, lanes, s16, rng, variants, pairs, repeats):
    case = Case(stream, lanes, s16, rng, variants)
    try:
        for v in variants:
            case.sample(v, 2)
        former = "k_mix_rows" if lanes >= 2 else "k_voice_rows"
        assert case.kernel("a") == former, case.kernel("a")
        assert all(case.kernel(v) == "k_program_rows" for v in variants if v != "a"), [case.kernel(v) for v in variants]
        us = {v: [] for v in variants}
        ratios = {v: [] for v in variants if v != "a"}
        for _ in range(pairs):
            got = {v: case.sample(v, repeats) for v in variants}
            for v in variants:
                us[v].extend(got[v])
                if v != "a":
                    ratios[v].append(statistics.median(got[v]) / statistics.median(got["a"]))
        row = {"lanes": lanes, "baseline_kernel": former, "us": {v: summary(us[v]) for v in variants}}
        row["over_baseline"] = {v: {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3), "pairs": pairs} for v, r in ratios.items()}
        return row
    finally:
        case.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated rounds per case (at least five)")
    ap.add_argument("--repeats", type=int, default=6, help="event pairs per variant per round")
    ap.add_argument("--baseline-only", action="store_true", help="variant (a) alone, with nothing the parent commit lacks")
    ap.add_argument("--only", choices=["a", "b", "c"], help="one variant, untimed: the run to collect counters in")
    ap.add_argument("--lanes", type=int, default=4, help="K of the --only run")
    ap.add_argument("--calls", type=int, default=60, help="calls of the --only run")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("program_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated rounds")
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    if args.only:
        case = Case(stream, args.lanes, s16, rng, (args.only,))
        try:
            case.sample(args.only, max(1, args.calls // PER))
            print(f"{args.only}: K = {args.lanes}, {case.kernel(args.only)}")
        finally:
            case.close()
        return
    variants = ("a",) if args.baseline_only else ("a", "b", "c")
    rows = []
    for lanes in (1, 4, 16):
        rows.append(bench_case(stream, lanes, s16, rng, variants, args.pairs, args.repeats))
        r = rows[-1]
        text = f"K = {lanes:2d}  (a) {r['us']['a']['median']:8.2f} us ({r['baseline_kernel']}, spread {r['us']['a']['spread']})"
        for v in variants[1:]:
            o = r["over_baseline"][v]
            text += f"  ({v}) {r['us'][v]['median']:8.2f} us, ratio {o['median']} ({o['min']} - {o['max']})"
        print(text, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2", "calls_per_event_pair": PER,
              "empty_event_pair_us": round(statistics.median(timed(stream, lambda: None, 1, 30)), 2), "cases": rows}
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
