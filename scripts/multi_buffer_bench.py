"""K queued device buffers: K chained mix_device calls against one mix_device_multi call (4096 EAX reverbs, stereo, defaults, one process).

    python scripts/multi_buffer_bench.py [--rounds 5] [--round-ms 200] [--json out.json]
    python scripts/multi_buffer_bench.py --pmc-run        # a few multi calls only, for a counter run of its own (rocprofv3 --pmc)

The two ways alternate round by round (single, multi, single, multi, ...); a round repeats its K buffers for at least --round-ms and
reports microseconds per 256 frames.  Every buffer is an allocation of its own, as an engine's ring of buffers would be."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import Batch  # noqa: E402

N = 4096


def make_batch():
    b = Batch(N, desc.FMT_STEREO, 48000, 1)
    b.set_effect_type(0, desc.EAX_REVERB)
    b.apply_changes()
    return b


def make_buffers(frames, k):
    srcs = [torch.empty(N * frames * 2, device="cuda").uniform_(-1, 1) for _ in range(k)]
    dsts = [torch.empty_like(s) for s in srcs]
    torch.cuda.synchronize()
    return [s.data_ptr() for s in srcs], [d.data_ptr() for d in dsts], (srcs, dsts)


def warm(b, frames, sp, dp):
    # ordinary calls until the device has proven every instance steady, then a few of each way
    for _ in range(8):
        for s, d in zip(sp, dp):
            b.mix_device(frames, s, d)
        b.synchronize()
        if b.plan(0)[1] == N:
            break
    for _ in range(3):
        b.mix_device_multi(frames, sp, dp)
    b.synchronize()


def one_round(b, frames, sp, dp, multi, round_ms):
    reps = 0
    b.synchronize()
    t0 = time.perf_counter()
    while True:
        if multi:
            b.mix_device_multi(frames, sp, dp)
        else:
            for s, d in zip(sp, dp):
                b.mix_device(frames, s, d)
        reps += 1
        if reps % 4 == 0 and (time.perf_counter() - t0) * 1e3 >= round_ms:
            break
    b.synchronize()
    dt = time.perf_counter() - t0
    return dt / (reps * len(sp) * frames / 256) * 1e6   # us per 256 frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--pmc-run", action="store_true")
    args = ap.parse_args()
    b = make_batch()
    if args.pmc_run:
        frames, k = 256, 8
        sp, dp, keep = make_buffers(frames, k)
        warm(b, frames, sp, dp)
        for _ in range(4):
            b.mix_device_multi(frames, sp, dp)
        b.synchronize()
        print(json.dumps({"pmc_run": True, "frames": frames, "buffers": k, "multi_counts": b.multi_counts(), "kernel": b.last_reverb_kernel}))
        return
    out = {"instances": N, "channels": 2, "rounds": args.rounds, "round_ms": args.round_ms, "configs": []}
    for frames, k in ((256, 8), (64, 32)):
        sp, dp, keep = make_buffers(frames, k)
        warm(b, frames, sp, dp)
        c0 = b.multi_counts()
        single, multi = [], []
        for _ in range(args.rounds):
            single.append(one_round(b, frames, sp, dp, False, args.round_ms))
            multi.append(one_round(b, frames, sp, dp, True, args.round_ms))
        c1 = b.multi_counts()
        ms, mm = statistics.median(single), statistics.median(multi)
        rec = {"frames": frames, "buffers": k,
               "single_us_per_256": round(ms, 2), "single_spread": [round(min(single), 2), round(max(single), 2)],
               "multi_us_per_256": round(mm, 2), "multi_spread": [round(min(multi), 2), round(max(multi), 2)],
               "multi_below_single_pct": round(100.0 * (ms - mm) / ms, 1), "rate_ratio": round(ms / mm, 3),
               "passes": c1[1] - c0[1], "buffers_in_passes": c1[0] - c0[0], "kernel": b.last_reverb_kernel,
               "gsamples_per_s_multi": round(N * 256 / (mm * 1e-6) / 1e9, 2)}
        out["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        del keep
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    b.close()


if __name__ == "__main__":
    main()
