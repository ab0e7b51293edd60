"""Bus sends (oalsfx_batch_set_send_routing, oalsfx_batch_set_send_ramps): what the longer member lists and the ramp kernel cost.

    python scripts/sends_bench.py [--rounds 5] [--parent ab/liboalsfx_hip_parent.so] [--json out.json]
    python scripts/sends_bench.py --child            # one process, the library OALSFX_LIB names, one JSON line

4096 instances, 256 stereo frames, into 1 and into 64 buses.  A child process times oalsfx_batch_downmix_device alone on a caller's stream
between two HIP events, 20 calls per event pair divided by 20, 40 pairs, median:
  plain    send 0 only, no ramp: the two kernels of the bus downmix (every library has this one)
  ramps    send 0 only, every send ramping (2^24 frames, so that the ramps outlast the run): level 1 is k_downmix_ramp_chunks
  sends2   sends 0 and 1 routed, no ramp: twice the members, every row read twice
  sends4   all four sends routed, no ramp
The driver runs the children in alternated rounds -- the parent's library (built from the parent commit into ab/, as scripts/ab_libs.py
does), then this one -- and reports the median over the rounds of each figure, the range of the parent's own rounds (the
parent-against-parent spread that any difference has to be set against) and the ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, FRAMES, CALLS, PAIRS = 4096, 256, 20, 40


def child():
    import numpy as np
    import torch

    from oalsfxpp_amd import desc, lib
    from oalsfxpp_amd.api import Batch

    so = lib.load()
    has_sends = hasattr(so, "oalsfx_batch_set_send_ramps")
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.standard_normal((N, FRAMES, 2)).astype(np.float32)).cuda()
    side = torch.cuda.Stream()
    result = {"sends": has_sends}

    def timed(b, n_buses):
        dst = torch.empty((n_buses, FRAMES, 2), dtype=torch.float32, device="cuda")
        for _ in range(CALLS):
            b.downmix_device(FRAMES, src.data_ptr(), n_buses, dst.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        us = []
        for _ in range(PAIRS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(side)
            for _ in range(CALLS):
                b.downmix_device(FRAMES, src.data_ptr(), n_buses, dst.data_ptr(), stream=side.cuda_stream)
            t1.record(side)
            t1.synchronize()
            us.append(t0.elapsed_time(t1) * 1000.0 / CALLS)
        return round(statistics.median(us), 3)

    for n_buses in (1, 64):
        gain = rng.uniform(0, 1, N).astype(np.float32)
        configs = ["plain"] + (["ramps", "sends2", "sends4"] if has_sends else [])
        for config in configs:
            with Batch(N, desc.FMT_STEREO, 48000, 1) as b:
                b.set_routing(np.arange(N) % n_buses, gain)
                if config == "ramps":
                    b.set_send_ramps(1.0 - gain, 1 << 24)
                for send in range(1, {"sends2": 2, "sends4": 4}.get(config, 1)):
                    b.set_routing((np.arange(N) + send) % n_buses, gain, send=send)
                result[f"{config}_{n_buses}"] = timed(b, n_buses)
                uploads = b.downmix_uploads()
            assert uploads == 1, (config, uploads)
    print(json.dumps(result), flush=True)


def run_child(library):
    env = dict(os.environ)
    if library:
        env["OALSFX_LIB"] = library
    else:
        env.pop("OALSFX_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        sys.exit(f"child failed ({library or 'this tree'}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "liboalsfx_hip_parent.so"))
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.child:
        return child()
    rounds = {"parent": [], "change": []}
    for _ in range(args.rounds):
        if os.path.exists(args.parent):
            rounds["parent"].append(run_child(args.parent))
        rounds["change"].append(run_child(""))
    report = {"shape": f"{N} instances x {FRAMES} frames x stereo", "rounds": args.rounds, "per_round": rounds}
    median = lambda side, key: round(statistics.median(r[key] for r in rounds[side]), 3)
    for n_buses in (1, 64):
        row = {}
        if rounds["parent"]:
            values = [r[f"plain_{n_buses}"] for r in rounds["parent"]]
            row["parent_plain_us"] = median("parent", f"plain_{n_buses}")
            row["parent_rounds_min_max_us"] = [min(values), max(values)]
        for config in ("plain", "ramps", "sends2", "sends4"):
            row[f"{config}_us"] = median("change", f"{config}_{n_buses}")
        row["ramps_over_plain"] = round(row["ramps_us"] / row["plain_us"], 3)
        row["sends2_over_plain"] = round(row["sends2_us"] / row["plain_us"], 3)
        row["sends4_over_plain"] = round(row["sends4_us"] / row["plain_us"], 3)
        report[f"{n_buses}_buses"] = row
    text = json.dumps(report, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
