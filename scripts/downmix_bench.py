"""Bus downmix (oalsfx_batch_downmix_device, oalsfx_batch_mix_downmix): what it costs and what it saves.

    python scripts/downmix_bench.py [--steps 60] [--warmup 10] [--json out.json] [--only host|kernel|join]

host    BASELINE configs[1] (4096 EAX reverbs, stereo, 256 frames, page-locked buffers) into 1 and into 64 buses.  Baseline: what a caller
        does without the feature -- oalsfx_batch_mix, then the same two-level sum on the host (NumPy, vectorised over the chunks); the
        GPU-and-copy part and the host sum are timed separately.  Candidate: oalsfx_batch_mix_downmix.  Same process, steps alternated,
        host clock around calls that end in a synchronise; medians and p10-p90.  The two results are compared bit for bit on the way.
        The three legs of the baseline (copy in, kernels, copy out) come from oalsfx_batch_mix_timed.
kernel  downmix_device alone on a caller's stream between two HIP events: 4096 x 256 x stereo into 1, 8 and 64 buses, 32 768 instances
        into 1 bus, 64 frames (the short-row shape), and 4, 2 and 1 floats per access (oalsfx_debug_downmix_vector).  One call per event
        pair (uncorrected: an empty pair measures about 4 us here), and 20 calls per pair divided by 20.  Bytes: the routed rows read
        once; the rate is set against the 8 TB/s of the HBM.
join    200 steps of mix_device + downmix_device(hip_stream NULL) against 200 steps of mix_device alone (chained), one synchronise at
        the end, five rounds alternated: the difference is the end of the chained run every step plus the downmix."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc, lib  # noqa: E402
from oalsfxpp_amd.api import DOWNMIX_CHUNK, Batch  # noqa: E402

FRAMES = 256
HBM_BYTES_PER_S = 8e12
_fp = C.POINTER(C.c_float)


def spread(us):
    q = statistics.quantiles(us, n=10)
    return {"median_us": round(statistics.median(us), 2), "p10_us": round(q[0], 2), "p90_us": round(q[-1], 2), "samples": len(us)}


def host_sum(y, members, gains, n_buses):
    """The contract's two-level sum with the members of every bus as a [chunks][32] table (a bus's members a multiple of 32 here)."""
    out = np.zeros((n_buses,) + y.shape[1:], dtype=np.float32)
    for b in range(n_buses):
        rows = y[members[b]]                             # [chunks][32][frames][channels]
        p = np.zeros((rows.shape[0],) + y.shape[1:], dtype=np.float32)
        for k in range(DOWNMIX_CHUNK):
            p = p + rows[:, k] * gains[b][:, k, None, None]
        acc = np.zeros(y.shape[1:], dtype=np.float32)
        for j in range(p.shape[0]):
            acc = acc + p[j]
        out[b] = acc
    return out


def bench_host(steps, warmup):
    n = 4096
    so = lib.load()
    result = {}
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect_type(0, desc.EAX_REVERB)
        b.apply_changes()
        src, dst = b.pinned_array(FRAMES), b.pinned_array(FRAMES)
        buses_all = b.pinned_array(FRAMES)               # (room for up to n buses; the first n_buses rows are used)
        rng = np.random.default_rng(0)
        src[:] = rng.uniform(-1, 1, src.shape).astype(np.float32)
        gain = rng.uniform(0, 1, n).astype(np.float32)
        legs = (C.c_double * 3)()
        for n_buses in (1, 64):
            bus = np.arange(n) % n_buses
            b.set_routing(bus, gain)
            members = [np.nonzero(bus == k)[0].reshape(-1, DOWNMIX_CHUNK) for k in range(n_buses)]
            gains = [gain[m] for m in members]
            out = buses_all[:n_buses]
            base_gpu, base_sum, cand, leg_rows = [], [], [], []
            for step in range(warmup + steps):
                t0 = time.perf_counter()
                ok = so.oalsfx_batch_mix(b._h, FRAMES, src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp))
                t1 = time.perf_counter()
                host_sum(dst, members, gains, n_buses)
                t2 = time.perf_counter()
                assert ok
                t3 = time.perf_counter()
                ok = so.oalsfx_batch_mix_downmix(b._h, FRAMES, src.ctypes.data_as(_fp), n_buses, out.ctypes.data_as(_fp))
                t4 = time.perf_counter()
                assert ok, b.error
                if step >= warmup:
                    base_gpu.append((t1 - t0) * 1e6)
                    base_sum.append((t2 - t1) * 1e6)
                    cand.append((t4 - t3) * 1e6)
            for _ in range(10):
                assert so.oalsfx_batch_mix_timed(b._h, FRAMES, src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp), legs)
                leg_rows.append(list(legs))
            result[f"{n_buses}_buses"] = {
                "baseline_mix_gpu_and_copy": spread(base_gpu), "baseline_host_sum_numpy": spread(base_sum), "mix_downmix": spread(cand),
                "baseline_legs_us_copy_in_kernels_copy_out": [round(statistics.median(r[k] for r in leg_rows), 2) for k in range(3)],
                "bytes_copied_out": {"baseline": int(dst.nbytes), "mix_downmix": int(out.nbytes)}}
    # bit for bit: each call advances the reverbs, so the plain mix and mix_downmix are compared on two batches in the same state
    with Batch(n, desc.FMT_STEREO, 48000, 1) as a, Batch(n, desc.FMT_STEREO, 48000, 1) as c:
        for t in (a, c):
            t.set_effect_type(0, desc.EAX_REVERB)
            t.apply_changes()
        bus = np.arange(n) % 64
        c.set_routing(bus, gain)
        members = [np.nonzero(bus == k)[0].reshape(-1, DOWNMIX_CHUNK) for k in range(64)]
        same = True
        for _ in range(3):
            y = a.mix(src)
            got = c.mix_downmix(src, 64)
            same = same and got.tobytes() == host_sum(y, members, [gain[m] for m in members], 64).tobytes()
        result["mix_downmix_equals_mix_plus_host_sum_bit_for_bit"] = bool(same)
    return result


def bench_kernel(repeats):
    so = lib.load()
    result = {}
    stream = torch.cuda.Stream()
    shapes = [(4096, FRAMES, 1), (4096, FRAMES, 8), (4096, FRAMES, 64), (32768, FRAMES, 1), (4096, 64, 1), (4096, 64, 64), (4096, 2048, 1)]
    try:
        for n, frames, n_buses in shapes:
            with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
                b.set_routing(np.arange(n) % n_buses, np.full(n, 0.5, dtype=np.float32))
                src = torch.rand((n, frames, 2), dtype=torch.float32, device="cuda")
                out = torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda")
                nbytes = src.numel() * 4
                for width in ((4, 2, 1) if frames == FRAMES and n == 4096 else (4,)):
                    so.oalsfx_debug_downmix_vector(width)
                    for _ in range(5):
                        b.downmix_device(frames, src.data_ptr(), n_buses, out.data_ptr(), stream=stream.cuda_stream)
                    stream.synchronize()
                    single, burst = [], []
                    for per, sink in ((1, single), (20, burst)):
                        for _ in range(repeats):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            for _ in range(per):
                                b.downmix_device(frames, src.data_ptr(), n_buses, out.data_ptr(), stream=stream.cuda_stream)
                            e1.record(stream)
                            stream.synchronize()
                            sink.append(e0.elapsed_time(e1) * 1e3 / per)
                    med = statistics.median(burst)
                    result[f"{n}x{frames}x2_into_{n_buses}_width{width}"] = {
                        "one_call_per_event_pair": spread(single), "twenty_calls_per_event_pair_per_call": spread(burst), "bytes_read": nbytes,
                        "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "share_of_8_tb_per_s": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
        empty = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            e1.record(stream)
            stream.synchronize()
            empty.append(e0.elapsed_time(e1) * 1e3)
        result["empty_event_pair"] = spread(empty)
    finally:
        so.oalsfx_debug_downmix_vector(4)
    return result


def bench_join(rounds=5, steps=200):
    n, n_buses = 4096, 1
    result = {}
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect_type(0, desc.EAX_REVERB)
        b.apply_changes()
        src = torch.rand((n, FRAMES, 2), dtype=torch.float32, device="cuda") * 2 - 1
        dst = torch.empty_like(src)
        out = torch.empty((n_buses, FRAMES, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(40):
            b.mix_device(FRAMES, src.data_ptr(), dst.data_ptr())
            b.synchronize()
        alone, both = [], []
        chained_alone = chained_both = 0
        for _ in range(rounds):
            for with_downmix, sink in ((False, alone), (True, both)):
                b.synchronize()
                before = b.chained_calls
                t0 = time.perf_counter()
                for _ in range(steps):
                    b.mix_device(FRAMES, src.data_ptr(), dst.data_ptr())
                    if with_downmix:
                        b.downmix_device(FRAMES, dst.data_ptr(), n_buses, out.data_ptr())
                b.synchronize()
                sink.append((time.perf_counter() - t0) / steps * 1e6)
                if with_downmix:
                    chained_both += b.chained_calls - before
                else:
                    chained_alone += b.chained_calls - before
        result = {"mix_device_alone_us_per_step": [round(v, 2) for v in alone], "mix_device_and_downmix_us_per_step": [round(v, 2) for v in both],
                  "median_alone_us": round(statistics.median(alone), 2), "median_with_downmix_us": round(statistics.median(both), 2),
                  "chained_calls_alone": chained_alone, "chained_calls_with_downmix": chained_both, "steps_per_round": steps}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--only", choices=["host", "kernel", "join"])
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("downmix_bench.py measures on the GPU; none is visible")
    result = {"device": torch.cuda.get_device_name(0), "chunk": DOWNMIX_CHUNK}
    if args.only in (None, "kernel"):
        result["kernel"] = bench_kernel(args.repeats)
    if args.only in (None, "join"):
        result["join"] = bench_join()
    if args.only in (None, "host"):
        result["host"] = bench_host(args.steps, args.warmup)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
