"""Level meters (oalsfx_batch_meter_device, oalsfx_batch_mix_downmix_meter): what they cost beside the downmix and the plain mix.

    python scripts/meter_bench.py [--steps 60] [--warmup 10] [--repeats 50] [--json out.json] [--only kernel|host]

kernel  meter_device alone and downmix_device alone (1 bus) on a caller's stream between two HIP events, in one process, alternated per
        shape: 4096 x 256 x stereo (BASELINE configs[1]), 32 768 x 256 x stereo and 4096 x 2048 x stereo.  Both read the same bytes; the
        meter is one launch where the downmix is two.  One call per event pair (uncorrected: the empty pair is recorded beside it), and
        20 calls per pair divided by 20.  Bytes: the rows read once; the rate is set against the 8 TB/s of the HBM.
host    BASELINE configs[1] (4096 EAX reverbs, stereo, 256 frames, page-locked buffers): oalsfx_batch_mix, oalsfx_batch_mix_downmix and
        oalsfx_batch_mix_downmix_meter (voices and buses, with carry; and the voices only) into 1 and into 64 buses, steps alternated
        in one process, host clock around calls that end in a synchronise; medians and p10-p90."""
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
from oalsfxpp_amd.api import METER_CARRY, METER_DTYPE, METER_LANES, Batch  # noqa: E402

FRAMES = 256
HBM_BYTES_PER_S = 8e12
_fp = C.POINTER(C.c_float)


def spread(us):
    q = statistics.quantiles(us, n=10)
    return {"median_us": round(statistics.median(us), 2), "p10_us": round(q[0], 2), "p90_us": round(q[-1], 2), "samples": len(us)}


def timed(stream, call, per, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(per):
            call()
        e1.record(stream)
        stream.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per)
    return out


def bench_kernel(repeats):
    result = {}
    stream = torch.cuda.Stream()
    for n, frames in ((4096, FRAMES), (32768, FRAMES), (4096, 2048)):
        with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
            b.set_routing(np.zeros(n, int), np.full(n, 0.5, dtype=np.float32))
            src = torch.rand((n, frames, 2), dtype=torch.float32, device="cuda") * 2 - 1
            out = torch.empty((1, frames, 2), dtype=torch.float32, device="cuda")
            meters = torch.zeros(n * METER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            nbytes = src.numel() * 4
            calls = {"meter_device": lambda: b.meter_device(n, frames, src.data_ptr(), meters.data_ptr(), 0.001, stream=stream.cuda_stream),
                     "meter_device_carry": lambda: b.meter_device(n, frames, src.data_ptr(), meters.data_ptr(), 0.001, carry=True, stream=stream.cuda_stream),
                     "downmix_device_1_bus": lambda: b.downmix_device(frames, src.data_ptr(), 1, out.data_ptr(), stream=stream.cuda_stream)}
            for call in calls.values():
                for _ in range(5):
                    call()
            stream.synchronize()
            row = {}
            samples = {name: ([], []) for name in calls}
            for _ in range(5):                                  # alternated, so that a drift of the box hits every call alike
                for name, call in calls.items():
                    samples[name][0].extend(timed(stream, call, 1, repeats // 5))
                    samples[name][1].extend(timed(stream, call, 20, repeats // 5))
            for name, (single, burst) in samples.items():
                med = statistics.median(burst)
                row[name] = {"one_call_per_event_pair": spread(single), "twenty_calls_per_event_pair_per_call": spread(burst), "bytes_read": nbytes,
                             "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "share_of_8_tb_per_s": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
            row["meter_over_downmix_twenty_calls"] = round(row["meter_device"]["twenty_calls_per_event_pair_per_call"]["median_us"] /
                                                           row["downmix_device_1_bus"]["twenty_calls_per_event_pair_per_call"]["median_us"], 3)
            row["meter_over_downmix_one_call"] = round(row["meter_device"]["one_call_per_event_pair"]["median_us"] /
                                                       row["downmix_device_1_bus"]["one_call_per_event_pair"]["median_us"], 3)
            result[f"{n}x{frames}x2"] = row
    result["empty_event_pair"] = spread(timed(stream, lambda: None, 1, repeats))
    return result


def bench_host(steps, warmup):
    n = 4096
    so = lib.load()
    result = {}
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect_type(0, desc.EAX_REVERB)
        b.apply_changes()
        src, dst, buses_all = b.pinned_array(FRAMES), b.pinned_array(FRAMES), b.pinned_array(FRAMES)
        records = (n + 64) * METER_DTYPE.itemsize
        pinned = so.oalsfx_pinned_alloc(records)
        assert pinned
        try:
            meters = np.frombuffer((C.c_char * records).from_address(pinned), dtype=METER_DTYPE)
            meters[:] = np.zeros(1, METER_DTYPE)
            rng = np.random.default_rng(0)
            src[:] = rng.uniform(-1, 1, src.shape).astype(np.float32)
            gain = rng.uniform(0, 1, n).astype(np.float32)
            for n_buses in (1, 64):
                b.set_routing(np.arange(n) % n_buses, gain)
                out = buses_all[:n_buses]
                s, d, o = src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp), out.ctypes.data_as(_fp)
                vm, bm = C.c_void_p(meters.ctypes.data), C.c_void_p(meters.ctypes.data + n * METER_DTYPE.itemsize)
                calls = {"mix": lambda: so.oalsfx_batch_mix(b._h, FRAMES, s, d),
                         "mix_downmix": lambda: so.oalsfx_batch_mix_downmix(b._h, FRAMES, s, n_buses, o),
                         "mix_downmix_meter_voices_and_buses_carry": lambda: so.oalsfx_batch_mix_downmix_meter(b._h, FRAMES, s, n_buses, o, 0.001, METER_CARRY, vm, bm),
                         "mix_downmix_meter_voices": lambda: so.oalsfx_batch_mix_downmix_meter(b._h, FRAMES, s, n_buses, o, 0.001, 0, vm, None)}
                times = {name: [] for name in calls}
                for step in range(warmup + steps):
                    for name, call in calls.items():
                        t0 = time.perf_counter()
                        ok = call()
                        t1 = time.perf_counter()
                        assert ok, b.error
                        if step >= warmup:
                            times[name].append((t1 - t0) * 1e6)
                row = {name: spread(v) for name, v in times.items()}
                row["bytes_copied_out"] = {"mix": int(dst.nbytes), "mix_downmix": int(out.nbytes),
                                           "mix_downmix_meter_voices_and_buses": int(out.nbytes) + (n + n_buses) * METER_DTYPE.itemsize}
                row["metered_over_plain_mix"] = round(row["mix_downmix_meter_voices_and_buses_carry"]["median_us"] / row["mix"]["median_us"], 3)
                result[f"{n_buses}_buses"] = row
        finally:
            del meters
            so.oalsfx_pinned_free(C.c_void_p(pinned))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--only", choices=["host", "kernel"])
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meter_bench.py measures on the GPU; none is visible")
    result = {"device": torch.cuda.get_device_name(0), "lanes": METER_LANES}
    if args.only in (None, "kernel"):
        result["kernel"] = bench_kernel(args.repeats)
    if args.only in (None, "host"):
        result["host"] = bench_host(args.steps, args.warmup)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
