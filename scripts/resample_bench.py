"""Resamplers (oalsfx_batch_set_fir_table, oalsfx_batch_set_resamplers): what a render through a 4- or 8-tap phase table costs beside the
linear render of the same records.

    python scripts/resample_bench.py [--steps 60] [--warmup 10] [--repeats 50] [--json out.json] [--only kernel|host]

kernel  sample_device alone on a caller's stream between two HIP events at 4096 x 256 x stereo (BASELINE configs[1]), S16 mono assets,
        looped, LINEAR set, steps near 1.0 (4096 +- 64) and near 2.0 (8192 +- 64); one batch, the same sampler records throughout,
        resamplers and envelopes set anew for every run and the runs taken in turn five times in one process, so that a drift of the
        box hits every one alike:
          k_sampler_rows              no table, no envelope: the linear render
          k_voice_rows                no table, one trivial envelope ACTIVE on row 0, which selects the kernel
          k_fir_rows, no table        one instance names a table, which selects the kernel; 4095 rows take its linear path
          k_fir_rows, T = 4 / T = 8   every row through a table of 8 or of 12 phase bits (Catmull-Rom / windowed sinc)
        Twenty calls per event pair divided by 20.  Bytes: the rows written once; the rate is set against the 8 TB/s of the HBM (the
        assets' reads, two bytes a tap, hit in the caches mostly and are not counted).
host    BASELINE configs[1] (4096 EAX reverbs, stereo, 256 frames, page-locked buffers): oalsfx_batch_play_downmix_meter (voices and buses,
        with carry, 64 buses) on two batches with the same samplers, one without tables and one with the 8-tap table on every row,
        steps alternated in one process, host clock around calls that end in a synchronise; medians and p10-p90.

Run each part as a step of its own, under a time limit, the second only if the first ended well:

    timeout -k 10 300 python scripts/resample_bench.py --only kernel --json kernel.json && \\
    timeout -k 10 300 python scripts/resample_bench.py --only host --json host.json"""
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
from oalsfxpp_amd.api import ENVELOPE_DTYPE, METER_CARRY, METER_DTYPE, RESAMPLER_NONE, SAMPLER_DTYPE, Batch, fir_cubic, fir_sinc  # noqa: E402

N, FRAMES = 4096, 256
ONE = 1 << desc.SAMPLER_FRAC_BITS
HBM_BYTES_PER_S = 8e12
ASSETS, ASSET_FRAMES = 256, 48000       # a pool's worth: a few hundred one-second sounds
TABLES = {0: ("T4_bits8", lambda: fir_cubic(8)), 1: ("T4_bits12", lambda: fir_cubic(12)),
          2: ("T8_bits8", lambda: fir_sinc(8, 8, 0.9)), 3: ("T8_bits12", lambda: fir_sinc(8, 12, 0.9))}
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


def records(n, s16, rng, around):
    """n looping, LINEAR records at steps within 64 of `around` over the assets (s16: [ASSETS][frames] mono)."""
    r = np.zeros(n, SAMPLER_DTYPE)
    r["frames"], r["loop_start"], r["loop_end"] = ASSET_FRAMES, 0, ASSET_FRAMES
    r["position"] = rng.integers(0, ASSET_FRAMES * ONE, n)
    r["step"] = rng.integers(around - 64, around + 65, n)
    r["flags"] = desc.SAMPLER_PLAYING | desc.SAMPLER_LOOP | desc.SAMPLER_LINEAR
    r["gain"][:, :2] = rng.uniform(0.2, 1.0, (n, 2))
    r["format"], r["channels"] = desc.PCM_S16, 1
    r["data"] = s16.data_ptr() + rng.integers(0, ASSETS, n) * (ASSET_FRAMES * 2)
    return r


def setting(run):
    """(resamplers, envelopes, the kernel the run must launch)."""
    tables, e = np.full(N, RESAMPLER_NONE), np.zeros(N, ENVELOPE_DTYPE)
    e["gain_from"], e["gain_to"] = 1.0, 1.0
    if run == "k_sampler_rows":
        return tables, e, "k_sampler_rows"
    if run == "k_voice_rows":
        e["flags"][0] = desc.ENV_ACTIVE
        return tables, e, "k_voice_rows"
    if run == "k_fir_rows_no_table":
        tables[0] = 0
    else:
        tables[:] = next(t for t, (name, _) in TABLES.items() if run.endswith(name))
    return tables, e, "k_fir_rows"


def bench_kernel(repeats):
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    runs = ("k_sampler_rows", "k_voice_rows", "k_fir_rows_no_table") + tuple("k_fir_rows_" + name for name, _ in TABLES.values())
    result = {}
    with Batch(N, desc.FMT_STEREO, 48000, 1) as b:
        for t, (_, make) in TABLES.items():
            b.set_fir_table(t, make())
        dst = torch.empty((N, FRAMES, 2), dtype=torch.float32, device="cuda")
        nbytes = dst.numel() * 4
        render = lambda: b.sample_device(FRAMES, dst.data_ptr(), stream=stream.cuda_stream)
        for pitch, around in (("steps_near_1.0", ONE), ("steps_near_2.0", 2 * ONE)):
            base = records(N, s16, rng, around)
            samples = {run: [] for run in runs}
            for _ in range(5):
                for run in runs:
                    tables, e, kernel = setting(run)
                    b.set_samplers(base)
                    b.set_envelopes(e)
                    b.set_resamplers(tables)
                    for _ in range(3):
                        render()
                    stream.synchronize()
                    assert b.last_render_kernel() == kernel, (run, b.last_render_kernel())
                    samples[run].extend(timed(stream, render, 20, repeats // 5))
            row = {}
            for run, burst in samples.items():
                med = statistics.median(burst)
                row[run] = {"twenty_calls_per_event_pair_per_call": spread(burst), "bytes": nbytes, "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3),
                            "share_of_8_tb_per_s": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
            base_us = row["k_sampler_rows"]["twenty_calls_per_event_pair_per_call"]["median_us"]
            for run in runs[1:]:
                row[run]["over_k_sampler_rows"] = round(row[run]["twenty_calls_per_event_pair_per_call"]["median_us"] / base_us, 3)
            result[pitch] = row
    result["empty_event_pair"] = spread(timed(stream, lambda: None, 1, repeats))
    return {f"{N}x{FRAMES}x2": result}


def bench_host(steps, warmup):
    so = lib.load()
    rng = np.random.default_rng(0)
    n_buses = 64
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    base = records(N, s16, rng, ONE + ONE // 2)
    gain = rng.uniform(0, 1, N).astype(np.float32)
    nrec = (N + n_buses) * METER_DTYPE.itemsize
    with Batch(N, desc.FMT_STEREO, 48000, 1) as plain, Batch(N, desc.FMT_STEREO, 48000, 1) as tabled:
        pinned = [so.oalsfx_pinned_alloc(nrec), so.oalsfx_pinned_alloc(nrec)]
        assert all(pinned)
        try:
            calls = {}
            for name, b, mem in (("without_tables", plain, pinned[0]), ("eight_taps_on_every_row", tabled, pinned[1])):
                b.set_effect_type(0, desc.EAX_REVERB)
                b.apply_changes()
                b.set_routing(np.arange(N) % n_buses, gain)
                b.set_samplers(base)
                if b is tabled:
                    b.set_fir_table(0, fir_sinc(8, 12, 0.9))
                    b.set_resamplers(np.zeros(N, np.int64))
                C.memset(mem, 0, nrec)
                out = b.pinned_array(FRAMES)[:n_buses]
                calls[name] = (b, lambda b=b, out=out, mem=mem: so.oalsfx_batch_play_downmix_meter(
                    b._h, FRAMES, n_buses, out.ctypes.data_as(_fp), 0.001, METER_CARRY, C.c_void_p(mem), C.c_void_p(mem + N * METER_DTYPE.itemsize)))
            times = {name: [] for name in calls}
            for step in range(warmup + steps):
                for name, (b, call) in calls.items():
                    t0 = time.perf_counter()
                    ok = call()
                    t1 = time.perf_counter()
                    assert ok, b.error
                    if step >= warmup:
                        times[name].append((t1 - t0) * 1e6)
            assert plain.last_render_kernel() == "k_sampler_rows" and tabled.last_render_kernel() == "k_fir_rows"
            row = {name: spread(v) for name, v in times.items()}
            row["with_over_without"] = round(row["eight_taps_on_every_row"]["median_us"] / row["without_tables"]["median_us"], 3)
        finally:
            for mem in pinned:
                so.oalsfx_pinned_free(C.c_void_p(mem))
    return {f"play_downmix_meter_{N}_eax_reverbs_{n_buses}_buses": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--only", choices=["host", "kernel"])
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench.py measures on the GPU; none is visible")
    result = {"device": torch.cuda.get_device_name(0)}
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
