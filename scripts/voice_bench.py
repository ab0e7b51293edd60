"""Voice envelopes (oalsfx_batch_set_envelopes): what a render with envelopes costs beside the samplers' render of the same records.

    python scripts/voice_bench.py [--steps 60] [--warmup 10] [--repeats 50] [--json out.json] [--only kernel|host] [--channels 2]

kernel  sample_device alone on a caller's stream between two HIP events at 4096 x 256 x stereo (BASELINE configs[1]), S16 mono assets,
        looped, linear, random steps; one batch, the same sampler records throughout, the envelopes set anew for every run and the runs
        taken in turn five times in one process, so that a drift of the box hits every one alike:
          k_sampler_rows          no envelope ACTIVE: the launch the parent commit has
          k_voice_rows, idle      one trivial envelope ACTIVE on row 0, which selects the kernel; 4095 rows take its samplers' path
          k_voice_rows, ramps     a gain ramp under way on every row
          k_voice_rows, glides    a gain ramp and a pitch glide under way on every row
        Twenty calls per event pair divided by 20, and one call per pair (uncorrected: the empty pair is recorded beside it).  Bytes:
        the rows written once; the rate is set against the 8 TB/s of the HBM.  meter_device over the same rows beside them.
        --channels 1, 2, 4, 6, 7 or 8 takes the kernels of another output format (6: the 5.1 instantiations) over the same mono assets.
host    BASELINE configs[1] (4096 EAX reverbs, stereo, 256 frames, page-locked buffers): oalsfx_batch_play_downmix_meter (voices and buses,
        with carry, 64 buses) on two batches with the same samplers, one without envelopes and one with a ramp and a glide on every row,
        steps alternated in one process, host clock around calls that end in a synchronise; medians and p10-p90.

Run each part as a step of its own, under a time limit, the second only if the first ended well:

    timeout -k 10 300 python scripts/voice_bench.py --only kernel --json kernel.json && \\
    timeout -k 10 300 python scripts/voice_bench.py --only host --json host.json"""
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
from oalsfxpp_amd.api import ENVELOPE_DTYPE, METER_CARRY, METER_DTYPE, SAMPLER_DTYPE, Batch  # noqa: E402

N, FRAMES = 4096, 256
ONE = 1 << desc.SAMPLER_FRAC_BITS
HBM_BYTES_PER_S = 8e12
ASSETS, ASSET_FRAMES = 256, 48000       # a pool's worth: a few hundred one-second sounds
RUNS = ("k_sampler_rows", "k_voice_rows_idle", "k_voice_rows_ramps", "k_voice_rows_ramps_and_glides")
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


FORMATS = {1: desc.FMT_MONO, 2: desc.FMT_STEREO, 4: desc.FMT_QUAD, 6: desc.FMT_5POINT1, 7: desc.FMT_6POINT1, 8: desc.FMT_7POINT1}


def records(n, s16, rng, channels=2):
    """n looping, interpolating records at random steps over the assets (s16: [ASSETS][frames] mono)."""
    r = np.zeros(n, SAMPLER_DTYPE)
    r["frames"], r["loop_start"], r["loop_end"] = ASSET_FRAMES, 0, ASSET_FRAMES
    r["position"] = rng.integers(0, ASSET_FRAMES * ONE, n)
    r["step"] = rng.integers(ONE // 2, 2 * ONE, n)
    r["flags"] = desc.SAMPLER_PLAYING | desc.SAMPLER_LOOP | desc.SAMPLER_LINEAR
    r["gain"][:, :channels] = rng.uniform(0.2, 1.0, (n, channels))
    r["format"], r["channels"] = desc.PCM_S16, 1
    r["data"] = s16.data_ptr() + rng.integers(0, ASSETS, n) * (ASSET_FRAMES * 2)
    return r


def envelopes(run, steps, rng, channels=2):
    """The envelopes of a run: ramps of 2^24 and glides of 2^20 frames, so that thousands of calls of 256 frames stay inside both."""
    n = len(steps)
    e = np.zeros(n, ENVELOPE_DTYPE)
    if run == "k_sampler_rows":
        return e
    e["gain_from"], e["gain_to"] = 1.0, 1.0
    if run == "k_voice_rows_idle":
        e["flags"][0] = desc.ENV_ACTIVE
        return e
    e["flags"] = desc.ENV_ACTIVE
    e["ramp_frames"] = 1 << 24
    e["gain_from"][:, :channels] = rng.uniform(0.0, 1.0, (n, channels))
    e["gain_to"][:, :channels] = rng.uniform(0.0, 1.0, (n, channels))
    e["gain_step"] = (e["gain_to"] - e["gain_from"]) / np.float32(1 << 24)
    if run == "k_voice_rows_ramps_and_glides":
        e["flags"] |= desc.ENV_GLIDE
        e["glide_frames"] = 1 << 20
        e["step_to"] = rng.integers(ONE // 2, 2 * ONE, n)
        e["glide_slope"] = ((e["step_to"].astype(np.int64) - steps.astype(np.int64)) << 16) // (1 << 20)     # (toward minus infinity: inside the range too)
    return e


def bench_kernel(repeats, channels):
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    result = {}
    with Batch(N, FORMATS[channels], 48000, 1) as b:
        dst = torch.empty((N, FRAMES, channels), dtype=torch.float32, device="cuda")
        meters = torch.zeros(N * METER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        nbytes = dst.numel() * 4
        render = lambda: b.sample_device(FRAMES, dst.data_ptr(), stream=stream.cuda_stream)
        meter = lambda: b.meter_device(N, FRAMES, dst.data_ptr(), meters.data_ptr(), 0.001, stream=stream.cuda_stream)
        base = records(N, s16, rng, channels)
        samples = {run: ([], []) for run in RUNS + ("meter_device",)}
        for _ in range(5):
            for run in RUNS:
                b.set_samplers(base)                                 # the same records, and steps no glide has moved
                b.set_envelopes(envelopes(run, base["step"], rng, channels))
                for _ in range(3):
                    render()
                stream.synchronize()
                assert b.last_render_kernel() == ("k_sampler_rows" if run == "k_sampler_rows" else "k_voice_rows")
                samples[run][0].extend(timed(stream, render, 1, repeats // 5))
                samples[run][1].extend(timed(stream, render, 20, repeats // 5))
            samples["meter_device"][0].extend(timed(stream, meter, 1, repeats // 5))
            samples["meter_device"][1].extend(timed(stream, meter, 20, repeats // 5))
        for run, (single, burst) in samples.items():
            med = statistics.median(burst)
            result[run] = {"one_call_per_event_pair": spread(single), "twenty_calls_per_event_pair_per_call": spread(burst), "bytes": nbytes,
                           "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "share_of_8_tb_per_s": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
        base_us = result["k_sampler_rows"]["twenty_calls_per_event_pair_per_call"]["median_us"]
        for run in RUNS[1:]:
            result[run]["over_k_sampler_rows"] = round(result[run]["twenty_calls_per_event_pair_per_call"]["median_us"] / base_us, 3)
    result["empty_event_pair"] = spread(timed(stream, lambda: None, 1, repeats))
    return {f"{N}x{FRAMES}x{channels}": result}


def bench_host(steps, warmup):
    so = lib.load()
    rng = np.random.default_rng(0)
    n_buses = 64
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    base = records(N, s16, rng)
    gain = rng.uniform(0, 1, N).astype(np.float32)
    nrec = (N + n_buses) * METER_DTYPE.itemsize
    with Batch(N, desc.FMT_STEREO, 48000, 1) as plain, Batch(N, desc.FMT_STEREO, 48000, 1) as shaped:
        pinned = [so.oalsfx_pinned_alloc(nrec), so.oalsfx_pinned_alloc(nrec)]
        assert all(pinned)
        try:
            calls = {}
            for name, b, mem in (("without_envelopes", plain, pinned[0]), ("ramps_and_glides_on_every_row", shaped, pinned[1])):
                b.set_effect_type(0, desc.EAX_REVERB)
                b.apply_changes()
                b.set_routing(np.arange(N) % n_buses, gain)
                b.set_samplers(base)
                if b is shaped:
                    b.set_envelopes(envelopes(RUNS[3], base["step"], rng))
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
            assert plain.last_render_kernel() == "k_sampler_rows" and shaped.last_render_kernel() == "k_voice_rows"
            row = {name: spread(v) for name, v in times.items()}
            row["with_over_without"] = round(row["ramps_and_glides_on_every_row"]["median_us"] / row["without_envelopes"]["median_us"], 3)
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
    ap.add_argument("--channels", type=int, default=2, choices=sorted(FORMATS), help="of the kernel part's output format")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("voice_bench.py measures on the GPU; none is visible")
    result = {"device": torch.cuda.get_device_name(0)}
    if args.only in (None, "kernel"):
        result["kernel"] = bench_kernel(args.repeats, args.channels)
    if args.only in (None, "host"):
        result["host"] = bench_host(args.steps, args.warmup)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
