"""Samplers (oalsfx_batch_sample_device, oalsfx_batch_play_downmix_meter): what a render costs beside the copy in it replaces.

    python scripts/sampler_bench.py [--steps 60] [--warmup 10] [--repeats 50] [--json out.json] [--only kernel|host]

kernel  sample_device alone on a caller's stream between two HIP events, alternated with meter_device on the same shapes in one process:
        4096 x 256 x stereo (BASELINE configs[1]), 32 768 x 256 x stereo and 4096 x 2048 x stereo.  Variants: S16 mono looped linear at a
        step of 4096 and at random steps, F32 stereo, all voices stopped.  Twenty calls per event pair divided by 20, and one call per pair
        (uncorrected: the empty pair is recorded beside it).  Bytes: the rows written once; the rate is set against the 8 TB/s of the
        HBM.  Beside them the copy-in leg of oalsfx_batch_mix as oalsfx_batch_mix_timed reports it in the same process.
host    BASELINE configs[1] (4096 EAX reverbs, stereo, 256 frames, page-locked buffers): oalsfx_batch_mix_downmix_meter against
        oalsfx_batch_play_downmix_meter (voices and buses, with carry; and the voices only) into 1 and into 64 buses, steps alternated
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
from oalsfxpp_amd.api import METER_CARRY, METER_DTYPE, SAMPLER_DTYPE, Batch  # noqa: E402

FRAMES = 256
ONE = 1 << desc.SAMPLER_FRAC_BITS
HBM_BYTES_PER_S = 8e12
ASSETS, ASSET_FRAMES = 256, 48000       # a pool's worth: a few hundred one-second sounds
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


def records(n, variant, s16, f32, rng):
    """n looping records over the assets (s16: [ASSETS][frames] mono, f32: [ASSETS][frames][2])."""
    r = np.zeros(n, SAMPLER_DTYPE)
    which = rng.integers(0, ASSETS, n)
    r["frames"], r["loop_start"], r["loop_end"] = ASSET_FRAMES, 0, ASSET_FRAMES
    r["position"] = rng.integers(0, ASSET_FRAMES * ONE, n)
    r["step"] = rng.integers(ONE // 2, 2 * ONE, n) if variant == "s16_mono_loop_linear_random_step" else ONE
    r["flags"] = 0 if variant == "stopped" else desc.SAMPLER_PLAYING | desc.SAMPLER_LOOP | desc.SAMPLER_LINEAR
    r["gain"][:, :2] = rng.uniform(0.2, 1.0, (n, 2))
    if variant == "f32_stereo_loop_linear":
        r["format"], r["channels"] = desc.PCM_F32, 2
        r["data"] = f32.data_ptr() + which * (ASSET_FRAMES * 2 * 4)
    else:
        r["format"], r["channels"] = desc.PCM_S16, 1
        r["data"] = s16.data_ptr() + which * (ASSET_FRAMES * 2)
    return r


VARIANTS = ("s16_mono_loop_linear_step_4096", "s16_mono_loop_linear_random_step", "f32_stereo_loop_linear", "stopped")


def copy_in_leg(b, frames, repeats):
    """The copy-in leg of oalsfx_batch_mix from page-locked memory, by the library's own events: microseconds."""
    so = lib.load()
    src, dst = b.pinned_array(frames), b.pinned_array(frames)
    src[:] = 0.25
    legs = (C.c_double * 3)()
    out = []
    for k in range(repeats + 3):
        assert so.oalsfx_batch_mix_timed(b._h, frames, src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp), legs), b.error
        if k >= 3:
            out.append(legs[0])
    return out


def bench_kernel(repeats):
    result = {}
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    f32 = torch.rand((ASSETS, ASSET_FRAMES, 2), dtype=torch.float32, device="cuda") * 2 - 1
    for n, frames in ((4096, FRAMES), (32768, FRAMES), (4096, 2048)):
        with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
            dst = torch.empty((n, frames, 2), dtype=torch.float32, device="cuda")
            meters = torch.zeros(n * METER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            nbytes = dst.numel() * 4
            render = lambda: b.sample_device(frames, dst.data_ptr(), stream=stream.cuda_stream)
            meter = lambda: b.meter_device(n, frames, dst.data_ptr(), meters.data_ptr(), 0.001, stream=stream.cuda_stream)
            row = {}
            for variant in VARIANTS:
                b.set_samplers(records(n, variant, s16, f32, rng))
                for _ in range(5):
                    render()
                    meter()
                stream.synchronize()
                samples = {"sample_device": ([], []), "meter_device": ([], [])}
                for _ in range(5):                                  # alternated, so that a drift of the box hits every call alike
                    for name, call in (("sample_device", render), ("meter_device", meter)):
                        samples[name][0].extend(timed(stream, call, 1, repeats // 5))
                        samples[name][1].extend(timed(stream, call, 20, repeats // 5))
                cell = {}
                for name, (single, burst) in samples.items():
                    med = statistics.median(burst)
                    cell[name] = {"one_call_per_event_pair": spread(single), "twenty_calls_per_event_pair_per_call": spread(burst),
                                  "bytes_written" if name == "sample_device" else "bytes_read": nbytes, "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3),
                                  "share_of_8_tb_per_s": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}
                row[variant] = cell
            if frames <= 2048:
                row["copy_in_leg_of_mix"] = spread(copy_in_leg(b, frames, max(10, repeats // 2)))
                row["copy_in_over_render_step_4096"] = round(row["copy_in_leg_of_mix"]["median_us"] /
                                                             row[VARIANTS[0]]["sample_device"]["twenty_calls_per_event_pair_per_call"]["median_us"], 2)
            result[f"{n}x{frames}x2"] = row
    result["empty_event_pair"] = spread(timed(stream, lambda: None, 1, repeats))
    return result


def bench_host(steps, warmup):
    n = 4096
    so = lib.load()
    result = {}
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_effect_type(0, desc.EAX_REVERB)
        b.apply_changes()
        b.set_samplers(records(n, VARIANTS[0], s16, None, rng))
        src, buses_all = b.pinned_array(FRAMES), b.pinned_array(FRAMES)
        nrec = (n + 64) * METER_DTYPE.itemsize
        pinned = so.oalsfx_pinned_alloc(nrec)
        assert pinned
        try:
            meters = np.frombuffer((C.c_char * nrec).from_address(pinned), dtype=METER_DTYPE)
            meters[:] = np.zeros(1, METER_DTYPE)
            src[:] = rng.uniform(-1, 1, src.shape).astype(np.float32)
            gain = rng.uniform(0, 1, n).astype(np.float32)
            for n_buses in (1, 64):
                b.set_routing(np.arange(n) % n_buses, gain)
                out = buses_all[:n_buses]
                s, o = src.ctypes.data_as(_fp), out.ctypes.data_as(_fp)
                vm, bm = C.c_void_p(meters.ctypes.data), C.c_void_p(meters.ctypes.data + n * METER_DTYPE.itemsize)
                calls = {"mix_downmix_meter_voices_and_buses_carry": lambda: so.oalsfx_batch_mix_downmix_meter(b._h, FRAMES, s, n_buses, o, 0.001, METER_CARRY, vm, bm),
                         "play_downmix_meter_voices_and_buses_carry": lambda: so.oalsfx_batch_play_downmix_meter(b._h, FRAMES, n_buses, o, 0.001, METER_CARRY, vm, bm),
                         "mix_downmix_meter_voices": lambda: so.oalsfx_batch_mix_downmix_meter(b._h, FRAMES, s, n_buses, o, 0.001, 0, vm, None),
                         "play_downmix_meter_voices": lambda: so.oalsfx_batch_play_downmix_meter(b._h, FRAMES, n_buses, o, 0.001, 0, vm, None)}
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
                row["bytes_copied_in"] = {"mix_downmix_meter": int(src.nbytes), "play_downmix_meter": 0}
                row["play_over_mix"] = round(row["play_downmix_meter_voices_and_buses_carry"]["median_us"] /
                                             row["mix_downmix_meter_voices_and_buses_carry"]["median_us"], 3)
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
        sys.exit("sampler_bench.py measures on the GPU; none is visible")
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
