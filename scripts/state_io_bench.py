"""Snapshot and restore of 4096 EAX reverbs (stereo, 48 kHz): time per direction, against reading every delay line back with read_ring;
and what a restored batch needs to get back to the proven-steady builds, to multi-buffer passes and to the source's step time.

    python scripts/state_io_bench.py [--instances 4096] [--repeats 10] [--json out.json]

Snapshot and restore are timed with HIP events recorded on the batch's own stream around the call (the stream handle is asked for, so
that batch runs in stream order).  The window holds the whole call: for a snapshot the copy of the call's tables and host records
to the device and the copy kernel; for a restore also the wait for the batch's stream, the read of the blob's records to the host, the
host's bookkeeping and the parameter upload before its copy.  The copy kernel's own time: run the script under
`rocprofv3 --kernel-trace --stats` (k_state_copy).  Bytes moved per direction: the blob, read once and written once.  read_ring is timed
with the host clock (it is synchronous, one hipMemcpy per slab).

After a restore: the calls until every instance is listed as proven steady again (plan(0)[1] == n, the FP builds; one synchronise per
call), the calls until mix_device_multi (8 buffers of 256 frames) takes a multi-buffer pass, and the step time of chained 256-frame calls
in windows of 16 (host clock, one synchronise per window) against the source batch timed the same way right before, and over 200 calls
with one synchronise, as bench.py times its headline."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc  # noqa: E402
from oalsfxpp_amd.api import Batch  # noqa: E402

FRAMES = 256


def make(n):
    b = Batch(n, desc.FMT_STEREO, 48000, 1)
    b.set_effect_type(0, desc.EAX_REVERB)
    b.apply_changes()
    return b


def step_times(b, src, dst, windows, per=16):
    out = []
    for _ in range(windows):
        b.synchronize()
        t0 = time.perf_counter()
        for _ in range(per):
            b.mix_device(FRAMES, src.data_ptr(), dst.data_ptr())
        b.synchronize()
        out.append((time.perf_counter() - t0) / per * 1e6)
    return out


def restored(n, blob, nbytes, src, dst):
    b = make(n)
    step_times(b, src, dst, 1, 4)
    b.restore(None, blob.data_ptr(), nbytes)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    n = args.instances
    src = torch.empty(n * FRAMES * 2, device="cuda").uniform_(-1, 1)
    dst = torch.empty_like(src)

    a = make(n)
    step_times(a, src, dst, 40)   # proven steady, chained
    nbytes = a.snapshot_bytes()
    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a.snapshot(None, blob.data_ptr(), nbytes)
    a.synchronize()
    ring_floats = a.read_ring(0, 0).size
    moved = nbytes   # read once and written once per direction

    # snapshot / restore on a batch whose stream is handed out (stream order, events on that stream)
    t = make(n)
    step_times(t, src, dst, 2)
    stream = torch.cuda.ExternalStream(t.stream)
    snap_ms, rest_ms = [], []
    for r in range(args.repeats + 2):
        for which, out in (("snapshot", snap_ms), ("restore", rest_ms)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if which == "snapshot":
                t.snapshot(None, blob.data_ptr(), nbytes)
            else:
                t.restore(None, blob.data_ptr(), nbytes)
            e1.record(stream)
            t.synchronize()
            if r >= 2:
                out.append(e0.elapsed_time(e1))
    t.close()

    # today's alternative: read_ring per slab (host clock)
    ring = np.empty(ring_floats, dtype=np.float32)
    t0 = time.perf_counter()
    k = min(n, 512)
    for i in range(k):
        a._lib.oalsfx_batch_read_ring(a._h, i, 0, ring.ctypes.data_as(np.ctypeslib.ctypes.POINTER(np.ctypeslib.ctypes.c_float)), ring_floats)
    read_ring_ms = (time.perf_counter() - t0) * 1e3 * n / k

    # a restored batch: back to the proven-steady builds (plan), to multi-buffer passes, to the source's step time
    b = restored(n, blob, nbytes, src, dst)
    calls_to_fp = None
    for k in range(1, 65):
        b.mix_device(FRAMES, src.data_ptr(), dst.data_ptr())
        b.synchronize()
        if b.plan(0)[1] == n:
            calls_to_fp = k
            break
    b.close()
    bufs = [torch.empty_like(src) for _ in range(16)]
    b = restored(n, blob, nbytes, src, dst)
    calls_to_multi = None
    for r in range(1, 17):
        before = b.multi_counts()[1]
        b.mix_device_multi(FRAMES, [src.data_ptr()] * 8, [d.data_ptr() for d in bufs[:8]])
        b.synchronize()
        if b.multi_counts()[1] > before:
            calls_to_multi = (r - 1) * 8   # the calls before the first pass
            break
    b.close()
    steady = step_times(a, src, dst, 8)
    b = restored(n, blob, nbytes, src, dst)
    after = step_times(b, src, dst, 8)
    target = statistics.median(steady) * 1.03
    back = next(((w + 1) * 16 for w, us in enumerate(after) if us <= target), None)

    def long_run(x):
        x.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            x.mix_device(FRAMES, src.data_ptr(), dst.data_ptr())
        x.synchronize()
        return (time.perf_counter() - t0) / 200 * 1e6
    long_source, long_restored = long_run(a), long_run(b)

    med = lambda v: statistics.median(v)
    rec = {
        "instances": n, "blob_bytes": nbytes, "ring_floats_per_instance": ring_floats,
        "snapshot_ms": med(snap_ms), "restore_ms": med(rest_ms),
        "snapshot_tbps_read_plus_write": 2 * moved / (med(snap_ms) * 1e-3) / 1e12,
        "restore_tbps_read_plus_write": 2 * moved / (med(rest_ms) * 1e-3) / 1e12,
        "snapshot_ms_all": snap_ms, "restore_ms_all": rest_ms,
        "read_ring_all_instances_ms": read_ring_ms,
        "calls_to_proven_steady": calls_to_fp, "calls_before_first_multi_buffer_pass": calls_to_multi,
        "source_us_per_call_by_window_of_16": steady, "restored_us_per_call_by_window_of_16": after,
        "calls_back_within_3pct_of_source": back,
        "us_per_call_200_calls_source": long_source, "us_per_call_200_calls_restored_after_the_windows": long_restored,
    }
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)
    a.close(); b.close()


if __name__ == "__main__":
    main()
