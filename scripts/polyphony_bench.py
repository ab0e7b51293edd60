"""Polyphony (oalsfx_batch_set_polyphony): what one pass over K voices per instance costs beside the only way to get K voices without
it: K renders of one voice per instance into K buffers, which does not even sum them.

    python scripts/polyphony_bench.py [--pairs 5] [--repeats 6] [--per 10] [--yardstick-lib path/to/liboalsfx_hip.so] [--json out.json]

Shape: 4096 instances x 256 frames x stereo, mono 16-bit assets, looped, LINEAR set, steps near 1.0 (4096 +- 64).  Every run is
sample_device alone on one stream between two HIP events, `per` calls (or `per` rounds of K calls) per event pair divided by `per`.

  one pass    this library, a batch of polyphony K: one k_mix_rows launch renders and sums the K voices of every instance.
  K launches  K batches of polyphony 1 of the yardstick library, batch k holding the voices of lane k, rendered one after the other
              into K buffers: K launches of k_fir_rows (T = 8) or k_sampler_rows (plain).  The yardstick library is --yardstick-lib, a
              build of the commit in front of polyphony, loaded beside this one; without it, this library, whose batches of one lane
              launch what that commit launched.

Cases: K = 2, 4, 8 and 16 with every lane playing, plain (no table) and through an 8-tap table of 12 phase bits on every voice; and
K = 8 with one lane in eight playing (lane k of instance i plays where k == i mod 8), plain and tabled, beside the K = 8 launches of
the same voices (seven of which render silence).  The two sides of a case are taken in turn `pairs` times in one process, so that a
drift of the box hits both alike; per pair the ratio of the medians, and over the pairs the ratios' median, minimum and maximum.

Run it as one step under a time limit:

    timeout -k 10 600 python scripts/polyphony_bench.py --json polyphony.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oalsfxpp_amd import desc, lib  # noqa: E402
from oalsfxpp_amd.api import SAMPLER_DTYPE, Batch, fir_sinc  # noqa: E402

N, FRAMES = 4096, 256
ONE = 1 << desc.SAMPLER_FRAC_BITS
ASSETS, ASSET_FRAMES = 256, 48000       # a pool's worth: a few hundred one-second sounds


class PlainBatches:
    """K batches of one lane each on a library given by path, through the calls every build has (raw ctypes: two builds cannot share
    the Python mirror's single handle)."""

    def __init__(self, path, lanes):
        so = self.so = C.CDLL(path)
        for name in ("oalsfx_batch_create", "oalsfx_batch_destroy", "oalsfx_batch_error", "oalsfx_batch_set_fir_table", "oalsfx_batch_set_samplers",
                     "oalsfx_batch_set_resamplers", "oalsfx_batch_sample_device", "oalsfx_batch_synchronize", "oalsfx_debug_last_render_kernel"):
            getattr(so, name).restype, getattr(so, name).argtypes = lib.SIGNATURES[name]
        self.handles = [C.c_void_p(so.oalsfx_batch_create(N, desc.FMT_STEREO, 48000, 1, 0)) for _ in range(lanes)]
        assert all(h.value for h in self.handles)
        self.dst = [torch.empty((N, FRAMES, 2), dtype=torch.float32, device="cuda") for _ in range(lanes)]

    def check(self, ok, h):
        assert ok, self.so.oalsfx_batch_error(h).decode()

    def set(self, records, table):
        """records [lanes][N]; table: None, or the coefficients every voice goes through."""
        for h, r in zip(self.handles, records):
            r = np.ascontiguousarray(r)
            self.check(self.so.oalsfx_batch_set_samplers(h, None, N, C.c_void_p(r.ctypes.data)), h)
            if table is not None:
                self.check(self.so.oalsfx_batch_set_fir_table(h, 0, table.shape[1], table.shape[0].bit_length() - 1, C.c_void_p(table.ctypes.data)), h)
                self.check(self.so.oalsfx_batch_set_resamplers(h, None, N, (C.c_int * N)()), h)

    def render(self, stream):
        for h, dst in zip(self.handles, self.dst):
            self.check(self.so.oalsfx_batch_sample_device(h, FRAMES, C.c_void_p(dst.data_ptr()), C.c_void_p(stream.cuda_stream)), h)

    def kernel(self):
        return {(self.so.oalsfx_debug_last_render_kernel(h) or b"").decode() for h in self.handles}

    def close(self):
        for h in self.handles:
            self.so.oalsfx_batch_synchronize(h)
            self.so.oalsfx_batch_destroy(h)


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


def voices(lanes, s16, rng, sparse):
    """records [lanes][N]: looping, LINEAR voices at steps within 64 of 1.0 over the assets; sparse: lane k of instance i plays where
    k == i mod lanes, the others are in the state after creation but for a channel count the setters take."""
    r = np.zeros((lanes, N), SAMPLER_DTYPE)
    r["frames"], r["loop_start"], r["loop_end"] = ASSET_FRAMES, 0, ASSET_FRAMES
    r["position"] = rng.integers(0, ASSET_FRAMES * ONE, (lanes, N))
    r["step"] = rng.integers(ONE - 64, ONE + 65, (lanes, N))
    r["flags"] = desc.SAMPLER_PLAYING | desc.SAMPLER_LOOP | desc.SAMPLER_LINEAR
    r["gain"][:, :, :2] = rng.uniform(0.2, 1.0, (lanes, N, 2))
    r["format"], r["channels"] = desc.PCM_S16, 1
    r["data"] = s16.data_ptr() + rng.integers(0, ASSETS, (lanes, N)) * (ASSET_FRAMES * 2)
    if sparse:
        idle = np.arange(lanes)[:, None] != np.arange(N)[None, :] % lanes
        r[idle] = np.zeros(1, SAMPLER_DTYPE)
        r["channels"][idle] = 1
    return r


def bench_case(stream, yardstick, lanes, tabled, sparse, s16, rng, pairs, repeats, per):
    records = voices(lanes, s16, rng, sparse)
    table = fir_sinc(8, 12, 0.9) if tabled else None
    plain = PlainBatches(yardstick, lanes)
    try:
        with Batch(N, desc.FMT_STEREO, 48000, 1) as b:
            b.set_polyphony(lanes)
            if tabled:
                b.set_fir_table(0, table)
            for k in range(lanes):
                b.set_samplers(records[k], lane=k)
                if tabled:
                    b.set_resamplers(np.zeros(N, np.int64), lane=k)
            plain.set(records, table)
            dst = torch.empty((N, FRAMES, 2), dtype=torch.float32, device="cuda")
            one_pass = lambda: b.sample_device(FRAMES, dst.data_ptr(), stream=stream.cuda_stream)
            launches = lambda: plain.render(stream)
            for _ in range(3):
                one_pass()
                launches()
            stream.synchronize()
            assert b.last_render_kernel() == "k_mix_rows" and plain.kernel() == {"k_fir_rows" if tabled else "k_sampler_rows"}, (b.last_render_kernel(), plain.kernel())
            ours, theirs, ratios = [], [], []
            for _ in range(pairs):
                a, t = timed(stream, one_pass, per, repeats), timed(stream, launches, per, repeats)
                ours.extend(a)
                theirs.extend(t)
                ratios.append(statistics.median(a) / statistics.median(t))
            b.synchronize()
    finally:
        plain.close()
    return {"lanes": lanes, "table": "T8_bits12" if tabled else "none", "playing": "one lane in %d" % lanes if sparse else "every lane",
            "one_pass_us": {"median": round(statistics.median(ours), 2), "min": round(min(ours), 2), "max": round(max(ours), 2)},
            "k_launches_us": {"median": round(statistics.median(theirs), 2), "min": round(min(theirs), 2), "max": round(max(theirs), 2)},
            "one_pass_over_k_launches": {"median": round(statistics.median(ratios), 3), "min": round(min(ratios), 3), "max": round(max(ratios), 3), "pairs": pairs}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="alternated pairs per case (at least five)")
    ap.add_argument("--repeats", type=int, default=6, help="event pairs per side per pair")
    ap.add_argument("--per", type=int, default=10, help="calls (rounds of K calls) per event pair")
    ap.add_argument("--yardstick-lib", default=lib.LIB_PATH, help="the library whose one-lane batches are the K launches")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("polyphony_bench.py measures on the GPU; none is visible")
    if args.pairs < 5:
        sys.exit("at least five alternated pairs")
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    s16 = torch.randint(-32768, 32767, (ASSETS, ASSET_FRAMES), dtype=torch.int16, device="cuda")
    yardstick = os.path.abspath(args.yardstick_lib)
    cases = [(lanes, tabled, False) for tabled in (False, True) for lanes in (2, 4, 8, 16)] + [(8, False, True), (8, True, True)]
    rows = [bench_case(stream, yardstick, lanes, tabled, sparse, s16, rng, args.pairs, args.repeats, args.per) for lanes, tabled, sparse in cases]
    dense = {(r["lanes"], r["table"]): r for r in rows if r["playing"] == "every lane"}
    for r in rows:
        if r["playing"] != "every lane":
            r["sparse_over_dense_one_pass"] = round(r["one_pass_us"]["median"] / dense[(r["lanes"], r["table"])]["one_pass_us"]["median"], 3)
    result = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{FRAMES}x2", "yardstick_lib": os.path.relpath(yardstick, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
              "empty_event_pair_us": round(statistics.median(timed(stream, lambda: None, 1, 30)), 2), "cases": rows}
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
