"""A child process for tests/test_gpu_sends.py::test_the_kernels_a_downmix_launches, run under a kernel trace: downmix calls of a small
batch in four stretches, so that the trace's downmix kernels in launch order can be held against EXPECTED.

    send 0 only, 2 calls                                           the plain pair
    all four sends routed, no ramp, 2 calls                        the plain pair
    a ramp of 100 frames on one routed send, 4 calls of 64 frames  the ramp kernel while it runs (2 calls), then the plain pair again
    a ramp on a send routed nowhere, 2 calls                       the plain pair: such a ramp runs on the clock alone"""
import os
import sys

PLAIN, RAMP = ["k_downmix_chunks<4>", "k_downmix_sums<4>"], ["k_downmix_ramp_chunks<4>", "k_downmix_sums<4>"]
EXPECTED = PLAIN * 2 + PLAIN * 2 + RAMP * 2 + PLAIN * 2 + PLAIN * 2


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    from oalsfxpp_amd import desc
    from oalsfxpp_amd.api import Batch

    n, frames, n_buses = 100, 64, 2   # 50 members and more per bus: several chunks, so level 2 is launched too
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((n, frames, 2)).astype(np.float32)).cuda()
    out = torch.empty((n_buses, frames, 2), dtype=torch.float32, device="cuda")
    gain = np.linspace(0, 1, n).astype(np.float32)

    def calls(count):
        for _ in range(count):
            b.downmix_device(frames, x.data_ptr(), n_buses, out.data_ptr())
        b.synchronize()

    with Batch(n, desc.FMT_STEREO, 48000, 1) as b:
        b.set_routing(np.arange(n) % n_buses, gain)
        calls(2)
        for send in (1, 2, 3):
            b.set_routing((np.arange(n) + send) % n_buses, gain, send=send)
        calls(2)
        b.set_send_ramps([0.5], 100, first=3, send=2)
        calls(4)
        assert b.get_send(3, 2)[2:] == (0.5, 0)
        b.set_routing([-1], None, first=5, send=3)
        calls(1)
        b.set_send_ramps([0.25], 1000, first=5, send=3)
        calls(1)
        assert b.get_send(5, 3)[3] == 1000 - frames
    print("ok", float(out.abs().max()))


if __name__ == "__main__":
    main()
