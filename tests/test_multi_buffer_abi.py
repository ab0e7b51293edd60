"""CPU: the multi-buffer entry points (oalsfx_batch_mix_device_multi, oalsfx_group_mix_device_multi, oalsfx_batch_multi_counts) --
the kernels they launch as the gfx950 code object describes them, and the argument errors that need no device."""
import ctypes as C

from oalsfxpp_amd import lib
from test_kernel_resources import kernels


def test_the_multi_buffer_kernels_fit_four_workgroups_per_cu():
    """k_reverb_steady_multi<channels, CR>: the FP builds with the buffer table, held to what the grid of kinds is held to (four 256-thread
    workgroups per CU: at most 128 VGPRs and 40 960 B of LDS) and without scratch, like every proven build."""
    multi = {k: v for k, v in kernels().items() if k.startswith("k_reverb_steady_multi<")}
    assert sorted(multi) == ["k_reverb_steady_multi<1, 0>", "k_reverb_steady_multi<1, 2>", "k_reverb_steady_multi<2, 0>", "k_reverb_steady_multi<2, 2>"], sorted(multi)
    for name, r in multi.items():
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs"
        assert r["lds"] <= 40960, f"{name}: {r['lds']} B of LDS"
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"


def test_null_batch_and_group_fail_with_a_message():
    so = lib.load()
    src = (C.c_void_p * 2)()
    dst = (C.c_void_p * 2)()
    assert so.oalsfx_batch_mix_device_multi(None, 256, 2, src, dst, None) == 0
    assert so.oalsfx_last_error() == b"Null batch."
    assert so.oalsfx_batch_multi_counts(None, None, None) == 0
    assert so.oalsfx_group_mix_device_multi(None, 256, 2, src, dst) == 0
    assert so.oalsfx_group_last_error() == b"Null group."
