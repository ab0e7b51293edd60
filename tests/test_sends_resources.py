"""CPU: what the gfx950 code object says about the bus sends' level-1 kernel (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): the three k_downmix_ramp_chunks<V> exist, keep nothing in scratch memory or LDS, and a SIMD
holds no fewer of their wavefronts than of k_downmix_chunks<V> -- the pass is a stream of loads, and what hides their latency is the
wavefronts in flight."""
from test_kernel_resources import kernels


def waves_per_simd(vgprs):
    """gfx950: 512 registers per lane and SIMD, handed out in blocks of 8, at most 8 wavefronts."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_the_ramp_kernels_are_built_and_keep_nothing_in_scratch_or_lds():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_downmix_ramp_chunks<")}
    assert sorted(ks) == [f"k_downmix_ramp_chunks<{v}>" for v in (1, 2, 4)], sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"


def test_a_simd_holds_as_many_wavefronts_as_of_the_plain_kernel():
    ks = kernels()
    for v in (1, 2, 4):
        ramp, plain = ks[f"k_downmix_ramp_chunks<{v}>"], ks[f"k_downmix_chunks<{v}>"]
        print(v, ramp["vgpr"], plain["vgpr"])
        assert waves_per_simd(ramp["vgpr"]) >= waves_per_simd(plain["vgpr"]), f"V = {v}: {ramp['vgpr']} VGPRs against {plain['vgpr']}"
