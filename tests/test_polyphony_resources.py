"""CPU: what the gfx950 code object says about the polyphony kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_mix_rows<C, V> exist, none keeps anything in scratch memory or in LDS,
and none takes more than 128 VGPRs."""
from test_kernel_resources import kernels
from test_voice_resources import WIDTHS


def test_the_mix_kernels_are_built_and_keep_nothing_in_scratch_or_lds():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_mix_")}
    assert sorted(ks) == sorted(f"k_mix_rows<{c}, {v}>" for c, vs in WIDTHS for v in vs), sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"
