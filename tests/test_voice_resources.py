"""CPU: what the gfx950 code object says about the voice envelopes' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_voice_rows<C, V> and k_voice_upload exist, none keeps anything in scratch
memory or in LDS, and the samplers' thirteen kernels are still the samplers' alone."""
from test_kernel_resources import kernels

WIDTHS = ((1, (1,)), (2, (1, 2)), (4, (1, 2, 4)), (6, (1, 2)), (7, (1,)), (8, (1, 2, 4)))


def test_the_voice_kernels_are_built_and_keep_nothing_in_scratch_or_lds():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_voice_")}
    # channels x floats per store as for the samplers, and the kernel that puts set envelopes in place
    assert sorted(ks) == sorted([f"k_voice_rows<{c}, {v}>" for c, vs in WIDTHS for v in vs] + ["k_voice_upload"]), sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"


def test_the_samplers_kernels_are_the_samplers_alone():
    names = [k for k in kernels() if k.startswith("k_sampler_")]
    assert len(names) == 13 and not [k for k in names if "voice" in k]
