"""CPU: what the gfx950 code object says about the resamplers' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_fir_rows<C, V> and k_fir_upload exist, none keeps anything in scratch
memory or in LDS, none takes more than 128 VGPRs, and the samplers' and the envelopes' thirteen kernels each are still theirs alone."""
from test_kernel_resources import kernels
from test_voice_resources import WIDTHS


def test_the_fir_kernels_are_built_and_keep_nothing_in_scratch_or_lds():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_fir_")}
    assert sorted(ks) == sorted([f"k_fir_rows<{c}, {v}>" for c, vs in WIDTHS for v in vs] + ["k_fir_upload"]), sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["lds"] == 0, f"{name}: {r['lds']} B of LDS"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"


def test_the_samplers_and_the_voices_kernels_are_unchanged():
    names = sorted(kernels())
    want = [f"rows<{c}, {v}>" for c, vs in WIDTHS for v in vs] + ["upload"]
    for prefix in ("k_sampler_", "k_voice_"):
        assert sorted(k for k in names if k.startswith(prefix)) == sorted(prefix + w for w in want), prefix
    assert not [k for k in names if "fir" in k and not k.startswith("k_fir_")]
