"""CPU: what the gfx950 code object says about the voice filters' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_biquad_rows<C, V> and k_biquad_upload exist, none keeps anything in
scratch memory, none takes more than 128 VGPRs, a render kernel's LDS is the four wavefronts' C rows of 4 + 64 floats at most, and the
kernels of the other renders are the sets they were."""
import pytest

from test_kernel_resources import kernels
from test_voice_resources import WIDTHS

ROWS = [f"<{c}, {v}>" for c, vs in WIDTHS for v in vs]


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_the_biquad_kernels_are_built_within_their_budget(ks):
    mine = {k: v for k, v in ks.items() if k.startswith("k_biquad_")}
    assert sorted(mine) == sorted([f"k_biquad_rows{w}" for w in ROWS] + ["k_biquad_upload"]), sorted(mine)
    for name, r in mine.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"
        channels = int(name[name.index("<") + 1:name.index(",")]) if "<" in name else 0
        assert r["lds"] <= 4 * channels * 68 * 4, f"{name}: {r['lds']} B of LDS"


def test_the_other_renders_kernels_are_the_sets_they_were(ks):
    for prefix, extra in (("k_sampler_", ["k_sampler_upload"]), ("k_voice_", ["k_voice_upload"]), ("k_fir_", ["k_fir_upload"]), ("k_mix_", [])):
        family = prefix + "rows"
        assert sorted(k for k in ks if k.startswith(prefix)) == sorted([family + w for w in ROWS] + extra), prefix
    for name in ks:
        if name.startswith("k_biquad_"):
            assert "fir" not in name and "voice" not in name
