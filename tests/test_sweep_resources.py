"""CPU: what the gfx950 code object says about the voice filter sweeps' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_sweep_rows<C, V>, the twelve k_sweep_program_rows<C, V> and
k_sweep_upload exist, none keeps anything in scratch memory, none takes more than 128 VGPRs, a render kernel's LDS is the four
wavefronts' C + 2 rows of 4 + 64 floats at most, no name says `fir`, and the kernels of the other renders are the sets they were.
(That the code of the kernels which share the moved filter stage and filter_recurrence.hpp is the parent commit's is a comparison of two
commits' compiler output, minutes of compiling and the parent's sources: scripts/row_kernels_asm_diff.py --sources biquad support_kernels
program polyphony, whose table for this change is committed in profiles/sweeps/README.md -- every kernel `identical`.)"""
import pytest

from test_kernel_resources import kernels
from test_voice_resources import WIDTHS

ROWS = [f"<{c}, {v}>" for c, vs in WIDTHS for v in vs]


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_the_sweep_kernels_are_built_within_their_budget(ks):
    mine = {k: v for k, v in ks.items() if k.startswith("k_sweep_")}
    assert len(ROWS) == 12
    assert sorted(mine) == sorted([f"k_sweep_rows{w}" for w in ROWS] + [f"k_sweep_program_rows{w}" for w in ROWS] + ["k_sweep_upload"]), sorted(mine)
    for name, r in mine.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"
        channels = int(name[name.index("<") + 1:name.index(",")]) if "<" in name else 0
        bound = 4 * (channels + 2) * 68 * 4 if "<" in name else 0
        assert r["lds"] <= bound, f"{name}: {r['lds']} B of LDS"
        for word in ("fir", "voice", "mix", "sampler", "meter", "downmix", "biquad"):
            assert word not in name, name


def test_the_other_renders_kernels_are_the_sets_they_were(ks):
    for prefix, extra in (("k_sampler_", ["k_sampler_upload"]), ("k_voice_", ["k_voice_upload"]), ("k_fir_", ["k_fir_upload"]), ("k_mix_", []),
                          ("k_biquad_", ["k_biquad_upload"])):
        family = prefix + "rows"
        assert sorted(k for k in ks if k.startswith(prefix)) == sorted([family + w for w in ROWS] + extra), prefix
    assert sorted(k for k in ks if k.startswith("k_program_")) == sorted([f"k_program_rows{w}" for w in ROWS] + [f"k_program_biquad_rows{w}" for w in ROWS] + ["k_program_upload"])
