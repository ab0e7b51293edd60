"""CPU: what the gfx950 code object says about the filter programs' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the twelve k_filter_program_rows<C, V>, the twelve k_filter_program_env_rows<C, V>
and k_filter_program_upload exist, none keeps anything in scratch memory, none takes more than 128 VGPRs, and a render kernel's LDS is the
four wavefronts' C + 2 rows of 4 + 64 floats at most.  (That the code of the kernels which share the row body is the parent commit's is a
comparison of two commits' compiler output, minutes of compiling and the parent's sources: scripts/row_kernels_asm_diff.py --sources
biquad sweep support_kernels program polyphony, whose table for this change is committed in profiles/filter_programs/README.md -- every
kernel `identical`.)"""
import pytest

from test_kernel_resources import kernels
from test_voice_resources import WIDTHS

ROWS = [f"<{c}, {v}>" for c, vs in WIDTHS for v in vs]


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_the_filter_program_kernels_are_built_within_their_budget(ks):
    mine = {k: v for k, v in ks.items() if k.startswith("k_filter_program_")}
    assert len(ROWS) == 12
    assert sorted(mine) == sorted([f"k_filter_program_rows{w}" for w in ROWS] + [f"k_filter_program_env_rows{w}" for w in ROWS] + ["k_filter_program_upload"]), sorted(mine)
    for name, r in mine.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"
        channels = int(name[name.index("<") + 1:name.index(",")]) if "<" in name else 0
        bound = 4 * (channels + 2) * 68 * 4 if "<" in name else 0
        assert r["lds"] <= bound, f"{name}: {r['lds']} B of LDS"
        assert "fir" not in name, name


def test_no_other_kernel_carries_the_name(ks):
    assert not [k for k in ks if "filter_program" in k and not k.startswith("k_filter_program_")]
