"""CPU: what the gfx950 code object says about the sampler streams' kernels (the metadata notes of the built library, as
tests/test_kernel_resources.py reads them): exactly the 25 k_stream_* kernels exist -- the twelve k_stream_rows<C, V>, the twelve k_stream_filter_rows<C, V> and
k_stream_upload --, none keeps anything in scratch memory, none takes more than 128 VGPRs but k_stream_rows at seven channels (DESIGN.md
4o: 130, in the allocation unit of 8 that is 136 and three wavefronts per SIMD where the others have four; it is held to that),
k_stream_rows has no LDS (the records between spans are carried in registers) and k_stream_filter_rows k_filter_program_env_rows' at
most, C + 2 rows per wavefront, and no name says
`fir`, `voice`, `mix`, `sampler`, `program`, `sweep` or `biquad`: the sets the other renders' tests pin stay what they were."""
import pytest

from test_kernel_resources import kernels
from test_voice_resources import WIDTHS

ROWS = [f"<{c}, {v}>" for c, vs in WIDTHS for v in vs]
OVER = {"k_stream_rows<7, 1>": 136}     # the widths that do not fit 128 VGPRs without scratch, and what they are held to instead


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_the_stream_kernels_are_built_within_their_budget(ks):
    # (k_stream_pattern<N> is the bandwidth probe of support_kernels.hip, older than the streams and no render)
    mine = {k: v for k, v in ks.items() if k.startswith("k_stream_") and not k.startswith("k_stream_pattern<")}
    assert len(ROWS) == 12
    assert sorted(mine) == sorted([f"k_stream_rows{w}" for w in ROWS] + [f"k_stream_filter_rows{w}" for w in ROWS] + ["k_stream_upload"]), sorted(mine)
    assert len(mine) == 25
    for name, r in mine.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["vgpr"] <= OVER.get(name, 128), f"{name}: {r['vgpr']} VGPRs"
        channels = int(name[name.index("<") + 1:name.index(",")]) if "<" in name else 0
        bound = 4 * (channels + 2) * 68 * 4 if name.startswith("k_stream_filter_rows") else 0
        assert r["lds"] <= bound, f"{name}: {r['lds']} B of LDS"
        for word in ("fir", "voice", "mix", "sampler", "program", "sweep", "biquad", "meter", "downmix"):
            assert word not in name, name


def test_the_other_renders_kernels_are_the_sets_they_were(ks):
    for prefix, extra in (("k_sampler_", ["k_sampler_upload"]), ("k_voice_", ["k_voice_upload"]), ("k_fir_", ["k_fir_upload"]), ("k_mix_", []),
                          ("k_biquad_", ["k_biquad_upload"])):
        family = prefix + "rows"
        assert sorted(k for k in ks if k.startswith(prefix)) == sorted([family + w for w in ROWS] + extra), prefix
