"""CPU: what the gfx950 code object says about the kernels of calls that join a queued launch (the metadata notes of the built library,
as tests/test_kernel_resources.py reads them).  The four k_reverb_steady_joined<channels, CR> exist, keep nothing in scratch, take at most
128 VGPRs and at most 40 960 B of LDS -- four workgroups per CU, as the launches they take turns with.  The gate in front of them stays
one small wavefront: beside four workgroups of 120 registers a SIMD has 32 left (512 - 4 x 120), and a gate that needed more would find
no place until a workgroup leaves (profiles/r04n_places_and_the_gate/)."""
from test_kernel_resources import kernels


def test_the_joined_builds_fit_four_workgroups_per_cu():
    ks = {k: v for k, v in kernels().items() if k.startswith("k_reverb_steady_joined")}
    assert sorted(ks) == sorted(f"k_reverb_steady_joined<{c}, {cr}>" for c in (1, 2) for cr in (0, 2)), sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch per lane"
        assert r["vgpr"] <= 128, f"{name}: {r['vgpr']} VGPRs: fewer than four wavefronts per SIMD"
        assert r["lds"] <= 40960, f"{name}: {r['lds']} B of LDS: fewer than four workgroups per CU"


def test_the_gate_stays_small():
    r = kernels()["k_chain_gate"]
    print("k_chain_gate", r)
    assert r["scratch"] == 0 and r["lds"] == 0, r
    assert r["vgpr"] <= 32, f"k_chain_gate: {r['vgpr']} VGPRs: no place beside four 120-register workgroups"
