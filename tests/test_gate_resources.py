"""Build-time resources of the audio gate's kernels (audiosdr_amd/csrc/asdr_gate.hip): the set of kernels, no scratch, no spills, at
most 128 VGPRs, and LDS only where the scan uses it -- the per-wave counts of a tile (16 bytes) and of the index step (32 bytes)."""
from test_build_properties import _resources

# kernel (a substring of the mangled name) -> LDS bytes per workgroup, as built
LDS = {"asdr_gate_energy_kernelILb0EE": 0,    # energy to the scratch
       "asdr_gate_energy_kernelILb1EE": 16,   # one-block form: energy + fold; the tile's four wave counts
       "asdr_gate_fold_kernel": 16,
       "asdr_gate_index_kernel": 32,
       "asdr_gate_packet_kernel": 0}


def test_gate_sources_are_in_the_build():
    from audiosdr_amd import build as b
    assert "asdr_gate.hip" in b.SOURCES and "asdr_gate_host.cpp" in b.SOURCES
    assert "asdr_gate.hip" in b.DEPS and "asdr_gate_device.h" in b.DEPS and any(d.endswith("asdr_gate.h") for d in b.DEPS)


def test_gate_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_gate.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS), sorted(res)                  # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds, (k, r)
