"""Build-time resources of the audio resampler's kernels (audiosdr_amd/csrc/asdr_resample.hip): the set of kernels, no scratch, no
spills, at most 128 VGPRs, and no static LDS -- the 64 rows' windows live in dynamic LDS sized per launch (64 * row_words * 4 bytes,
at most 64 KiB: asdr_resample_host.cpp sizes the tile to that and refuses a geometry past it)."""
from test_build_properties import _resources

# kernel (a substring of the mangled name) -> static LDS bytes per workgroup, as built
LDS = {"asdr_resample_kernel": 0,
       "asdr_resample_carry_kernel": 0}


def test_resample_sources_are_in_the_build():
    from audiosdr_amd import build as b
    assert "asdr_resample.hip" in b.SOURCES and "asdr_resample_host.cpp" in b.SOURCES
    assert "asdr_resample.hip" in b.DEPS and "asdr_resample_host.cpp" in b.DEPS and "asdr_resample_device.h" in b.DEPS
    assert any(d.endswith("asdr_resample.h") for d in b.DEPS)


def test_resample_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_resample.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS), sorted(res)                  # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds, (k, r)
