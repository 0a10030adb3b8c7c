"""Build-time resources of the audio codec's kernels (audiosdr_amd/csrc/asdr_codec.hip): the set of kernels, no scratch, no spills, at
most 128 VGPRs and at most 64 KiB of LDS per workgroup.  The G.711 pass uses no LDS at all (its exponent is a find-first-bit, not a
table); the ADPCM pass holds the step table, the 64 rows' input rows and one staged chunk of 64 rows x 33 words in static LDS."""
from test_build_properties import _resources

# kernel (a substring of the mangled name) -> static LDS bytes per workgroup, as built
LDS = {"asdr_codec_g711_kernelILi1E": 0,
       "asdr_codec_g711_kernelILi2E": 0,
       "asdr_codec_adpcm_kernel": 4 * (96 + 64 + 64 * 33)}


def test_codec_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_codec.hip" in b.SOURCES and "asdr_codec_host.cpp" in b.SOURCES
    assert "asdr_codec.hip" in b.DEPS and "asdr_codec_host.cpp" in b.DEPS and "asdr_codec_device.h" in b.DEPS
    assert any(d.endswith("asdr_codec.h") for d in b.DEPS)
    assert A.AudioCodec is not None


def test_codec_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_codec.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS), sorted(res)                  # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds <= 65536, (k, r)
