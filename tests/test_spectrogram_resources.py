"""Build-time resources of the audio spectrogram's kernels (audiosdr_amd/csrc/asdr_spectrogram.hip): the set of kernels, no scratch, no
spills, at most 128 VGPRs and at most 64 KiB of LDS per workgroup.  The small mapping (one wave per transform, N <= 1024) holds four
transforms of 512 complex points, the large one (a workgroup per transform) one of 4096; the carry kernel uses no LDS."""
from test_build_properties import _resources

# kernel (a substring of the mangled name) -> static LDS bytes per workgroup, as built
LDS = {"asdr_spectrogram_kernelILi64E": 4 * 512 * 8,
       "asdr_spectrogram_kernelILi256E": 4096 * 8,
       "asdr_spectrogram_carry_kernel": 0}


def test_spectrogram_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_spectrogram.hip" in b.SOURCES and "asdr_spectrogram_host.cpp" in b.SOURCES
    assert "asdr_spectrogram.hip" in b.DEPS and "asdr_spectrogram_host.cpp" in b.DEPS and "asdr_spectrogram_device.h" in b.DEPS
    assert any(d.endswith("asdr_spectrogram.h") for d in b.DEPS)
    assert A.AudioSpectrogram is not None


def test_spectrogram_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_spectrogram.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS), sorted(res)                  # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds <= 65536, (k, r)
