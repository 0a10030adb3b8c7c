"""Build-time resources of the CW decoder's kernels (audiosdr_amd/csrc/asdr_cw.hip): the set of kernels (the pass in two
instantiations, of 64 and of 16 channels per workgroup, the collect's count, index and copy passes, and clear's), no scratch, no
spills, at most 128 VGPRs.  An instantiation of the pass holds the mixer's table (1,024 words) and, per row, its phase and step and
two blocks' four (aI, aQ) pairs in static LDS: 4,096 + 72 bytes a row, 8,704 and 5,248 bytes."""
import os
import re

from test_build_properties import _resources

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# template argument as the mangled name spells it -> static LDS bytes per workgroup, as built
LDS = {"Li64E": 4096 + 64 * (4 + 4 + 2 * 4 * 8), "Li16E": 4096 + 16 * (4 + 4 + 2 * 4 * 8)}
COLLECT = {"asdr_cw_count_kernel": 16, "asdr_cw_index_kernel": 32, "asdr_cw_copy_kernel": 0, "asdr_cw_clear_kernel": 0}


def test_cw_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_cw.hip" in b.SOURCES and "asdr_cw_host.cpp" in b.SOURCES
    assert "asdr_cw.hip" in b.DEPS and "asdr_cw_host.cpp" in b.DEPS and "asdr_cw_device.h" in b.DEPS
    assert any(d.endswith("asdr_cw.h") for d in b.DEPS)
    assert A.CwDecoder is not None and (A.CW_ROWS, A.CW_NARROW_ROWS, A.CW_WIDE_CHANNELS, A.CW_MAX_RING) == (64, 16, 32768, 64)
    with open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_cw_device.h")) as f:
        text = f.read()
    for name, value in (("ROWS", 64), ("NARROW_ROWS", 16), ("WIDE_CHANNELS", 32768), ("THREADS", 256), ("TABLE_WORDS", 1024),
                        ("LOADED_BYTES", 64), ("TILE", 256)):
        assert re.search(r"#define ASDR_CW_%s %d\b" % (name, value), text), name


def test_cw_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_cw.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS) + len(COLLECT), sorted(res)                                     # the set of kernels is pinned
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
    for k, lds in LDS.items():
        names = [n for n in res if k in n and "asdr_cw_kernel" in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds <= 65536, (k, r)
    for k, lds in COLLECT.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert 0 < r.get("VGPRs", 0) <= 32 and r.get("LDS Size [bytes/block]", -1) == lds, (k, r)


def test_design_states_the_lds_figures():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text[text.index("### 3.20"):]
    section = section[:re.search(r"\n#{2,3} ", section[4:]).start() + 4]
    assert "8,704" in section and "5,248" in section and sorted(LDS.values()) == [5248, 8704]
