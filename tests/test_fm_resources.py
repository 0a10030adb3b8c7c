"""Build-time resources of the FM demodulator's kernel (audiosdr_amd/csrc/asdr_fm.hip): the set of kernels, no scratch, no spills, at
most 128 VGPRs and at most 64 KiB of LDS per workgroup.  The kernel holds a staged block of its rows x 65 words, the rows' N and P
sums, their two carry words and their gains in static LDS: 288 bytes per row, 18,432 bytes in the 64-row instantiation and 4,608 in
the 16-row one."""
import os
import re

from test_build_properties import _resources

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# kernel (a substring of the mangled name) -> static LDS bytes per workgroup, as built
LDS = {"asdr_fm_kernelILi%dEE" % rows: rows * (4 * 65 + 2 * 8 + 3 * 4) for rows in (64, 16)}


def test_fm_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_fm.hip" in b.SOURCES and "asdr_fm_host.cpp" in b.SOURCES
    assert "asdr_fm.hip" in b.DEPS and "asdr_fm_host.cpp" in b.DEPS and "asdr_fm_device.h" in b.DEPS
    assert any(d.endswith("asdr_fm.h") for d in b.DEPS)
    assert A.FmDemodulator is not None and (A.FM_ROWS, A.FM_NARROW_ROWS, A.FM_WIDE_CHANNELS, A.FM_CHUNK_BLOCKS) == (64, 16, 32768, 1)
    with open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_fm_device.h")) as f:
        text = f.read()
    for name, value in (("ROWS", 64), ("NARROW_ROWS", 16), ("WIDE_CHANNELS", 32768), ("CHUNK_BLOCKS", 1)):
        assert re.search(r"#define ASDR_FM_%s %d\b" % (name, value), text), name


def test_fm_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_fm.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS), sorted(res)                  # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds <= 65536, (k, r)


def test_design_states_the_lds_figure():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text[text.index("### 3.14"):]
    section = section[:re.search(r"\n#{2,3} ", section[4:]).start() + 4]
    assert "18,432" in section and "4,608" in section and sorted(LDS.values()) == [4608, 18432]
