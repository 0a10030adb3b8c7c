"""Build-time resources of the DCS squelch's kernel (audiosdr_amd/csrc/asdr_dcs.hip): the set of kernels (two instantiations, of 64
and of 16 channels per workgroup), no scratch, no spills, at most 128 VGPRs.  An instantiation holds, per row, a ring of two blocks
(129 words), the last 32 decimated values (33 words), the block's eight bit-filter outputs (9 words) and the mute masks of two blocks,
and the table of 128 words, in static LDS: 692 bytes a row + 512, 44,800 and 11,584 bytes."""
import os
import re

from test_build_properties import _resources

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# template argument as the mangled name spells it -> static LDS bytes per workgroup, as built
LDS = {"Li64E": 64 * 4 * (129 + 33 + 9 + 2) + 4 * 128, "Li16E": 16 * 4 * (129 + 33 + 9 + 2) + 4 * 128}


def test_dcs_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_dcs.hip" in b.SOURCES and "asdr_dcs_host.cpp" in b.SOURCES
    assert "asdr_dcs.hip" in b.DEPS and "asdr_dcs_host.cpp" in b.DEPS and "asdr_dcs_device.h" in b.DEPS
    assert any(d.endswith("asdr_dcs.h") for d in b.DEPS)
    assert A.DcsSquelch is not None and (A.DCS_ROWS, A.DCS_NARROW_ROWS, A.DCS_WIDE_CHANNELS, A.DCS_MAX_CODES) == (64, 16, 32768, 128)
    with open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_dcs_device.h")) as f:
        text = f.read()
    for name, value in (("ROWS", 64), ("NARROW_ROWS", 16), ("WIDE_CHANNELS", 32768), ("THREADS", 256), ("RING_PITCH", 129), ("D_PITCH", 33),
                        ("S_PITCH", 9), ("HALF", 1312)):
        assert re.search(r"#define ASDR_DCS_%s %d\b" % (name, value), text), name


def test_dcs_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_dcs.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS) and all("asdr_dcs_kernel" in n for n in res), sorted(res)      # the set of kernels is pinned
    for k, lds in LDS.items():
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, sorted(res))
        r = res[names[0]]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("VGPRs", 0) <= 128, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == lds <= 65536, (k, r)


def test_design_states_the_lds_figures():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text[text.index("### 3.18"):]
    section = section[:re.search(r"\n#{2,3} ", section[4:]).start() + 4]
    assert "44,800" in section and "11,584" in section and sorted(LDS.values()) == [11584, 44800]
