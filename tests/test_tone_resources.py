"""Build-time resources of the tone squelch's kernel (audiosdr_amd/csrc/asdr_tone.hip): the set of kernels, no scratch, no spills, at
most 128 VGPRs and at most 64 KiB of LDS per workgroup.  The kernel holds, for its 16 rows, a ring of two blocks x 129 words and a
staged output block x 65 words, eight d per row, the window's three verdict words per row, and the cosine table of 1,024 words in
static LDS: 17,344 bytes."""
import os
import re

from test_build_properties import _resources

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ROWS = 16
# kernel (a substring of the mangled name) -> static LDS bytes per workgroup, as built
LDS = {"asdr_tone_kernel": ROWS * (4 * 129 + 4 * 65 + 4 * 8 + 2 * 8 + 4) + 4 * 1024}


def test_tone_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_tone.hip" in b.SOURCES and "asdr_tone_host.cpp" in b.SOURCES
    assert "asdr_tone.hip" in b.DEPS and "asdr_tone_host.cpp" in b.DEPS and "asdr_tone_device.h" in b.DEPS
    assert any(d.endswith("asdr_tone.h") for d in b.DEPS)
    assert A.ToneSquelch is not None and (A.TONE_ROWS, A.TONE_WAVE_ROWS, A.TONE_MAX_TONES) == (16, 4, 64)
    with open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_tone_device.h")) as f:
        text = f.read()
    for name, value in (("ROWS", 16), ("WAVE_ROWS", 4), ("THREADS", 256), ("RING_PITCH", 129), ("OUT_PITCH", 65), ("TABLE", 1024)):
        assert re.search(r"#define ASDR_TONE_%s %d\b" % (name, value), text), name


def test_tone_kernel_does_not_spill_and_keeps_its_bounds():
    res = _resources("asdr_tone.hip")
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
    section = text[text.index("### 3.15"):]
    section = section[:re.search(r"\n#{2,3} ", section[4:]).start() + 4]
    assert "17,344" in section and list(LDS.values()) == [17344]
