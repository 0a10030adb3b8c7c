"""Build-time resources of the packet decoder's kernels (audiosdr_amd/csrc/asdr_packet.hip): the set of kernels (the pass in two
instantiations, of 64 and of 16 channels per workgroup, the collect's count, index and copy passes, and clear's), no scratch, no spills, at most
128 VGPRs.  An instantiation of the pass holds, per row, a ring of two blocks (129 words), the last 64 decimated values (65 words), the
two sign words of a block and the row's space_boost in static LDS: 788 bytes a row, 50,432 and 12,608 bytes."""
import os
import re

from test_build_properties import _resources

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# template argument as the mangled name spells it -> static LDS bytes per workgroup, as built
LDS = {"Li64E": 64 * 4 * (129 + 65 + 2 + 1), "Li16E": 16 * 4 * (129 + 65 + 2 + 1)}
COLLECT = {"asdr_packet_count_kernel": 16, "asdr_packet_index_kernel": 32, "asdr_packet_copy_kernel": 0, "asdr_packet_clear_kernel": 0}


def test_packet_sources_are_in_the_build(A):
    from audiosdr_amd import build as b
    assert "asdr_packet.hip" in b.SOURCES and "asdr_packet_host.cpp" in b.SOURCES
    assert "asdr_packet.hip" in b.DEPS and "asdr_packet_host.cpp" in b.DEPS and "asdr_packet_device.h" in b.DEPS
    assert any(d.endswith("asdr_packet.h") for d in b.DEPS)
    assert A.PacketDecoder is not None and (A.PACKET_ROWS, A.PACKET_NARROW_ROWS, A.PACKET_WIDE_CHANNELS, A.PACKET_MAX_RING) == (64, 16, 32768, 16)
    with open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_packet_device.h")) as f:
        text = f.read()
    for name, value in (("ROWS", 64), ("NARROW_ROWS", 16), ("WIDE_CHANNELS", 32768), ("THREADS", 256), ("RING_PITCH", 129), ("D_PITCH", 65),
                        ("HALF", 74), ("LOADED_BYTES", 80), ("TILE", 256), ("SLOT_PIECES", 22), ("SLOTS_PER_GROUP", 11)):
        assert re.search(r"#define ASDR_PACKET_%s %d\b" % (name, value), text), name


def test_packet_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_packet.hip")
    print(sorted((n, r) for n, r in res.items()))
    assert len(res) == len(LDS) + len(COLLECT), sorted(res)                                     # the set of kernels is pinned
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
    for k, lds in LDS.items():
        names = [n for n in res if k in n and "asdr_packet_kernel" in n]
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
    section = text[text.index("### 3.19"):]
    section = section[:re.search(r"\n#{2,3} ", section[4:]).start() + 4]
    assert "50,432" in section and "12,608" in section and sorted(LDS.values()) == [12608, 50432]
