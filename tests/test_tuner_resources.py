"""Build-time resources of the digital tuner's kernels (audiosdr_amd/csrc/asdr_tuner.hip): no spills, and the filter kernel's
dynamic LDS (at most 37,120 B for D = 63, L = 1024) leaves room for several workgroups per compute unit.  hipcc cross-compiles
without a GPU; the remark parsing is test_build_properties.py's."""
from test_build_properties import _resources


def test_tuner_kernels_do_not_spill():
    res = _resources("asdr_tuner.hip")
    names = sorted(res)
    assert any("asdr_tuner_kernel" in n for n in names) and any("asdr_tuner_history_kernel" in n for n in names), names
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) <= 64, (name, r)
