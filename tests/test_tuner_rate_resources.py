"""Build-time resources of a rate bank's stage-2 kernel (audiosdr_amd/csrc/asdr_tuner_resample.hip): no spills, at most 64 VGPRs
like the stage-1 kernels, and its static LDS window (2,112 dwords) within what several workgroups per compute unit can share."""
from test_build_properties import _resources


def test_resample_kernel_does_not_spill_and_keeps_its_vgpr_bound():
    res = _resources("asdr_tuner_resample.hip")
    names = [n for n in res if "asdr_tuner_resample_kernel" in n]
    assert names, sorted(res)
    for name in names:
        r = res[name]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) <= 64, (name, r)
        assert r.get("LDS Size [bytes/block]", 0) <= 2112 * 4 + 256, (name, r)
