"""Build-time resources of a fast-convolution bank's kernels (audiosdr_amd/csrc/asdr_tuner_fastconv.hip): no spills, at most 128
VGPRs, and at most 64 KB of LDS per workgroup."""
from test_build_properties import _resources

KERNELS = ("asdr_tuner_fc_forward_kernel", "asdr_tuner_fc_channel_kernel", "asdr_tuner_fc_history_kernel")


def test_fastconv_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_tuner_fastconv.hip")
    for k in KERNELS:
        names = [n for n in res if k in n]
        assert names, (k, sorted(res))
        for name in names:
            r = res[name]
            assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
            assert r.get("VGPRs", 0) <= 128, (name, r)
            assert r.get("LDS Size [bytes/block]", 0) <= 65536, (name, r)
