"""Build-time resources of the monitors' kernels (audiosdr_amd/csrc/asdr_tuner_monitor.hip): no scratch, no spills, at most 128
VGPRs and at most 64 KB of LDS per workgroup -- the bar tests/test_tuner_fastconv_resources.py sets for their neighbours; the
spectrum kernel uses no LDS at all, and the level sibling of the channel kernel no more than the channel kernel itself."""
from test_build_properties import _resources

KERNELS = ("asdr_tuner_fc_spectrum_kernel", "asdr_tuner_fc_channel_level_kernel", "asdr_tuner_fc_level_fold_kernel")


def test_monitor_kernels_do_not_spill_and_keep_their_bounds():
    res = _resources("asdr_tuner_monitor.hip")
    for k in KERNELS:
        names = [n for n in res if k in n]
        assert names, (k, sorted(res))
        if k == "asdr_tuner_fc_spectrum_kernel":
            assert len(names) == 4, names                     # rect / hann x sum / peak
        for name in names:
            r = res[name]
            assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
            assert r.get("VGPRs", 0) <= 128, (name, r)
            assert r.get("LDS Size [bytes/block]", 0) <= 65536, (name, r)
            if k != "asdr_tuner_fc_channel_level_kernel":
                assert r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    plain = next(r for n, r in _resources("asdr_tuner_fastconv.hip").items() if "asdr_tuner_fc_channel_kernel" in n)
    level = next(r for n, r in res.items() if "asdr_tuner_fc_channel_level_kernel" in n)
    assert level["LDS Size [bytes/block]"] == plain["LDS Size [bytes/block]"] == 2048
