"""Build-time resources of the input formats' kernels (audiosdr_amd/csrc/asdr_tuner.hip, asdr_tuner_fastconv.hip): every
instantiation exists, none spills or uses scratch, and each keeps the bounds its CS16 counterpart is held to -- 64 VGPRs for the
direct-form kernels (test_tuner_resources.py), 128 VGPRs and 64 KB of LDS for the fast-convolution ones
(test_tuner_fastconv_resources.py).  hipcc cross-compiles without a GPU; the remark parsing is test_build_properties.py's."""
from test_build_properties import _resources

FORMATS = 4      # CU8, CS8, CF32, RS16
COMPLEX = 3      # the fast-convolution forward kernel's instantiations (RS16 has the real-input kernel)


def check(res, stem, count, vgprs):
    names = [n for n in res if stem in n]
    assert len(names) == count, (stem, sorted(res))
    for name in names:
        r = res[name]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) <= vgprs, (name, r)
        assert r.get("LDS Size [bytes/block]", 0) <= 65536, (name, r)


def test_direct_form_format_kernels_keep_the_cs16_kernels_bounds():
    res = _resources("asdr_tuner.hip")
    check(res, "asdr_tuner_fmt_kernel", FORMATS, 64)
    check(res, "asdr_tuner_fmt_history_kernel", FORMATS, 64)


def test_fastconv_format_kernels_keep_their_bounds():
    res = _resources("asdr_tuner_fastconv.hip")
    check(res, "asdr_tuner_fc_fmt_forward_kernel", COMPLEX, 128)
    check(res, "asdr_tuner_fc_fmt_history_kernel", FORMATS, 128)
    check(res, "asdr_tuner_fc_real_forward_kernel", 1, 128)
