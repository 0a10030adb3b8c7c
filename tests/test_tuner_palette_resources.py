"""Build-time properties of the palette's channel kernel (audiosdr_amd/csrc/asdr_tuner_palette.hip): both instantiations without
scratch or spills, at most 128 VGPRs and no more than the kernel whose place each takes, exactly that kernel's 2,048 bytes of LDS;
and the channel step's statements, which now stand in three files, are the same text in all three but for the palette's stated
changes (the row base, and the gain in the scale)."""
import os
import re

from test_build_properties import CSRC, _resources


def test_palette_kernels_do_not_spill_and_keep_the_channel_kernels_budget():
    res = _resources("asdr_tuner_palette.hip")
    names = sorted(n for n in res if "asdr_tuner_fc_channel_palette_kernel" in n)
    assert len(names) == 2 and len(res) == 2, sorted(res)     # LEVELS = 0, 1 and nothing else
    plain = next(r for n, r in _resources("asdr_tuner_fastconv.hip").items() if "asdr_tuner_fc_channel_kernel" in n)
    level = next(r for n, r in _resources("asdr_tuner_monitor.hip").items() if "asdr_tuner_fc_channel_level_kernel" in n)
    for name in names:
        r = res[name]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert 0 < r["VGPRs"] <= 128, (name, r)
        assert r["LDS Size [bytes/block]"] == 2048, (name, r)
        other = level if "ILi1E" in name else plain                # the kernel this instantiation is launched instead of
        assert r["VGPRs"] <= other["VGPRs"], (name, r, other)


def channel_step(path, kernel):
    """The statements of a channel kernel from the first pass to the end of the store loop, one stripped line each."""
    with open(os.path.join(CSRC, path)) as f:
        text = f.read()
    body = text[text.index("void " + kernel + "("):]
    body = body[body.index("  // pass p = 1"):]
    body = body[:body.index("    oq[n] = ") ]
    return [ln.strip() for ln in body.splitlines() if ln.strip()]


def test_the_three_copies_of_the_channel_step_are_one_text():
    plain = channel_step("asdr_tuner_fastconv.hip", "asdr_tuner_fc_channel_kernel")
    level = channel_step("asdr_tuner_monitor.hip", "asdr_tuner_fc_channel_level_kernel")
    pal = channel_step("asdr_tuner_palette.hip", "asdr_tuner_fc_channel_palette_kernel")
    assert len(plain) > 30 and level == plain
    gain = [ln for ln in pal if ln.startswith("const float scale = unit * gain;")]
    assert len(gain) == 1
    pal = [re.sub(r"^const float unit = ldexpf", "const float scale = ldexpf", ln) for ln in pal if ln not in gain]
    assert pal == plain, [(a, b) for a, b in zip(pal, plain) if a != b][:3]
