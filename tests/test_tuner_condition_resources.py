"""Build-time properties of the conditioning pre-pass (audiosdr_amd/csrc/asdr_tuner_condition.hip) under the build's own flags:
every instantiation -- five formats x (write, sum, both), and CS16 by dwords for rows that start on a sample -- without scratch
memory or spills, within 128 VGPRs, and with no LDS beyond the workgroup reduction of the sums (DESIGN.md 3.8.6 has the counts)."""
from test_build_properties import _resources


def test_condition_kernels_do_not_spill_and_fit_128_vgprs():
    res = _resources("asdr_tuner_condition.hip")
    assert len(res) == 18 and all("asdr_tuner_condition_kernel" in n for n in res), sorted(res)
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert 0 < r["VGPRs"] <= 128, (name, r)
        sums = "Lb1ELb" in name.split("ILi")[1][3:]             # <F, WRITE, STATS, ALIGNED>: the third argument
        assert r["LDS Size [bytes/block]"] == (192 if sums else 0), (name, r)
    print({n: (r["VGPRs"], r["LDS Size [bytes/block]"]) for n, r in sorted(res.items())})
