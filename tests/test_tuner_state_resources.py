"""Build-time properties of the tuner state-record kernels (audiosdr_amd/csrc/asdr_tuner_state.hip) under the build's own flags:
exactly the gather and the scatter kernel, pure copies -- no scratch, no spills, no LDS, far below 128 VGPRs (DESIGN.md 3.8.7 has the
counts)."""
from test_build_properties import _resources


def test_tuner_state_kernels_are_two_lean_copies():
    res = _resources("asdr_tuner_state.hip")
    assert sorted(res) == ["asdr_tuner_state_gather_kernel", "asdr_tuner_state_scatter_kernel"], sorted(res)
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert 0 < r["VGPRs"] <= 128, (name, r)
        assert r["LDS Size [bytes/block]"] == 0, (name, r)
    print({n: r["VGPRs"] for n, r in sorted(res.items())})


def test_tuner_state_kernels_are_built_into_the_library():
    import audiosdr_amd as A
    from audiosdr_amd import build as b
    assert "asdr_tuner_state.hip" in b.SOURCES
    L = A.load_library()
    assert A.tuner._lib().asdr_tuner_channel_record_bytes() == 2560
    assert hasattr(L, "asdr_launch_tuner_state_gather") and hasattr(L, "asdr_launch_tuner_state_scatter")
