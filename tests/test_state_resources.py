"""Build-time properties of the state-record kernels (audiosdr_amd/csrc/asdr_state.hip) under the build's own flags: exactly the gather
and the scatter kernel, pure copies -- no scratch, no spills, no LDS, far below 128 VGPRs (DESIGN.md 3.9 has the counts)."""
from test_build_properties import _resources


def test_state_kernels_are_two_lean_copies():
    res = _resources("asdr_state.hip")
    assert sorted(res) == ["asdr_state_gather_kernel", "asdr_state_scatter_kernel"], sorted(res)
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert 0 < r["VGPRs"] <= 128, (name, r)
        assert r["LDS Size [bytes/block]"] == 0, (name, r)
    print({n: r["VGPRs"] for n, r in sorted(res.items())})


def test_state_kernels_are_built_into_the_library_and_stay_out_of_the_chain_census():
    import audiosdr_amd as A
    from audiosdr_amd import build as b
    assert "asdr_state.hip" in b.SOURCES
    L = A.load_library()
    names = {L.asdr_kernels_name(i).decode() for i in range(L.asdr_kernels_count())}
    assert not any("state" in n for n in names - {"asdr_stream_snapshot_kernel", "asdr_stream_restore_kernel"})
    assert L.asdr_state_record_bytes() == 6400
