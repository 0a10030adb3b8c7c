"""The plain kind's one-block kernels with the one-sample-skew audio pipelines (biquad_pipe_skew1, ASDR_PIPE_SKEW1_MASK) keep the resources
their occupancy stands on: <= 168 VGPRs (three waves per SIMD), no scratch, and the four-wave workgroup's 52,800 B of LDS (three workgroups
per CU).  Cross-compiles for gfx950 without a GPU and reads the compiler's own resource remarks."""
import pytest

from test_build_properties import _resources

KERNELS = ("asdr_update_kernel_mw", "asdr_update_kernel_mw_u", "asdr_update_kernel_one")


@pytest.fixture(scope="module")
def resources():
    return _resources("asdr_kernels.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_registers_and_scratch(resources, name):
    r = resources[name]
    assert r["VGPRs"] <= 168 and r.get("VGPRs Spill", 0) == 0 and r["ScratchSize [bytes/lane]"] == 0, r


@pytest.mark.parametrize("name", KERNELS[:2])
def test_four_wave_workgroup_lds(resources, name):
    assert resources[name]["LDS Size [bytes/block]"] == 52800, resources[name]
