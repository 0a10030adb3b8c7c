"""Build-time properties of the two four-wave chain kernels with the ring FIR (audiosdr_amd/csrc/asdr_fir.h hilbert_fir_rows_ring), read
from the compiler's kernel info: at most 168 VGPRs (three waves per SIMD), no scratch and no spills, 52,800 bytes of LDS (three
workgroups per CU) -- and every other caller of the Hilbert FIR still on the chunked function."""
import os
import re

from test_build_properties import CSRC, _resources

FOUR_WAVE = ("asdr_update_kernel_mw", "asdr_update_kernel_mw_u")


def test_four_wave_kernels_keep_registers_scratch_and_lds():
    res = _resources("asdr_kernels.hip")
    for name in FOUR_WAVE:
        r = res[name]
        assert 0 < r["VGPRs"] <= 168, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 52800, (name, r)


def test_only_the_four_wave_form_takes_the_ring_fir():
    with open(os.path.join(CSRC, "asdr_kernels.hip")) as f:
        text = f.read()
    calls = [ln.strip() for ln in text.splitlines() if re.search(r"\bhilbert_fir_ring\(L\b", ln)]
    assert len(calls) == 1 and calls[0].startswith("if constexpr (MW && WAVES == 4 && ASDR_MW_FIR_RING != 0"), calls
    assert len(re.findall(r"\bhilbert_fir_rows_ring\(", text)) == 1          # (its one wrapper)
    for src in os.listdir(CSRC):
        if src not in ("asdr_kernels.hip", "asdr_fir.h"):
            with open(os.path.join(CSRC, src)) as f:
                assert "hilbert_fir_rows_ring" not in f.read(), src
