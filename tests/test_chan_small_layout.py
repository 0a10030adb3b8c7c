"""ChanSmall (audiosdr_amd/csrc/asdr_device.h): what the plain kind of the chain kernel reads and writes every block -- the IF and audio biquad states
and its sixteen scalar words -- lies in the first 256 bytes of a 512-byte row, i.e. in two aligned 128-byte lines; the AM image state, the PLL words
and the padding lie behind them.  The pieces the kernels move as 16-byte groups are 16-byte aligned.  A stand-alone host program compiled
against the header prints the offsets; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HOT = ("if_state", "af_state", "phase_ssb", "phase_am", "nb_avg", "am_carrier", "agc_gain", "agc_old_abs", "agc_hang_counter", "nb_slot_unused",
       "status", "nb_gain", "hil_slot")
COLD = ("img_state", "pll_y_re", "pll_y_im", "pll_prev_filt", "pll_d0", "pll_d1", "pll_phase_est", "pll_freq", "pad_")
SRC = """#include <cstddef>
#include <cstdio>
#include "asdr_device.h"
#define F(m) std::printf(#m " %zu %zu\\n", offsetof(ChanSmall, m), sizeof(((ChanSmall *)0)->m))
int main() {
  std::printf("sizeof %zu 0\\n", sizeof(ChanSmall));
  FIELDS
  return 0;
}
"""


def test_plain_kind_fields_in_the_first_two_lines(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "layout.cpp"
    src.write_text(SRC.replace("FIELDS", " ".join("F(%s);" % m for m in HOT + COLD)))
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "audiosdr_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    field = {name: (int(off), int(size)) for name, off, size in (line.split() for line in out.splitlines())}
    assert field["sizeof"][0] == 512
    for m in HOT:
        off, size = field[m]
        assert off + size <= 256, "%s at %d..%d is not in the first 256 bytes" % (m, off, off + size)
    for m in COLD:
        assert field[m][0] >= 256, "%s at %d is among the plain kind's fields" % (m, field[m][0])
    assert sum(field[m][1] for m in HOT) == 256                      # ... which they fill: 128 + 64 + 64
    assert field["if_state"] == (0, 128) and field["af_state"] == (128, 64)
    for m in ("if_state", "af_state", "img_state", "phase_ssb", "agc_gain", "status", "pll_y_im", "pll_phase_est"):
        assert field[m][0] % 16 == 0, "%s at %d: the 16-byte group it starts is not aligned" % (m, field[m][0])
    # the groups a state record's 16-byte pieces are made of (asdr_state.hip): the words between them keep their order
    assert [field[m][0] for m in ("phase_ssb", "phase_am", "nb_avg", "am_carrier")] == [192, 196, 200, 204]
    assert [field[m][0] for m in ("agc_gain", "agc_old_abs", "agc_hang_counter", "nb_slot_unused")] == [208, 212, 216, 220]
    assert [field[m][0] for m in ("status", "nb_gain", "hil_slot")] == [224, 228, 252]
