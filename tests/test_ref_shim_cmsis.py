"""The stand-in CMSIS functions of oracle/ref_shim/arm_math.h -- `arm_cfft_f32` (128 points, forward, bit-reversed) and
`arm_cmplx_mag_squared_f32`, which the reference's image detector calls -- pinned bit for bit against outputs of the reference's own
Cortex-M4 objects (tests/golden/cmsis_cfft128_vectors.npz, cmsis_mag_squared_vectors.npz; executed on tests/thumb_emu.py when the
fixtures were made).  A tiny harness is compiled against the stand-in header alone, with no reference code and the recipe's flags, so a
wrong stand-in fails here and not in the detector tests of tests/test_reference_binary.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import ref_build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "arm_math.h"
#include "arm_const_structs.h"
// harness cfft <in.bin> <n_vectors> <out.bin>: arm_cfft_f32(&arm_cfft_sR_f32_len128, v, 0, 1) on every 256-float vector
// harness mag  <in.bin> <n> <out.bin>: arm_cmplx_mag_squared_f32 of 2 n floats, out of place, then in place: 2 n floats out
int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const int n = atoi(argv[3]), cfft = !strcmp(argv[1], "cfft");
  const size_t n_in = cfft ? (size_t)n * 256 : (size_t)n * 2, n_out = cfft ? n_in : (size_t)n * 2;
  float *x = (float *)calloc(n_in, 4), *y = (float *)calloc(n_out, 4);
  FILE *f = fopen(argv[2], "rb");
  if (!f || fread(x, 4, n_in, f) != n_in) return 3;
  fclose(f);
  if (cfft) {
    for (int v = 0; v < n; v++) arm_cfft_f32(&arm_cfft_sR_f32_len128, x + 256 * v, 0, 1);
    memcpy(y, x, n_in * 4);
  } else {
    arm_cmplx_mag_squared_f32(x, y, n);
    arm_cmplx_mag_squared_f32(x, x, n);
    memcpy(y + n, x, (size_t)n * 4);
  }
  f = fopen(argv[4], "wb");
  if (!f || fwrite(y, 4, n_out, f) != n_out) return 4;
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(ref_build.CXX)
    if cxx is None:
        pytest.skip("no C++ compiler (%s) on this machine" % ref_build.CXX)
    d = tmp_path_factory.mktemp("shim_cmsis")
    (d / "harness.cpp").write_text(HARNESS)
    exe = str(d / "harness")
    subprocess.run([cxx] + ref_build.FLAGS + ["-I", ref_build.SHIM, str(d / "harness.cpp"), "-o", exe], check=True, capture_output=True)
    return exe, d


def _run(harness, mode, x, n):
    exe, d = harness
    np.ascontiguousarray(x, np.float32).tofile(str(d / "in.bin"))
    subprocess.run([exe, mode, str(d / "in.bin"), str(n), str(d / "out.bin")], check=True, capture_output=True)
    return np.fromfile(str(d / "out.bin"), dtype=np.uint32)


def test_stand_in_cfft128_equals_the_reference_objects(harness):
    g = np.load(os.path.join(GOLDEN, "cmsis_cfft128_vectors.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) == 14
    got = _run(harness, "cfft", np.concatenate([g["x_%d" % i] for i in range(len(names))]), len(names)).reshape(len(names), 256)
    for i, name in enumerate(names):
        bad = np.nonzero(got[i] != g["y_bits_%d" % i])[0]
        assert bad.size == 0, "%s: %d of 256 words differ from the reference's arm_cfft_f32, first at word %d" % (name, bad.size, bad[0])


def test_stand_in_mag_squared_equals_the_reference_object(harness):
    g = np.load(os.path.join(GOLDEN, "cmsis_mag_squared_vectors.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) >= 14
    for i, name in enumerate(names):
        x, want = g["x_%d" % i], g["y_bits_%d" % i]
        n = x.size // 2
        got = _run(harness, "mag", x, n)
        assert np.array_equal(got[:n], want), name + " (out of place)"
        assert np.array_equal(got[n:], want), name + " (in place, as the detector calls it)"
