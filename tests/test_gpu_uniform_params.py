"""The four-wave chain kernel with the settings group's parameter row as launch constants (asdr_update_kernel_mw_u, include/asdr.h
asdr_params_uniform_groups): a bank configured by broadcast setters takes it, a per-channel setting sends the group back to the kernels
that read the rows, and the audio is the oracle's bit for bit on every channel either way.  C2's settings (USB, audio filter; blanker
and AGC on by default), banks of 512 channels = the 64 waves from which the four-wave form is taken.  Every case checks the launch
census (which kernels ran)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import Hip

pytestmark = pytest.mark.gpu

UNIQ = 8                      # distinct input rows (channel c gets row c % UNIQ): one oracle run each
MW_U, MW = "asdr_update_kernel_mw_u", "asdr_update_kernel_mw"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _tile(a, n):
    return np.ascontiguousarray(np.tile(a, ((n + a.shape[0] - 1) // a.shape[0], 1, 1))[:n])


def _inputs(total, **kw):
    from audiosdr_amd.synth import make_iq
    fc = 6890.0 - 600.0 + 20.0 * (np.arange(UNIQ) % 5)
    return make_iq(UNIQ, total, fc=fc, A=0.3, noise=0.02, **kw)


def _c2(sdr):
    sdr.setDemodMode(1); sdr.enableAudioFilter()


def _census(gpu):
    """update kernels launched since the last call (the reset kernel of a batch's first call is no update kernel)"""
    return {k: v for k, v in gpu.binding.kernels_launched(reset=True).items() if k != "asdr_reset_kernel"}


class _Run:
    """A batch of n channels on device rows of `total` blocks; step(T, stream) runs the next T blocks as single-block calls."""

    def __init__(self, gpu, n, bI, bQ, configure):
        self.gpu, self.n, self.total, self.pos = gpu, n, bI.shape[1], 0
        self.hip = Hip()
        self.dI, self.dQ = self.hip.upload(_tile(bI, n)), self.hip.upload(_tile(bQ, n))
        self.dO = self.hip.malloc(n * self.total * 256)
        self.caller = self.hip.stream()
        self.b = gpu.AudioSDRBatch(n)
        configure(self.b)
        gpu.binding.kernels_launched(reset=True)

    def step(self, T, stream):
        for _ in range(T):
            off = self.pos * 256
            self.b.update_device_strided(self.dI + off, self.dQ + off, self.dO + off, 1, self.total, self.total, stream)
            self.pos += 1

    def audio(self):
        self.b.synchronize(); self.hip.sync(self.caller)
        return self.hip.download(self.dO, (self.n, self.total, 128), np.int16)

    def close(self):
        self.hip.free_all(); self.b.close()


def _oracle(ao, bI, bQ, configure, changes=()):
    """[UNIQ][total][128]: one oracle per input row; changes = ((block, fn), ...) applied in front of that block"""
    total = bI.shape[1]
    out = np.empty((bI.shape[0], total, 128), dtype=np.int16)
    cuts = [0] + [blk for blk, _ in changes] + [total]
    for c in range(bI.shape[0]):
        o = ao.OracleSDR()
        configure(o)
        for i in range(len(cuts) - 1):
            if i > 0:
                changes[i - 1][1](o)
            lo, hi = cuts[i], cuts[i + 1]
            if hi > lo:
                out[c, lo:hi] = o.update(bI[c, lo:hi], bQ[c, lo:hi]).reshape(hi - lo, 128)
    return out


def _same(got, want_rows, n):
    want = _tile(want_rows, n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())


@pytest.fixture(scope="module")
def c2_case(ao):
    """C2's settings on 12 blocks: inputs and the oracle's audio, shared (and left alone) by the cases below"""
    bI, bQ = _inputs(12, impulse_every=1700)
    want = _oracle(ao, bI, bQ, _c2)
    want.setflags(write=False)
    return bI, bQ, want


@pytest.mark.parametrize("n", [512, 520])
def test_broadcast_bank_takes_the_launch_constant_form(gpu, c2_case, n):
    """512 channels: 16 full workgroups.  520: the last workgroup holds one wave of channels and three of padding -- every channel is
    compared, the last 8 included.  8 blocks on the batch's own streams, 4 on a caller's."""
    bI, bQ, want = c2_case
    r = _Run(gpu, n, bI, bQ, _c2)
    r.step(8, gpu.STREAM_BATCH)
    r.step(4, r.caller)
    got = r.audio()
    assert _census(gpu) == {MW_U: 12}
    assert r.b.params_uniform_groups()[0] == 1
    _same(got, want, n)
    r.close()


def _nondefault(sdr):
    _c2(sdr)
    sdr.setDemodMode(0)                                   # LSB: the other sign of the sideband combine, another frequency shift
    sdr.setInputGain(0.5); sdr.setIQgainBalance(1.02)     # the scale and envelope paths of gains other than 1
    sdr.setAudioFilter(2); sdr.setAGCmode(2)
    sdr.setOutputGain(0.5); sdr.setNoiseBlankerThresholdDb(10.0)


def test_constants_that_are_not_the_defaults(gpu, ao):
    bI, bQ = _inputs(9, impulse_every=900)
    r = _Run(gpu, 512, bI, bQ, _nondefault)
    r.step(6, gpu.STREAM_BATCH)
    r.step(3, r.caller)
    got = r.audio()
    assert _census(gpu) == {MW_U: 9}
    _same(got, _oracle(ao, bI, bQ, _nondefault), 512)
    r.close()


def test_one_channel_differs_then_a_broadcast_restores(gpu, ao):
    """3 blocks uniform | channel 37's output gain 0.7: 3 blocks on the kernels that read the rows | broadcast 0.5: 3 blocks on the
    launch-constant form again.  All 512 channels stay exact: the state carries across both switches."""
    bI, bQ = _inputs(9, impulse_every=1100)
    n = 512
    r = _Run(gpu, n, bI, bQ, _c2)
    r.step(3, gpu.STREAM_BATCH)
    r.b.synchronize()
    assert _census(gpu) == {MW_U: 3}
    r.b.setOutputGain(0.7, ch=37)
    r.step(3, gpu.STREAM_BATCH)
    r.b.synchronize()
    assert _census(gpu) == {MW: 3} and r.b.params_uniform_groups()[0] == 0
    r.b.setOutputGain(0.5)
    r.step(3, gpu.STREAM_BATCH)
    got = r.audio()
    assert _census(gpu) == {MW_U: 3} and r.b.params_uniform_groups()[0] == 1
    want = _tile(_oracle(ao, bI, bQ, _c2), n)
    c = 37 % UNIQ
    want[37] = _oracle(ao, bI[c:c + 1], bQ[c:c + 1], _c2, changes=((3, lambda o: o.setOutputGain(0.7)), (6, lambda o: o.setOutputGain(0.5))))[0]
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d samples differ, first at %s" % (len(bad), bad[0].tolist())
    r.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
try:
    import torch  # noqa: F401  (before the library: tests/conftest.py)
except ImportError:
    pass
import audiosdr_amd as A
from tests import test_gpu_uniform_params as T
A.load_library()
bI, bQ = T._inputs(12, impulse_every=1700)
r = T._Run(A, 512, bI, bQ, T._c2)
r.step(8, A.STREAM_BATCH); r.step(4, r.caller)
got = r.audio()
np.save(sys.argv[2], got)
print("CENSUS", sorted(T._census(A).items()), r.b.params_uniform_groups()[0])
r.close()
"""


def test_switched_off_in_the_environment(gpu, c2_case, tmp_path):
    """ASDR_NO_UNIFORM_PARAMS=1 (read when a batch is created, so a process of its own): the same audio from the kernels that read the rows."""
    bI, bQ, want = c2_case
    out = str(tmp_path / "audio.npy")
    env = dict(os.environ, ASDR_NO_UNIFORM_PARAMS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "CENSUS [('%s', 12)] 1" % MW in p.stdout, p.stdout[-500:]   # (the group is still known to be uniform: only the launch form is off)
    _same(np.load(out), want, 512)


def _general_paths(sdr):
    _c2(sdr)
    sdr.setAGChangTime(0.0)


def test_blanker_and_agc_general_paths(gpu, ao):
    """An impulse in every block (the blanker's general path: detections, re-scanned envelopes) and no AGC hang time (the AGC's general
    per-sample form) through the launch-constant instantiation."""
    bI, bQ = _inputs(9, impulse_every=128)
    r = _Run(gpu, 512, bI, bQ, _general_paths)
    r.step(6, gpu.STREAM_BATCH)
    r.step(3, r.caller)
    got = r.audio()
    assert _census(gpu) == {MW_U: 9}
    _same(got, _oracle(ao, bI, bQ, _general_paths), 512)
    r.close()
