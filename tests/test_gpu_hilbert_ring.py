"""The Hilbert stage of the four-wave chain kernels -- FIR windows sliding through a register ring (audiosdr_amd/csrc/asdr_fir.h
hilbert_fir_rows_ring), the history staged in front of it (asdr_kernels.hip; the variant with one LDS store per 16 bytes is archived as
profiles/experiments/r06_mw_hist_b128.diff) -- against the oracle at tolerance 0, with inputs aimed at what those two touch: every position of the 383-sample
window, both slots of the history ring, the seams between a channel's lanes and between the 32-float pieces of a block.

Blanker off, unit gains.  Channel c carries, on top of low noise, ONE full-scale sample at position c mod 384 of the first three blocks;
five single-block calls move it through the new, the previous and the oldest block of the window.  LSB, USB, CW-LSB and WSPR, by
broadcast (asdr_update_kernel_mw_u) and with one row in the middle of a workgroup changed (asdr_update_kernel_mw), on 512 channels (16
whole workgroups) and 544 (the last workgroup is a single wave).  The demodulator's output row (tap DEMOD) is compared bit for bit on
every 37th channel, the int16 audio on every channel, the launch census after every block.  One more case drives +-32767 alternating
through the same path.  The oracles run once per (mode, form) on the 544-channel bank; the 512-channel bank is its first 512 channels."""
import numpy as np
import pytest

import four_wave_scenarios as F
from cases import LSB, USB, CW_LSB, WSPR
from helpers import S, f32_bits
from test_gpu_uniform_params import _Run, _census

pytestmark = pytest.mark.gpu

BLOCKS = 5
WINDOW = 384
N_MAX = 544
_QUIET = [S("disableNoiseBlanker"), S("setInputGain", 1.0), S("setOutputGain", 1.0)]
_MODES = {"lsb": LSB, "usb": USB, "cwl": CW_LSB, "wspr": WSPR}


def impulse_rows():
    """384 rows: row r = low noise plus one full-scale sample (I = 32767, Q = -32768) at sample r of the 640"""
    from audiosdr_amd.synth import make_iq
    I, Q = make_iq(WINDOW, BLOCKS, A=0.0, noise=0.002)
    I = np.array(I).reshape(WINDOW, BLOCKS * 128); Q = np.array(Q).reshape(WINDOW, BLOCKS * 128)
    r = np.arange(WINDOW)
    I[r, r] = 32767; Q[r, r] = -32768
    return I.reshape(WINDOW, BLOCKS, 128), Q.reshape(WINDOW, BLOCKS, 128)


def alternating_rows():
    """2 rows of +-32767 alternating from sample to sample, I against Q and row against row in opposite phase"""
    s = np.where(np.arange(BLOCKS * 128) % 2 == 0, 32767, -32767).astype(np.int16)
    I = np.stack([s, -s]).reshape(2, BLOCKS, 128); Q = np.stack([-s, s]).reshape(2, BLOCKS, 128)
    return I, Q


def scenario(mname, rows_differ, rows=impulse_rows):
    setup = [S("setDemodMode", _MODES[mname])] + _QUIET
    if rows_differ:                                      # (not a gain: the gains stay 1)
        setup.append(S("setAGCstaticGain", 20.0, sel=F.MID))
    return F.Scenario("%s-%s" % (mname, "rows" if rows_differ else "uniform"), rows, setup, n=N_MAX, expect="r" if rows_differ else "u", taps=True)


_REFERENCE = {}


def reference(ao, sc):
    """the scenario's inputs and oracles on the 544-channel bank, made once and shared"""
    if sc.name not in _REFERENCE:
        bI, bQ = sc.rows()
        bI.setflags(write=False); bQ.setflags(write=False)
        run = F.OracleRun(ao, sc, bI, bQ, taps_for=range(0, N_MAX, 37))
        run.audio.setflags(write=False)
        _REFERENCE[sc.name] = (bI, bQ, run)
    return _REFERENCE[sc.name]


def run_bank(gpu, ao, sc, n):
    bI, bQ, run = reference(ao, sc)
    demod = gpu.TAPS.index("DEMOD")

    def configure(b):
        b.enable_taps(True)
        F.apply_to_batch(b, sc.setup, n)

    r = _Run(gpu, n, bI, bQ, configure)
    try:
        for blk in range(BLOCKS):
            r.step(1, gpu.STREAM_BATCH if blk < 3 else r.caller)
            got = _census(gpu)
            assert got == sc.census(blk), "block %d: launched %s, expected %s" % (blk, got, sc.census(blk))
            taps = r.b.read_taps()
            for c in range(0, n, 37):
                ref = run.taps[run.of_channel[c]][blk][demod]
                bad = np.flatnonzero(f32_bits(taps["DEMOD"][c]) != f32_bits(ref))
                assert bad.size == 0, "block %d channel %d: %d DEMOD samples differ, first at %d" % (blk, c, bad.size, bad[0])
        got = r.audio()
        bad = np.argwhere(got != run.want()[:n])
        assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())
    finally:
        r.close()


@pytest.mark.parametrize("n", [512, N_MAX])
@pytest.mark.parametrize("rows_differ", [False, True], ids=["uniform", "rows"])
@pytest.mark.parametrize("mname", sorted(_MODES))
def test_an_impulse_at_every_position_of_the_window(gpu, ao, mname, rows_differ, n):
    run_bank(gpu, ao, scenario(mname, rows_differ), n)


def test_full_scale_alternation(gpu, ao):
    """+-32767 alternating (finite everywhere: the largest steps the int16 input can make) through the staging and the ring FIR, USB by broadcast, 544 channels"""
    sc = scenario("usb", False, rows=alternating_rows)
    sc.name = "usb-uniform-alternating"
    run_bank(gpu, ao, sc, N_MAX)
