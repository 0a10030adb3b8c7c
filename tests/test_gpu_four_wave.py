"""The four-wave chain kernels (asdr_update_kernel_mw_u: the group's parameter row as launch constants; asdr_update_kernel_mw: the rows
read per channel) over the whole control surface, against the oracle at tolerance 0: int16 audio of every channel and block, the status
getters on every channel, the 12 stage taps as bit patterns on sampled channels.  Banks of 512 channels and more -- the library's own
threshold for the form (64 waves of one direct settings group), no environment switch -- as single-block calls on the batch's streams
and on a caller's.  EVERY case asserts the launch census block by block: what ran is the four-wave kernel the scenario names (and
params_uniform_groups() agrees with which of the two), never whatever the launcher might have fallen back to.

The scenarios (settings scripts, inputs, seeds) are tests/four_wave_scenarios.py's; tests/test_four_wave_scenarios.py shows without a GPU
that they reach the AGC regimes they are there for and that the schedule gives the launch forms asserted here."""
import numpy as np
import pytest

import four_wave_scenarios as F
from helpers import f32_bits
from test_gpu_uniform_params import _Run, _census

pytestmark = pytest.mark.gpu


def _status_blocks(T):
    return set(range(T)) if T <= 64 else set(range(11, T, 50)) | {T - 1}


def _oracle_status(o):
    return (o.AGCisActive(), o.NoiseBlankerDetection(), o.getSAMphaseLockStatus(), int(f32_bits(o.getSAMfrequency()).ravel()[0]),
            int(f32_bits(o.getAMcarrierLevel()).ravel()[0]))


class _Oracles(F.OracleRun):
    """... which also keeps every oracle's status getters after the blocks the GPU side reads them at"""

    def __init__(self, ao, sc, bI, bQ, taps_for=None):
        self.status_blocks = _status_blocks(bI.shape[1])
        super().__init__(ao, sc, bI, bQ, taps_for=taps_for)

    def after_block(self, i, blk, o):
        if blk in self.status_blocks:
            self.status.setdefault(blk, {})[i] = _oracle_status(o)


def _check_status(r, run, blk):
    st = r.b.read_status()
    got = np.stack([st["agc_active"], st["nb_detected"], st["sam_locked"], f32_bits(st["sam_frequency"]).astype(np.int64),
                    f32_bits(st["am_carrier"]).astype(np.int64)], axis=1)
    want = np.array([run.status[blk][i] for i in run.of_channel], dtype=np.int64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "status after block %d: %d words differ, first at (channel, getter) %s" % (blk, len(bad), bad[0].tolist())


def _run_scenario(gpu, ao, sc):
    bI, bQ = sc.rows()
    T = bI.shape[1]
    tap_channels = [c for c in F.TAP_CHANNELS if c < sc.n] if sc.taps else None
    run = _Oracles(ao, sc, bI, bQ, taps_for=tap_channels)

    def configure(b):
        if sc.taps:
            b.enable_taps(True)
        F.apply_to_batch(b, sc.setup, sc.n)

    r = _Run(gpu, sc.n, bI, bQ, configure)
    try:
        on_caller = T - max(1, T // 3)                   # the last third of the blocks on a caller's stream
        for blk in range(T):
            if blk in sc.script:
                r.b.synchronize(); r.hip.sync(r.caller)
                F.apply_to_batch(r.b, sc.script[blk], sc.n)
            r.step(1, gpu.STREAM_BATCH if blk < on_caller else r.caller)
            got, want = _census(gpu), sc.census(blk)
            if want is None:                             # the scenario leaves the form here: whatever runs, it is neither four-wave kernel
                assert got and F.MW not in got and F.MW_U not in got, "block %d: %s" % (blk, got)
            else:
                assert got == want, "block %d: launched %s, expected %s" % (blk, got, want)
            assert r.b.params_uniform_groups()[0] == sc.uniform_groups(blk), "block %d" % blk
            if sc.taps:
                taps = r.b.read_taps()
                for c in tap_channels:
                    ref = run.taps[run.of_channel[c]][blk]
                    for t, name in enumerate(gpu.TAPS):
                        assert np.array_equal(f32_bits(taps[name][c]), f32_bits(ref[t])), "block %d channel %d tap %s" % (blk, c, name)
            if blk in run.status_blocks:
                _check_status(r, run, blk)
        got = r.audio()
        bad = np.argwhere(got != run.want())
        assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())
    finally:
        r.close()


_MATRIX = [F.matrix_scenario(cfg, rows) for cfg in F.matrix_configs() for rows in (False, True)]


@pytest.mark.parametrize("sc", _MATRIX, ids=lambda sc: sc.name)
def test_mode_and_enable_matrix(gpu, ao, sc):
    """LSB, USB, CW-LSB, CW-USB, AM, WSPR and two mode values outside 0..6 (reached after three USB blocks; one of them without the kept
    row) against blanker, audio filter, AGC (modes 0..3) and mute on and off; every configuration by broadcast alone (the launch-constant
    form) and with one field of one channel in the middle of a workgroup changed (the row-reading form)."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("sc", F.rows_scenarios(), ids=lambda sc: sc.name)
def test_rows_that_differ_inside_one_direct_group(gpu, ao, sc):
    """Every channel with gains, IQ balance, blanker threshold and AGC constants of its own (all 32 rows of a workgroup different; unit gain
    beside other gains in every wave); audio filter tables, then AGC tables, that differ between channels 0..263 and 264..511 -- a cut
    inside a workgroup, with the table index ascending with the channel so that the group stays direct: the census is the proof."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("sc", F.agc_scenarios(), ids=lambda sc: sc.name)
def test_agc_regimes(gpu, ao, sc):
    """Hang counts 0, 1, 127, 128, 129, 255, 256 and 4,410 one per workgroup, all in every wave, and one channel per workgroup at 127;
    AGC modes 1..3; the default counter running out on a fresh bank.  Status after every block.  Which chain each workgroup takes in
    which block -- lean, general, quiet, and the changes between them -- is shown by tests/test_four_wave_scenarios.py."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("seed", F.CHANGING_SEEDS)
def test_settings_changing_on_a_running_bank(gpu, ao, seed):
    """Blanker off and on, USB -> AM -> CW -> USB, an unknown mode and back by broadcast; one channel's mode away for three blocks (no direct
    group meanwhile); non-key fields by broadcast or on single channels in between.  The census of every block follows the settings."""
    _run_scenario(gpu, ao, F.changing_scenario(seed))


@pytest.mark.parametrize("sc", F.edge_scenarios(), ids=lambda sc: sc.name)
def test_edge_inputs(gpu, ao, sc):
    """Full-scale squares, Nyquist alternation, DC, single spikes, -32768 and silence in USB, CW and AM with input gain 1 (the unit-gain
    short division, x = 0 included), 4, and both alternating by channel (no wave is all unit gain); int16 wrap at the output."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("sc", F.denormal_scenarios(), ids=lambda sc: sc.name)
def test_decay_into_denormals(gpu, ao, sc):
    """12 signal blocks, 400 silent ones, 12 signal blocks: 424 single-block launches of the four-wave kernels."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("sc", F.tap_scenarios(), ids=lambda sc: sc.name)
def test_stage_taps(gpu, ao, sc):
    """All 12 taps of every block on every 37th channel and the last one, through both instantiations, USB and AM."""
    _run_scenario(gpu, ao, sc)


@pytest.mark.parametrize("sc", F.geometry_scenarios(), ids=lambda sc: sc.name)
def test_geometry(gpu, ao, sc):
    """A last workgroup of 1, 2 or 3 waves; 64 whole waves beside a remainder wave on the general kernel; a direct group that starts at
    channel 512 behind 512 SAM channels (which take their own three launches), as launch constants and with one row changed."""
    _run_scenario(gpu, ao, sc)
