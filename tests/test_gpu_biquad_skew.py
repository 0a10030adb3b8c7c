"""The biquad pipelines of the plain kind on the cases chosen for the pipeline with ONE SAMPLE of stage skew (biquad_pipe_skew1: what the
audio cascades run; the IF band-pass and the AM image filter keep the chunked form and run the same cases): the fill and drain slots carrying
the only non-zero samples, every audio table, a table change inside a workgroup, state running down through the denormals.
Against the oracle at tolerance 0, in the style of tests/test_gpu_four_wave.py: single-block calls, the launch census asserted
for every block (what is compared is asdr_update_kernel_mw_u / asdr_update_kernel_mw, or asdr_update_kernel_one for the small bank, never a
fall-back), the int16 audio of every channel and block, and the stage taps (IF_I, IF_Q and AUDIO_FILT among them) as bit patterns on every
37th channel where a scenario takes them.  Banks of 512 channels (64 waves: the smallest that reach the four-wave form) and 520 (a partial
last workgroup)."""
import numpy as np
import pytest

import four_wave_scenarios as F
from cases import USB, AM, imp, am
from helpers import S
from test_gpu_four_wave import _run_scenario

pytestmark = pytest.mark.gpu

ONE = "asdr_update_kernel_one"
C2 = [S("setDemodMode", USB), S("enableAudioFilter")]            # bench.py's configure_c2: blanker and AGC are on by default
BANKS = (512, 520)
AUDIO_TABLES = tuple(range(10))                                  # setAudioFilter's ids (10 is the bypass value: no cascade runs)


def _rows(total, sig=imp, **kw):
    return lambda: F.signal_rows(total, sig, impulse_every=300, **kw)


@pytest.mark.parametrize("n", BANKS)
def test_c2_by_broadcast(gpu, ao, n):
    """case 1: C2 settings by broadcast (launch constants), 6 blocks, all taps on every 37th channel"""
    _run_scenario(gpu, ao, F.Scenario("c2-uniform-%d" % n, _rows(6), C2, n=n, taps=True))


@pytest.mark.parametrize("n", BANKS)
def test_c2_one_row_changed(gpu, ao, n):
    """case 2: one field of one channel in the middle of a workgroup changed: the row-reading form"""
    _run_scenario(gpu, ao, F.Scenario("c2-rows-%d" % n, _rows(6), C2 + [S("setOutputGain", 0.7, sel=F.MID)], n=n, expect="r", taps=True))


@pytest.mark.parametrize("table", AUDIO_TABLES)
def test_every_audio_table(gpu, ao, table):
    """case 3: every audio filter table through the audio duty's cascades"""
    _run_scenario(gpu, ao, F.Scenario("audio-table-%d" % table, _rows(3), C2 + [S("setAudioFilter", table)], taps=True))


@pytest.mark.parametrize("n", BANKS)
def test_audio_table_changes_inside_a_workgroup(gpu, ao, n):
    """case 3: the audio table changes at channel 264 (a multiple of 8, not of 32); the indices ascend, so the group stays direct"""
    setup = C2 + [S("setAudioFilter", 3, sel=lambda c: c < F.CUT), S("setAudioFilter", 8, sel=lambda c: c >= F.CUT)]
    _run_scenario(gpu, ao, F.Scenario("audio-table-cut-%d" % n, _rows(3), setup, n=n, expect="r", taps=True))


@pytest.mark.parametrize("n", BANKS)
def test_am(gpu, ao, n):
    """case 4: AM: the image cascades run beside the audio cascades"""
    _run_scenario(gpu, ao, F.Scenario("am-%d" % n, _rows(3, am), [S("setDemodMode", AM), S("enableAudioFilter")], n=n, taps=True))


def _edge_rows(total=4, U=12):
    """zero except at samples 0..2 and 125..127 of each block: one of the six alone in rows 0..5, all six in the others; values of their own"""
    rng = np.random.default_rng(77)
    pos = [0, 1, 2, 125, 126, 127]
    I = np.zeros((U, total, 128), np.int16); Q = np.zeros((U, total, 128), np.int16)
    for r in range(U):
        for p in ([pos[r]] if r < 6 else pos):
            I[r, :, p] = rng.integers(-30000, 30000, total); Q[r, :, p] = rng.integers(-30000, 30000, total)
    return I, Q


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("n", BANKS)
def test_edge_samples(gpu, ao, n, gain):
    """case 5: the fill and drain slots carry the only non-zero samples; blanker off, so the block the filter sees is the block sent"""
    setup = C2 + [S("disableNoiseBlanker"), S("setInputGain", gain)]
    _run_scenario(gpu, ao, F.Scenario("edges-%d-gain%g" % (n, gain), _edge_rows, setup, n=n, taps=True))


def _decay_rows(total=64):
    from audiosdr_amd.synth import make_iq
    I, Q = make_iq(4, 1, fc=6290.0 + 25.0 * np.arange(4), A=0.9, m=0.5)
    Z = np.zeros((4, total - 1, 128), np.int16)
    return np.concatenate([I, Z], axis=1), np.concatenate([Q, Z], axis=1)


@pytest.mark.parametrize("n", BANKS)
def test_decay_into_denormals(gpu, ao, n):
    """case 6: one loud block, then 63 silent ones: the IF cascades' state runs down into the denormals (from block 16 on) and stays there"""
    _run_scenario(gpu, ao, F.Scenario("decay-%d" % n, _decay_rows, C2, n=n))


@pytest.mark.parametrize("n", [24, 64])
def test_small_bank_on_the_one_wave_kernel(gpu, ao, n):
    """asdr_update_kernel_one takes the same routine: C2 settings, 4 blocks"""
    _run_scenario(gpu, ao, F.Scenario("c2-one-%d" % n, _rows(4), C2, n=n, expect={ONE: 1}, uniform_groups=1, taps=True))
