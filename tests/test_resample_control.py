"""The audio resampler's control plane (include/asdr_resample.h) on an ASDR_NO_DEVICE resampler: the exported names, the refusals
of rates and filters (each leaves everything as it was), the position arithmetic at large N, the state calls on the host copy, and
the calls that need a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import resample_ref as RR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def custom(A, up, down, taps, shift=15, n=4):
    return A.AudioResampler(n, device=A.NO_DEVICE, up=up, down=down, taps=taps, shift=shift)


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_resample.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_resampler_\w+)\s*\(", text)))
    assert len(declared) == 19 and "asdr_resampler_update_device" in declared and "asdr_resampler_create_custom" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.RESAMPLE_EXPORTS) == declared
    others = set(A.binding.EXPORTS) | set(A.GATE_EXPORTS) | set(A.TUNER_EXPORTS) | set(A.FRONT_EXPORTS)
    assert not [n for n in A.RESAMPLE_EXPORTS if n in others]
    assert A.RESAMPLE_STATE_SAMPLES == RR.STATE == 256 and A.RESAMPLE_FS_IN == RR.FS_IN and A.RESAMPLE_DEFAULT_RATES == RR.DEFAULT_RATES


def test_creation_values(A):
    r = A.AudioResampler(5, fs_out=12000, device=A.NO_DEVICE)
    assert (r.n_channels, r.up, r.down, r.taps_per_phase()) == (5, 40, 147, 116) and r._L.asdr_resampler_n_channels(r._h) == 5
    assert r.fs_out == 12000.0 and r.position() == 0 and r.output_position() == 0
    assert not r.read_state().any() and r.read_state().shape == (5, 256)
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.AudioResampler(n, device=A.NO_DEVICE)
    r.close()


def test_rates_are_refused(A):
    one = np.array([16384], dtype=np.int16)
    for fs, why in ((48000, "interpolation"), (44101, "interpolation"), (0, "positive"), (-8000, "positive"), (2000, "16 U"), (44099, "1..512")):
        with pytest.raises(A.AsdrError, match=why):
            A.AudioResampler(2, fs_out=fs, device=A.NO_DEVICE)
    for up, down, why in ((2, 1, "interpolation"), (513, 600, "1..512"), (0, 4, "1..512"), (1, 17, "16 U"), (512, 8193, "16 U")):
        with pytest.raises(A.AsdrError, match=why):
            custom(A, up, down, np.tile(one, max(up, 1)))
    for up, down in ((1, 1), (1, 16), (512, 512), (512, 8192), (3, 4)):           # the corners are accepted
        r = custom(A, up, down, np.tile(one, up))
        assert (r.up, r.down, r.taps_per_phase()) == (up, down, 1)
        r.close()


def test_filters_are_refused_and_a_refusal_changes_nothing(A):
    up, down = 3, 4
    good = np.zeros(up * 256, dtype=np.int16)                                     # K = 256 is accepted
    good[0::3] = 255                                                              # phase 0: 256 * 255 = 65280
    good[1], good[4] = 32767, -32768                                              # phase 1: 32767 + 32768 = 65535 exactly
    assert RR.accepted(up, down, good, 7)
    r = custom(A, up, down, good, shift=7)
    assert r.taps_per_phase() == 256 and np.array_equal(r.get_taps()[0], good) and r.get_taps()[1] == 7
    over = good.copy(); over[7] = 1                                               # phase 1: 65536
    assert not RR.accepted(up, down, over, 7)
    with pytest.raises(A.AsdrError, match="65536 > 65535"):
        custom(A, up, down, over)
    with pytest.raises(A.AsdrError, match="65536 > 65535"):
        r.set_filter(over, shift=7)
    with pytest.raises(A.AsdrError, match="1..256"):
        r.set_filter(np.zeros(up * 257, dtype=np.int16))
    with pytest.raises(A.AsdrError, match="1..256"):
        custom(A, up, down, np.zeros(up * 257, dtype=np.int16))
    for shift in (-1, 16):
        with pytest.raises(A.AsdrError, match="shift"):
            r.set_filter(good, shift=shift)
    with pytest.raises(A.AsdrError, match="taps"):
        r.set_filter(np.zeros(up * 2 + 1, dtype=np.int16))                        # not a multiple of U
    assert np.array_equal(r.get_taps()[0], good) and r.get_taps()[1] == 7 and r.taps_per_phase() == 256
    short = np.array([100, -200, 300], dtype=np.int16)
    r.set_filter(short, shift=0)
    assert r.taps_per_phase() == 1 and r.get_taps()[0].tolist() == [100, -200, 300] and r.get_taps()[1] == 0 and r.delay() == (3 - 1) / 6.0
    r.close()


@pytest.mark.parametrize("fs", [12000, 8000, 11025])
@pytest.mark.parametrize("n0", [0, 2**31 - 1, 2**32, 2**40, 2**50])
def test_position_arithmetic(A, fs, n0):
    r = A.AudioResampler(1, fs_out=fs, device=A.NO_DEVICE)
    up, down = RR.ratio(fs)
    r.set_position(n0)
    assert r.position() == n0 and r.output_position() == RR.ceil_div(n0 * up, down)
    for nb in (0, 1, 7, 646, 65535):
        j0, j1 = RR.out_range(n0, n0 + 128 * nb, up, down)
        assert r.out_samples(nb) == j1 - j0
    assert r.position() == n0                                                     # out_samples moves nothing
    for bad in (-1, 2**50 + 1, 2**62):
        with pytest.raises(A.AsdrError, match="position"):
            r.set_position(bad)
    with pytest.raises(A.AsdrError, match="n_blocks"):
        r.out_samples(65536)
    assert r.position() == n0
    r.reset()
    assert r.position() == 0 and r.output_position() == 0
    r.close()


def test_state_calls_work_on_the_host_copy(A):
    rng = np.random.default_rng(2)
    r = A.AudioResampler(6, fs_out=8000, device=A.NO_DEVICE)
    rec = rng.integers(-32768, 32768, size=(3, 256)).astype(np.int16)
    r.write_state(rec, channels=[5, 0, 2])
    want = np.zeros((6, 256), dtype=np.int16)
    want[[5, 0, 2]] = rec
    assert np.array_equal(r.read_state(), want)
    other = rng.integers(-32768, 32768, size=(3, 256)).astype(np.int16)
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):                        # a bad channel: no record is written
        with pytest.raises(A.AsdrError, match="bad channel"):
            r.write_state(other, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        r.write_state(np.zeros((7, 256), dtype=np.int16))
    with pytest.raises(A.AsdrError, match="records for"):
        r.write_state(other, channels=[1, 2])
    assert np.array_equal(r.read_state(), want)
    r.write_state(other[:2])                                                      # channels 0, 1
    want[:2] = other[:2]
    assert np.array_equal(r.read_state(), want)
    r.set_position(12345 * 128)
    moved = A.AudioResampler(6, fs_out=12000, device=A.NO_DEVICE)                 # a record does not depend on the rate
    moved.write_state(r.read_state())
    assert np.array_equal(moved.read_state(), want)
    r.reset()
    assert not r.read_state().any() and r.position() == 0 and r.taps_per_phase() == 174
    r.synchronize()
    r.close(); moved.close()


def test_the_signal_path_needs_a_device(A):
    r = A.AudioResampler(3, device=A.NO_DEVICE)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        r.update_device(4096, 1, 8192, 64)
    assert r.position() == 0
    L = r._L
    assert L.asdr_resampler_n_channels(None) == -1 and L.asdr_resampler_position(None) == -1 and L.asdr_resampler_up(None) == -1
    assert math.isnan(L.asdr_resampler_delay(None)) and L.asdr_resampler_reset(None) == -1
    r.close()
