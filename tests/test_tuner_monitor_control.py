"""The monitors' control plane (include/asdr_tuner.h, "Monitors") on ASDR_NO_DEVICE banks: argument checks that keep the old
configuration, the getters, direct-form and rate banks refusing with a message, reads failing without a device, the exports, the
frequency helper, and a check that the new sources name no scalar memory-write instruction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

NEW = ["asdr_tuner_spectrum_enable", "asdr_tuner_spectrum_bins", "asdr_tuner_spectrum_window", "asdr_tuner_spectrum_mode",
       "asdr_tuner_spectrum_read", "asdr_tuner_spectrum_device", "asdr_tuner_spectrum_frames", "asdr_tuner_spectrum_clear",
       "asdr_tuner_levels_enable", "asdr_tuner_levels_enabled", "asdr_tuner_levels_read", "asdr_tuner_levels_device",
       "asdr_tuner_levels_frames", "asdr_tuner_levels_clear"]


@pytest.fixture
def T(A):
    return lambda fs=2400000, R=16, n=4, s=2: A.TunerBank.fastconv(n, s, fs, R, device=A.NO_DEVICE)


def test_every_newly_declared_function_is_exported(A):
    with open(os.path.join(ROOT, "include", "asdr_tuner.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(asdr_tuner_(?:spectrum|levels)_\w+)\s*\(", text))
    assert declared == set(NEW)
    L = C.CDLL(A.library_path())
    assert [n for n in NEW if not hasattr(L, n) or n not in A.TUNER_EXPORTS] == []
    for name, value in (("ASDR_TUNER_WIN_RECT", 0), ("ASDR_TUNER_WIN_HANN", 1), ("ASDR_TUNER_MON_SUM", 0), ("ASDR_TUNER_MON_PEAK", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), text)


def test_monitors_are_off_at_creation_and_enable_sets_the_getters(A, T):
    t = T()
    assert t.spectrum_bins() == 0 and t.spectrum_config() is None and not t.levels_enabled()
    assert t.spectrum_frames() == -1 and t.levels_frames() == -1
    t.enable_spectrum(4096)
    assert t.spectrum_bins() == 4096 and t.spectrum_config() == (4096, "hann", "sum") and t.spectrum_frames() == 0
    t.enable_spectrum(256, "rect", "peak")
    assert t.spectrum_config() == (256, "rect", "peak")
    t.enable_spectrum(t.fft_size(), window=A.tuner.SPECTRUM_WINDOWS["hann"], mode=A.tuner.SPECTRUM_MODES["peak"])
    assert t.spectrum_config() == (4096, "hann", "peak")
    t.enable_levels()
    assert t.levels_enabled() and t.levels_frames() == 0
    t.reset()                                                   # reset keeps the configuration
    assert t.spectrum_config() == (4096, "hann", "peak") and t.levels_enabled()
    t.set_frequency(1000.0); t.set_channel_filter(np.ones(3, np.float32)); t.set_input_format("cu8")
    assert t.spectrum_config() == (4096, "hann", "peak") and t.levels_enabled()
    t.enable_spectrum(0)
    t.enable_levels(False)
    assert t.spectrum_bins() == 0 and t.spectrum_config() is None and not t.levels_enabled()


def test_rejected_arguments_keep_the_old_configuration(A, T):
    t = T()
    t.enable_spectrum(1024, "rect", "peak")
    for bins in (128, 255, 300, 1000, 8192, -256, 1 << 20):
        with pytest.raises(A.AsdrError, match="power of two"):
            t.enable_spectrum(bins)
        assert t.spectrum_config() == (1024, "rect", "peak")
    for window in (2, -1, "hamming"):
        with pytest.raises(A.AsdrError, match="window"):
            t.enable_spectrum(512, window=window)
        assert t.spectrum_config() == (1024, "rect", "peak")
    for mode in (2, -1, "mean"):
        with pytest.raises(A.AsdrError, match="mode"):
            t.enable_spectrum(512, mode=mode)
        assert t.spectrum_config() == (1024, "rect", "peak")
    small = T(44100 * 2, 2)                                     # N = 512: B is 256 or 512
    small.enable_spectrum(512); small.enable_spectrum(256)
    with pytest.raises(A.AsdrError, match="256..512"):
        small.enable_spectrum(1024)
    assert small.spectrum_bins() == 256


def test_direct_form_and_rate_banks_refuse_with_a_message(A):
    for d in (A.TunerBank(2, 1, 4, device=A.NO_DEVICE), A.TunerBank(2, 1, 50, fs_in=2400000, device=A.NO_DEVICE)):
        for call in (lambda: d.enable_spectrum(256), lambda: d.enable_spectrum(0), d.spectrum, d.clear_spectrum, d.spectrum_tensor,
                     d.enable_levels, lambda: d.enable_levels(False), d.levels, d.clear_levels, d.levels_tensor):
            with pytest.raises(A.AsdrError, match="fast-convolution"):
                call()
        assert d.spectrum_bins() == 0 and not d.levels_enabled() and d.spectrum_frames() == -1 and d.levels_frames() == -1


def test_reads_fail_without_a_device_and_when_off(A, T):
    t = T()
    for call in (t.spectrum, t.clear_spectrum, t.spectrum_tensor):
        with pytest.raises(A.AsdrError, match="spectrum monitor is off"):
            call()
    for call in (t.levels, t.clear_levels, t.levels_tensor):
        with pytest.raises(A.AsdrError, match="level monitor is off"):
            call()
    t.enable_spectrum(256); t.enable_levels()
    for call in (t.spectrum, t.clear_spectrum, t.spectrum_tensor, t.levels, t.clear_levels, t.levels_tensor):
        with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
            call()
    L = t._L
    assert L.asdr_tuner_spectrum_enable(None, 256, 0, 0) == -1 and b"null tuner bank" in L.asdr_last_error()
    assert L.asdr_tuner_levels_read(None, None, None, 0) == -1 and L.asdr_tuner_spectrum_device(None) is None
    assert L.asdr_tuner_spectrum_bins(None) == 0 and L.asdr_tuner_levels_enabled(None) == 0


def test_spectrum_frequencies(A):
    f = A.spectrum_frequencies(2400000, 256)
    assert f.dtype == np.float64 and f.shape == (256,)
    assert f[0] == 0.0 and f[1] == 9375.0 and f[127] == 127 * 9375.0 and f[128] == -1200000.0 and f[255] == -9375.0


def test_new_sources_name_no_scalar_memory_write():
    """The monitors write with vector stores only: no scalar store, scalar atomic or scalar cache write-back by name."""
    words = re.compile(r"s_(?:buffer_|scratch_)?store|s_(?:buffer_)?atomic|s_dcache_(?:wb|discard)", re.I)
    for rel in ("audiosdr_amd/csrc/asdr_tuner_monitor.hip", "audiosdr_amd/csrc/asdr_tuner_device.h", "audiosdr_amd/tuner.py",
                "tests/tuner_monitor_ref.py"):
        with open(os.path.join(ROOT, rel)) as f:
            assert not words.search(f.read()), rel
