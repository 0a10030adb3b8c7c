"""The audio spectrogram's control plane (include/asdr_spectrogram.h) on an ASDR_NO_DEVICE spectrogram: the exported names, the
refusals of sizes, hops, bands, windows, channels and positions (each leaves everything as it was), the getters, the frame
arithmetic at large T, the state calls on the host copy, and the call that needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import spectrogram_ref as SR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def make(A, n=4, N=1024, H=512, k0=0, B=None, **kw):
    return A.AudioSpectrogram(n, n_fft=N, hop=H, first_bin=k0, n_bins=B, device=A.NO_DEVICE, **kw)


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_spectrogram.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_spectrogram_\w+)\s*\(", text)))
    assert len(declared) == 20 and "asdr_spectrogram_update_device" in declared and "asdr_spectrogram_set_window" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.SPECTROGRAM_EXPORTS) == declared
    others = (set(A.binding.EXPORTS) | set(A.GATE_EXPORTS) | set(A.TUNER_EXPORTS) | set(A.FRONT_EXPORTS) | set(A.RESAMPLE_EXPORTS)
              | set(A.CODEC_EXPORTS))
    assert not [n for n in A.SPECTROGRAM_EXPORTS if n in others]
    assert A.SPECTROGRAM_SIZES == SR.SIZES and A.SPECTROGRAM_MAX_SAMPLES == SR.MAX_SAMPLES
    assert A.SPECTROGRAM_WINDOWS == ("rect", "hann", "custom") and A.SPECTROGRAM_KINDS == ("power", "complex")


def test_creation_values_and_getters(A):
    s = make(A, n=5, N=8192, H=4096, k0=956, B=137, window="hann", kind="power")
    L, h = s._L, s._h
    assert (s.n_channels, s.n_fft, s.hop, s.first_bin, s.n_bins, s.kind, s.window_kind, s.frame_floats) == (5, 8192, 4096, 956, 137, "power", "hann", 137)
    assert (L.asdr_spectrogram_n_channels(h), L.asdr_spectrogram_n_fft(h), L.asdr_spectrogram_hop(h), L.asdr_spectrogram_first_bin(h),
            L.asdr_spectrogram_n_bins(h), L.asdr_spectrogram_window_kind(h), L.asdr_spectrogram_output_kind(h)) == (5, 8192, 4096, 956, 137, 1, 0)
    assert np.array_equal(s.get_window(), SR.window("hann", 8192))
    assert s.position() == 0 and s.frame_position() == 0 and s.read_state().shape == (5, 8192) and not s.read_state().any()
    hz = s.bin_hz(12000)
    assert hz.shape == (137,) and hz[0] == 956 * 12000 / 8192 and abs(hz[68] - 1500.0) == 0 and hz[1] - hz[0] == 12000 / 8192
    s.close()
    d = make(A, N=256, H=16, kind="complex", window="rect")     # the defaults of the band: all N / 2 + 1 bins
    assert (d.first_bin, d.n_bins, d.frame_floats, d.kind, d.window_kind) == (0, 129, 258, "complex", "rect") and (d.get_window() == 1).all()
    d.close()
    for N in SR.SIZES:                                          # every size, both ends of the hop
        for H in (N // 16, N):
            s = make(A, N=N, H=H, k0=N // 2, B=1)
            assert (s.n_fft, s.hop, s.first_bin, s.n_bins) == (N, H, N // 2, 1)
            s.close()
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            make(A, n=n)


def test_parameters_are_refused(A):
    for N in (0, 64, 100, 127, 129, 1000, 3000, 16384, -1024):
        with pytest.raises(A.AsdrError, match="power of two in 128..8192"):
            make(A, N=N, H=max(N // 2, 1), B=1)
    for N, H in ((1024, 63), (1024, 1025), (1024, 0), (1024, -512), (128, 7), (8192, 511)):
        assert not SR.accepted(N, H, 0, 1)
        with pytest.raises(A.AsdrError, match="hop"):
            make(A, N=N, H=H)
    for k0, B in ((0, 514), (513, 1), (512, 2), (-1, 5), (0, 0), (3, -1), (2**30, 2**30)):
        assert not SR.accepted(1024, 512, k0, B)
        with pytest.raises(A.AsdrError, match="band"):
            make(A, k0=k0, B=B)
    with pytest.raises(A.AsdrError, match="window"):
        make(A, window="blackman")
    with pytest.raises(A.AsdrError, match="window"):
        make(A, window="custom")                                # custom is what set_window makes, not a creation value
    with pytest.raises(A.AsdrError, match="kind"):
        make(A, kind="db")
    L = make(A)._L
    assert not L.asdr_spectrogram_create(1, 1024, 512, 0, 1, 0, 2, A.NO_DEVICE) and b"kind" in L.asdr_last_error()
    assert not L.asdr_spectrogram_create(1, 1024, 512, 0, 1, 3, 0, A.NO_DEVICE) and b"window" in L.asdr_last_error()


def test_windows_are_refused_and_a_refusal_changes_nothing(A):
    N = 256
    s = make(A, N=N, H=64, window="hann")
    good = np.linspace(-2.0, 3.0, N).astype(np.float32)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy(); bad[N - 1] = bad_value
        with pytest.raises(A.AsdrError, match="255 is not finite"):
            s.set_window(bad)
        with pytest.raises(A.AsdrError, match="not finite"):
            make(A, N=N, H=64, window=bad)
    with pytest.raises(A.AsdrError, match="values for"):
        s.set_window(good[:-1])
    assert s.window_kind == "hann" and np.array_equal(s.get_window(), SR.window("hann", N))
    rec = np.arange(4 * N, dtype=np.int16).reshape(4, N)
    s.write_state(rec); s.set_position(777)
    s.set_window(good)                                          # keeps the records and the position
    assert s.window_kind == "custom" and np.array_equal(s.get_window(), good) and s.position() == 777 and np.array_equal(s.read_state(), rec)
    c = make(A, N=N, H=64, window=good)
    assert c.window_kind == "custom" and np.array_equal(c.get_window(), good)
    s.close(); c.close()


@pytest.mark.parametrize("N,H", [(128, 8), (1024, 511), (8192, 4096), (8192, 8192)])
@pytest.mark.parametrize("t0", [0, 5, 2**31 - 1, 2**32, 2**40 + 3, 2**50])
def test_position_arithmetic(A, N, H, t0):
    s = make(A, n=1, N=N, H=H)
    s.set_position(t0)
    assert s.position() == t0 and s.frame_position() == SR.frames_at(t0, N, H)
    for ns in (0, 1, 35, H - 1, H, N - 1, N, 120000, 2**24):
        assert s.out_frames(ns) == SR.frames_at(t0 + ns, N, H) - SR.frames_at(t0, N, H)
    assert s.position() == t0                                   # out_frames moves nothing
    for bad in (-1, 2**50 + 1, 2**62):
        with pytest.raises(A.AsdrError, match="position"):
            s.set_position(bad)
    for bad in (-1, 2**24 + 1):
        with pytest.raises(A.AsdrError, match="n_samples"):
            s.out_frames(bad)
    assert s.position() == t0 and s.frame_position() == SR.frames_at(t0, N, H)
    s.reset()
    assert s.position() == 0 and s.frame_position() == 0
    s.close()


def test_state_calls_work_on_the_host_copy(A):
    rng = np.random.default_rng(2)
    N = 512
    s = make(A, n=6, N=N, H=100, k0=7, B=9, window="rect", kind="complex")
    rec = rng.integers(-32768, 32768, size=(3, N)).astype(np.int16)
    s.write_state(rec, channels=[5, 0, 2])
    want = np.zeros((6, N), dtype=np.int16)
    want[[5, 0, 2]] = rec
    assert np.array_equal(s.read_state(), want)
    other = rng.integers(-32768, 32768, size=(3, N)).astype(np.int16)
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):      # a bad channel: no record is written
        with pytest.raises(A.AsdrError, match="bad channel"):
            s.write_state(other, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        s.write_state(np.zeros((7, N), dtype=np.int16))
    with pytest.raises(A.AsdrError, match="records for"):
        s.write_state(other, channels=[1, 2])
    assert np.array_equal(s.read_state(), want)
    s.write_state(other[:2])                                    # channels 0, 1
    want[:2] = other[:2]
    assert np.array_equal(s.read_state(), want)
    s.set_position(12345)
    moved = make(A, n=6, N=N, H=512, window="hann")             # a record depends on N alone
    moved.write_state(s.read_state())
    assert np.array_equal(moved.read_state(), want) and moved.position() == 0
    s.reset()
    assert not s.read_state().any() and s.position() == 0
    assert (s.n_fft, s.hop, s.first_bin, s.n_bins, s.kind, s.window_kind) == (N, 100, 7, 9, "complex", "rect")   # reset keeps the parameters
    s.synchronize()
    s.close(); moved.close()


def test_the_signal_path_needs_a_device(A):
    s = make(A, n=3)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        s.update_device(4096, 1024, 8192, 64)
    assert s.position() == 0
    L = s._L
    assert L.asdr_spectrogram_n_channels(None) == -1 and L.asdr_spectrogram_position(None) == -1 and L.asdr_spectrogram_n_fft(None) == -1
    assert L.asdr_spectrogram_frame_position(None) == -1 and L.asdr_spectrogram_reset(None) == -1 and L.asdr_spectrogram_out_frames(None, 5) == -1
    s.close()


def test_the_decoder_rates_feed_whole_symbols(A):
    """12 000 Hz with N = 8192 is a WSPR symbol; the resampler's default recipe at 12 800 Hz (U / M = 128 / 441) exists, and N = 2048
    there is an FT8 symbol with bins 6.25 Hz apart."""
    r = A.AudioResampler(1, fs_out=12800, device=A.NO_DEVICE)
    assert (r.up, r.down, r.fs_out) == (128, 441, 12800.0)
    r.close()
    s = make(A, n=1, N=2048, H=2048, k0=240, B=8, window="rect")
    assert np.array_equal(s.bin_hz(12800), 1500 + 6.25 * np.arange(8))
    s.close()
    s = make(A, n=1, N=8192, H=8192, k0=1024, B=4, window="rect")
    assert np.array_equal(s.bin_hz(12000), 1500 + 12000 / 8192 * np.arange(4))
    s.close()
