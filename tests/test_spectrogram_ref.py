"""tests/spectrogram_ref.py, the float64 restatement of include/asdr_spectrogram.h, held to an explicit-sum DFT and to known answers: a
bin-centre tone, DC and Nyquist, the frame count F(T) against a brute-force count, split invariance; the tolerance table of
tests/test_gpu_spectrogram.py recomputed; and two end-to-end usefulness checks on synthetic audio -- the spectrogram of a 4-FSK
signal with WSPR's symbol length and tone spacing at 12 kHz, and of an 8-FSK signal with FT8's at 12.8 kHz, returns the symbols."""
import numpy as np
import pytest

import spectrogram_ref as SR


def explicit(x, w, N, k0, B):
    n = np.arange(N, dtype=np.float64)
    v = np.asarray(x, dtype=np.float64) * np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.array([np.sum(v * np.exp(-2j * np.pi * k * n / N)) for k in range(k0, k0 + B)]) / N


@pytest.mark.parametrize("window", ["rect", "hann"])
def test_the_restatement_is_the_explicit_sum_at_128(window):
    rng = np.random.default_rng(1)
    N = 128
    w = SR.window(window, N)
    for k0, B in ((0, 65), (0, 1), (64, 1), (17, 30)):
        x = rng.integers(-32768, 32768, size=N).astype(np.int16)
        assert np.abs(SR.frames64(x, w, N, k0, B) - explicit(x, w, N, k0, B)).max() < 1e-9
    ref = SR.SpectrogramRef(2, N, 32, 17, 30, w, "complex")   # the bank cuts frame f at f H
    x = rng.integers(-32768, 32768, size=(2, 300)).astype(np.int16)
    X = ref.update(x)
    assert X.shape == (2, 6, 30)
    for c in range(2):
        for f in range(6):
            assert np.abs(X[c, f] - explicit(x[c, 32 * f:32 * f + N], w, N, 17, 30)).max() < 1e-9


def test_hann_is_formed_in_float64_and_rounded():
    for N in SR.SIZES:
        w = SR.window("hann", N)
        assert w.dtype == np.float32 and w[0] == 0.0 and w[N // 2] == 1.0 and np.array_equal(w[1:], w[:0:-1])
        assert (SR.window("rect", N) == 1.0).all()


@pytest.mark.parametrize("N", [128, 2048, 8192])
def test_a_bin_centre_tone_reads_a2_over_4_and_a2_over_16(N):
    A, k = 12000.0, N // 8 + 3
    x = A * np.cos(2 * np.pi * k * np.arange(N) / N + 0.3)
    for window, want in (("rect", A * A / 4), ("hann", A * A / 16)):
        X = SR.frames64(x, SR.window(window, N), N, k - 2, 5)
        p = X.real ** 2 + X.imag ** 2
        assert abs(p[2] - want) < 1e-6 * want
        assert (p[[0, 4]] < 1e-12 * want).all() and p[1] < (1e-12 if window == "rect" else 0.26) * want


def test_dc_and_nyquist_bins():
    N = 256
    dc, ny = np.full(N, -32768, dtype=np.int16), (32767 * (-1) ** np.arange(N)).astype(np.int16)
    rect, hann = SR.window("rect", N), SR.window("hann", N)
    assert np.allclose(SR.frames64(dc, rect, N, 0, 2), [-32768, 0], atol=1e-9)
    assert np.allclose(SR.frames64(ny, rect, N, N // 2 - 1, 2), [0, 32767], atol=1e-9)
    assert np.allclose(SR.frames64(dc, hann, N, 0, 3), [-16384, 8192, 0], atol=1e-2)
    assert np.allclose(SR.frames64(ny, hann, N, N // 2 - 2, 3), [0, -8191.75, 16383.5], atol=1e-2)
    assert SR.frames64(ny, rect, N, N // 2, 1).imag == 0 and SR.frames64(dc, rect, N, 0, 1).imag == 0


@pytest.mark.parametrize("N,H", [(128, 128), (128, 8), (128, 37), (1024, 64), (1024, 1024), (1024, 511), (8192, 512), (8192, 4097)])
def test_frame_count_against_a_brute_force_count(N, H):
    assert SR.accepted(N, H, 0, 1)
    for T in list(range(0, 3 * N + 5, 1 if N == 128 else 61)) + [N - 1, N, N + H - 1, N + H, 2**40 + 7]:
        brute = sum(1 for f in range(0, 3 * N // H + 8) if f * H + N <= T) if T < 2**40 else (T - N) // H + 1
        assert SR.frames_at(T, N, H) == brute


def test_parameter_ranges():
    assert SR.accepted(128, 8, 0, 65) and SR.accepted(8192, 8192, 4096, 1) and SR.accepted(8192, 512, 956, 137)
    for N, H, k0, B in ((64, 32, 0, 1), (16384, 8192, 0, 1), (1000, 500, 0, 1), (128, 7, 0, 1), (128, 129, 0, 1), (128, 64, 0, 66), (128, 64, 65, 1),
                        (128, 64, -1, 2), (128, 64, 0, 0)):
        assert not SR.accepted(N, H, k0, B)


@pytest.mark.parametrize("kind", ["power", "complex"])
def test_split_invariance_of_the_restatement(kind):
    rng = np.random.default_rng(3)
    n, N, H, total = 2, 256, 100, 1500
    x = rng.integers(-32768, 32768, size=(n, total)).astype(np.int16)
    whole = SR.SpectrogramRef(n, N, H, 3, 50, SR.window("hann", N), kind).update(x)
    assert whole.shape[1] == SR.frames_at(total, N, H) == 13
    for size in (1, 35, H, H + 1, N - 1):
        r = SR.SpectrogramRef(n, N, H, 3, 50, SR.window("hann", N), kind)
        parts = [r.update(x[:, a:a + size]) for a in range(0, total, size)]
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
        assert np.array_equal(r.state, x[:, -N:]) and r.T == total


def test_the_tolerance_table_is_what_the_model_gives():
    """EPS_A of tests/test_gpu_spectrogram.py, recomputed here to 10 %; its order of magnitude is that of float32 on peaks of
    hundreds to thousands."""
    import test_gpu_spectrogram as G
    assert sorted(G.EPS_A) == sorted((N, w) for N in SR.SIZES for w in ("rect", "hann"))
    for (N, w), eps in G.EPS_A.items():
        assert abs(G.compute_eps(N, w) - eps) <= 0.1 * eps, (N, w)
        assert 2e-4 < eps < 6e-3


def fsk(symbols, tones_hz, fs, n_sym, amplitude, rng, sigma):
    """Continuous-phase FSK as int16, in noise."""
    f = np.repeat(np.asarray(tones_hz, dtype=np.float64)[symbols], n_sym)
    phase = 2 * np.pi * np.cumsum(f) / fs
    return np.clip(np.rint(amplitude * np.cos(phase) + sigma * rng.standard_normal(f.size)), -32768, 32767).astype(np.int16)


def test_wspr_symbols_come_back_at_12_khz():
    """162 four-FSK symbols at 1 500 Hz + {0, 1, 2, 3} 12 000 / 8192 Hz, N = H = 8192: bin 1024 is 1 500 Hz exactly, and the
    per-frame arg-max over the four bins returns the symbols (amplitude 1 000 in noise of sigma 3 000)."""
    rng = np.random.default_rng(4)
    fs, N = 12000, 8192
    symbols = rng.integers(0, 4, size=162)
    assert 1500 * N % fs == 0 and 1500 * N // fs == 1024
    x = fsk(symbols, 1500 + np.arange(4) * fs / N, fs, N, 1000.0, rng, 3000.0)
    ref = SR.SpectrogramRef(1, N, N, 1024, 4, SR.window("rect", N), "power")
    p = np.concatenate([ref.update(part[None]) for part in np.array_split(x, 7)], axis=1)[0]
    assert p.shape == (162, 4) and np.array_equal(p.argmax(axis=1), symbols)


def test_ft8_symbols_come_back_at_12_8_khz():
    """79 eight-FSK symbols at 1 500 Hz + {0 .. 7} 6.25 Hz, 12 800 Hz (a resampler with U / M = 128 / 441), N = H = 2048."""
    rng = np.random.default_rng(5)
    fs, N = 12800, 2048
    symbols = rng.integers(0, 8, size=79)
    assert fs / N == 6.25 and 1500 * N // fs == 240 and 44100 * 128 == fs * 441
    x = fsk(symbols, 1500 + np.arange(8) * 6.25, fs, N, 1000.0, rng, 3000.0)
    ref = SR.SpectrogramRef(1, N, N, 240, 8, SR.window("rect", N), "power")
    p = ref.update(x[None])[0]
    assert p.shape == (79, 8) and np.array_equal(p.argmax(axis=1), symbols)
