"""tests/tuner_monitor_ref.py (the restatement of include/asdr_tuner.h, "Monitors") against known answers: tones on and between
bin centres under both windows, Parseval, grouping, the symmetry of a real source, the zeros before position 0, peak against sum,
and the levels against the unrounded stage 1 of tests/tuner_fastconv_ref.py."""
import numpy as np
import pytest

import tuner_fastconv_ref as F
import tuner_monitor_ref as M

R = 4
FS = 44100 * R
H, N, _ = F.sizes(R)


def tone(k, n, amp=1000.0, phase=0.3):
    """amp e^{j (2 pi k m / N + phase)}, complex [1][n] (k in bins of Fs_in / N, any real)."""
    return (amp * np.exp(1j * (2 * np.pi * k * np.arange(n) / N + phase)))[None, :]


def mon(n_bins=N, window="rect", mode="sum", n_src=1, **kw):
    return M.MonitorRef(F.TunerFastconvRef(1, n_src, FS, R), n_bins, window, mode, **kw)


def test_bin_centred_tone_under_both_windows():
    A, k = 1000.0, 37
    for window in M.WINDOWS:
        m = mon(window=window)
        frames = m.update(tone(k, 5 * H, A))
        for P, _ in frames[2:]:                               # from the third frame on the window is all tone
            rest = np.ones(N, bool)
            if window == "rect":
                assert abs(P[0, k] - A * A) <= 1e-12 * A * A
                rest[k] = False
            else:
                assert abs(P[0, k] - A * A / 4) <= 1e-12 * A * A
                assert abs(P[0, k - 1] - A * A / 16) <= 1e-12 * A * A and abs(P[0, k + 1] - A * A / 16) <= 1e-12 * A * A
                rest[k - 1:k + 2] = False
            assert P[0, rest].max() < 1e-20 * A * A


def test_hann_side_lobes_fall_40_db_below_rect_ten_bins_from_a_tone_between_bins():
    k = 100.5
    P = {w: mon(window=w).update(tone(k, 3 * H))[2][0][0] for w in M.WINDOWS}
    # closed forms: the rect kernel |sin(pi d) / (N sin(pi d / N))|, the hann kernel its three-term combine, at offset d bins
    def dirichlet(d):
        return np.exp(1j * np.pi * d * (N - 1) / N) * np.sin(np.pi * d) / (N * np.sin(np.pi * d / N))
    for j in (110, 111, 90):
        d = k - j
        rect = abs(dirichlet(d)) ** 2
        hann = abs(dirichlet(d) / 2 - (dirichlet(d + 1) + dirichlet(d - 1)) / 4) ** 2
        assert abs(P["rect"][j] / 1e6 - rect) <= 1e-9 * rect and abs(P["hann"][j] / 1e6 - hann) <= 1e-6 * hann
        assert 10 * np.log10(hann / rect) <= -40.0
        assert 10 * np.log10(P["hann"][j] / P["rect"][j]) <= -40.0


def test_parseval_and_grouping():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 4 * H)) * 3000 + 1j * rng.standard_normal((2, 4 * H)) * 3000
    full = {w: mon(window=w, n_src=2).update(x) for w in M.WINDOWS}
    for f in range(4):
        win = np.concatenate([np.zeros((2, H)) if f == 0 else x[:, (f - 1) * H:f * H], x[:, f * H:(f + 1) * H]], axis=1)
        mean = (np.abs(win) ** 2).mean(axis=1)
        assert np.allclose(full["rect"][f][0].sum(axis=1), mean, rtol=1e-12, atol=0)
    for w in M.WINDOWS:
        for B in (256, 512, N // 2):
            grouped = mon(B, w, n_src=2).update(x)
            for f in range(4):
                want = full[w][f][0].reshape(2, B, N // B).sum(axis=2)
                assert np.allclose(grouped[f][0], want, rtol=1e-12, atol=0)


def test_real_source_is_symmetric():
    rng = np.random.default_rng(2)
    x = rng.integers(-20000, 20000, size=(1, 3 * H)).astype(np.float64) + 0j
    for w in M.WINDOWS:
        for P, _ in mon(window=w).update(x):
            assert np.allclose(P[0], P[0][(N - np.arange(N)) % N], rtol=1e-12, atol=1e-12 * P.max())


def test_first_frame_sees_the_zeros_before_position_0():
    frames = mon().update(tone(9, 2 * H))
    assert abs(frames[0][0].sum() / frames[1][0].sum() - 0.5) <= 1e-12


def test_peak_is_at_least_the_mean_and_accumulation_follows_the_modes():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 6 * H)) * 100 + tone(50.3, 6 * H, 500.0)
    s, p = mon(256, "hann", "sum"), mon(256, "hann", "peak")
    fs = s.update(x[:, :2 * H]) + s.update(x[:, 2 * H:])
    p.update(x)
    assert s.frames == p.frames == 6
    assert np.array_equal(s.acc, sum(P for P, _ in fs)) or np.allclose(s.acc, sum(P for P, _ in fs), rtol=1e-15)
    assert np.array_equal(p.acc, np.maximum.reduce([P for P, _ in fs]))
    assert (p.acc >= s.acc / s.frames).all()
    assert np.allclose(s.amplitude(), np.sqrt(s.acc / 6)) and np.allclose(p.amplitude(), np.sqrt(p.acc))
    s.clear_spectrum()
    assert s.frames == 0 and not s.acc.any()


@pytest.mark.parametrize("g", [None, [1.0]])
def test_level_is_the_energy_of_the_unrounded_stage_1(g):
    rng = np.random.default_rng(4)
    fws = [0, 0x12345678, 0x9E3779B9, (1 << 31) + 12345]
    ref = F.TunerFastconvRef(len(fws), 2, FS, R, g=g)
    for c, fw in enumerate(fws):
        ref.set_source(c % 2, ch=c); ref.set_frequency_word(fw, ch=c)
    m = M.MonitorRef(ref, levels=True)
    total = np.zeros(len(fws))
    for nf in (1, 3):
        iq = rng.integers(-20000, 20000, size=(2, nf * H, 2))
        m.update(iq)
        z = ref.update(iq, keep_float=True)[2]
        total += (np.abs(z) ** 2).sum(axis=1)
    assert m.level_frames == 4
    assert np.allclose(m.level, total, rtol=1e-9, atol=0)
    assert np.allclose(m.rms(), np.sqrt(total / (128 * 4)), rtol=1e-9)


def test_f32_model_stays_close_and_frequencies():
    import scipy.fft
    rng = np.random.default_rng(5)
    win = (rng.integers(-20000, 20000, size=(1, N)) + 1j * rng.integers(-20000, 20000, size=(1, N))).astype(np.complex128)
    X32 = scipy.fft.fft(win.astype(np.complex64), axis=1)
    for w in M.WINDOWS:
        a, b = M.powers(np.fft.fft(win, axis=1), 256, w), M.powers(X32, 256, w, f32=True)
        assert np.abs(np.sqrt(a) - np.sqrt(b)).max() < 1e-2
    f = M.frequencies(FS, 256)
    assert f[0] == 0 and f[1] == FS / 256 and f[128] == -FS / 2 and f[255] == -FS / 256
