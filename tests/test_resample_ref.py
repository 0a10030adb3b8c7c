"""tests/resample_ref.py against itself and against the header's numbers (include/asdr_resample.h): the vectorised restatement
against an explicit per-output loop, splitting invariance, the per-call counts, the known answers of the default 12 kHz and 8 kHz
filters, and the defaults table recomputed from the taps the library's getters return (an ASDR_NO_DEVICE resampler)."""
import numpy as np
import pytest

import resample_ref as RR

CUSTOM = (3, 4, 7, 9)     # U, M, K, shift


def custom_taps(rng, up, K, bound=150):
    return rng.integers(-bound, bound + 1, size=up * K).astype(np.int16)


def rate_case(which, rng):
    if which == "custom":
        up, down, K, shift = CUSTOM
        return up, down, custom_taps(rng, up, K, 3000), shift
    up, down = RR.ratio(which)
    taps, shift = RR.default_filter(which)
    return up, down, taps, shift


@pytest.mark.parametrize("which", [12000, 8000, 11025, "custom"])
def test_vectorised_restatement_equals_the_loop(which):
    rng = np.random.default_rng(5)
    up, down, taps, shift = rate_case(which, rng)
    x = rng.integers(-32768, 32768, size=(2, 5, 128)).astype(np.int16)
    ref = RR.ResampleRef(2, up, down, taps, shift)
    got = np.concatenate([ref.update(x[:, :1]), ref.update(x[:, 1:3]), ref.update(x[:, 3:])], axis=1)
    assert got.shape[1] == RR.ceil_div(5 * 128 * up, down) == ref.output_position()
    for c in range(2):
        assert np.array_equal(got[c], RR.loop_outputs(x[c].reshape(-1), up, down, taps, shift, 0, got.shape[1]))
    assert np.array_equal(ref.state, x.reshape(2, -1)[:, -256:])


@pytest.mark.parametrize("which", [12000, 8000, 32000, "custom"])
def test_splitting_into_calls_changes_nothing(which):
    rng = np.random.default_rng(6)
    up, down, taps, shift = rate_case(which, rng)
    nb = 40
    x = rng.integers(-32768, 32768, size=(3, nb, 128)).astype(np.int16)
    whole = RR.ResampleRef(3, up, down, taps, shift).update(x)
    for trial in range(3):
        ref = RR.ResampleRef(3, up, down, taps, shift)
        parts, b = [], 0
        while b < nb:
            size = int(rng.integers(1, 9))
            want = ref.out_samples(min(size, nb - b))
            parts.append(ref.update(x[:, b:b + size]))
            assert parts[-1].shape[1] == want
            b += size
        assert np.array_equal(np.concatenate(parts, axis=1), whole)


@pytest.mark.parametrize("fs,counts", [(12000, {34, 35}), (8000, {23, 24}), (11025, {32}), (22050, {64}), (44100, {128})])
def test_per_call_counts(fs, counts):
    up, down = RR.ratio(fs)
    taps, shift = RR.default_filter(fs)
    ref = RR.ResampleRef(1, up, down, taps, shift)
    seen, total = set(), 0
    z = np.zeros((1, 1, 128), dtype=np.int16)
    for k in range(500):
        n = ref.update(z).shape[1]
        seen.add(n); total += n
        assert total == RR.ceil_div((k + 1) * 128 * up, down)
    assert seen == counts
    for n0 in (2**31 - 1, 2**32, 2**40):
        j0, j1 = RR.out_range(n0, n0 + 128, up, down)
        assert j0 == -((-n0 * up) // down) and j1 - j0 in counts


def tone(f, n, amp=20000):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / RR.FS_IN)).astype(np.int16)


def resampled(fs, x):
    up, down = RR.ratio(fs)
    taps, shift = RR.default_filter(fs)
    nb = x.size // 128
    return RR.ResampleRef(1, up, down, taps, shift).update(x[:nb * 128].reshape(1, nb, 128))[0].astype(np.float64)[400:]


def test_known_answer_a_passband_tone_keeps_its_amplitude():
    """1500 Hz, amplitude 20000, at 12 kHz: a least-squares fit of sin / cos at 1500 Hz gives the amplitude within 0.01 dB."""
    y = resampled(12000, tone(1500.0, 160 * 128))
    t = np.arange(y.size) / 12000.0
    basis = np.stack([np.sin(2 * np.pi * 1500.0 * t), np.cos(2 * np.pi * 1500.0 * t)], axis=1)
    amp = np.hypot(*np.linalg.lstsq(basis, y, rcond=None)[0])
    db = 20 * np.log10(amp / 20000.0)
    print("1500 Hz at 12 kHz: %.5f dB" % db)
    assert abs(db) <= 0.01
    assert np.abs(y - basis @ np.linalg.lstsq(basis, y, rcond=None)[0]).max() < 20000 * 10 ** (-60 / 20)   # and nothing else


@pytest.mark.parametrize("fs", [12000, 8000])
@pytest.mark.parametrize("f", [6973.0, 9000.0, 10500.0, 13500.0, 20000.0])
def test_known_answer_out_of_band_tones_are_gone(fs, f):
    """The spectral peak (Hann window, scaled so that a sine of amplitude A peaks at A) is at or below -78 dB of the input."""
    y = resampled(fs, tone(f, 160 * 128))
    w = np.hanning(y.size)
    peak = np.abs(np.fft.rfft(y * w)).max() / (w.sum() / 2)
    db = 20 * np.log10(max(peak, 1e-9) / 20000.0)
    print("%g Hz at %d Hz: %.2f dB" % (f, fs, db))
    assert db <= -78.0


TABLE = {8000: (80, 441, 174, 74.0), 11025: (1, 4, 126, 68.0), 12000: (40, 147, 116, 75.0), 16000: (160, 441, 88, 78.0),
         22050: (1, 2, 64, 72.0), 24000: (80, 147, 58, 78.0), 32000: (320, 441, 44, 79.0)}


@pytest.mark.parametrize("fs", sorted(TABLE))
def test_defaults_table_from_the_c_getters(A, fs):
    up, down, K, stop_min = TABLE[fs]
    r = A.AudioResampler(2, fs_out=fs, device=A.NO_DEVICE)
    taps, shift = r.get_taps()
    assert (r.up, r.down, r.taps_per_phase(), shift) == (up, down, K, 15) == RR.ratio(fs) + (K, 15)
    assert r.delay() == (up * K - 1) / (2.0 * up)
    h = taps.astype(np.int64).reshape(K, up)
    assert (h.sum(axis=0) == 32768).all()
    assert int(np.abs(h).sum(axis=0).max()) <= 65535 and RR.accepted(up, down, taps, shift)
    db, f = RR.response_db(taps, up)
    stop = -db[f >= 0.58 * fs].max()
    ripple = np.abs(db[f <= 0.42 * fs]).max()
    print("%d Hz: K %d, max sum|h| %d, stop band %.2f dB, passband %.5f dB" % (fs, K, np.abs(h).sum(axis=0).max(), stop, ripple))
    assert stop >= stop_min and ripple <= 0.01
    mine, my_shift = RR.default_filter(fs)                    # the numpy design: the same recipe, up to the libm's last bit
    assert my_shift == 15 and mine.size == taps.size and np.abs(mine.astype(np.int64) - taps).max() <= 1
    r.close()


def test_the_identity(A):
    r = A.AudioResampler(1, fs_out=44100, device=A.NO_DEVICE)
    taps, shift = r.get_taps()
    assert (r.up, r.down, taps.tolist(), shift) == (1, 1, [16384], 14) and r.delay() == 0.0
    x = np.random.default_rng(1).integers(-32768, 32768, size=(1, 2, 128)).astype(np.int16)
    assert np.array_equal(RR.ResampleRef(1, 1, 1, taps, shift).update(x)[0], x.reshape(-1))
    r.close()
