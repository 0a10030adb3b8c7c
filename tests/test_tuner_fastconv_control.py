"""Fast-convolution banks of the digital tuner (include/asdr_tuner.h, "Fast-convolution banks") on ASDR_NO_DEVICE banks: creation
rules (a fractional Fs_mid included), U / M and out-block counts against tests/tuner_fastconv_ref.py, the channel-filter setters,
read_state after retunes, the filter calls refusing the wrong kind of bank, and the Python round trips."""
import numpy as np
import pytest

import tuner_fastconv_ref as F

EXAMPLES = {(2400000, 16): (147, 500), (20000000, 128): (882, 3125), (61440000, 512): (147, 400), (44100 * 2, 2): (1, 1),
            (44100 * 1024, 1024): (1, 1), (176400 * 1024, 1024): (1, 4), (2400000, 32): (147, 250)}


@pytest.fixture
def T(A):
    return lambda fs, R, n=4, s=2: A.TunerBank.fastconv(n, s, fs, R, device=A.NO_DEVICE)


def test_creation_rules_and_messages(A, T):
    for fs, R, what in ((2400000, 3, "power of two"), (2400000, 1, "power of two"), (2400000 * 2048, 2048, "power of two"),
                        (2400000, 64, r"\[44100, 176400\]"), (2400000, 8, r"\[44100, 176400\]"), (0, 16, "positive"),
                        (-2400000, 16, "positive"), (44101 * 2, 2, "U > 2048")):
        with pytest.raises(A.AsdrError, match=what):
            T(fs, R)
        assert not F.valid(fs, R)
    with pytest.raises(A.AsdrError, match="n_channels"):
        A.TunerBank.fastconv(0, 1, 2400000, 16, device=A.NO_DEVICE)
    with pytest.raises(A.AsdrError, match="n_sources"):
        A.TunerBank.fastconv(4, 0, 2400000, 16, device=A.NO_DEVICE)
    t = T(2500000, 16)                                          # Fs_mid = 156,250 Hz
    assert t.ratio() == F.ratio(2500000, 16) == (882, 3125)
    frac = next(f for f in range(2400001, 2500000) if f % 16 and F.valid(f, 16))   # Fs_mid fractional
    b = T(frac, 16)
    assert b.fs_in == frac and b.ratio() == F.ratio(frac, 16) and b.decimation == 16 and b.fft_size() == 4096


def test_ratio_sizes_and_suggestion(A, T):
    for (fs, R), ud in EXAMPLES.items():
        t = T(fs, R)
        assert t.ratio() == ud == F.ratio(fs, R), (fs, R)
        assert t.fft_size() == 256 * R and t.decimation == R and t.fs_in == fs and t.output_position() == t.position() == 0
    assert A.TunerBank(2, 1, 4, device=A.NO_DEVICE).fft_size() == 0
    assert A.TunerBank(2, 1, 50, fs_in=2400000, device=A.NO_DEVICE).fft_size() == 0
    assert A.suggest_fft_decimation(2400000) == 32 and A.fastconv_ratio(2400000, 32) == (147, 250)
    assert A.suggest_fft_decimation(20000000) == 128
    assert A.suggest_fft_decimation(61440000) == 1024                  # 147 / 200, the same U as R = 512
    assert A.suggest_fft_decimation(44100 * 8) == 8
    assert A.suggest_fft_decimation(1000) is None and A.suggest_fft_decimation(44101) is None
    for fs in (2048000, 3000000, 10000000, 30720000, 122880000):
        R = A.suggest_fft_decimation(fs)
        assert R is not None and F.valid(fs, R)
        assert all(F.ratio(fs, r)[0] >= F.ratio(fs, R)[0] for r in (1 << k for k in range(1, 11)) if F.valid(fs, r))


def test_out_blocks_follow_the_rate_timing(A, T):
    rng = np.random.default_rng(3)
    for fs, R in ((2400000, 16), (20000000, 128), (61440000, 512), (44100 * 4, 4)):
        t = T(fs, R, 1, 1)
        h2, g2 = t.get_resampler()
        ref = F.TunerFastconvRef(1, 1, fs, R, h2=h2, g2=g2)
        n_u = 0
        for _ in range(30):
            nf = int(rng.integers(0, 9))
            assert t.out_blocks(nf) == ref.out_blocks(nf), (fs, R, nf)
        if ref.pass_through():
            assert t.out_blocks(7) == 7
        else:
            U, M = F.ratio(fs, R)
            assert t.out_blocks(7) == F.RR.blocks_out(n_u + 7 * 128, U, M)


def test_default_filters(A, T):
    for fs, R in ((2400000, 16), (20000000, 128), (61440000, 512), (44100 * 2, 2), (176400 * 4, 4)):
        t = T(fs, R)
        g = t.get_channel_filter()
        assert g.dtype == np.float32 and g.size == 129
        assert np.allclose(g, F.default_channel_filter(fs / R).astype(np.float32), rtol=0, atol=2e-8)
        h2, g2 = t.get_resampler()
        U, M = t.ratio()
        if U == M == 1:
            assert list(h2) == [16384] and g2 == 1
        else:
            K = h2.size // U
            assert h2.size % U == 0 and K == 2 * -(-6 * fs // (44100 * R)) and g2 == 0
            assert all(int(h2[ph::U].astype(np.int64).sum()) == 32768 for ph in range(U))


def test_channel_filter_setter(A, T):
    t = T(2400000, 16)
    g0 = t.get_channel_filter()
    for bad, what in ((np.zeros(0, np.float32), "1..129"), (np.ones(130, np.float32), "1..129"),
                      (np.array([1.0, np.nan], np.float32), "finite"), (np.array([np.inf], np.float32), "finite")):
        with pytest.raises(A.AsdrError, match=what):
            t.set_channel_filter(bad)
        assert np.array_equal(t.get_channel_filter(), g0)
    for L in (1, 7, 129):
        g = np.random.default_rng(L).standard_normal(L).astype(np.float32)
        t.set_channel_filter(g)
        assert np.array_equal(t.get_channel_filter(), g)
    t.reset()
    assert t.get_channel_filter().size == 129 and np.array_equal(t.get_channel_filter(), g)   # reset keeps the filter


def test_channel_filter_setter_takes_every_finite_tap(A, T):
    """Lg = 1 and Lg = 129 at the ends of the range, and taps that are finite but extreme: denormals, +-3e38, -0.0."""
    t = T(44100 * 4, 4)
    tiny = np.array([1e-45, -1e-40, 1.17549421e-38], dtype=np.float32)            # two denormals and one just below FLT_MIN
    assert tiny[0] != 0 and tiny[1] != 0
    for g in (np.array([3e38], np.float32), np.array([-3e38], np.float32), tiny, np.array([-0.0, 1.0], np.float32),
              np.concatenate([np.full(128, 1e-45, np.float32), np.array([3e38], np.float32)])):
        t.set_channel_filter(g)
        got = t.get_channel_filter()
        assert got.size == g.size and got.tobytes() == g.tobytes()
    with pytest.raises(A.AsdrError, match="1..129"):
        t.set_channel_filter(np.full(130, 1e-45, np.float32))
    assert t.get_channel_filter().size == 129


def test_filter_calls_refuse_the_wrong_kind_of_bank(A, T):
    t = T(2400000, 16)
    with pytest.raises(A.AsdrError, match="set_channel_filter"):
        t.set_filter(np.array([16384], np.int16), 1)
    with pytest.raises(A.AsdrError, match="get_channel_filter"):
        t.get_filter()
    for d in (A.TunerBank(2, 1, 4, device=A.NO_DEVICE), A.TunerBank(2, 1, 50, fs_in=2400000, device=A.NO_DEVICE)):
        with pytest.raises(A.AsdrError, match="set_filter"):
            d.set_channel_filter(np.ones(3, np.float32))
        with pytest.raises(A.AsdrError, match="get_filter"):
            d.get_channel_filter()
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.update_rate(np.zeros((2, 16 * 128, 2), np.int16))


def test_setters_and_read_state_after_retunes(A, T):
    fs, R = 20000000, 128
    t = T(fs, R, 5, 3)
    ref = F.TunerFastconvRef(5, 3, fs, R)
    for o in (t, ref):
        o.set_source(2, ch=1); o.set_frequency(-1_234_567.8, ch=1); o.set_frequency_word(0x89ABCDEF, ch=3)
        o.set_phase(0x1234, ch=4); o.set_frequency(9_999_999.0)
    st = t.read_state()
    assert list(st["src"]) == list(ref.src) and list(st["fw"]) == list(ref.fw)
    assert list(st["pos_a"]) == list(ref.pos_a) and list(st["ph_a"]) == list(ref.ph_a)
    assert int(st["fw"][1]) == F.RR.fw_from_hz(9_999_999.0, fs)
    for bad in (3, -1):
        with pytest.raises(A.AsdrError, match="source"):
            t.set_source(bad, ch=0)
    with pytest.raises(A.AsdrError, match="frequency"):
        t.set_frequency(fs / 2 + 1.0, ch=0)
    with pytest.raises(A.AsdrError, match="channel"):
        t.set_phase(0, ch=5)
    # the continuous re-anchor carries the fine NCO's phase (rw, not fw) across a position change
    ref.P = 7 * ref.H
    k0, rw = F.coarse(ref.fw[2], R)
    want = (int(ref.ph_a[2]) + int(rw) * (ref.P - int(ref.pos_a[2]))) & 0xFFFFFFFF
    ref.set_frequency_word(5, ch=2)
    assert int(ref.ph_a[2]) == want and int(ref.pos_a[2]) == ref.P
    t.reset()
    st = t.read_state()
    assert not st["fw"].any() and not st["src"].any() and t.position() == 0
