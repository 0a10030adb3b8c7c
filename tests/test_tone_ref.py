"""tests/tone_ref.py, the numpy restatement of include/asdr_tone.h, held to known answers: every CTCSS tone decoded under voice-band
noise, nothing decoded from noise alone, the accumulators' bound, the high-pass against the Butterworth formula and a float64
cascade, the open / hang / close rule on designed verdicts, and that splitting a sequence into calls changes nothing."""
import math

import numpy as np
import pytest

import tone_ref as TR

FS = 44100.0


def test_tables():
    assert TR.H.size == 46 and int(TR.H.sum()) == 4096 and TR.H[0] == 1 and TR.H[22] == TR.H[23] == 192 and (TR.H == TR.H[::-1]).all()
    assert TR.C[0] == 16384 and TR.C[256] == 0 and TR.C[512] == -16384 and TR.C[768] == 0 and np.abs(TR.C).max() == 16384
    s = TR.steps_from_hz(TR.CTCSS)
    assert len(s) == 50 and s[0] == math.floor(67.0 * 16 * 2**32 / 44100 + 0.5) == 104403740 and s[-1] < 2**31
    assert TR.steps_from_hz([100.0, 100.0]) is None and TR.steps_from_hz([1378.0]) is None and TR.steps_from_hz([]) is None
    assert TR.steps_from_hz([1377.9]) is not None and TR.steps_from_hz([1.0] * 65) is None
    assert TR.min_power(1000, 64) == (128 * 1000 * 64) ** 2 // 4 == 16777216000000
    assert TR.STATE_DTYPE.itemsize == 704 and 704 % 16 == 0


@pytest.fixture(scope="module")
def noise():
    """300 .. 3000 Hz noise of rms 6000, [200][3 * 128 * 128]: enough for three windows of 128 blocks."""
    return TR.voice_noise(np.random.default_rng(50), (200, 3 * 128 * 128), 6000.0)


@pytest.mark.parametrize("W", [64, 128])
def test_all_50_tones_under_voice_noise(noise, W):
    """Channel 4 t + j carries tone t, 0.3 % low (j < 2) or high, at amplitude 1,000 (j even) or 3,277.  Every window after the first
    decodes the right index with the creation dominance and min_power = tone_min_power(A, W)."""
    m = 3 * W * 128
    amps = np.array([1000, 3277] * 100)
    off = np.array([0.997, 0.997, 1.003, 1.003] * 50)
    x = np.stack([TR.tone_wave(m, TR.CTCSS[c // 4] * off[c], amps[c], phase=0.1 * c) for c in range(200)]) + noise[:, :m]
    r = TR.ToneRef(200)
    r.set_window(W)
    for c in range(200):
        r.set_min_power(TR.min_power(amps[c], W), ch=c)
    x = TR.to_int16(x).reshape(200, 3 * W, 128)
    worst_ratio, worst_level = np.inf, np.inf
    for w in range(3):
        out, unmuted = r.update(x[:, w * W:(w + 1) * W])
        assert np.array_equal(out, x[:, w * W:(w + 1) * W]) and unmuted.all()       # PASS, no sections: an exact pass
        if w == 0:
            continue
        st = r.st
        assert np.array_equal(st["detected"], np.arange(200) // 4), np.flatnonzero(st["detected"] != np.arange(200) // 4)
        assert np.array_equal(st["last_best"], st["detected"])
        worst_ratio = min(worst_ratio, (st["last_power"].astype(np.float64) / np.maximum(st["last_other"].astype(np.float64), 1.0)).min())
        worst_level = min(worst_level, (st["last_power"].astype(np.float64) / (128.0 * amps * W) ** 2).min())
    print("W", W, "worst P_best / other", worst_ratio, "worst P_best / (128 A W)^2", worst_level)
    assert worst_ratio >= 4.0 and worst_level >= 0.25
    assert np.array_equal(r.st["windows"], np.full(200, 3)) and np.array_equal(r.decoded_hz(), np.repeat(TR.CTCSS, 4))


def test_noise_alone_detects_nothing(noise):
    W, n = 64, 40
    rng = np.random.default_rng(51)
    x = np.concatenate([TR.to_int16(noise[:n // 2, :3 * W * 128]), rng.integers(-32768, 32768, size=(n // 2, 3 * W * 128)).astype(np.int16)])
    r = TR.ToneRef(n)
    r.set_min_power(TR.min_power(1000, W))
    r.set_want(TR.ANY)
    for w in range(3):
        out, unmuted = r.update(x.reshape(n, 3 * W, 128)[:, w * W:(w + 1) * W])
        assert (r.st["detected"] == -1).all() and not out.any() and not unmuted.any()
    assert not r.st["open"].any() and not r.st["openings"].any() and (r.st["windows"] == 3).all() and (r.st["last_best"] >= 0).all()


def test_full_scale_square_wave_keeps_the_accumulators_below_2_30():
    W = 128
    k = np.arange(W * 128)
    x = np.where(np.sin(2.0 * np.pi * 67.0 * k / FS) >= 0.0, 32767, -32768).astype(np.int16).reshape(1, W, 128)
    r = TR.ToneRef(1)
    r.set_window(W)
    peak = 0
    for b in range(W - 1):
        r.update(x[:, b:b + 1])
        peak = max(peak, int(np.abs(r.st["acc"]).max()))
    print("peak |acc| / 2^31:", peak / 2.0**31)
    assert 0.25 * 2**31 < peak < 2**30
    r.update(x[:, W - 1:])
    assert int(r.st["detected"][0]) == 0 and not r.st["acc"].any() and int(r.st["last_power"][0]) > 2**57


def test_d_reaches_minus_32768_and_the_sums_2_32():
    """A constant -32768 gives d = -32768 once the history is full, and R = -2^32 on a tone whose phase stays in slot 0."""
    x = np.full((1, 2, 128), -32768, dtype=np.int16)
    r = TR.ToneRef(1)
    r.set_tones([0.0001])
    r.update(x)
    assert (TR.decimate(r.st["hist"], x[:, 1].astype(np.int64)) == -32768).all()
    assert int(r.st["acc"][0, 0, 0]) < -(2**32 >> 9) and int(r.st["acc"][0, 0, 1]) == 0


# ---- the high-pass
def butterworth_power(f, fc, order):
    return 1.0 / (1.0 + (math.tan(math.pi * fc / FS) / math.tan(math.pi * f / FS)) ** (2 * order))


@pytest.mark.parametrize("sections", [1, 2, 3])
def test_designed_sections_follow_the_butterworth_formula(sections):
    coef = TR.highpass_design(300.0, sections)
    for f in (50.0, 100.0, 150.0, 254.1, 300.0, 1000.0):
        z = np.exp(-2j * np.pi * f / FS)
        h = 1.0
        for b0, b1, b2, a1, a2 in coef:
            h *= (b0 + b1 * z + b2 * z * z) / (2.0**28 + a1 * z + a2 * z * z)
        assert abs(10.0 * math.log10(abs(h) ** 2) - 10.0 * math.log10(butterworth_power(f, 300.0, 2 * sections))) < 0.1, f
    assert abs(10.0 * math.log10(butterworth_power(100.0, 300.0, 6)) + 57.26) < 0.01


def float_cascade(x, fc, sections):
    K = math.tan(math.pi * fc / FS)
    y = np.asarray(x, dtype=np.float64)
    for k in range(sections):
        q = 2.0 * math.sin(math.pi * (2 * k + 1) / (4.0 * sections))
        n = 1.0 / (1.0 + q * K + K * K)
        b, a1, a2 = (n, -2.0 * n, n), 2.0 * (K * K - 1.0) * n, (1.0 - q * K + K * K) * n
        out = np.zeros_like(y)
        x1 = x2 = y1 = y2 = 0.0
        for i, u in enumerate(y):
            o = b[0] * u + b[1] * x1 + b[2] * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, u, y1, o
            out[i] = o
        y = out
    return y


def test_the_integer_cascade_is_within_1_lsb_of_float64():
    rng = np.random.default_rng(52)
    x = rng.integers(-32768, 32768, size=8192).astype(np.int64)
    hp = np.zeros((1, 3, 4), dtype=np.int64)
    y = TR.highpass(x[None, :], TR.highpass_design(300.0, 3), hp)[0]
    want = np.clip(float_cascade(x, 300.0, 3), -32768, 32767)
    err = y - want
    print("rms error", np.sqrt((err * err).mean()), "max", np.abs(err).max(), "largest state 2^%.1f" % math.log2(np.abs(hp).max()))
    assert np.abs(err).max() <= 1.0 and np.abs(hp).max() < 2**30


def test_a_100_hz_tone_is_down_57_db_and_a_square_wave_keeps_the_states_small():
    """Behind the three-section 300 Hz design a full-scale 100 Hz tone leaves 32767 * 10^(-57.26 / 20) = 44.8 LSB; the output's
    rounding (at most 1 LSB against the float64 cascade, above) moves that by at most 20 log10(45.8 / 44.8) = 0.2 dB."""
    coef = TR.highpass_design(300.0, 3)
    x = TR.to_int16(TR.tone_wave(8820, 100.0, 32767.0)).astype(np.int64)
    y = TR.highpass(x[None, :], coef, np.zeros((1, 3, 4), dtype=np.int64))[0][4410:].astype(np.float64)      # ten whole periods, settled
    down = -20.0 * math.log10(math.sqrt(2.0 * (y * y).mean()) / 32767.0)
    print("100 Hz down by", down, "dB")
    assert abs(down - 57.26) < 0.5
    k = np.arange(8820)
    sq = np.where(np.sin(2.0 * np.pi * 300.0 * k / FS) >= 0.0, 32767, -32768).astype(np.int64)
    hp = np.zeros((1, 3, 4), dtype=np.int64)
    peak = 0
    for a in range(0, sq.size, 441):
        TR.highpass(sq[None, a:a + 441], coef, hp)
        peak = max(peak, int(np.abs(hp).max()))
    print("largest state 2^%.2f" % math.log2(peak))
    assert peak < 2**30
    assert np.array_equal(TR.highpass(sq[None, :100], [], hp), sq[None, :100])   # 0 sections: y = x


# ---- the state machine
def walk(want, hang, verdicts):
    """A one-channel reference through windows whose accumulators are set by hand: verdict v >= 0 puts all the power on tone v, -1
    spreads it evenly (no dominance).  Returns open after each window."""
    r = TR.ToneRef(1)
    r.set_want(want); r.set_hang(hang); r.set_min_power(1000)
    seen = []
    for v in verdicts:
        r.st["acc"][0, :50, 0] = 100
        if v >= 0:
            r.st["acc"][0, v, 0] = 1000
        r.window_end(np.array([0]))
        assert int(r.st["detected"][0]) == v
        seen.append(int(r.st["open"][0]))
    return seen, r


def test_open_hang_close_rule():
    seen, r = walk(5, 2, [-1, 5, -1, -1, -1, 5, 3, 3, 3, 3])
    assert seen == [0, 1, 1, 1, 0, 1, 1, 1, 0, 0]
    assert int(r.st["openings"][0]) == 2 and int(r.st["matches"][0]) == 2 and int(r.st["windows"][0]) == 10 and int(r.st["last_best"][0]) == 3
    seen, r = walk(5, 0, [5, -1, 5, 5, 4])
    assert seen == [1, 0, 1, 1, 0] and int(r.st["openings"][0]) == 2 and int(r.st["matches"][0]) == 3
    seen, r = walk(5, 1, [5, -1, 5, -1, -1])                        # a match inside the hang refills it
    assert seen == [1, 1, 1, 1, 0] and int(r.st["openings"][0]) == 1
    seen, r = walk(TR.ANY, 0, [-1, 7, 9, -1])
    assert seen == [0, 1, 1, 0] and int(r.st["matches"][0]) == 2
    seen, r = walk(TR.PASS, 3, [-1, 7, -1])
    assert seen == [1, 1, 1] and int(r.st["matches"][0]) == 3 and int(r.st["openings"][0]) == 1 and int(r.st["hang_left"][0]) == 3
    seen, r = walk(5, 255, [5] + [-1] * 255 + [-1])
    assert seen == [1] * 256 + [0]


def test_the_verdict_at_its_edges():
    r = TR.ToneRef(1)
    r.set_tones([100.0, 110.0, 120.0, 130.0]); r.set_want(TR.ANY)
    def verdict(acc, min_power=0, dominance=64):
        r.set_min_power(min_power); r.set_dominance(dominance)
        r.st["acc"][0, :4, 0] = acc
        r.window_end(np.array([0]))
        return int(r.st["detected"][0]), int(r.st["last_best"][0]), int(r.st["last_power"][0]), int(r.st["last_other"][0])
    assert verdict([0, 0, 0, 0]) == (0, 0, 0, 0)                     # all equal: the lowest index, and 0 >= 0 on both tests
    assert verdict([0, 0, 0, 0], min_power=1) == (-1, 0, 0, 0)
    assert verdict([32, 32, 16, 16]) == (0, 0, 1024, 256)            # a neighbour does not count; 16 * 4 >= 64 * 1 at equality
    assert verdict([32, 32, 16, 16], dominance=65) == (-1, 0, 1024, 256)
    assert verdict([32, 32, 16, 16], min_power=1024) == (0, 0, 1024, 256)
    assert verdict([32, 32, 16, 16], min_power=1025) == (-1, 0, 1024, 256)
    assert verdict([1, 2, 3, 40]) == (3, 3, 1600, 4)                 # |t - best| >= 2: tones 0 and 1
    r.set_tones([100.0])
    r.st["acc"][0, 0] = (-2**31, -2**31)
    r.window_end(np.array([0]))
    assert int(r.st["last_power"][0]) == 2**63 and int(r.st["last_other"][0]) == 0 and int(r.st["detected"][0]) == 0


# ---- splits
def test_splitting_a_sequence_into_calls_changes_nothing():
    W, n, nb = 16, 6, 40
    rng = np.random.default_rng(53)
    table = [70.0 + 30.0 * k for k in range(8)]                    # a window of 16 blocks (46 ms) resolves 21.5 Hz
    x = TR.to_int16(np.stack([TR.tone_wave(nb * 128, table[c], 3000.0) for c in range(n)]) + rng.normal(0.0, 2000.0, size=(n, nb * 128)))
    x = x.reshape(n, nb, 128)

    def fresh():
        r = TR.ToneRef(n)
        r.set_tones(table); r.set_window(W); r.set_highpass(TR.highpass_design(300.0, 3)); r.set_min_power(TR.min_power(1000, W))
        for c in range(n):
            r.set_want((TR.PASS, TR.ANY, 2, 0, 4, TR.ANY)[c], ch=c); r.set_hang(c % 2, ch=c)
        return r
    whole = fresh()
    out, unmuted = whole.update(x)
    assert whole.st["detected"].tolist() == [0, 1, 2, 3, 4, 5] and unmuted[:, -1].tolist() == [1, 1, 1, 0, 1, 1] and not unmuted[1:, :W].any()
    for sizes in ([1] * nb, [2] * (nb // 2), [3] * 13 + [1], [W - 1, W + 1, 8], [W + 1, W - 1, 8]):
        r, a, parts = fresh(), 0, []
        for s in sizes:
            parts.append(r.update(x[:, a:a + s])[0])
            a += s
        assert a == nb and np.array_equal(np.concatenate(parts, axis=1), out) and r.records().tobytes() == whole.records().tobytes()
        assert r.blocks == nb
