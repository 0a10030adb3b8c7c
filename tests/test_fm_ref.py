"""tests/fm_ref.py, the numpy restatement of include/asdr_fm.h, held to float64 and to known answers: the CORDIC discriminator
against atan2 with the bound the header derives, its register magnitudes, the demodulated tone, the tuning-offset meter, the
bypasses, the squelch's worked sequences, call splitting and the helpers.  The library's own helpers and the package's export are
checked here too, so every test needs the FM stage to exist."""
import math

import numpy as np
import pytest

import fm_ref as F

# atan(2^-19) is the residual rotation; each of the 20 iterations and the normalising shift truncates both registers by less than
# one unit of a vector no shorter than 2^28: 21 sqrt(2) 2^-28 rad in all
DISCRIMINATOR_BOUND = math.atan(2.0 ** -19) + 21.0 * math.sqrt(2.0) * 2.0 ** -28


@pytest.fixture(scope="module")
def fm(A):
    assert A.FmDemodulator is not None
    return A


def operand_sets():
    """int64 [4][n]: (I, Q, Ip, Qp) -- 10^6 over the full range, 2 10^5 with amplitudes below 40, and the special ones."""
    rng = np.random.default_rng(11)
    full = rng.integers(-32768, 32768, size=(4, 1000000))
    small = rng.integers(-39, 40, size=(4, 200000))
    special = np.array([[-32768, -32768, -32768, -32768],      # re = 2^31
                        [32767, 0, 32767, 0], [0, 32767, 0, 32767], [1, 0, 1, 0],                 # the positive real axis
                        [0, 1, 1, 0], [0, 32767, 32767, 0], [0, -32768, -32768, 0],               # the positive imaginary axis
                        [0, -1, 1, 0], [0, -32768, 32767, 0],                                     # the negative imaginary axis
                        [-1, 0, 1, 0], [-32768, 0, 32767, 0], [32767, 0, -32768, 0], [0, -3, 0, 3],   # re < 0 with im = 0
                        [-32768, 32767, 32767, 32767], [32767, -32768, 32767, 32767],             # the largest |im|
                        [1, 1, 1, -1], [39, -39, -39, 39], [0, 0, 0, 0], [5, 7, 0, 0]]).T
    return np.concatenate([full, small, special], axis=1)


def test_discriminator_against_atan2(fm):
    I, Q, Ip, Qp = operand_sets()
    assert I.size >= 10**6
    re, im = F.conj_product(I, Q, Ip, Qp)
    assert re.max() == 1 << 31 and np.abs(im).max() <= 1 << 31
    theta, peak = F.discriminator(re, im, with_peak=True)
    assert theta.min() >= -(1 << 31) and theta.max() < (1 << 31)
    zero = (re == 0) & (im == 0)
    assert zero.any() and (theta[zero] == 0).all()
    want = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    err = np.abs((theta / 2.0 ** 31 * np.pi - want + np.pi) % (2.0 * np.pi) - np.pi)[~zero]
    print("largest error %.4g rad, bound %.4g; largest register 2^%.3f" % (err.max(), DISCRIMINATOR_BOUND, np.log2(peak.max())))
    assert err.max() <= DISCRIMINATOR_BOUND
    assert peak.max() < (1 << 31)                              # int32 holds every register throughout
    axis = (im == 0) & (re < 0)
    assert axis.any() and (np.abs(np.abs(theta[axis].astype(np.float64)) - 2.0 ** 31) * np.pi / 2.0 ** 31 <= DISCRIMINATOR_BOUND).all()


def test_the_atan_table(fm):
    assert F.ATAN[0] == 1 << 29 and F.ATAN[1] == 316933406 and F.ATAN[19] == 1304 and len(F.ATAN) == 20


def tone(n_blocks, **kw):
    I, Q = F.fm_iq(128 * n_blocks, 8000.0, **kw)
    return I.reshape(1, n_blocks, 128), Q.reshape(1, n_blocks, 128)


def test_known_answer_1khz_tone(fm):
    """3 kHz deviation under the gain of 5 kHz: 0.6 of full scale, times the sinc of the one-sample phase difference."""
    I, Q = tone(8)
    r = F.FmRef(1)
    assert int(r.gain[0]) == 144502
    out = r.update(I, Q)[0].reshape(-1).astype(np.float64)
    n = np.arange(out.size)
    want = 0.6 * 32767.0 * np.sinc(1000.0 / 44100.0) * np.cos(2.0 * np.pi * 1000.0 * (n - 0.5) / 44100.0)
    err = np.abs(out - want)[2:]
    print("largest error %.2f LSB" % err.max())
    assert err.max() <= 10.0
    assert r.st["last_noise"][0] < 10**9 and r.st["open_blocks"][0] == 8 and r.st["openings"][0] == 1


def test_tuning_offset_meter_and_dc_removal(fm):
    """An unmodulated carrier 1,500 Hz off tune, at amplitude 30000: the input rounding that costs up to 8.1 LSB of v at amplitude
    8000 scales with 1 / amplitude to 2.2 LSB here, which leaves room for the meter's own rounding inside |y| <= 3."""
    nb = 64
    I, Q = F.fm_iq(128 * nb, 30000.0, deviation_hz=0.0, offset_hz=1500.0)
    r = F.FmRef(1)
    r.set_dc_shift(8)
    out = r.update(I.reshape(1, nb, 128), Q.reshape(1, nb, 128))[0].reshape(-1)
    got = r.offset_hz(5000.0)[0]
    print("offset %.2f Hz, settled |y| <= %d" % (got, np.abs(out[-2048:]).max()))
    assert abs(got - 1500.0) <= 15.0
    assert np.abs(out[-2048:]).max() <= 3
    assert abs(out[0]) > 1000 or abs(out[1]) > 1000            # before it settles the offset is there


def test_bypasses_give_v(fm):
    rng = np.random.default_rng(3)
    I, Q = (rng.integers(-32768, 32768, size=(5, 3, 128)).astype(np.int16) for _ in range(2))
    r, probe = F.FmRef(5), F.FmRef(5)
    assert (r.deemphasis == 32768).all() and (r.hp_shift == 0).all()
    out = r.update(I, Q)[0]
    v = probe.demodulate(I.reshape(5, -1), Q.reshape(5, -1))[0]
    assert np.array_equal(out.reshape(5, -1), v) and (r.st["m"] == 0).all()
    assert np.array_equal(r.st["s"], v[:, -1] << 15)
    r2 = F.FmRef(5)
    r2.set_deemphasis(976); r2.set_dc_shift(4)
    assert not np.array_equal(r2.update(I, Q)[0], out)


def noise_rows(levels):
    """(I, Q) int16 [1][len][128] whose blocks have about the wanted noise: 0 -> a clean carrier (N = 0 behind the first block), 1 ->
    full-range noise."""
    rng = np.random.default_rng(8)
    I = np.full((1, len(levels), 128), 12000, dtype=np.int16)
    Q = np.zeros_like(I)
    for b, loud in enumerate(levels):
        if loud:
            I[0, b], Q[0, b] = rng.integers(-32768, 32768, size=(2, 128))
    return I, Q


def squelch_sequence(noise, open_noise, close_noise, hang):
    r = F.FmRef(1)
    r.set_squelch(open_noise, close_noise, hang)
    N = np.array(noise, dtype=np.uint64)
    return [int(r.squelch(N[k:k + 1], N[k:k + 1])[0]) for k in range(len(noise))], r


def test_the_squelch_table(fm):
    """asdr_gate.h's two worked sequences with the inequality mirrored (asdr_fm.h)."""
    opens, r = squelch_sequence([9, 0, 9, 9, 9, 9], 0, 5, 2)
    assert opens == [0, 1, 1, 1, 0, 0] and r.st["openings"][0] == 1 and r.st["open_blocks"][0] == 3 and r.st["last_noise"][0] == 9
    opens, r = squelch_sequence([1, 0, 1, 6, 6], 0, 5, 0)
    assert opens == [0, 1, 1, 0, 0]
    opens, r = squelch_sequence([5, 6, 5, 7, 5], 5, 6, 0)      # exactly at the thresholds
    assert opens == [1, 1, 1, 0, 1] and r.st["openings"][0] == 2
    opens, r = squelch_sequence([1 << 41] * 3, 1 << 41, 1 << 41, 0)   # the creation values: always open
    assert opens == [1, 1, 1]


def test_muted_blocks_are_zeros_while_the_state_advances(fm):
    levels = [0, 0, 1, 1, 1, 0, 0]
    I, Q = noise_rows(levels)
    r, free = F.FmRef(1), F.FmRef(1)
    for x in (r, free):
        x.set_deemphasis(8550); x.set_dc_shift(6)
    r.set_squelch(10**11, 3 * 10**11, 1)
    out, opens = r.update(I, Q)
    want, _ = free.update(I, Q)
    # block 2 is held by the hang; the block after the noise has three large w at most (3 * 2^34 < 10^11) and opens again
    assert opens[0].tolist() == [1, 1, 1, 0, 0, 1, 1]
    assert not out[0, 3:5].any() and np.array_equal(out[0, :3], want[0, :3]) and np.array_equal(out[0, 5:], want[0, 5:])
    assert want[0, 3].any() and want[0, 4].any()
    for k in ("prev_i", "prev_q", "v1", "v2", "s", "m", "last_noise", "last_power"):
        assert r.st[k][0] == free.st[k][0], k
    assert r.st["openings"][0] == 2 and r.st["open_blocks"][0] == 5 and r.st["hang_left"][0] == 1


def test_split_calls_equal_one_call(fm):
    rng = np.random.default_rng(4)
    n = 6
    I, Q = (rng.integers(-32768, 32768, size=(n, 7, 128)) >> rng.integers(0, 12, size=(n, 7, 1)) for _ in range(2))
    I, Q = I.astype(np.int16), Q.astype(np.int16)

    def make():
        r = F.FmRef(n)
        for c in range(n):
            r.set_gain(1 + 2796202 * c, ch=c); r.set_deemphasis((1, 976, 8550, 32768, 5, 20000)[c], ch=c)
            r.set_dc_shift((0, 1, 15, 8, 4, 0)[c], ch=c)
        r.set_squelch(3 * 10**11, 6 * 10**11, 1)
        return r
    whole, parts = make(), make()
    out, opens = whole.update(I, Q)
    pieces = [parts.update(I[:, a:b], Q[:, a:b]) for a, b in ((0, 1), (1, 3), (3, 7))]
    assert np.array_equal(np.concatenate([p[0] for p in pieces], axis=1), out)
    assert np.array_equal(np.concatenate([p[1] for p in pieces], axis=1), opens)
    assert whole.state_tuples() == parts.state_tuples() and whole.blocks == parts.blocks == 7
    assert 0 < opens.sum() < opens.size


def test_helper_values(fm):
    assert F.gain_from_deviation(5000.0) == 144502 and F.deemphasis_from_tau_us(750.0) == 976 and F.deemphasis_from_tau_us(75.0) == 8550
    assert fm.fm_gain_from_deviation(5000.0) == 144502 and fm.fm_deemphasis_from_tau_us(750.0) == 976
    assert fm.fm_deemphasis_from_tau_us(75.0) == 8550
    for hz in (43.1, 44.0, 2500.0, 3000.0, 75000.0, 1e8, 722500000.0):
        assert fm.fm_gain_from_deviation(hz) == F.gain_from_deviation(hz)
    for t in (0.001, 1.0, 50.0, 318.0, 1e4, 7e5):
        assert fm.fm_deemphasis_from_tau_us(t) == F.deemphasis_from_tau_us(t)
    assert F.gain_from_deviation(43.0) is None and F.gain_from_deviation(1e10) is None and F.deemphasis_from_tau_us(1e7) is None
    for call, x in ((fm.fm_gain_from_deviation, 43.0), (fm.fm_gain_from_deviation, 1e10), (fm.fm_gain_from_deviation, 0.0),
                    (fm.fm_gain_from_deviation, float("nan")), (fm.fm_deemphasis_from_tau_us, 1e7), (fm.fm_deemphasis_from_tau_us, -1.0)):
        with pytest.raises(fm.AsdrError, match="outside"):
            call(x)
