"""The restatement of the source conditioning (tests/tuner_condition_ref.py; include/asdr_tuner.h, "Source conditioning") against
known answers: the identity on every int16 value, the clamps where only a 64-bit accumulation is right, the sums of a hand-made
row in every format, the estimator's failure conditions, and the quality known answer: one tone through a receiver with gain and
phase imbalance and a DC offset, whose estimated correction puts the image at least 90 dB and the DC at least 84 dB below it."""
import numpy as np

import tuner_condition_ref as CR
import tuner_formats_ref as FM


def test_the_identity_is_exact_on_every_int16_value():
    every = np.arange(-32768, 32768, dtype=np.int64)
    sweep = np.array([-32768, -32767, -12345, -256, -1, 0, 1, 255, 256, 12345, 32766, 32767], dtype=np.int64)
    for part in (0, 1):                                        # every value of one part x a sweep of the other
        x = np.empty((every.size, sweep.size, 2), dtype=np.int16)
        x[..., part] = every[:, None]
        x[..., 1 - part] = sweep[None, :]
        assert np.array_equal(CR.condition(x, CR.IDENTITY), x)
    real = np.stack([every, np.zeros_like(every)], axis=-1).astype(np.int16)
    assert np.array_equal(CR.condition(real, CR.IDENTITY, "rs16"), real)
    assert np.array_equal(CR.condition_raw(every.astype(np.int16), CR.IDENTITY, "rs16"), every.astype(np.int16))


def condition_int32(x, c):
    """condition() with p a + g b + 32768 wrapped to 32 bits at every step: what the statement is NOT."""
    d_r, d_i, p, g = c
    a = x[..., 0].astype(np.int64) - d_r
    b = x[..., 1].astype(np.int64) - d_i
    wrap = lambda v: ((v + 2**31) % 2**32) - 2**31
    acc = wrap(wrap(wrap(p * a) + wrap(g * b)) + 32768)
    return np.stack([np.clip(a, -32768, 32767), np.clip(acc >> 16, -32768, 32767)], axis=-1).astype(np.int16)


# (xr, xi), (d_r, d_i, p, g) -> (xr', xi'), worked by hand from the statement
RAIL_CASES = [
    # a = b = 65535: p a + g b + 32768 = 2147450880 + 8589803520 + 32768 = 10737287168 -> >> 16 = 163838 -> 32767
    ((32767, 32767), (-32768, -32768, 32768, 131072), (32767, 32767)),
    # a = b = -65535: -2147450880 - 8589803520 + 32768 = -10737221632 -> >> 16 = -163837 -> -32768
    ((-32768, -32768), (32767, 32767, 32768, 131072), (-32768, -32768)),
    # a = 65535, b = -65535, p = -32768: the same sum as the line above
    ((32767, -32768), (-32768, 32767, -32768, 131072), (32767, -32768)),
    # a = -65535, b = 65535, p = -32768: the first line's sum
    ((-32768, 32767), (32767, -32768, -32768, 131072), (-32768, 32767)),
    # a = 0, b = 40000 (xi = 32767, d_i = -7233): 131072 * 40000 + 32768 = 5242912768 -> >> 16 = 80000 -> 32767
    ((0, 32767), (0, -7233, 0, 131072), (0, 32767)),
    # inside the clamps: a = 65535 (xr' clamps), b = -16384: -32768 * 65535 + 131072 * -16384 + 32768 = -4294901760 -> -65535 -> -32768
    ((32767, -16384), (-32768, 0, -32768, 131072), (32767, -32768)),
    # no clamp on xi': a = 1000, b = -2000, p = 3277, g = 69468: 3277000 - 138936000 + 32768 = -135626232 -> >> 16 = -2070 (floor of -2069.49)
    ((1000, -2000), (0, 0, 3277, 69468), (1000, -2070)),
]


def test_known_answers_at_the_rails_need_the_int64_path():
    differ = 0
    for x, c, want in RAIL_CASES:
        xa = np.array([x], dtype=np.int16)
        got = CR.condition(xa, c)
        assert tuple(int(v) for v in got[0]) == want, (x, c, got, want)
        differ += not np.array_equal(condition_int32(xa, c), got)
    assert differ >= 5                                         # a 32-bit evaluation of the same cases is told apart
    assert tuple(condition_int32(np.array([[0, 32767]], np.int16), (0, -7233, 0, 131072))[0]) == (0, 14464)


def test_rs16_takes_only_the_real_offset():
    raw = np.array([-32768, -1, 0, 1, 32767, 100], dtype=np.int16)
    got = CR.condition_raw(raw, (-5, 999, -32768, 131072), "rs16")
    assert got.tolist() == [-32763, 4, 5, 6, 32767, 105]
    assert CR.condition_raw(raw, (32767, 0, 0, 65536), "rs16").tolist() == [-32768, -32768, -32767, -32766, 0, -32667]


def test_sums_of_hand_made_rows():
    assert CR.stats(np.array([[3, -4], [32767, 0], [-32768, -32768], [10, 10]], np.int16), "cs16") == (
        4, 12, -32762, 9 + 32767**2 + 32768**2 + 100, 16 + 32768**2 + 100, -12 + 32768**2 + 100, 2)
    # CU8: x = 256 a - 32640; rails 0 and 255
    assert CR.stats(np.array([[0, 255], [128, 127], [255, 255]], np.uint8), "cu8") == (
        3, -32640 + 128 + 32640, 32640 - 128 + 32640, 2 * 32640**2 + 128**2, 2 * 32640**2 + 128**2, -32640**2 - 128**2 + 32640**2, 2)
    # CS8: x = 256 a; rails -128 and 127
    assert CR.stats(np.array([[-128, 1], [127, 127], [2, -3]], np.int8), "cs8") == (
        3, 256, 256 * 125, 65536 * (128**2 + 127**2 + 4), 65536 * (1 + 127**2 + 9), 65536 * (-128 + 127**2 - 6), 2)
    # CF32: x = sat16(rint(32768 a)); clipped: |a| >= 1 or not finite (NaN converts to 0 and still counts)
    raw = np.array([[1.0, 0.0], [np.nan, 0.5], [-0.25, np.inf], [0.999, -0.999], [-1.0, 0.0]], np.float32)
    x = FM.to_cs16(raw, "cf32").astype(np.int64)
    assert x.tolist() == [[32767, 0], [0, 16384], [-8192, 32767], [32735, -32735], [-32768, 0]]
    assert CR.stats(raw, "cf32") == (5, int(x[:, 0].sum()), int(x[:, 1].sum()), int((x[:, 0]**2).sum()), int((x[:, 1]**2).sum()),
                                     int((x[:, 0] * x[:, 1]).sum()), 4)
    # RS16: the three sums with xi are 0
    assert CR.stats(np.array([5, -32768, 32767, -7], np.int16), "rs16") == (4, -3, 0, 25 + 32768**2 + 32767**2 + 49, 0, 0, 2)


def test_estimator_failure_conditions_and_the_real_form():
    assert CR.estimate((1, 5, 5, 25, 25, 25, 0)) is None                      # n < 2
    assert CR.estimate((4, 40, 4, 400, 30, 40, 0)) is None                    # xr constant: v_rr = 0
    assert CR.estimate((4, 10, 20, 30, 120, 60, 0)) is None                   # xi = 2 xr: det = 0
    assert CR.estimate((4, 0, 0, 4 * 10**6, 4, 0, 0)) is None                 # gh = 1000: g out of range
    assert CR.estimate((4, 0, 0, 4, 4 * 10**4, 0, 0)) is None                 # gh = 0.01: g out of range
    assert CR.estimate((4, 0, 0, 400, 400, 300, 0)) is None                   # rho = 0.75: p = -74310 out of range
    assert CR.estimate((4, 0, 0, 400, 400, 0, 0)) == (0, 0, 0, 65536)
    assert CR.estimate((4, 10, 0, 30, 0, 0, 0)) == (2, 0, 0, 65536)           # RS16 form: rint(2.5) = 2, half to even
    assert CR.estimate((4, 14, 0, 49, 0, 0, 0)) == (4, 0, 0, 65536)           # RS16 form needs no variance: rint(3.5) = 4
    assert CR.estimate((1, 14, 0, 196, 0, 0, 0)) is None


def test_quality_known_answer():
    """65 536 samples of a tone of amplitude 12 000 on bin 5001, Q gain 1.06, phase error 4 degrees, DC (310.4, -777.3).  Bounds:
    a Q16 coefficient step bounds the residual image amplitude by 2^-17 = -102 dB, 12 dB are left for the input's own rounding:
    image <= -90 dB; a DC residual of at most 0.5 LSB per part is 0.707 / 12 000 = -84.6 dB: DC <= -84 dB.  Measured: image
    -26.8 dB before, -109.0 dB after; DC -87.5 dB after."""
    x = CR.known_answer_rows()
    before, _ = CR.image_and_dc_db(x)
    print("image before %.2f dB" % before)
    assert -27.5 < before < -26.0                              # the fault is there to correct
    st = CR.stats(x, "cs16")
    words = CR.estimate(st)
    print("words", words, "unrounded", CR.estimate(st, unrounded=True))
    image, dc = CR.image_and_dc_db(CR.condition(x, words))
    print("image after %.2f dB, DC after %.2f dB" % (image, dc))
    assert words == CR.KA_WORDS == (310, -777, -4583, 61977)
    assert image <= -90.0
    assert dc <= -84.0

