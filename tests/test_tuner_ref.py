"""Known answers of tests/tuner_ref.py, the numpy statement of the digital tuner's arithmetic (include/asdr_tuner.h) that the GPU
tests compare the HIP kernel with, and of the generated NCO table (audiosdr_amd/csrc/asdr_tuner_tables.h)."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import tuner_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def lowpass(D, L):
    """A plain windowed-sinc low-pass in Q15 (unit DC gain within rounding), for the tone tests."""
    n = np.arange(L) - (L - 1) / 2.0
    h = np.sinc(n / D * 0.8) * np.hamming(L)
    return np.round(32768.0 * h / h.sum()).astype(np.int64)


def test_nco_table_is_the_float64_formula():
    k = np.arange(4096)
    assert np.array_equal(R.NCO_C, np.round(32767.0 * np.cos(2 * np.pi * k / 4096)))
    assert (R.NCO_C[0], R.NCO_S[0], R.NCO_C[1024], R.NCO_S[1024], R.NCO_C[2048], R.NCO_S[3072]) == (32767, 0, 0, 32767, -32767, -32767)
    text = open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_tuner_tables.h")).read()
    words = [int(w, 16) for w in re.findall(r"\(int32_t\)0x([0-9a-f]{8})", text)]
    assert len(words) == 4096
    w = np.array(words, dtype=np.int64)
    c, s = (w & 0xFFFF).astype(np.uint16).view(np.int16), ((w >> 16) & 0xFFFF).astype(np.uint16).view(np.int16)
    assert np.array_equal(c, R.NCO_C) and np.array_equal(s, R.NCO_S)


def test_table_generator_check_passes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_tuner_tables.py"), "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_impulse_with_zero_frequency_gives_scaled_decimated_taps():
    D, L, g = 4, 23, 3
    h = np.arange(1, L + 1) * 37 - 300
    ref = R.TunerRef(1, 1, D, h, g)
    m0 = 5
    x = np.zeros((1, 128 * D, 2), dtype=np.int64)
    x[0, m0, 0] = 32767
    I, Q = ref.update(x)
    z0 = (32767 * 32767 + 16384) >> 15                       # theta = 0: C = 32767, S = 0
    assert z0 == 32766
    s, r = 15 - g, 1 << (14 - g)
    want = np.zeros(128, dtype=np.int64)
    for n in range(128):
        k = n * D + D - 1 - m0
        if 0 <= k < L:
            want[n] = max(-32768, min(32767, (int(h[k]) * z0 + r) >> s))
    assert np.array_equal(I[0, 0], want) and not Q.any()
    assert np.count_nonzero(want) == 6                      # taps k = 2, 6, ..., 22 of the 23


def test_rounding_at_half_lsb_and_saturation():
    # filter rounding: h = {1}, g = 14 -> (z + 1) >> 1: +1/2 rounds up, -1/2 rounds up to 0 (floor of the shifted sum)
    z = np.array([1, -1, 3, -3, 2, -2], dtype=np.int64)
    assert list(R.fir_decimate(z, [1], 1, 14, 6)) == [1, 0, 2, -1, 1, -1]
    # mixer rounding: (v + 16384) >> 15 with v = xr C[0] = -32767 -> floor(-0.49997) = -1; v = +32767 -> 1
    zr, zi = R.mix(np.array([-1, 1]), np.array([0, 0]), np.array([0, 0]))
    assert list(zr) == [-1, 1] and list(zi) == [0, 0]
    # mixer saturation: (-32768, -32768) at 45 degrees (C = S = 23170) -> -46340 -> -32768, and zi = 0
    zr, zi = R.mix(np.array([-32768]), np.array([-32768]), np.array([512 << 20]))
    assert (R.NCO_C[512], R.NCO_S[512]) == (23170, 23170) and zr[0] == -32768 and zi[0] == 0
    zr, zi = R.mix(np.array([32767]), np.array([-32768]), np.array([(4096 - 512) << 20]))   # C = 23170, S = -23170: zr = +46340
    assert zr[0] == 32767
    # output saturation: sum |h| = 65534 at g = 15 (s = 0)
    assert list(R.fir_decimate(np.array([32767, 32767, -32768, -32768]), [32767, 32767], 1, 15, 3)) == [32767, -32767, -32768]


def test_phase_wraps_at_2_to_the_32():
    assert list(R.theta(np.arange(4), 0, 0xFFFFFFF0, 0x8)) == [0xFFFFFFF0, 0xFFFFFFF8, 0, 8]
    assert list(R.theta(np.array([10**12, 10**12 + 1]), 0, 0, 1 << 31)) == [0, 1 << 31]
    # (m - pos_a) * fw is taken mod 2^32 even when the product exceeds 64 bits
    m = np.array([(1 << 40) + 3])
    assert int(R.theta(m, 0, 7, 0xFFFFFFFF)[0]) == (7 + ((1 << 40) + 3) * 0xFFFFFFFF) % (1 << 32)


def tone(f, fs, n, amp=12000.0, m0=0):
    m = np.arange(m0, m0 + n)
    ph = 2 * np.pi * f * m / fs
    return np.stack([np.round(amp * np.cos(ph)), np.round(amp * np.sin(ph))], axis=-1).astype(np.int64)


def test_tone_tuned_to_its_frequency_is_constant_after_the_transient():
    D, L = 8, 97
    fs = 44100.0 * D
    f = 52_345.0
    ref = R.TunerRef(1, 1, D, lowpass(D, L), 0)
    ref.set_frequency(f)
    I, Q = ref.update(tone(f, fs, 4 * 128 * D)[None])
    i, q = I.reshape(-1)[L // D + 1:].astype(float), Q.reshape(-1)[L // D + 1:].astype(float)
    assert abs(i.mean() - 12000) < 40 and i.std() < 8 and abs(q).max() < 40, (i.mean(), i.std(), abs(q).max())
    assert abs(I.reshape(-1)[0]) < abs(i.mean()) / 2                 # the transient: the history before P = 0 is zeros


def test_tone_offset_by_delta_appears_at_delta():
    D, L = 4, 49
    fs = 44100.0 * D
    f, delta = -30_000.0, 1_500.0
    ref = R.TunerRef(1, 1, D, lowpass(D, L), 0)
    ref.set_frequency(f)
    I, Q = ref.update(tone(f + delta, fs, 32 * 128 * D)[None])
    z = (I.reshape(-1) + 1j * Q.reshape(-1).astype(float))[64:]
    spec = np.abs(np.fft.fft(z * np.hanning(z.size)))
    peak = np.fft.fftfreq(z.size, 1 / 44100.0)[np.argmax(spec)]
    assert abs(peak - delta) < 44100.0 / z.size * 1.5, peak


def test_retune_flushes_history_and_keeps_the_phase_continuous():
    D, L = 1, 9
    ref = R.TunerRef(1, 1, D, [4096] * L, 0)
    fw = R.fw_from_hz(3000.0, D)
    ref.set_frequency_word(fw)
    x = tone(7000.0, 44100.0, 128 * 3)
    ref.update(x[None, :128])
    P = ref.P
    th_before = int(R.theta(P, ref.pos_a[0], ref.ph_a[0], ref.fw[0]))
    ref.set_frequency_word(fw)                                     # same value: still a retune
    assert ref.pos_a[0] == P and ref.ph_a[0] == th_before
    I, _ = ref.update(x[None, 128:256])
    zr, zi = ref.z(0, np.arange(P - 4, P + 4))
    assert not zr[:4].any() and not zi[:4].any() and zr[4:].any()
    # the phase continues: z after the retune equals z of a channel that never retuned
    cont = R.TunerRef(1, 1, D, [4096] * L, 0)
    cont.set_frequency_word(fw)
    cont.update(x[None, :128]); cont.update(x[None, 128:256])
    a, b = ref.z(0, np.arange(P, P + 64)), cont.z(0, np.arange(P, P + 64))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the first output after the retune sees one sample only (L = 9, D = 1: output n uses samples n - 8 .. n)
    zr0 = int(ref.z(0, np.array([P]))[0][0])
    assert I[0, 0, 0] == (4096 * zr0 + 16384) >> 15
    # set_phase sets the anchor phase itself
    ref.set_phase(123 << 20)
    assert ref.ph_a[0] == 123 << 20 and ref.pos_a[0] == ref.P


def test_frequency_word_rounding():
    assert R.fw_from_hz(0.0, 1) == 0
    assert R.fw_from_hz(22050.0, 1) == 1 << 31
    assert R.fw_from_hz(-22050.0, 1) == 1 << 31
    assert R.fw_from_hz(-1.0, 48) == (2**32 - round(2**32 / (44100.0 * 48))) & 0xFFFFFFFF
    assert R.fw_from_hz(44100.0 * 2 / 2**32 * 0.5, 2) == 1                   # exactly half a word: away from zero


def small_taps(rng, L):
    """L random taps with sum |h| <= 65535."""
    return rng.integers(-60, 60, size=L, endpoint=True)


PLACED_FWS = [0, 1 << 31, 0x01234567, 0xFFFFFFFF, R.fw_from_hz(-7_123.5, 1), 0x80000001]


def placed_pair(D, L, rng):
    h = small_taps(rng, L)
    a, b = (R.TunerRef(len(PLACED_FWS), 2, D, h, 2) for _ in range(2))
    for o in (a, b):
        for c, fw in enumerate(PLACED_FWS):
            o.set_source(c % 2, ch=c); o.set_frequency_word(fw, ch=c)
        o.set_phase(0xCAFEF00D, ch=3)
    return a, b


def retunes(rng, L):
    """One setter of every kind, a filter change and the all-channel forms."""
    h1 = small_taps(rng, max(1, L - 8))
    return [lambda o: o.set_frequency(12_345.6, ch=1),
            lambda o: o.set_frequency_word(0x0FEDCBA9, ch=0),
            lambda o: o.set_phase(0xDEADBEEF, ch=3),
            lambda o: o.set_source(0, ch=5),
            lambda o: o.set_filter(h1, 3),
            lambda o: o.set_phase(77 << 20),
            lambda o: o.set_frequency(-40_000.0),
            lambda o: o.set_source(1)]


def same_state(a, b):
    return a.P == b.P and all(list(getattr(a, k)) == list(getattr(b, k)) for k in ("src", "fw", "pos_a", "ph_a"))


@pytest.mark.parametrize("D,L", [(7, 85), (64, 1024)])
def test_a_placed_reference_equals_a_stepped_one(D, L):
    """place_at(P, tail) against 281 blocks of stepping, the same buffer of 20 blocks fed over and over as the GPU suite feeds its
    banks (tests/test_gpu_tuner_positions.py places references past 2^30 and 2^32, where stepping is out of reach).  One channel
    is retuned during the feed -- the placed reference is moved there by place_at(P) alone -- and the last call is one block, so
    that at D = 7 the tail of 1024 samples spans two calls.  Then every kind of retune: the next calls' I and Q bit for bit, P and
    the anchors."""
    rng = np.random.default_rng(300 + D)
    blk = 128 * D
    a, b = placed_pair(D, L, rng)
    fed = rng.integers(-20000, 20000, size=(2, 20 * blk, 2), endpoint=True)
    counts = []
    for rep in range(14):
        if rep == 6:
            b.place_at(a.P)
            for o in (a, b):
                o.set_frequency_word(0x2468ACE1, ch=2); o.set_phase(0x13579BDF, ch=4)
        a.update(fed)
        counts.append(fed.shape[1])
    a.update(fed[:, :blk])
    counts.append(blk)
    b.place_at(a.P, R.fed_tail(fed, counts, 1024))
    assert b.x0 == b.P - 1024 and same_state(a, b) and a.P == 281 * blk
    assert list(a.pos_a) == [0, 0, 120 * blk, 0, 120 * blk, 0]
    for k, st in enumerate([lambda o: None] + retunes(rng, L)):
        st(a); st(b)
        iq = rng.integers(-20000, 20000, size=(2, (1 + k % 3) * blk, 2), endpoint=True)
        (aI, aQ), (bI, bQ) = a.update(iq), b.update(iq)
        assert np.array_equal(aI, bI) and np.array_equal(aQ, bQ), k
        assert same_state(a, b), k
    assert aI.any() and aQ.any()


@pytest.mark.parametrize("D,L", [(7, 85), (64, 1024)])
def test_placed_past_2_to_the_32_nothing_overflows(D, L):
    """A reference placed 12,345 blocks past 2^32 (at D = 64 that is 2^32 + 12,345 * 128 D; at D = 7 the first block boundary
    past 2^32 takes the place of 2^32) with a seeded tail, two calls with a retune between them, every numpy warning and
    floating-point flag an error.  The outputs equal those of a reference placed at 12,345 * 128 D with the same tail, whose
    anchor phases were advanced by the distance between the two in Python integers."""
    rng = np.random.default_rng(32 + D)
    blk = 128 * D
    far, near = placed_pair(D, L, rng)
    tail = rng.integers(-20000, 20000, size=(2, 1500, 2), endpoint=True)
    P_far, P_near = (-(-(1 << 32) // blk) + 12345) * blk, 12345 * blk
    for c in range(near.n):
        near.ph_a[c] = (int(near.ph_a[c]) + (P_far - P_near) * int(near.fw[c])) % (1 << 32)
    with warnings.catch_warnings(), np.errstate(all="raise"):
        warnings.simplefilter("error")
        far.place_at(P_far, tail)
        near.place_at(P_near, tail)
        for k in range(2):
            iq = rng.integers(-20000, 20000, size=(2, (2 - k) * blk, 2), endpoint=True)
            (fI, fQ), (nI, nQ) = far.update(iq), near.update(iq)
            assert np.array_equal(fI, nI) and np.array_equal(fQ, nQ) and fI.any()
            assert far.P == near.P + P_far - P_near
            for o in (far, near):
                o.set_frequency_word(0x0FEDCBA9, ch=1); o.set_frequency(-1_234.5)
            assert list(far.ph_a) == list(near.ph_a)
            assert list(far.pos_a) == [far.P] * far.n and int(far.P) > 1 << 32


def test_a_read_outside_the_held_tail_raises():
    """z() never makes up a sample: before the tail's first sample, after its last, and in an update() that follows a place_at(P)
    without a tail (unless every channel was re-anchored at P: then nothing before P is read)."""
    D, L = 7, 85
    rng = np.random.default_rng(8)
    blk = 128 * D
    ref, _ = placed_pair(D, L, rng)
    tail = rng.integers(-20000, 20000, size=(2, 1024, 2), endpoint=True)
    P = 5000 * blk
    ref.place_at(P, tail)
    ref.z(0, np.arange(P - 1024, P))
    for m in (P - 1025, P):
        with pytest.raises(AssertionError, match="outside"):
            ref.z(0, np.array([m]))
    with pytest.raises(AssertionError):
        ref.place_at(P, tail[:, :1023])                                # shorter than the longest filter's reach
    iq = rng.integers(-20000, 20000, size=(2, blk, 2), endpoint=True)
    ref.place_at(P)
    with pytest.raises(AssertionError, match="outside"):
        ref.update(iq)
    ref.place_at(P)
    ref.set_phase(0)                                                   # every anchor at P: zeros before it, by the statement
    I, _ = ref.update(iq)
    assert I.any() and ref.P == P + blk
