"""Source conditioning of the digital tuner (include/asdr_tuner.h, "Source conditioning") on ASDR_NO_DEVICE banks of all three
kinds: the creation state, the ranges and that a rejected call keeps the old state, ASDR_ALL, reset, the reads that need a device,
and the estimator asdr_tuner_iq_estimate against the restatement tests/tuner_condition_ref.py -- on the quality known answer, on
200 seeded random statistics and on each of its failure conditions."""
import ctypes
import os
import re

import numpy as np
import pytest

import tuner_condition_ref as CR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW = ["asdr_tuner_set_iq_correction", "asdr_tuner_get_iq_correction", "asdr_tuner_iq_stats_enable", "asdr_tuner_iq_stats_enabled",
       "asdr_tuner_iq_stats_read", "asdr_tuner_iq_stats_clear", "asdr_tuner_iq_estimate", "asdr_tuner_iq_track",
       "asdr_tuner_condition_launches"]


def banks(A, n_src=3):
    return [("plain", A.TunerBank(4, n_src, 4, device=A.NO_DEVICE)),
            ("rate", A.TunerBank(4, n_src, 50, fs_in=2400000, device=A.NO_DEVICE)),
            ("fastconv", A.TunerBank.fastconv(4, n_src, 2400000, 16, device=A.NO_DEVICE))]


def test_the_new_symbols_are_declared_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_tuner.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = ctypes.CDLL(A.library_path())
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text) and hasattr(L, n) and n in A.TUNER_EXPORTS, n
    assert A.IQ_CORRECTION_DTYPE.itemsize == 16 and A.IQ_STATS_DTYPE.itemsize == 56
    assert A.IQ_STATS_DTYPE.names == CR.STAT_NAMES


def test_creation_state_ranges_and_rejection_keeps_the_state(A):
    good = (-123, 456, -7890, 70000)
    for kind, t in banks(A):
        assert all(t.iq_correction(s) == CR.IDENTITY == A.IQ_IDENTITY for s in range(3)), kind
        assert not t.iq_stats_enabled() and t.condition_launches() == 0
        t.set_iq_correction(words=good, source=1)
        for k, (lo, hi) in enumerate(CR.RANGES):
            for v in (lo, hi):                                 # both ends of every range are taken
                w = list(good); w[k] = v
                t.set_iq_correction(words=w, source=2)
                assert t.iq_correction(2) == tuple(w), (kind, k, v)
            for v in (lo - 1, hi + 1, -2**31, 2**31 - 1):      # one past them is not
                w = list(CR.IDENTITY); w[k] = v
                for source in (0, 1, A.ALL):
                    with pytest.raises(A.AsdrError, match="must be in"):
                        t.set_iq_correction(words=w, source=source)
        for source in (-2, 3, 1 << 20):
            with pytest.raises(A.AsdrError, match="source index"):
                t.set_iq_correction(words=good, source=source)
            with pytest.raises(A.AsdrError, match="source index"):
                t.iq_correction(source)
        with pytest.raises(A.AsdrError, match="source index"):
            t.iq_correction(A.ALL)
        assert t.iq_correction(0) == CR.IDENTITY and t.iq_correction(1) == good, kind
        assert t.iq_correction(2) == (good[0], good[1], good[2], CR.RANGES[3][1]), kind
        L, h = t._L, t._h
        assert L.asdr_tuner_set_iq_correction(h, 0, None) == -1 and L.asdr_tuner_get_iq_correction(h, 0, None) == -1
        assert L.asdr_tuner_set_iq_correction(None, 0, None) == -1 and L.asdr_tuner_condition_launches(None) == -1
        assert L.asdr_tuner_iq_stats_enabled(None) == 0


def test_all_sources_floats_and_reset(A):
    for kind, t in banks(A):
        t.set_iq_correction(dc=(310.4, -777.3), cross=-0.0699, gain=0.9457)
        want = (310, -777, int(np.rint(-0.0699 * 65536)), int(np.rint(0.9457 * 65536)))
        assert want == (310, -777, -4581, 61977)
        assert [t.iq_correction(s) for s in range(3)] == [want] * 3, kind
        t.set_iq_correction(source=1)                          # the defaults are the identity
        assert t.iq_correction(1) == CR.IDENTITY and t.iq_correction(0) == want and t.iq_correction(2) == want
        with pytest.raises(A.AsdrError, match="gain_q16"):
            t.set_iq_correction(gain=2.5)
        with pytest.raises(A.AsdrError, match="cross_q16"):
            t.set_iq_correction(cross=0.51)
        t.enable_iq_stats()
        t.set_input_format("cu8")
        t.reset()                                              # keeps the corrections, as it keeps the format
        assert [t.iq_correction(s) for s in range(3)] == [want, CR.IDENTITY, want], kind
        assert t.iq_stats_enabled() and t.input_format() == "cu8" and t.position() == 0


def test_reads_need_a_device_and_the_statistics_on(A):
    for kind, t in banks(A):
        for call in (t.iq_stats, t.clear_iq_stats, t.track_iq):
            with pytest.raises(A.AsdrError, match="statistics are off"):
                call()
        t.enable_iq_stats()
        assert t.iq_stats_enabled()
        for call in (t.iq_stats, lambda: t.iq_stats(clear=False), t.clear_iq_stats, t.track_iq, lambda: t.track_iq(1)):
            with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
                call()
        with pytest.raises(A.AsdrError, match="source index"):
            t.track_iq(3)
        t.enable_iq_stats(False)
        assert not t.iq_stats_enabled() and t.condition_launches() == 0, kind
        assert all(t.iq_correction(s) == CR.IDENTITY for s in range(3))


def test_estimate_equals_the_restatement_on_the_known_answer(A):
    st = CR.stats(CR.known_answer_rows(), "cs16")
    assert A.estimate_iq_correction(st) == CR.estimate(st) == CR.KA_WORDS
    rec = np.zeros(1, dtype=A.IQ_STATS_DTYPE)
    for k, v in zip(CR.STAT_NAMES, st):
        rec[k] = v
    assert A.estimate_iq_correction(rec[0]) == CR.KA_WORDS     # an element of TunerBank.iq_stats()


def random_stats(seed):
    """The sums of 64 .. 4095 samples of Gaussian noise through a random gain (0.8 .. 1.25) and phase (+-15 degrees) imbalance with
    a random DC offset (+-3000), as int16."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(64, 4096))
    g, ph = rng.uniform(0.8, 1.25), np.deg2rad(rng.uniform(-15, 15))
    amp = rng.uniform(200, 9000)
    dc = rng.uniform(-3000, 3000, size=2)
    i, q0 = rng.normal(0, amp, n), rng.normal(0, amp, n)
    q = g * (q0 * np.cos(ph) + i * np.sin(ph))
    x = np.clip(np.rint(np.stack([i + dc[0], q + dc[1]], -1)), -32768, 32767).astype(np.int16)
    return CR.stats(x, "cs16")


def test_estimate_equals_the_restatement_on_200_random_statistics(A):
    """Seeds 0 .. 199, chosen (checked here, on every run) so that no unrounded word lies within 1e-6 of a half-integer: a last-bit
    difference between two correct float64 evaluations could not move a word."""
    seen = set()
    for seed in range(200):
        st = random_stats(seed)
        raw = CR.estimate(st, unrounded=True)
        assert raw is not None and min(abs((v % 1.0) - 0.5) for v in raw) >= 1e-6, (seed, raw)
        want = CR.estimate(st)
        assert A.estimate_iq_correction(st) == want, (seed, st, want)
        seen.add(want)
    assert len(seen) == 200


FAILURES = [((1, 5, 5, 25, 25, 25, 0), "fewer than two"), ((0, 0, 0, 0, 0, 0, 0), "fewer than two"),
            ((-3, 0, 0, 0, 1, 0, 0), "fewer than two"),
            ((4, 40, 4, 400, 30, 40, 0), "no variance"),                       # xr constant
            ((4, 10, 20, 30, 120, 60, 0), "fully correlated"),                 # xi = 2 xr
            ((4, 10, 4, 30, 4, 10, 0), "fully correlated"),                    # xi constant: v_ii = 0
            ((4, 0, 0, 4 * 10**6, 4, 0, 0), "outside its range"),              # gh = 1000
            ((4, 0, 0, 4, 4 * 10**4, 0, 0), "outside its range"),              # gh = 0.01
            ((4, 0, 0, 400, 400, 300, 0), "outside its range"),                # p = -74310
            ((4, 160000, 0, 4 * 40000**2 + 4, 4, 0, 0), "outside its range"),  # m_r = 40000
            ((4, 200000, 0, 10**10, 0, 0, 0), "outside its range")]            # RS16 form, d_r = 50000


def test_each_failure_condition_of_the_estimator(A):
    L = A.TunerBank(1, 1, 1, device=A.NO_DEVICE)._L
    for st, why in FAILURES:
        assert CR.estimate(st) is None, st
        with pytest.raises(A.AsdrError, match=why):
            A.estimate_iq_correction(st)
        rec = np.array([st], dtype=A.IQ_STATS_DTYPE)
        out = np.array([(11, 22, 33, 44)], dtype=A.IQ_CORRECTION_DTYPE)
        assert L.asdr_tuner_iq_estimate(rec.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert out[0].tolist() == (11, 22, 33, 44), st          # the output is untouched
    assert L.asdr_tuner_iq_estimate(None, None) == -1
    # the RS16 form: the three sums with xi all zero give d_r alone, and need no variance
    for st in ((4, 10, 0, 30, 0, 0, 0), (4, 14, 0, 49, 0, 0, 0), (1000, -777300, 0, 10**12, 0, 0, 17)):
        assert A.estimate_iq_correction(st) == CR.estimate(st) == (int(np.rint(st[1] / st[0])), 0, 0, 65536)
