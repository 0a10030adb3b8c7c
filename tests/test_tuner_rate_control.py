"""Rate banks of the digital tuner (include/asdr_tuner.h, "Rate banks") on ASDR_NO_DEVICE banks: creation constraints, U / M,
the frequency word at Fs_in, the set_resampler rules, the block timing against tests/tuner_rate_ref.py, the default filters'
responses, and the reference's stage 2 against a direct float64 statement."""
import warnings

import numpy as np
import pytest

import tuner_rate_ref as RR
import tuner_ref as R

EXAMPLES = {(48000, 1): (147, 160), (96000, 1): (147, 320), (2400000, 50): (147, 160), (2048000, 32): (441, 640),
            (10000000, 64): (882, 3125), (7 * 44100, 7): (1, 1), (192000, 2): (147, 320), (3000000, 20): (147, 500)}


@pytest.fixture
def T(A):
    return lambda fs, D, n=4, s=2: A.TunerBank(n, s, D, fs_in=fs, device=A.NO_DEVICE)


def test_creation_constraints_and_messages(A, T):
    for fs, D, what in ((2400001, 50, "multiple"), (2400000, 7, "multiple"), (44099, 1, r"\[44100, 176400\]"),
                        (176401, 1, r"\[44100, 176400\]"), (2400000, 64, r"\[44100, 176400\]"), (64 * 176400 + 64, 64, r"\[44100, 176400\]"),
                        (88200 * 40, 100, "decimation"), (0, 1, "positive"), (-48000, 1, "positive"),
                        (44101, 1, "U > 2048"), (96001 * 2, 2, "U > 2048")):
        with pytest.raises(A.AsdrError, match=what):
            T(fs, D)
    with pytest.raises(A.AsdrError, match="n_channels"):
        A.TunerBank(0, 1, 1, fs_in=48000, device=A.NO_DEVICE)
    t = T(176400, 1)                                            # the edges are accepted
    assert t.ratio() == (1, 4) and t.fs_in == 176400
    assert T(44100, 1).ratio() == (1, 1)


def test_ratio_of_the_examples(T):
    for (fs, D), ud in EXAMPLES.items():
        t = T(fs, D)
        assert t.ratio() == ud == RR.ratio(fs, D), (fs, D)
        assert t.fs_in == fs and t.decimation == D and t.output_position() == 0


def test_plain_bank_is_a_rate_bank_at_d_times_44100(A, T):
    for D in (1, 2, 7, 48, 64):
        p = A.TunerBank(3, 2, D, device=A.NO_DEVICE)
        r = T(44100 * D, D, 3, 2)
        assert p.fs_in == 44100 * D and p.ratio() == r.ratio() == (1, 1)
        hp, gp = p.get_filter()
        hr, gr = r.get_filter()
        assert np.array_equal(hp, hr) and gp == gr
        assert p.get_resampler() == r.get_resampler() or (list(p.get_resampler()[0]) == [16384] == list(r.get_resampler()[0]))
        assert r.get_resampler()[1] == 1 and p.out_blocks(5) == r.out_blocks(5) == 5


def test_frequency_word_rounding_at_the_bank_rate(A, T):
    for fs, D in ((48000, 1), (2400000, 50), (10000000, 64), (2048000, 32)):
        t = T(fs, D, 2, 1)
        for hz in (0.0, 1.0, -1.0, 1234.5678, -fs / 2, fs / 2, fs / 3, -fs / 7, 0.5 * fs / 2 ** 32 * 3, 100_000.25):
            if abs(hz) > fs / 2:
                continue
            t.set_frequency(hz, ch=1)
            assert int(t.read_state()["fw"][1]) == RR.fw_from_hz(hz, fs), (fs, hz)
        for bad in (fs / 2 * (1 + 1e-12), -fs / 2 - 1.0, float("nan")):
            with pytest.raises(A.AsdrError, match="frequency"):
                t.set_frequency(bad, ch=0)
    assert RR.fw_from_hz(1234.5, 44100 * 7) == R.fw_from_hz(1234.5, 7)


def test_resampler_rules(A, T):
    t = T(2048000, 32, 1, 1)
    U, M = t.ratio()
    h0, g0 = t.get_resampler()
    assert h0.size == U * 18 and g0 == 0
    bad = [(np.ones(U + 1), 0, "multiple of U"), (np.ones(U - 1), 0, "multiple of U"), (np.zeros(0), 0, "multiple of U"),
           (np.ones(U * 65), 0, "1..64"), (np.ones(U * 2), 16, "gain"), (np.ones(U * 2), -1, "gain")]
    heavy = np.zeros(U * 3, dtype=np.int16)
    heavy[[5, U + 5, 2 * U + 5]] = [32767, 32767, 2]                       # phase 5 sums to 65536
    bad.append((heavy, 0, "65535"))
    for h, g, what in bad:
        with pytest.raises(A.AsdrError, match=what):
            t.set_resampler(np.asarray(h, dtype=np.int16), g)
        h1, g1 = t.get_resampler()
        assert np.array_equal(h1, h0) and g1 == g0                          # the old resampler is kept
    heavy[2 * U + 5] = 1                                                   # exactly 65535: accepted
    t.set_resampler(heavy, 15)
    h1, g1 = t.get_resampler()
    assert np.array_equal(h1, heavy) and g1 == 15
    t.set_resampler(np.arange(U * 64, dtype=np.int64) % 7 - 3, 2)          # K = 64
    assert t.get_resampler()[0].size == U * 64


def test_out_blocks_against_the_reference_over_long_irregular_runs(A, T):
    """The C count from a fresh bank for every frame count a call can take, and the reference's timing over long irregular runs
    (every written block complete, the next one not, 0 .. n_frames + 1 blocks per call, 0-block calls).  The C count after real
    calls and after reset is compared with the reference on the GPU (test_gpu_tuner_rate.py)."""
    rng = np.random.default_rng(7)
    for fs, D in ((48000, 1), (96000, 1), (2048000, 32), (10000000, 64), (3000000, 20), (176400, 1), (44100 * 5, 5)):
        U, M = RR.ratio(fs, D)
        t = T(fs, D, 1, 1)
        for nf in list(range(0, 40)) + [255, 1000, 4097, 65535]:
            assert t.out_blocks(nf) == RR.blocks_out(128 * nf, U, M), (fs, D, nf)
        with pytest.raises(A.AsdrError, match="n_frames"):
            t.out_blocks(65536)
        n_u, out, zeros = 0, 0, 0
        for call in range(3000):
            nf = int(rng.choice([1, 1, 2, 3, 7, 16]))
            nb = max(0, RR.blocks_out(n_u + 128 * nf, U, M) - out)
            assert 0 <= nb <= nf + 1
            zeros += nb == 0
            n_u += 128 * nf
            out += nb
            b_last, _ = RR.b_phi(128 * out - 1, U, M)
            b_next, _ = RR.b_phi(128 * out + 127, U, M)
            assert b_last <= n_u - 1 < b_next                               # written blocks complete, the next one not
        assert (zeros > 0) == (M > U)


def test_out_blocks_is_exact_far_out(A, T):
    """64-bit positions: after 2^40 output samples the count still follows b_j exactly (no j M overflow)."""
    for fs, D in ((10000000, 64), (48000, 1), (2048000, 32)):
        U, M = RR.ratio(fs, D)
        for j_out in (1 << 40, (1 << 41) + 128 * 12345):
            n_u = (j_out * M) // U + 3
            nb = RR.blocks_out(n_u, U, M)
            b, _ = RR.b_phi(128 * nb - 1, U, M)
            b2, _ = RR.b_phi(128 * nb + 127, U, M)
            assert b <= n_u - 1 < b2
            assert b == (128 * nb - 1) * M // U                             # Python ints: no overflow anywhere


def test_suggest_decimation(A):
    assert A.suggest_decimation(48000) == 1
    assert A.suggest_decimation(2400000) == 50
    assert A.suggest_decimation(10000000) == 64
    assert A.suggest_decimation(44100 * 64) == 64
    assert A.suggest_decimation(2048000) == 40                             # 51.2 kHz: U / M = 441 / 512
    assert A.suggest_decimation(44099) is None and A.suggest_decimation(64 * 176400 + 1) is None
    assert A.suggest_decimation(44101) is None                             # no D gives U <= 2048
    for fs in (48000, 96000, 192000, 2048000, 2400000, 3000000, 6000000, 8000000, 10000000, 250000):
        D = A.suggest_decimation(fs)
        A.TunerBank(1, 1, D, fs_in=fs, device=A.NO_DEVICE).close()        # valid
        for D2 in range(D + 1, 65):
            assert A.rate_ratio(fs, D2) is None
            with pytest.raises(A.AsdrError):
                A.TunerBank(1, 1, D2, fs_in=fs, device=A.NO_DEVICE)


def response_db(h, fs, nfft=1 << 21):
    """(f, |H(f)| in dB) of Q15 taps h at rate fs, on an nfft-point grid from 0 to fs / 2."""
    H = np.abs(np.fft.rfft(h.astype(np.float64) / 32768.0, nfft))
    return np.arange(H.size) * fs / nfft, 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("fs,D", [(2400000, 50), (2048000, 32), (10000000, 64), (3000000, 20), (192000, 2), (48000, 1)])
def test_default_responses(T, fs, D):
    t = T(fs, D, 1, 1)
    mid = fs // D
    U, M = t.ratio()
    h, g = t.get_filter()
    if D > 1:
        assert g == 0 and np.array_equal(h, h[::-1]) and np.abs(h.astype(int)).sum() <= 65535
        L1 = 2 * -(-6 * D * mid * 20900 // (44100 * (mid - 23200))) + 1
        assert h.size == L1 <= 769
        f, db = response_db(h, fs, 1 << 20)
        p = db[f <= 11200]
        assert p.max() - p.min() <= 0.05 and abs(p.mean()) < 0.05, (p.min(), p.max())
        # everything that folds into 0 - 12 kHz at Fs_mid: |f - k Fs_mid| <= 12 kHz for some k >= 1
        folds = np.abs(f - np.round(f / mid) * mid) <= 12000
        assert -db[folds & (f >= mid - 12000)].max() >= 60.0
    else:
        assert list(h) == [16384] and g == 1
    h2, g2 = t.get_resampler()
    K = h2.size // U
    assert g2 == 0 and K == 2 * -(-6 * mid // 44100)
    phases = h2.reshape(K, U).astype(np.int64)
    assert (phases.sum(axis=0) == 32768).all() and (np.abs(phases).sum(axis=0) <= 65535).all()
    f, db = response_db(h2, U * mid)                                        # the prototype, at U Fs_mid
    db -= 20 * np.log10(U)
    p = db[f <= 11200]
    assert p.max() - p.min() <= 0.05 and abs(p.mean()) < 0.05, (p.min(), p.max())
    assert -db[f >= 44100 - 12000].max() >= 80.0                            # what folds into 0 - 12 kHz at 44.1 kHz, and the images


def test_reference_stage2_against_zero_stuff_filter_keep(A):
    """y = every M-th sample of (u zero-stuffed by U, filtered by h2 at the prototype rate), in float64, before rounding."""
    rng = np.random.default_rng(3)
    for U, M, K in ((3, 4, 5), (147, 160, 4), (1, 3, 6), (2, 7, 3)):
        h2 = rng.integers(-3000, 3000, size=U * K)
        u = rng.integers(-32768, 32768, size=(2, 400))
        g2 = 0
        n = (400 * U) // M - 2
        got = RR.resample(u, h2, U, M, g2, 0, n)
        z = np.zeros((2, 400 * U))
        z[:, ::U] = u
        full = np.stack([np.convolve(z[c], h2.astype(np.float64))[: 400 * U] for c in range(2)])
        want = np.clip(np.floor((full[:, ::M][:, :n] + 16384) / 32768.0), -32768, 32767)
        assert np.array_equal(got, want), (U, M, K)


def test_rate_bank_update_calls_need_a_device(A, T):
    t = T(48000, 1, 2, 1)
    with pytest.raises(A.AsdrError, match="HIP device"):
        t.update_rate(np.zeros((1, 128, 2), dtype=np.int16))
    with pytest.raises(A.AsdrError):
        t.update(np.zeros((1, 128, 2), dtype=np.int16))


PLACED = {(48000, 1): (33, 12), (10000000, 64): (1024, 64)}         # (Fs_in, D): (L, K)


def placed_pair(fs, D, rng, n_ch=3):
    L, K = PLACED[fs, D]
    U, _ = RR.ratio(fs, D)
    h, h2 = rng.integers(-60, 60, size=L, endpoint=True), rng.integers(-500, 500, size=U * K, endpoint=True)
    a, b = (RR.TunerRateRef(n_ch, 1, D, fs, h, 2, h2, 1) for _ in range(2))
    for o in (a, b):
        for c, fw in enumerate([0x01234567, 1 << 31, 0xFFFFFFFF][:n_ch]):
            o.set_frequency_word(fw, ch=c)
        o.set_phase(0xCAFEF00D, ch=1)
    return a, b


def cs16(rng, n):
    return rng.integers(-20000, 20000, size=(1, n, 2), endpoint=True)


def same_state(a, b):
    return a.P == b.P and a.out_pos == b.out_pos and all(list(getattr(a, k)) == list(getattr(b, k)) for k in ("src", "fw", "pos_a", "ph_a"))


@pytest.mark.parametrize("fs,D", list(PLACED))
def test_a_placed_rate_reference_equals_a_stepped_one(fs, D):
    """TunerRateRef.place_at(P, tail) against 281 frames of stepping, one buffer of 20 frames fed over and over as the GPU suite
    feeds its banks (tests/test_gpu_tuner_positions.py places references where stepping is out of reach).  A channel is retuned
    during the feed (the placed reference is moved there by place_at(P) alone).  The tail is exactly as long as place_at asks.
    Then a retune of every kind, a new resampler and a new filter: the next calls' I and Q and block counts bit for bit, both
    positions and the anchors."""
    rng = np.random.default_rng(fs + D)
    blk = 128 * D
    a, b = placed_pair(fs, D, rng)
    L, K = PLACED[fs, D]
    fed = cs16(rng, 20 * blk)
    counts = []
    for rep in range(14):
        if rep == 6:
            b.place_at(a.P)
            for o in (a, b):
                o.set_frequency_word(0x2468ACE1, ch=2)
        a.update(fed)
        counts.append(fed.shape[1])
    a.update(fed[:, :blk])
    counts.append(blk)
    T = max(1024, a.tail_needed())
    assert a.tail_needed() == max(L - D, 0) + D * (K - 1 + -(-127 * a.M // a.U) + 2)
    b.place_at(a.P, R.fed_tail(fed, counts, T))
    assert same_state(a, b) and a.P == 281 * blk and b.u0 > 0
    h1, r1 = rng.integers(-60, 60, size=L - 8, endpoint=True), rng.integers(-500, 500, size=a.U * 7, endpoint=True)
    steps = [lambda o: None,
             lambda o: o.set_frequency(1_234.5, ch=1),
             lambda o: o.set_frequency_word(0x0FEDCBA9, ch=0),
             lambda o: o.set_phase(0xDEADBEEF, ch=2),
             lambda o: o.set_source(0, ch=1),
             lambda o: o.set_resampler(r1, 2),
             lambda o: o.set_filter(h1, 3),
             lambda o: o.set_phase(77 << 20),
             lambda o: o.set_frequency(-7_000.0)]
    for k, st in enumerate(steps):
        st(a); st(b)
        iq = cs16(rng, (1, 2, 7)[k % 3] * blk)
        assert a.out_blocks(iq.shape[1] // blk) == b.out_blocks(iq.shape[1] // blk)
        (aI, aQ), (bI, bQ) = a.update(iq), b.update(iq)
        assert np.array_equal(aI, bI) and np.array_equal(aQ, bQ), k
        assert same_state(a, b), k
    assert aI.any() and aQ.any()


@pytest.mark.parametrize("fs,D", list(PLACED))
def test_rate_reference_placed_past_2_to_the_32_nothing_overflows(fs, D):
    """Placed at 2^32 + 12,345 * 128 D with a seeded tail, then two calls with a retune between them, every numpy warning and
    floating-point flag an error; the block counts and positions against Python-integer arithmetic."""
    rng = np.random.default_rng(fs - D)
    blk = 128 * D
    ref, _ = placed_pair(fs, D, rng)
    P = (1 << 32) + 12345 * blk
    with warnings.catch_warnings(), np.errstate(all="raise"):
        warnings.simplefilter("error")
        ref.place_at(P, cs16(rng, max(1024, ref.tail_needed())))
        assert ref.out_pos == 128 * RR.blocks_out(P // D, ref.U, ref.M)
        for nf in (7, 16):
            n = ref.out_blocks(nf)
            I, Q = ref.update(cs16(rng, nf * blk))
            P += nf * blk
            assert n >= 1 and I.shape == (3, n, 128) and I.any() and Q.any()
            assert ref.P == P and ref.out_pos == 128 * RR.blocks_out(P // D, ref.U, ref.M)
            assert (128 * RR.blocks_out(P // D, ref.U, ref.M) - 1) * ref.M // ref.U <= P // D - 1      # the last block out is complete
            ref.set_frequency(-1_234.5)
            assert list(ref.pos_a) == [P] * 3


def test_a_rate_reference_read_outside_what_it_holds_raises():
    """Neither stage makes up a sample: a tail shorter than place_at asks, a retune inside the tail, a pass-through stage 2, u
    before what is held, and an update() after a place_at(P) without a tail are all refused."""
    fs, D = 48000, 1
    rng = np.random.default_rng(5)
    ref, _ = placed_pair(fs, D, rng)
    P = 4000 * 128
    with pytest.raises(AssertionError, match="needed"):
        ref.place_at(P, cs16(rng, 1024)[:, :ref.tail_needed() - 1])
    ref.place_at(P, cs16(rng, 1024))
    with pytest.raises(AssertionError, match="before"):
        RR.resample(ref.u, ref.h2, ref.U, ref.M, ref.g2, ref.out_pos - 128 * 8, 128, 0, ref.u0)
    ref.update(cs16(rng, 128))
    ref.place_at(P)
    with pytest.raises(AssertionError):
        ref.update(cs16(rng, 128))
    ref.place_at(P - 128)
    ref.set_frequency_word(5, ch=0)                                      # an anchor at P - 128
    with pytest.raises(AssertionError, match="retune inside"):
        ref.place_at(P, cs16(rng, 1024))
    plain = RR.TunerRateRef(1, 1, 2, 88200)                              # U = M = 1, the pass-through
    with pytest.raises(AssertionError):
        plain.place_at(P, cs16(rng, 1024))
