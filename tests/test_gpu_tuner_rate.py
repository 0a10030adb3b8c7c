"""Rate banks of the digital tuner on the GPU (include/asdr_tuner.h, "Rate banks"): stage 1 + the stage-2 resampler kernel
(asdr_tuner_resample.hip) int16 bit-exact against tests/tuner_rate_ref.py, the block counts against the reference's timing, and end
to end with the chain behind it (rate bank -> asdr_update_device on one stream) against the reference -> the chain oracle."""
import numpy as np
import pytest

import tuner_rate_ref as RR
from helpers import Hip

pytestmark = pytest.mark.gpu

FWS = [0, 1 << 31, 0xFFF00000, 0x01234567, 0x7FFFFFFF, 0x80000001, 0x0FEDCBA9]
SRCS = [0, 0, 3, 0, 2, 3, 0]                        # 4 sources: source 1 empty, source 2 with one channel
SPLITS = [1, 2, 3, 7, 16, 1, 1, 3, 2]


def random_iq(rng, n_src, n, lo=-20000, hi=20000):
    return rng.integers(lo, hi, size=(n_src, n, 2), endpoint=True).astype(np.int16)


def random_taps(rng, L, total=60000):
    h = rng.standard_normal(L)
    h = np.round(h * total / max(np.abs(h).sum(), 1e-9)).astype(np.int64)
    while np.abs(h).sum() > 65535:
        h = h * 9 // 10
    if not h.any():
        h[0] = 1
    return h.astype(np.int16)


def random_resampler(rng, U, K, total=60000):
    """U K taps, every phase with sum |h2| <= 65535."""
    h2 = np.zeros((K, U), dtype=np.int16)
    for ph in range(U):
        h2[:, ph] = random_taps(rng, K, total)
    return h2.reshape(-1)


def make(gpu, fs, D, rng, n_ch=len(SRCS), n_src=4, L=None, K=None, g=1, g2=1):
    bank = gpu.TunerBank(n_ch, n_src, D, fs_in=fs)
    U, M = bank.ratio()
    h = random_taps(rng, L or int(rng.integers(1, 1025)))
    h2 = random_resampler(rng, U, K or int(rng.integers(1, 65)))
    bank.set_filter(h, g); bank.set_resampler(h2, g2)
    ref = RR.TunerRateRef(n_ch, n_src, D, fs, h, g, h2, g2)
    for c in range(n_ch):
        for o in (bank, ref):
            o.set_source(SRCS[c % len(SRCS)] % n_src, ch=c); o.set_frequency_word(FWS[c % len(FWS)], ch=c)
    return bank, ref


def check(bank, ref, iq):
    nf = iq.shape[1] // (128 * bank.decimation)
    n = bank.out_blocks(nf)
    assert n == ref.out_blocks(nf)
    I, Q = bank.update_rate(iq)
    wI, wQ = ref.update(iq)
    assert I.shape == wI.shape == (bank.n_channels, n, 128)
    bad = np.argwhere((I != wI) | (Q != wQ))
    assert bad.size == 0, "first mismatch at %s of %s" % (bad[0], I.shape)
    assert bank.position() == ref.P and bank.output_position() == ref.out_pos
    return I, Q


@pytest.mark.parametrize("fs,D", [(48000, 1), (96000, 1), (2400000, 50), (2048000, 32), (10000000, 64), (7 * 44100, 7)])
def test_bit_exact_at_every_rate_and_call_split(gpu, fs, D):
    rng = np.random.default_rng(fs + D)
    for K, g2 in ((int(rng.integers(2, 64)), 1), (64, 0), (1, 3)):
        bank, ref = make(gpu, fs, D, rng, K=K, g2=g2)
        zeros = 0
        for nf in SPLITS:
            zeros += check(bank, ref, random_iq(rng, 4, nf * 128 * D))[0].shape[1] == 0
        U, M = bank.ratio()
        assert (zeros > 0) == (M > U) or U == M
        bank.close()


def test_retunes_filter_and_resampler_changes_and_reset(gpu):
    fs, D = 2048000, 32
    rng = np.random.default_rng(17)
    bank, ref = make(gpu, fs, D, rng, n_ch=6, n_src=3, L=300, K=18)
    U, _ = bank.ratio()
    steps = [lambda o: o.set_frequency(123_456.7, ch=1),
             lambda o: o.set_frequency_word(FWS[3], ch=2),
             lambda o: o.set_phase(0xDEADBEEF, ch=3),
             lambda o: o.set_source(2, ch=0),
             lambda o: o.set_filter(h1, 3),
             lambda o: o.set_resampler(r1, 2),
             lambda o: o.set_frequency(-700_000.0),
             lambda o: o.set_resampler(r2, 0),
             lambda o: o.set_source(1)]
    h1, r1, r2 = random_taps(rng, 97), random_resampler(rng, U, 7), random_resampler(rng, U, 33)
    check(bank, ref, random_iq(rng, 3, 3 * 128 * D))
    for i, st in enumerate(steps):
        st(bank); st(ref)
        check(bank, ref, random_iq(rng, 3, (1 + i % 3) * 128 * D))
    bank.reset(); ref.reset()
    assert bank.position() == 0 and bank.output_position() == 0
    for nf in (1, 2, 5):
        check(bank, ref, random_iq(rng, 3, nf * 128 * D))
    bank.close()


def test_out_blocks_over_a_long_irregular_run(gpu):
    """One small bank, 120 calls of 1..16 frames at 10 MS/s (U / M = 882 / 3125), a reset half-way: every count, position and
    output against the reference."""
    fs, D = 10000000, 64
    rng = np.random.default_rng(300)
    bank, ref = make(gpu, fs, D, rng, n_ch=1, n_src=1, L=65, K=6)
    for call in range(120):
        if call == 60:
            bank.reset(); ref.reset()
            assert bank.out_blocks(1) == ref.out_blocks(1) == 0
        check(bank, ref, random_iq(rng, 1, int(rng.choice([1, 1, 2, 3, 7, 16])) * 128 * D))
    bank.close()


def test_rate_bank_at_d_44100_is_the_plain_bank(gpu):
    D, nb = 7, 3
    rng = np.random.default_rng(44100)
    plain, plain2 = gpu.TunerBank(5, 2, D), gpu.TunerBank(5, 2, D)
    rate = gpu.TunerBank(5, 2, D, fs_in=44100 * D)
    h = random_taps(rng, 85)
    hip = Hip()
    s = hip.stream()
    row = nb * 128 * 2
    dI, dQ, dI2, dQ2 = (hip.malloc(5 * row) for _ in range(4))
    for b in (plain, plain2, rate):
        b.set_filter(h, 1)
        for c in range(5):
            b.set_source(c % 2, ch=c); b.set_frequency(1000.0 * c - 2345.6, ch=c)
    for call in range(3):
        iq = random_iq(rng, 2, nb * 128 * D)
        dIQ = hip.upload(iq)
        plain.update_device(dIQ, dI, dQ, nb, stream=s)
        assert plain2.update_rate_device(dIQ, dI2, dQ2, nb, nb, stream=s) == nb
        hip.sync(s)
        a = hip.download(dI, (5, nb, 128), np.int16), hip.download(dQ, (5, nb, 128), np.int16)
        b = hip.download(dI2, (5, nb, 128), np.int16), hip.download(dQ2, (5, nb, 128), np.int16)
        c = rate.update_rate(iq)
        d = rate.update(iq) if call == 1 else None                       # U = M = 1: the plain entry point works too
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
        if d is not None:
            plain.update_device(dIQ, dI, dQ, nb, stream=s); plain2.update_rate_device(dIQ, dI2, dQ2, nb, nb, stream=s)
            hip.sync(s)
            assert np.array_equal(hip.download(dI, (5, nb, 128), np.int16), d[0])
    assert rate.output_position() == plain2.output_position() == plain.output_position()
    # a resampling bank refuses the plain entry points, naming the rate one
    r = gpu.TunerBank(2, 1, 1, fs_in=48000)
    with pytest.raises(gpu.AsdrError, match="update_rate"):
        r.update(np.zeros((1, 128, 2), dtype=np.int16))
    with pytest.raises(gpu.AsdrError, match="update_rate"):
        r.update_device(dIQ, dI, dQ, 1, stream=s)
    hip.free_all()
    for b in (plain, plain2, rate, r):
        b.close()


def test_pass_through_then_a_resampler_starts_from_zero_history(gpu):
    """U = M = 1 with the default (pass-through) stage 2, then a real resampler: u before that call counts as 0."""
    D = 2
    rng = np.random.default_rng(21)
    bank = gpu.TunerBank(3, 1, D, fs_in=44100 * D)
    h, g = bank.get_filter()
    ref = RR.TunerRateRef(3, 1, D, 44100 * D, h, g)
    for o in (bank, ref):
        for c in range(3):
            o.set_frequency_word(FWS[c + 1], ch=c)
    check(bank, ref, random_iq(rng, 1, 2 * 128 * D))
    r1 = random_taps(rng, 9)
    bank.set_resampler(r1, 1); ref.set_resampler(r1, 1)
    with pytest.raises(gpu.AsdrError, match="update_rate"):
        bank.update(random_iq(rng, 1, 128 * D))
    for nf in (1, 3):
        check(bank, ref, random_iq(rng, 1, nf * 128 * D))
    bank.set_resampler([16384], 1); ref.set_resampler([16384], 1)
    check(bank, ref, random_iq(rng, 1, 2 * 128 * D))
    bank.close()


def rail_resampler(rng, U, K):
    """U K taps with sum |h2| = 65535 in every phase exactly: all negative in phases 0, 3, 6, ..., all positive in 1, 4, 7, ...,
    random signs in the rest."""
    h2 = np.zeros((K, U), dtype=np.int64)
    for ph in range(U):
        a = rng.multinomial(65535, rng.dirichlet(np.ones(K)))
        while a.max() > 32767:
            a = rng.multinomial(65535, rng.dirichlet(np.ones(K)))
        h2[:, ph] = a * (-1 if ph % 3 == 0 else 1 if ph % 3 == 1 else rng.choice([-1, 1], size=K))
    return h2.reshape(-1).astype(np.int16)


@pytest.mark.parametrize("g2", [0, 4, 15])
def test_stage2_rails_and_gain_shifts(gpu, g2):
    """Stage 2 at its int32 edge: 96 kHz, D = 1 (147 / 320), stage 1 the pass filter, every phase of h2 with sum |h2| = 65535,
    inputs drawn from {-32768, 32767, -32767, 0} with runs of (-32768, -32768) and (32767, 32767).  The channels sit at fw = 0;
    those at a phase of +-45 degrees saturate the mixer, so u holds runs of -32768 exactly and an all-negative phase over such a
    run sums to 65535 * 32768 (+ 16384 at g2 = 0): the case behind the kernel's "exact in int32"."""
    fs, D, K, nf = 96000, 1, 8, 12
    rng = np.random.default_rng(200 + g2)
    bank = gpu.TunerBank(4, 1, D, fs_in=fs)
    U, M = bank.ratio()
    h2 = rail_resampler(rng, U, K)
    bank.set_filter([16384], 1); bank.set_resampler(h2, g2)
    ref = RR.TunerRateRef(4, 1, D, fs, [16384], 1, h2, g2)
    for c, ph in enumerate([0, 512 << 20, 3584 << 20, 1536 << 20]):
        for o in (bank, ref):
            o.set_phase(ph, ch=c)
    iq = rng.choice(np.array([-32768, 32767, -32767, 0], dtype=np.int16), size=(1, nf * 128, 2))
    iq[0, 300:400], iq[0, 700:800] = -32768, 32767
    I, Q = check(bank, ref, iq)
    assert not ref.fw.any() and (ref.u == -32768).any() and (ref.u == 32767).any()
    acc = RR.accumulate(ref.u, h2, U, M, 0, I.shape[1] * 128)                # the reference's sums reach both edges
    assert acc.max() == 65535 * 32768 == -acc.min() and acc.max() + 16384 < 1 << 31
    for y in (I, Q):
        assert (y == 32767).any() and (y == -32768).any()
    bank.close()


def test_strided_rows_and_the_capacity_error(gpu):
    fs, D, n_ch, n_src = 2400000, 50, 4, 2
    rng = np.random.default_rng(9)
    host, _ = make(gpu, fs, D, np.random.default_rng(1), n_ch=n_ch, n_src=n_src, L=553, K=14)
    dev, ref = make(gpu, fs, D, np.random.default_rng(1), n_ch=n_ch, n_src=n_src, L=553, K=14)
    hip = Hip()
    s = hip.stream()
    cap, out_stride = 6, 9
    out_bytes = n_ch * out_stride * 128 * 2
    dI, dQ = hip.malloc(out_bytes + 512), hip.malloc(out_bytes + 512)
    for nf in (3, 1, 5, 2):
        iq = random_iq(rng, n_src, nf * 128 * D)
        in_stride = nf * 128 * D + 40
        padded = np.zeros((n_src, in_stride, 2), dtype=np.int16)
        padded[:, :nf * 128 * D] = iq
        dIQ = hip.upload(padded)
        n = dev.out_blocks(nf)
        if n > 0:                                                         # one block short: refused, nothing changes
            pos, opos = dev.position(), dev.output_position()
            with pytest.raises(gpu.AsdrError, match="capacity"):
                dev.update_rate_device(dIQ, dI, dQ, nf, n - 1, in_stride_samples=in_stride, out_stride_blocks=out_stride, stream=s)
            assert dev.position() == pos and dev.output_position() == opos and dev.out_blocks(nf) == n
        with pytest.raises(gpu.AsdrError, match="stride"):
            dev.update_rate_device(dIQ, dI, dQ, nf, cap, in_stride_samples=in_stride, out_stride_blocks=cap - 1, stream=s)
        hip.fill(dI, 0x55, out_bytes + 512); hip.fill(dQ, 0x55, out_bytes + 512)
        got = dev.update_rate_device(dIQ, dI + 256, dQ + 256, nf, cap, in_stride_samples=in_stride, out_stride_blocks=out_stride,
                                     stream=s)
        hip.sync(s)
        assert got == n
        gI = hip.download(dI, (n_ch, out_stride, 128), np.int16, offset_bytes=256)
        gQ = hip.download(dQ, (n_ch, out_stride, 128), np.int16, offset_bytes=256)
        wI, wQ = host.update_rate(iq)
        rI, rQ = ref.update(iq)
        assert np.array_equal(wI, rI) and np.array_equal(wQ, rQ)
        assert np.array_equal(gI[:, :n], wI) and np.array_equal(gQ[:, :n], wQ)
        assert (gI[:, n:] == 0x5555).all() and (gQ[:, n:] == 0x5555).all()     # nothing outside the rows' blocks
        assert (hip.download(dI, (128,), np.int16) == 0x5555).all()
    hip.free_all()
    host.close(); dev.close()


def test_65536_channels_16_sources_at_2_4_msps(gpu):
    """T4-sized bank (default filters, 2.4 MS/s, D = 50): three calls of 16 frames, a seeded sample of 48 channels against the
    reference."""
    fs, D, n_ch, n_src, nf = 2400000, 50, 65536, 16, 16
    rng = np.random.default_rng(2400)
    bank = gpu.TunerBank(n_ch, n_src, D, fs_in=fs)
    h, g = bank.get_filter()
    h2, g2 = bank.get_resampler()
    srcs = (np.arange(n_ch) * 7) % n_src
    fws = rng.integers(0, 2**32, size=n_ch, dtype=np.uint64)
    for c in range(n_ch):
        bank.set_source(int(srcs[c]), ch=c); bank.set_frequency_word(int(fws[c]), ch=c)
    sample = sorted(set([0, 1, n_ch - 1] + [int(c) for c in rng.integers(0, n_ch, size=45)]))
    ref = RR.TunerRateRef(len(sample), n_src, D, fs, h, g, h2, g2)
    for i, c in enumerate(sample):
        ref.src[i], ref.fw[i] = int(srcs[c]), int(fws[c])
    hip = Hip()
    cap = nf + 1
    dI, dQ = hip.malloc(n_ch * cap * 256), hip.malloc(n_ch * cap * 256)
    s = hip.stream()
    for call in range(3):
        iq = random_iq(rng, n_src, nf * 128 * D)
        dIQ = hip.upload(iq)
        n = bank.update_rate_device(dIQ, dI, dQ, nf, cap, stream=s)
        hip.sync(s)
        wI, wQ = ref.update(iq)
        assert n == wI.shape[1]
        for i, c in enumerate(sample):
            gI = hip.download(dI, (n, 128), np.int16, offset_bytes=c * cap * 256)
            gQ = hip.download(dQ, (n, 128), np.int16, offset_bytes=c * cap * 256)
            assert np.array_equal(gI, wI[i]) and np.array_equal(gQ, wQ[i]), (call, c)
    hip.free_all()
    bank.close()


def synth(fs, n, tones, seed):
    """CS16 capture at fs: complex tones (offset Hz, amplitude) plus a little noise."""
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 2.0
    for f, a in tones:
        z = z + a * np.exp(2j * np.pi * f * t)
    return np.stack([np.round(z.real), np.round(z.imag)], axis=-1).astype(np.int16)


def test_end_to_end_2_4_msps_to_usb_audio(gpu, ao):
    """Rate bank (2.4 MS/s, D = 50) -> asdr_update_device (USB) on one stream, bit-exact against the reference -> the chain
    oracle; the audio peak where the USB tone belongs."""
    fs, D, nf = 2400000, 50, 48
    fc = 7_000_000.0
    dials = [fc + 250_000.0, fc - 410_000.0]
    iq = synth(fs, nf * 128 * D, [(dials[0] + 1200.0 - fc, 3000.0), (dials[1] + 700.0 - fc, 3000.0)], seed=24)
    sdr = gpu.AudioSDRBatch(2)
    tuner = gpu.TunerBank(2, 1, D, fs_in=fs)
    h, g = tuner.get_filter()
    h2, g2 = tuner.get_resampler()
    ref = RR.TunerRateRef(2, 1, D, fs, h, g, h2, g2)
    sdr.setDemodMode(gpu.USBmode)
    for c in range(2):
        hz = dials[c] - fc - sdr.getTuningOffset(c)
        tuner.set_frequency(hz, ch=c); ref.set_frequency(hz, ch=c)
    hip = Hip()
    s = hip.stream()
    dIQ = hip.upload(iq[None])
    n = tuner.out_blocks(nf)
    row = n * 128 * 2
    dI, dQ, dOut = hip.malloc(2 * row), hip.malloc(2 * row), hip.malloc(2 * row)
    assert tuner.update_rate_device(dIQ, dI, dQ, nf, n, stream=s) == n
    sdr.update_device(dI, dQ, dOut, n, stream=s)
    hip.sync(s)
    got = hip.download(dOut, (2, n, 128), np.int16)
    wI, wQ = ref.update(iq[None])
    assert np.array_equal(hip.download(dI, (2, n, 128), np.int16), wI)
    want, _ = ao.run_channels(lambda o, c: o.setDemodMode(ao.USBmode), wI, wQ)
    assert np.array_equal(got, want)
    for c, tone in enumerate((1200.0, 700.0)):
        a = got[c].reshape(-1)[n * 128 // 2:].astype(float)
        spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(a.size)))
        peak = np.fft.rfftfreq(a.size, 1 / 44100.0)[np.argmax(spec)]
        assert abs(peak - tone) < 20.0, (c, peak)
    hip.free_all()
    sdr.close(); tuner.close()


def test_tone_lands_in_its_bin_and_the_alias_is_rejected(gpu):
    """A carrier 1 kHz above the channel's frequency in a 2.4 MS/s capture comes out at +1 kHz of the 44.1 kHz I/Q; a second
    carrier 43 kHz above (it would fold to -5 kHz at Fs_mid = 48 kHz) comes out >= 60 dB down."""
    fs, D, nf = 2400000, 50, 200
    f0 = 310_000.0
    iq = synth(fs, nf * 128 * D, [(f0 + 1000.0, 8000.0), (f0 + 43000.0, 8000.0)], seed=7)
    bank = gpu.TunerBank(1, 1, D, fs_in=fs)
    bank.set_frequency(f0)
    I, Q = bank.update_rate(iq[None])
    z = (I.reshape(-1).astype(float) + 1j * Q.reshape(-1).astype(float))[4096:]
    n = 1 << 14
    z = z[:n]
    spec = np.abs(np.fft.fftshift(np.fft.fft(z * np.kaiser(n, 16.0))))
    f = np.fft.fftshift(np.fft.fftfreq(n, 1 / 44100.0))
    peak = f[np.argmax(spec)]
    assert abs(peak - 1000.0) < 5.0, peak
    alias = spec[np.abs(f + 5000.0) < 30.0].max()
    assert 20 * np.log10(spec.max() / alias) >= 60.0, 20 * np.log10(spec.max() / alias)
    bank.close()


def tuned(bank):
    for c in range(bank.n_channels):
        bank.set_source(c % bank.n_sources, ch=c); bank.set_frequency_word(FWS[c % len(FWS)], ch=c)
    return bank


def test_direct_and_rate_banks_alternating_between_two_streams(gpu):
    """A direct-form bank (D = 2) and a rate bank (96 kHz, D = 2: 48 kHz intermediate, 147 / 160), 7 channels on 2 sources: calls of
    2, 2, 4, 1, 3 frames alternate between two streams with no host synchronisation (the third is the largest, so the rate bank's
    intermediate grows between calls); outputs and positions equal a twin's that runs on one stream, bit for bit."""
    n_ch, n_src, D = 7, 2, 2
    rng = np.random.default_rng(96)
    hip = Hip()
    ss, s1 = [hip.stream(), hip.stream()], hip.stream()
    splits = [2, 2, 4, 1, 3]
    ins = [hip.upload(random_iq(rng, n_src, nf * 128 * D)) for nf in splits]
    caps = [nf + 1 for nf in splits]
    for make_bank in (lambda: gpu.TunerBank(n_ch, n_src, D), lambda: gpu.TunerBank(n_ch, n_src, D, fs_in=96000)):
        two, one = tuned(make_bank()), tuned(make_bank())
        rate = two.ratio() != (1, 1)
        assert two.ratio() == ((147, 160) if rate else (1, 1))
        bufs = [[hip.malloc(n_ch * c * 256) for _ in range(4)] for c in caps]
        hip.sync()
        ns = []
        for k, nf in enumerate(splits):
            if rate:
                a = two.update_rate_device(ins[k], bufs[k][0], bufs[k][1], nf, caps[k], stream=ss[k % 2])
                assert a == one.update_rate_device(ins[k], bufs[k][2], bufs[k][3], nf, caps[k], stream=s1)
            else:
                a = nf
                two.update_device(ins[k], bufs[k][0], bufs[k][1], nf, out_stride_blocks=caps[k], stream=ss[k % 2])
                one.update_device(ins[k], bufs[k][2], bufs[k][3], nf, out_stride_blocks=caps[k], stream=s1)
            ns.append(a)
        hip.sync()
        assert two.position() == one.position() == sum(splits) * 128 * D and two.output_position() == one.output_position() > 0
        for k, n in enumerate(ns):
            g = [hip.download(p, (n_ch, caps[k], 128), np.int16)[:, :n] for p in bufs[k]]
            assert np.array_equal(g[0], g[2]) and np.array_equal(g[1], g[3]), (rate, k)
            assert n == 0 or g[0].any()
        two.close(); one.close()
    hip.free_all()


def test_kept_buffers_grow_and_are_reused(gpu):
    """The rate bank above through the host form in calls of 1, 3, 1 and 2 frames: the host staging and the intermediate grow for
    the second call and are reused, larger than needed, by the calls behind it; every call against tuner_rate_ref."""
    rng = np.random.default_rng(147)
    bank, ref = make(gpu, 96000, 2, rng, n_ch=7, n_src=2, L=25, K=12)
    assert bank.ratio() == (147, 160)
    total = 0
    for nf in (1, 3, 1, 2):
        total += check(bank, ref, random_iq(rng, 2, nf * 128 * 2))[0].shape[1]
    assert total > 0
    bank.close()
