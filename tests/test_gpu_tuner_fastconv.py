"""Fast-convolution banks of the digital tuner on the GPU (include/asdr_tuner.h, "Fast-convolution banks";
asdr_tuner_fastconv.hip): u against the float64 restatement tests/tuner_fastconv_ref.py within +-1 (at most 2 % of samples off),
call splits bit-identical, rate configurations through the unchanged stage 2, a 65,536-channel bank, and the chain behind it."""
import numpy as np
import pytest

import tuner_fastconv_ref as F
from helpers import Hip

pytestmark = pytest.mark.gpu


def edge_words(R):
    H, N, q = F.sizes(R)
    return [0, 1 << 31, (1 << 31) - 1, (1 << 32) - 1, q // 2, q // 2 - 1, (1 << 32) - q // 2, (N // 2 - 1) * q + q // 2,
            0x9E3779B9, 0x01234567]


def cs16(rng, n_src, n, tones=(), fs=1.0, lo=-20000, hi=20000):
    x = rng.integers(lo, hi, size=(n_src, n, 2), endpoint=True).astype(np.float64)
    m = np.arange(n)
    for s, f, a in tones:
        x[s, :, 0] += a * np.cos(2 * np.pi * f * m / fs)
        x[s, :, 1] += a * np.sin(2 * np.pi * f * m / fs)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def compare(got, want, tol=1, frac=0.02, what=""):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max(initial=0) <= tol, (what, int(d.max()), np.argwhere(d == d.max())[0])
    assert d.size == 0 or (d != 0).mean() <= frac, (what, float((d != 0).mean()))


def setup_pair(bank, ref, srcs, fws):
    for c, (s, fw) in enumerate(zip(srcs, fws)):
        for o in (bank, ref):
            o.set_source(s, ch=c); o.set_frequency_word(fw, ch=c)


@pytest.mark.parametrize("R", [2, 16, 128, 1024])
def test_u_matches_the_restatement_with_pass_through_stage_2(gpu, R):
    fs = 44100 * R
    rng = np.random.default_rng(R)
    fws = edge_words(R)
    n_ch, n_src = len(fws), 3
    srcs = [c % n_src for c in range(n_ch)]
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    assert bank.ratio() == (1, 1) and bank.fft_size() == 256 * R
    ref = F.TunerFastconvRef(n_ch, n_src, fs, R)
    setup_pair(bank, ref, srcs, fws)
    splits = [1, 3, 2] if R == 1024 else [1, 3, 2, 5]
    for k, nf in enumerate(splits):
        if k == 1:
            for o in (bank, ref):
                o.set_frequency(fs * 0.123, ch=2); o.set_phase(0xDEADBEEF, ch=5); o.set_source(0, ch=4)
        if k == 2:
            for o in (bank, ref):
                o.set_frequency_word(0x7FFFF000, ch=0); o.set_phase(12345)
        tones = [(s, float(rng.uniform(-fs / 2, fs / 2)), 6000.0) for s in range(n_src)] + [(0, fs * 0.123 + 2000.0, 5000.0)]
        iq = cs16(rng, n_src, nf * 128 * R, tones, fs)
        I, Q = bank.update(iq)
        wI, wQ = ref.update(iq)
        compare(I, wI, what=(R, k)); compare(Q, wQ, what=(R, k))
        assert bank.position() == ref.P and bank.output_position() == ref.out_pos
    st = bank.read_state()
    assert list(st["ph_a"]) == list(ref.ph_a) and list(st["pos_a"]) == list(ref.pos_a)
    bank.reset(); ref.reset()
    setup_pair(bank, ref, srcs, fws)
    iq = cs16(rng, n_src, 2 * 128 * R)
    I, Q = bank.update(iq)
    wI, wQ = ref.update(iq)
    compare(I, wI, what="after reset"); compare(Q, wQ, what="after reset")
    bank.close()


@pytest.mark.parametrize("R", [16, 32])
def test_call_splits_are_bit_identical(gpu, R):
    fs = 44100 * R
    rng = np.random.default_rng(7 + R)
    n_ch, n_src, total = 9, 2, 12
    fws = [int(v) for v in rng.integers(0, 2 ** 32, size=n_ch, dtype=np.uint64)]
    iq = cs16(rng, n_src, total * 128 * R)
    outs = []
    for split in ([total], [1] * total, [5, 1, 2, 4], [3, 7, 2]):
        bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
        for c in range(n_ch):
            bank.set_source(c % n_src, ch=c); bank.set_frequency_word(fws[c], ch=c)
        parts, at = [], 0
        for nf in split:
            parts.append(bank.update(iq[:, at:at + nf * 128 * R]))
            at += nf * 128 * R
        outs.append((np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)))
        bank.close()
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])


@pytest.mark.parametrize("fs,R", [(2400000, 16), (20000000, 128), (61440000, 512)])
def test_rate_configurations_through_stage_2(gpu, fs, R):
    rng = np.random.default_rng(fs // 1000)
    n_ch, n_src = 6, 2
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    h2, g2 = bank.get_resampler()
    ref = F.TunerFastconvRef(n_ch, n_src, fs, R, h2=h2, g2=g2)
    fws = edge_words(R)[:n_ch]
    setup_pair(bank, ref, [c % n_src for c in range(n_ch)], fws)
    for k, nf in enumerate([1, 4, 2, 7, 1, 3]):
        if k == 3:
            for o in (bank, ref):
                o.set_frequency(-fs * 0.3, ch=1); o.set_phase(0x40000000, ch=2)
        iq = cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0)], fs)
        n = bank.out_blocks(nf)
        assert n == ref.out_blocks(nf)
        I, Q = bank.update_rate(iq)
        wI, wQ = ref.update(iq)
        assert I.shape == wI.shape == (n_ch, n, 128)
        compare(I, wI, tol=2, frac=1.0, what=k); compare(Q, wQ, tol=2, frac=1.0, what=k)
        assert bank.output_position() == ref.out_pos
    bank.close()


def test_65536_channels_16_sources_at_2_4_msps(gpu):
    fs, R, n_ch, n_src, nf = 2400000, 16, 65536, 16, 16
    rng = np.random.default_rng(65536)
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    h2, g2 = bank.get_resampler()
    srcs = (np.arange(n_ch) * 7) % n_src
    fws = rng.integers(0, 2 ** 32, size=n_ch, dtype=np.uint64)
    for c in range(n_ch):
        bank.set_source(int(srcs[c]), ch=c); bank.set_frequency_word(int(fws[c]), ch=c)
    sample = sorted(set([0, 1, n_ch - 1] + [int(c) for c in rng.integers(0, n_ch, size=61)]))
    ref = F.TunerFastconvRef(len(sample), n_src, fs, R, h2=h2, g2=g2)
    for i, c in enumerate(sample):
        ref.src[i], ref.fw[i] = int(srcs[c]), int(fws[c])
    hip = Hip()
    cap = nf + 1
    dI, dQ = hip.malloc(n_ch * cap * 256), hip.malloc(n_ch * cap * 256)
    s = hip.stream()
    for call in range(3):
        iq = cs16(rng, n_src, nf * 128 * R)
        dIQ = hip.upload(iq)
        n = bank.update_rate_device(dIQ, dI, dQ, nf, cap, stream=s)
        hip.sync(s)
        wI, wQ = ref.update(iq)
        assert n == wI.shape[1]
        for i, c in enumerate(sample):
            gI = hip.download(dI, (n, 128), np.int16, offset_bytes=c * cap * 256)
            gQ = hip.download(dQ, (n, 128), np.int16, offset_bytes=c * cap * 256)
            compare(gI, wI[i], tol=2, frac=1.0, what=(call, c)); compare(gQ, wQ[i], tol=2, frac=1.0, what=(call, c))
    hip.free_all()
    bank.close()


def test_fastconv_bank_into_the_chain_on_one_stream(gpu, ao):
    """Fast-convolution bank (2.4 MS/s, R = 16) -> asdr_update_device (USB) on one stream: the chain's audio equals the oracle run
    on the tuner's own output, bit for bit, and the tuner's output is the restatement's within +-2."""
    fs, R, nf = 2400000, 16, 48
    fc = 7_000_000.0
    dials = [fc + 250_000.0, fc - 410_000.0]
    rng = np.random.default_rng(24)
    n = nf * 128 * R
    t = np.arange(n) / fs
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 2.0
    for f, a in ((dials[0] + 1200.0 - fc, 3000.0), (dials[1] + 700.0 - fc, 3000.0)):
        z = z + a * np.exp(2j * np.pi * f * t)
    iq = np.stack([np.round(z.real), np.round(z.imag)], axis=-1).astype(np.int16)
    sdr = gpu.AudioSDRBatch(2)
    tuner = gpu.TunerBank.fastconv(2, 1, fs, R)
    h2, g2 = tuner.get_resampler()
    ref = F.TunerFastconvRef(2, 1, fs, R, h2=h2, g2=g2)
    sdr.setDemodMode(gpu.USBmode)
    for c in range(2):
        hz = dials[c] - fc - sdr.getTuningOffset(c)
        tuner.set_frequency(hz, ch=c); ref.set_frequency(hz, ch=c)
    hip = Hip()
    s = hip.stream()
    dIQ = hip.upload(iq[None])
    nb = tuner.out_blocks(nf)
    row = nb * 128 * 2
    dI, dQ, dOut = hip.malloc(2 * row), hip.malloc(2 * row), hip.malloc(2 * row)
    assert tuner.update_rate_device(dIQ, dI, dQ, nf, nb, stream=s) == nb
    sdr.update_device(dI, dQ, dOut, nb, stream=s)
    hip.sync(s)
    got = hip.download(dOut, (2, nb, 128), np.int16)
    tI, tQ = hip.download(dI, (2, nb, 128), np.int16), hip.download(dQ, (2, nb, 128), np.int16)
    wI, wQ = ref.update(iq[None])
    compare(tI, wI, tol=2, frac=1.0); compare(tQ, wQ, tol=2, frac=1.0)
    want, _ = ao.run_channels(lambda o, c: o.setDemodMode(ao.USBmode), tI, tQ)
    assert np.array_equal(got, want)
    for c, tone in enumerate((1200.0, 700.0)):
        a = got[c].reshape(-1)[nb * 128 // 2:].astype(float)
        spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(a.size)))
        peak = np.fft.rfftfreq(a.size, 1 / 44100.0)[np.argmax(spec)]
        assert abs(peak - tone) < 20.0, (c, peak)
    hip.free_all()
    sdr.close(); tuner.close()
