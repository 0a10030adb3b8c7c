"""The digital tuner bank on the GPU (include/asdr_tuner.h), int16 bit-exact against tests/tuner_ref.py, and end to end with the
chain behind it (tuner -> asdr_update_device on one stream) against tuner_ref -> the chain oracle."""
import numpy as np
import pytest

import tuner_ref as R
from helpers import Hip

pytestmark = pytest.mark.gpu

FWS = [0, 1 << 31, 0xFFF00000, R.fw_from_hz(-7_123.5, 1), 0x01234567, 0x7FFFFFFF, 0x80000001]


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


def configure(bank, ref, srcs, fws):
    for c, (s, fw) in enumerate(zip(srcs, fws)):
        bank.set_source(s, ch=c); ref.set_source(s, ch=c)
        bank.set_frequency_word(fw, ch=c); ref.set_frequency_word(fw, ch=c)


def check(bank, ref, iq):
    I, Q = bank.update(iq)
    wI, wQ = ref.update(iq)
    assert I.shape == wI.shape
    bad = np.argwhere((I != wI) | (Q != wQ))
    assert bad.size == 0, "first mismatch at %s of %s" % (bad[0], I.shape)
    return I, Q


@pytest.mark.parametrize("D", [1, 2, 7, 48, 64])
def test_every_decimation_and_filter_length(gpu, D):
    rng = np.random.default_rng(D)
    srcs = [0, 0, 3, 0, 2, 3, 0]                     # source 1 empty, source 2 with one channel
    for L in sorted({1, D, 12 * D + 1, 1024}):
        h = random_taps(rng, L)
        bank, ref = gpu.TunerBank(len(srcs), 4, D), R.TunerRef(len(srcs), 4, D, h, 2)
        bank.set_filter(h, 2)
        configure(bank, ref, srcs, FWS)
        for nb in (2, 1, 3):
            check(bank, ref, random_iq(rng, 4, nb * 128 * D))
        assert bank.position() == ref.P
        bank.close()


def test_call_splits_give_the_same_stream(gpu):
    D, L, T = 7, 85, 6
    rng = np.random.default_rng(11)
    h = random_taps(rng, L)
    iq = random_iq(rng, 2, T * 128 * D)
    outs = []
    for split in ([T], [1] * T, [1, 3, 2]):
        bank = gpu.TunerBank(5, 2, D)
        bank.set_filter(h, 1)
        for c in range(5):
            bank.set_source(c % 2, ch=c); bank.set_frequency_word(FWS[c], ch=c)
        got, at = [], 0
        for nb in split:
            got.append(np.concatenate(bank.update(iq[:, at:at + nb * 128 * D]), axis=-1))
            at += nb * 128 * D
        outs.append(np.concatenate(got, axis=1))
        bank.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    ref = R.TunerRef(5, 2, D, h, 1)
    for c in range(5):
        ref.set_source(c % 2, ch=c); ref.set_frequency_word(FWS[c], ch=c)
    wI, wQ = ref.update(iq)
    assert np.array_equal(outs[0], np.concatenate([wI, wQ], axis=-1))


def test_every_retune_kind_and_a_filter_change_between_calls(gpu):
    D = 3
    rng = np.random.default_rng(5)
    h0, h1 = random_taps(rng, 40), random_taps(rng, 77)
    bank, ref = gpu.TunerBank(6, 3, D), R.TunerRef(6, 3, D)
    bank.set_filter(h0, 0); ref.set_filter(h0, 0)
    configure(bank, ref, [0, 1, 2, 0, 1, 2], FWS[1:])
    steps = [lambda o: o.set_frequency(12_345.6, ch=1),
             lambda o: o.set_frequency_word(FWS[3], ch=2),
             lambda o: o.set_phase(0xDEADBEEF, ch=3),
             lambda o: o.set_source(2, ch=0),
             lambda o: o.set_frequency_word(FWS[4], ch=4),      # the same word again: still a retune (flush)
             lambda o: o.set_filter(h1, 3),
             lambda o: o.set_phase(77 << 20),                    # ASDR_ALL
             lambda o: o.set_frequency(-40_000.0),
             lambda o: o.set_source(1)]
    check(bank, ref, random_iq(rng, 3, 2 * 128 * D))
    for st in steps:
        st(bank); st(ref)
        check(bank, ref, random_iq(rng, 3, 128 * D))
    st = bank.read_state()
    assert list(st["pos_a"]) == list(ref.pos_a) and list(st["ph_a"]) == list(ref.ph_a) and list(st["fw"]) == list(ref.fw)
    bank.reset()
    ref2 = R.TunerRef(6, 3, D, h1, 3)
    check(bank, ref2, random_iq(rng, 3, 128 * D))


@pytest.mark.parametrize("g", [0, 4, 15])
def test_gain_shifts_with_saturating_inputs(gpu, g):
    D, L = 2, 31
    rng = np.random.default_rng(100 + g)
    h = random_taps(rng, L, total=65535)
    bank, ref = gpu.TunerBank(4, 1, D), R.TunerRef(4, 1, D, h, g)
    bank.set_filter(h, g)
    configure(bank, ref, [0] * 4, [0, 512 << 20, 1 << 31, 0xE0000000])
    iq = rng.choice(np.array([-32768, 32767, -32767, 0], dtype=np.int16), size=(1, 4 * 128 * D, 2))
    I, Q = check(bank, ref, iq)
    assert (np.abs(I.astype(int)) >= 32767).any()


def test_strided_rows_host_path_and_overlap_rejection(gpu):
    D, nb, n_ch, n_src = 5, 3, 4, 2
    rng = np.random.default_rng(9)
    h = random_taps(rng, 61)
    iq = random_iq(rng, n_src, nb * 128 * D)
    in_stride, out_stride = nb * 128 * D + 40, nb + 2                      # samples, blocks
    host = gpu.TunerBank(n_ch, n_src, D)
    dev = gpu.TunerBank(n_ch, n_src, D)
    for b in (host, dev):
        b.set_filter(h, 1)
        for c in range(n_ch):
            b.set_source(c % n_src, ch=c); b.set_frequency_word(FWS[c + 1], ch=c)
    hip = Hip()
    s = hip.stream()
    padded = np.zeros((n_src, in_stride, 2), dtype=np.int16)
    padded[:, :nb * 128 * D] = iq
    dIQ = hip.upload(padded)
    out_bytes = n_ch * out_stride * 128 * 2
    dI, dQ = hip.malloc(out_bytes), hip.malloc(out_bytes)
    hip.fill(dI, 0x55, out_bytes); hip.fill(dQ, 0x55, out_bytes)
    dev.update_device(dIQ, dI + 256, dQ + 256, nb, in_stride_samples=in_stride, out_stride_blocks=out_stride, stream=s)
    hip.sync(s)
    gI = hip.download(dI, (n_ch, out_stride, 128), np.int16)
    gQ = hip.download(dQ, (n_ch, out_stride, 128), np.int16)
    wI, wQ = host.update(iq)
    assert np.array_equal(gI[:, 1:1 + nb], wI) and np.array_equal(gQ[:, 1:1 + nb], wQ)
    assert (gI[:, 0] == 0x5555).all() and (gI[:, 1 + nb:] == 0x5555).all()               # nothing outside the rows' blocks
    pos = dev.position()
    with pytest.raises(gpu.AsdrError, match="overlap"):
        dev.update_device(dIQ, dIQ + 1024, dQ, 1, in_stride_samples=in_stride, stream=s)
    with pytest.raises(gpu.AsdrError, match="aligned"):
        dev.update_device(dIQ + 4, dI, dQ, 1, in_stride_samples=in_stride, stream=s)
    with pytest.raises(gpu.AsdrError, match="stride"):
        dev.update_device(dIQ, dI, dQ, nb, in_stride_samples=nb * 128 * D - 1, stream=s)
    assert dev.position() == pos
    hip.free_all()
    host.close(); dev.close()


def test_65536_channels_16_sources(gpu):
    """Every channel of a T3-sized bank (default filter, D = 48) compared; 64 distinct words per source, so the reference
    computes 1,024 distinct channels and each result is checked on the 64 channels that share it."""
    D, n_ch, n_src, nb = 48, 65536, 16, 4
    rng = np.random.default_rng(65536)
    words = [int(w) for w in rng.integers(0, 2**32, size=64, dtype=np.uint64)]
    words[0], words[1] = 0, 1 << 31
    srcs = [(c * 7) % n_src for c in range(n_ch)]
    fws = [words[(c // n_src) % 64] for c in range(n_ch)]
    bank = gpu.TunerBank(n_ch, n_src, D)
    h, g = bank.get_filter()
    ref = R.TunerRef(n_ch, n_src, D, h, g)
    for c in range(n_ch):
        bank.set_source(srcs[c], ch=c); bank.set_frequency_word(fws[c], ch=c)
        ref.src[c], ref.fw[c] = srcs[c], fws[c]
    for _ in range(2):
        check(bank, ref, random_iq(rng, n_src, nb * 128 * D))
    bank.close()


def synth_capture(D, n, fc, signals, seed):
    """CS16 wideband capture at D * 44.1 kHz centred at fc: a sum of complex components (f_rf, amplitude, am_depth, am_hz)."""
    fs = 44100.0 * D
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 30.0
    for f, a, depth, fm in signals:
        env = a * (1.0 + depth * np.cos(2 * np.pi * fm * t))
        z = z + env * np.exp(2j * np.pi * (f - fc) * t)
    return np.stack([np.round(z.real), np.round(z.imag)], axis=-1).astype(np.int16)


def test_end_to_end_wideband_to_audio(gpu, ao):
    """USB tone, AM carrier and WSPR tone in one D = 48 capture; channels tuned with hz = f - fc - getTuningOffset(); tuner ->
    asdr_update_device on one stream, bit-exact against tuner_ref -> the chain oracle, and each channel's audio peak where it belongs."""
    D, nb = 48, 64
    fc = 14_000_000.0
    usb_dial, am_carrier, wspr_dial = fc + 100_000.0, fc - 300_000.0, fc + 500_000.0
    signals = [(usb_dial + 1000.0, 3000.0, 0.0, 0.0), (am_carrier, 2000.0, 0.5, 700.0), (wspr_dial + 1500.0, 3000.0, 0.0, 0.0)]
    iq = synth_capture(D, nb * 128 * D, fc, signals, seed=48)
    modes = [gpu.USBmode, gpu.AMmode, gpu.WSPRmode]
    dials = [usb_dial, am_carrier, wspr_dial]
    expect_hz = [1000.0, 700.0, 1500.0]
    sdr = gpu.AudioSDRBatch(3)
    tuner = gpu.TunerBank(3, 1, D)
    h, g = tuner.get_filter()
    ref = R.TunerRef(3, 1, D, h, g)
    for c in range(3):
        sdr.setDemodMode(modes[c], ch=c)
        hz = dials[c] - fc - sdr.getTuningOffset(c)
        tuner.set_frequency(hz, ch=c); ref.set_frequency(hz, ch=c)
    hip = Hip()
    s = hip.stream()
    dIQ = hip.upload(iq[None])
    row = nb * 128 * 2
    dI, dQ, dOut = hip.malloc(3 * row), hip.malloc(3 * row), hip.malloc(3 * row)
    tuner.update_device(dIQ, dI, dQ, nb, stream=s)
    sdr.update_device(dI, dQ, dOut, nb, stream=s)
    hip.sync(s)
    got = hip.download(dOut, (3, nb, 128), np.int16)
    wI, wQ = ref.update(iq[None])
    assert np.array_equal(hip.download(dI, (3, nb, 128), np.int16), wI)

    def conf(o, c):
        o.setDemodMode([ao.USBmode, ao.AMmode, ao.WSPRmode][c])

    want, _ = ao.run_channels(conf, wI, wQ)
    assert np.array_equal(got, want)
    for c in range(3):
        a = got[c].reshape(-1)[nb * 128 // 2:].astype(float)
        spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(a.size)))
        peak = np.fft.rfftfreq(a.size, 1 / 44100.0)[np.argmax(spec)]
        assert abs(peak - expect_hz[c]) < 20.0, (c, peak)
    hip.free_all()
    sdr.close(); tuner.close()
