"""Input formats of the digital tuner on the GPU (include/asdr_tuner.h, "Input formats").

Complex formats (CU8, CS8, CF32), all three bank kinds: tolerance 0.  A bank of format F fed stored samples `raw` gives bit for
bit what an identically configured CS16 bank gives on tests/tuner_formats_ref.py's to_cs16(raw, F) through the existing entry
point (the converted values are exact in int16 and in float32), and direct-form / rate banks also equal tuner_ref / tuner_rate_ref
on the converted input.  The same for a change of format between calls, for RS16 on direct-form and rate banks (against (a, 0)),
for strided rows, and for call splits.

RS16 on fast-convolution banks computes X by a half-size transform, so it is held to the float64 restatement instead:
|u - clip(z)| <= 0.5 + EPS on each part with z = TunerFastconvRef.update((a, 0), keep_float=True), EPS from two float32 models of
the statement on the test's own inputs (RS_EPS below), and behind a real stage 2 to test_gpu_tuner_fastconv.py's Stage2Cap.  The
recipes (RS_CASES) and measure() are shared with test_tuner_formats_eps.py, which recomputes the table's small entries on the CPU."""
import collections

import numpy as np
import pytest

import tuner_fastconv_ref as F
import tuner_formats_ref as FM
import tuner_rate_ref as RR
import tuner_ref as TR
from helpers import Hip
from test_gpu_tuner_fastconv import Stage2Cap, clip16, compare_u

pytestmark = pytest.mark.gpu

# bank kinds of the bit-exact comparisons: name -> (kind, D or R, Fs_in or None)
CONFIGS = {
    "plain D=1": ("direct", 1, None), "plain D=48": ("direct", 48, None), "rate 2.4 MS/s D=50": ("direct", 50, 2400000),
    "fastconv R=2": ("fc", 2, 44100 * 2), "fastconv R=16": ("fc", 16, 44100 * 16), "fastconv R=128": ("fc", 128, 44100 * 128),
    "fastconv 2.4 MS/s R=16": ("fc", 16, 2400000), "fastconv 20 MS/s R=128": ("fc", 128, 20000000),
}
N_CH, N_SRC = 5, 2
FWS = [0x01234567, 0x9E3779B9, 0, 0x7FFFF000, 0xFEDCBA98]


def make_bank(gpu, config, n_ch=N_CH, n_src=N_SRC):
    kind, D, fs = CONFIGS[config]
    if kind == "fc":
        return gpu.TunerBank.fastconv(n_ch, n_src, fs, D)
    return gpu.TunerBank(n_ch, n_src, D, fs_in=fs)


def make_ref(bank, config, n_ch=N_CH, n_src=N_SRC):
    """tuner_ref / tuner_rate_ref with the bank's own taps for a direct-form or rate bank, None for a fast-convolution bank (its
    yardstick here is the CS16 bank)."""
    kind, D, fs = CONFIGS[config]
    if kind == "fc":
        return None
    h, g = bank.get_filter()
    if fs is None:
        return TR.TunerRef(n_ch, n_src, D, h, g)
    h2, g2 = bank.get_resampler()
    return RR.TunerRateRef(n_ch, n_src, D, fs, h, g, h2, g2)


def tune(objs, n_ch=N_CH, n_src=N_SRC):
    for o in objs:
        if o is not None:
            for c in range(n_ch):
                o.set_source(c % n_src, ch=c); o.set_frequency_word(FWS[c % len(FWS)] + 977 * (c // len(FWS)), ch=c)


def retune(objs):
    for o in objs:
        if o is not None:
            o.set_frequency_word(0x13579BDF, ch=1); o.set_phase(0xDEADBEEF, ch=3); o.set_source(0, ch=4)


def same(got, want, what):
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    for g, w, part in ((got[0], want[0], "I"), (got[1], want[1], "Q")):
        bad = np.argwhere(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, (what, part, len(bad), bad[0])


def run_pieces(gpu, config, pieces, do_retune=True):
    """pieces: [(fmt, raw)] fed call by call to one bank; the CS16 bank (and the restatement) get to_cs16 of each piece through
    update_rate.  Everything must agree bit for bit; returns the calls' (I, Q)."""
    bank, plain = make_bank(gpu, config), make_bank(gpu, config)
    ref = make_ref(bank, config)
    tune([bank, plain, ref])
    outs = []
    for k, (fmt, raw) in enumerate(pieces):
        if k == 1 and do_retune:
            retune([bank, plain, ref])
        conv = FM.to_cs16(raw, fmt)
        bank.set_input_format(fmt)
        got = bank.update_samples(raw)
        want = plain.update_rate(conv)
        same(got, want, (config, fmt, k, "against the CS16 bank"))
        if ref is not None:
            same(got, ref.update(conv), (config, fmt, k, "against the restatement"))
        assert bank.position() == plain.position() and bank.output_position() == plain.output_position()
        outs.append(got)
    bank.close(); plain.close()
    return outs


@pytest.mark.parametrize("fmt", FM.COMPLEX_FORMATS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_complex_formats_equal_the_cs16_bank_bit_for_bit(gpu, config, fmt):
    """Three calls of different frame counts (the history / window crosses calls), a retune before the second, two sources."""
    kind, D, fs = CONFIGS[config]
    rng = np.random.default_rng(sum(map(ord, config + fmt)))
    per = 128 * D
    fs_in = fs or 44100 * D
    pieces = [(fmt, FM.raw_noise(rng, fmt, N_SRC, nf * per, tones=[(0, 0.07 * fs_in, 6000.0), (1, -0.31 * fs_in, 5000.0)], fs=fs_in))
              for nf in (1, 3, 2)]
    outs = run_pieces(gpu, config, pieces)
    assert any(o[0].any() for o in outs)


@pytest.mark.parametrize("config", ["plain D=48", "rate 2.4 MS/s D=50", "fastconv R=16", "fastconv 20 MS/s R=128"])
def test_format_switch_mid_stream(gpu, config):
    """CU8, then CS16, then CF32, then CS8 on one bank: the carried history / window is converted samples."""
    kind, D, fs = CONFIGS[config]
    rng = np.random.default_rng(len(config))
    per = 128 * D
    pieces = [(fmt, FM.raw_noise(rng, fmt, N_SRC, nf * per)) for fmt, nf in (("cu8", 2), ("cs16", 1), ("cf32", 2), ("cs8", 1))]
    run_pieces(gpu, config, pieces, do_retune=False)


@pytest.mark.parametrize("config", ["plain D=1", "plain D=48", "rate 2.4 MS/s D=50"])
def test_rs16_on_direct_form_and_rate_banks(gpu, config):
    """Real samples: bit-exact against the restatements fed (a, 0) and against the CS16 bank fed the same."""
    kind, D, fs = CONFIGS[config]
    rng = np.random.default_rng(16 + D)
    per = 128 * D
    fs_in = fs or 44100 * D
    pieces = [("rs16", FM.raw_noise(rng, "rs16", N_SRC, nf * per, amp=30000, tones=[(0, 0.07 * fs_in, 2500.0)], fs=fs_in))
              for nf in (1, 3, 2)]
    outs = run_pieces(gpu, config, pieces)
    assert all(o[1].any() for o in outs if o[1].size)         # a real source still has a Q row after the mixer


# RS16 on a fast-convolution bank is not bit-exact with the CS16 bank (test_rs16_fastconv_* hold it to the restatement)
STRIDED = [(c, f) for c in ("plain D=48", "fastconv R=16", "fastconv 20 MS/s R=128") for f in ("cu8", "cs8", "cf32")] + [("plain D=48", "rs16")]


@pytest.mark.parametrize("config,fmt", STRIDED)
def test_strided_rows_through_device_pointers(gpu, config, fmt):
    """in_stride_samples larger than the row (a multiple of 16 bytes), the gap filled with a pattern no format maps to zero."""
    kind, D, fs = CONFIGS[config]
    rng = np.random.default_rng(sum(map(ord, config + fmt)) + 1)
    nf, per = 3, 128 * D
    n = nf * per
    raw = FM.raw_noise(rng, fmt, N_SRC, n)
    gap = 3 * (16 // FM.BYTES[fmt])
    padded = np.full((N_SRC, n + gap) + raw.shape[2:], 0x55, dtype=raw.dtype)
    padded[:, :n] = raw
    bank, plain = make_bank(gpu, config), make_bank(gpu, config)
    tune([bank, plain])
    bank.set_input_format(fmt)
    hip = Hip()
    s = hip.stream()
    nb = bank.out_blocks(nf)
    dIn, dI, dQ = hip.upload(padded), hip.malloc(N_CH * (nb + 1) * 256), hip.malloc(N_CH * (nb + 1) * 256)
    assert bank.update_samples_device(dIn, dI, dQ, nf, nb + 1, in_stride_samples=n + gap, stream=s) == nb
    hip.sync(s)
    got = (hip.download(dI, (N_CH, nb + 1, 128), np.int16)[:, :nb], hip.download(dQ, (N_CH, nb + 1, 128), np.int16)[:, :nb])
    same(got, plain.update_rate(FM.to_cs16(raw, fmt)), (config, fmt))
    with pytest.raises(gpu.AsdrError, match="16-byte aligned"):
        bank.update_samples_device(dIn, dI, dQ, nf, nb + 1, in_stride_samples=n + gap + 1, stream=s)
    assert bank.position() == n
    hip.free_all()
    bank.close(); plain.close()


def test_int16_entry_points_leave_a_cu8_bank_untouched(gpu):
    bank = make_bank(gpu, "plain D=48")
    bank.set_input_format("cu8")
    iq = np.zeros((N_SRC, 128 * 48, 2), np.int16)
    for call in (lambda: bank.update(iq), lambda: bank.update_rate(iq)):
        with pytest.raises(gpu.AsdrError, match="input format is CU8"):
            call()
    assert bank.position() == 0 and bank.output_position() == 0
    bank.close()


# ---- RS16 on fast-convolution banks ----------------------------------------------------------------------------------------
RsCase = collections.namedtuple("RsCase", "n_ch fs R events")
RS_R = [2, 8, 16, 32, 128, 1024]      # N / 2 in LDS with a radix-2 last pass (2, 8) and pure radix 4 (16); four-step (32, 128, 1024)


def rs_bins(R):
    """Coarse bins whose 256-bin gather (i) straddles bin 0 (50, -50), (ii) straddles N / 2 (N / 2 - 60, and -N / 2 itself),
    (iii) lies wholly in the conjugate half (-N / 4: bins -N / 4 - 128 .. -N / 4 + 127, all negative), (iv) sits on 0 and N / 2 - 1."""
    H, N, q = F.sizes(R)
    return [0, N // 2 - 1, 50, -50, N // 2 - 60, -N // 2, -N // 4, -N // 4 + (7 if N >= 1024 else 0)]


def rs_words(R):
    H, N, q = F.sizes(R)
    rws = [0, 0] + [(i * 0x9E3779B9) % q - q // 2 for i in range(1, 7)]
    return [(k0 * q + rw) & 0xFFFFFFFF for k0, rw in zip(rs_bins(R), rws)]


def real_rows(rng, n, fs, tones, amp=20000):
    x = rng.integers(-amp, amp, size=(1, n), endpoint=True).astype(np.float64)
    m = np.arange(n)
    for f, a in tones:
        x[0] += a * np.cos(2 * np.pi * f * m / fs + 0.3)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def bins_case(R):
    """Noise in +-20000 plus one real tone of 1500 per distinct |k0| (700 Hz above it: each shows in its channel and, mirrored,
    in the channel of -k0), three calls with a retune before the second (channel 6 moves to the mirror image of channel 2)."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(6400 + R)
    fws = rs_words(R)
    tones = [(k * fs / N + 700.0, 1500.0) for k in sorted(set(min(abs(k0), N // 2 - 2) for k0 in rs_bins(R)))]

    def events():
        yield ("set", lambda o: [o.set_frequency_word(fw, ch=c) for c, fw in enumerate(fws)])
        for k, nf in enumerate([1, 2] if R == 1024 else [1, 3, 2]):
            if k == 1:
                yield ("set", lambda o: (o.set_frequency_word((-fws[2]) & 0xFFFFFFFF, ch=6), o.set_phase(0xCAFEF00D, ch=3)))
            yield ("a", real_rows(rng, nf * H, fs, tones), (R, k))
    return RsCase(len(fws), fs, R, events())


def square_case(R):
    """A full-scale square wave (+-32767, period 80 R input samples = 80 samples of u) seen by channels at fw = 0 with phases 0, half a turn and a quarter turn (the filter's overshoot drives +32767 and -32768 on
    the real or the imaginary part), and by one at its fundamental; then the same through twice the default filter."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    fws = [0, 0, 0, F.RR.fw_from_hz(fs / (80.0 * R), fs), F.RR.fw_from_hz(-fs / (80.0 * R), fs)]

    def rows(m0, n):
        m = m0 + np.arange(n)
        half = 40 * R
        k = m // half
        return np.where(k % 2 == 0, 32767, -32767).astype(np.int16)[None, :]

    def events():
        yield ("set", lambda o: ([o.set_frequency_word(fw, ch=c) for c, fw in enumerate(fws)], o.set_phase(1 << 31, ch=1),
                                 o.set_phase(1 << 30, ch=2)))
        at = 0
        for k, nf in enumerate([2, 1, 2]):
            if k == 2:
                yield ("set", lambda o: o.set_channel_filter(2.0 * np.asarray(o.get_channel_filter(), dtype=np.float32)))
            yield ("a", rows(at, nf * H), (R, k))
            at += nf * H
    return RsCase(len(fws), fs, R, events())


RS_CASES = {"bins": bins_case, "square": square_case}
RS_CASE_R = {"bins": RS_R, "square": [2, 16, 32]}


def measure(recipe, R):
    """(largest |model - z| on either part over the recipe's own inputs, both clipped as compare_u clips, the model being the
    worse of TunerFastconvRef.stage1_f32 (complex64, full size) and tuner_formats_ref.stage1_half_f32 (complex64, half-size
    transform and untangle); peak |z|)."""
    case = RS_CASES[recipe](R)
    a, b, c = (F.TunerFastconvRef(case.n_ch, 1, case.fs, R) for _ in range(3))
    worst = peak = 0.0
    for ev in case.events:
        if ev[0] == "set":
            ev[1](a); ev[1](b); ev[1](c)
        else:
            iq = FM.to_cs16(ev[1], "rs16")
            z = a.update(iq, keep_float=True)[2]
            for w in (b.update(iq, keep_float=True, f32=True)[2], FM.stage1_half_f32(c, iq)):
                worst = max(worst, float(np.abs(clip16(w.real) - clip16(z.real)).max()), float(np.abs(clip16(w.imag) - clip16(z.imag)).max()))
            peak = max(peak, float(np.abs(z).max()))
    return worst, peak


# RS_EPS[recipe, R] = min(8 x measure(recipe, R)[0], 0.1) to three digits: the factor 8, its reasoning and the 0.1 ceiling are
# test_gpu_tuner_fastconv.py's (two correct float32 implementations differ in pass order, twiddle tables, the NCO's float phase
# and the place of 1 / N; the untangle adds one more twiddle product and two sums per bin, which the second model carries).
# Produced on the CPU by
#     python tests/test_gpu_tuner_formats.py
# (test_tuner_formats_eps.py recomputes the entries with R <= 16 to 10 %).
RS_EPS = {
    ("bins", 2): 0.0317,   # measured 0.00396 at peak |z| 20910
    ("bins", 8): 0.0145,   # measured 0.00181 at peak |z| 11343
    ("bins", 16): 0.012,   # measured 0.0015 at peak |z| 8365
    ("bins", 32): 0.00799,   # measured 0.000999 at peak |z| 6133
    ("bins", 128): 0.00722,   # measured 0.000903 at peak |z| 4788
    ("bins", 1024): 0.00475,   # measured 0.000593 at peak |z| 3399
    ("square", 2): 0.1,   # measured 0.0186 at peak |z| 77650: 8 x is 0.149, held to the 0.1 ceiling
    ("square", 16): 0.1,   # measured 0.0215 at peak |z| 76666: 8 x is 0.172, held to the 0.1 ceiling
    ("square", 32): 0.1,   # measured 0.0173 at peak |z| 76559: 8 x is 0.138, held to the 0.1 ceiling
}
assert max(RS_EPS.values(), default=0.0) <= 0.1


def rs_pair(gpu, case):
    bank = gpu.TunerBank.fastconv(case.n_ch, 1, case.fs, case.R)
    bank.set_input_format("rs16")
    assert bank.ratio() == (1, 1) and bank.fft_size() == 256 * case.R
    return bank, F.TunerFastconvRef(case.n_ch, 1, case.fs, case.R, g=bank.get_channel_filter())


def run_rs(bank, ref, events, eps):
    outs = []
    for ev in events:
        if ev[0] == "set":
            ev[1](bank); ev[1](ref)
        else:
            I, Q = bank.update_samples(ev[1])
            wI, wQ, z = ref.update(FM.to_cs16(ev[1], "rs16"), keep_float=True)
            print(ev[2], "max |got - z| = %.4f re, %.4f im (bound %.4f), peak |z| %.0f" % (
                np.abs(I.reshape(I.shape[0], -1) - clip16(z.real)).max(), np.abs(Q.reshape(Q.shape[0], -1) - clip16(z.imag)).max(),
                0.5 + eps, np.abs(z).max()))
            compare_u((I, Q), z, eps, ev[2])
            assert bank.position() == ref.P and bank.output_position() == ref.out_pos
            outs.append((I, Q, z))
    return outs


@pytest.mark.parametrize("R", RS_R)
def test_rs16_fastconv_u_within_half_plus_eps_of_float64(gpu, R):
    """Every gather position of rs_bins(): across bin 0, across N / 2, wholly in the conjugate half (the mirror image must come
    out), on k0 = 0 and on N / 2 - 1."""
    case = bins_case(R)
    bank, ref = rs_pair(gpu, case)
    outs = run_rs(bank, ref, case.events, RS_EPS["bins", R])
    assert len(outs) == (2 if R == 1024 else 3)
    bank.close()


@pytest.mark.parametrize("R", RS_CASE_R["square"])
def test_rs16_fastconv_full_scale_square_wave_drives_both_clamps(gpu, R):
    case = square_case(R)
    bank, ref = rs_pair(gpu, case)
    outs = run_rs(bank, ref, case.events, RS_EPS["square", R])
    I = np.concatenate([o[0].reshape(case.n_ch, -1) for o in outs], axis=1)
    Q = np.concatenate([o[1].reshape(case.n_ch, -1) for o in outs], axis=1)
    assert I[0].max() == 32767 and I[0].min() == -32768 and I[1].max() == 32767 and I[1].min() == -32768
    assert Q[2].max() == 32767 and Q[2].min() == -32768
    bank.close()


RS64 = dict(fs=64800000, R=512, n_ch=6, frames=[1, 4, 2, 3])


def rs64_inputs():
    """The real-stage-2 case: 64.8 MS/s, R = 512 (N = 131072, Fs_mid = 126.5625 kHz, 392 / 1125); noise plus a tone per channel."""
    fs, R = RS64["fs"], RS64["R"]
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(648)
    fws = rs_words(R)[:RS64["n_ch"]]
    tones = [(abs(k0) * fs / N + 900.0, 2000.0) for k0 in (50, N // 2 - 60)] + [(900.0, 2000.0)]
    return fws, [real_rows(rng, nf * H, fs, tones) for nf in RS64["frames"]]


def test_rs16_fastconv_through_a_real_stage_2_at_64_8_msps(gpu):
    """Behind stage 2 the Stage2Cap rule of test_gpu_tuner_fastconv.py, unchanged: +-2 on every sample, and no more samples off
    than the restatement shows when its own u is moved by +-1 on a seeded 2 % of samples."""
    fs, R, n_ch = RS64["fs"], RS64["R"], RS64["n_ch"]
    fws, calls = rs64_inputs()
    bank = gpu.TunerBank.fastconv(n_ch, 1, fs, R)
    assert bank.ratio() == (392, 1125) and bank.fft_size() == 131072
    bank.set_input_format("rs16")
    h2, g2 = bank.get_resampler()
    ref = F.TunerFastconvRef(n_ch, 1, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2)
    for o in (bank, ref):
        for c, fw in enumerate(fws):
            o.set_frequency_word(fw, ch=c)
    cap = Stage2Cap(648)
    for k, a in enumerate(calls):
        I, Q = bank.update_samples(a)
        wI, wQ = cap.update(ref, FM.to_cs16(a, "rs16"))
        assert I.shape == wI.shape
        cap.check(I, wI, what=k); cap.check(Q, wQ, what=k)
        assert bank.output_position() == ref.out_pos
    cap.finish("RS16 at 64.8 MS/s")
    bank.close()


@pytest.mark.parametrize("fmt,R", [("cu8", 16), ("cu8", 32), ("rs16", 16), ("rs16", 32)])
def test_call_splits_are_bit_identical(gpu, fmt, R):
    """One call of 4 frames equals calls of 1 + 3 frames, in LDS (R = 16) and four-step (R = 32)."""
    fs = 44100 * R
    rng = np.random.default_rng(R + len(fmt))
    raw = FM.raw_noise(rng, fmt, 2, 4 * 128 * R)
    outs = []
    for split in ([4], [1, 3]):
        bank = gpu.TunerBank.fastconv(N_CH, 2, fs, R)
        tune([bank], n_src=2)
        bank.set_input_format(fmt)
        parts, at = [], 0
        for nf in split:
            parts.append(bank.update_samples(raw[:, at:at + nf * 128 * R]))
            at += nf * 128 * R
        outs.append((np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)))
        bank.close()
    same(outs[1], outs[0], (fmt, R))
    assert outs[0][0].any()


def test_rs16_fastconv_bank_into_the_chain_on_one_stream(gpu, ao):
    """A real-sampled source (2.4 MS/s, R = 16) -> RS16 fast-convolution bank -> asdr_update_device (USB) on one stream: the
    chain's audio equals the oracle run on the bank's own I/Q rows, bit for bit; the rows are the restatement's within Stage2Cap."""
    fs, R, nf = 2400000, 16, 48
    dials = [450_000.0, 910_000.0]
    rng = np.random.default_rng(2416)
    n = nf * 128 * R
    t = np.arange(n) / fs
    x = rng.standard_normal(n) * 3.0
    for f, a in ((dials[0] + 1200.0, 6000.0), (dials[1] + 700.0, 6000.0)):
        x = x + a * np.cos(2 * np.pi * f * t)
    a16 = np.round(x).astype(np.int16)[None, :]
    sdr = gpu.AudioSDRBatch(2)
    tuner = gpu.TunerBank.fastconv(2, 1, fs, R)
    tuner.set_input_format("rs16")
    h2, g2 = tuner.get_resampler()
    ref = F.TunerFastconvRef(2, 1, fs, R, g=tuner.get_channel_filter(), h2=h2, g2=g2)
    cap = Stage2Cap(2416)
    sdr.setDemodMode(gpu.USBmode)
    for c in range(2):
        hz = dials[c] - sdr.getTuningOffset(c)
        tuner.set_frequency(hz, ch=c); ref.set_frequency(hz, ch=c)
    hip = Hip()
    s = hip.stream()
    dIn = hip.upload(a16)
    nb = tuner.out_blocks(nf)
    row = nb * 128 * 2
    dI, dQ, dOut = hip.malloc(2 * row), hip.malloc(2 * row), hip.malloc(2 * row)
    assert tuner.update_samples_device(dIn, dI, dQ, nf, nb, stream=s) == nb
    sdr.update_device(dI, dQ, dOut, nb, stream=s)
    hip.sync(s)
    got = hip.download(dOut, (2, nb, 128), np.int16)
    tI, tQ = hip.download(dI, (2, nb, 128), np.int16), hip.download(dQ, (2, nb, 128), np.int16)
    wI, wQ = cap.update(ref, FM.to_cs16(a16, "rs16"))
    cap.check(tI, wI); cap.check(tQ, wQ)
    cap.finish("RS16 into the chain")
    want, _ = ao.run_channels(lambda o, c: o.setDemodMode(ao.USBmode), tI, tQ)
    assert np.array_equal(got, want)
    for c, tone in enumerate((1200.0, 700.0)):
        y = got[c].reshape(-1)[nb * 128 // 2:].astype(float)
        spec = np.abs(np.fft.rfft((y - y.mean()) * np.hanning(y.size)))
        peak = np.fft.rfftfreq(y.size, 1 / 44100.0)[np.argmax(spec)]
        assert abs(peak - tone) < 20.0, (c, peak)
    hip.free_all()
    sdr.close(); tuner.close()


if __name__ == "__main__":                                    # the RS_EPS table: measured on the CPU, pasted in above
    for recipe, Rs in RS_CASE_R.items():
        for R in Rs:
            worst, peak = measure(recipe, R)
            note = "" if 8 * worst <= 0.1 else ": 8 x is %.3g, held to the 0.1 ceiling" % (8 * worst)
            print('    ("%s", %d): %.3g,   # measured %.3g at peak |z| %.0f%s' % (recipe, R, min(8 * worst, 0.1), worst, peak, note), flush=True)
