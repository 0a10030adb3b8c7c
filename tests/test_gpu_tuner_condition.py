"""Source conditioning of the digital tuner on the GPU (include/asdr_tuner.h, "Source conditioning").

The yardstick is the library's own unchanged CS16 path, tolerance 0: a bank with corrections, fed stored rows `raw` of format F,
must write bit for bit what an identically configured bank without any correction writes when fed
tests/tuner_condition_ref.py's condition(to_cs16(raw)) as CS16 (RS16 for real rows) -- fast-convolution banks included: the same
kernels on the same input are deterministic.  The statistics are integers and must equal the restatement's exactly.

Every case feeds the bank through device pointers with in_stride_samples larger than the row and the gap filled with the format's
rail value, so a stride error shows in the output and in `clipped`; rows start and end on tuner_formats_ref.specials(fmt)."""
import numpy as np
import pytest

import tuner_condition_ref as CR
import tuner_formats_ref as FM
from helpers import Hip

pytestmark = pytest.mark.gpu

FWS = [0x01234567, 0x9E3779B9, 0x7FFFF000, 0xFEDCBA98]
LIMITS_A, LIMITS_B = (-32768, 32767, 32768, 131072), (32767, -32768, -32768, 32768)
MILD_A, MILD_B = CR.KA_WORDS, (-1234, 4321, 2500, 70000)
RAIL = {"cs16": 32767, "rs16": 32767, "cu8": 255, "cs8": 127, "cf32": 1.0}


def t1_filter():
    """The 257-tap filter of tools/bench_tuner.py's config T1."""
    L = 257
    return np.round(np.hamming(L) * np.sinc((np.arange(L) - (L - 1) / 2) * 0.5) * 16384 / 2).astype(np.int16)


def plain(gpu, n_ch=4, n_src=2):
    def make():
        t = gpu.TunerBank(n_ch, n_src, 1)
        t.set_filter(t1_filter(), 0)
        return t
    return make


def rate(gpu):
    return lambda: gpu.TunerBank(4, 2, 2, fs_in=96000)


def fastconv(gpu, R, n_ch=4, n_src=2):
    return lambda: gpu.TunerBank.fastconv(n_ch, n_src, 44100 * R, R)


def tune(t, srcs=None):
    for c in range(t.n_channels):
        t.set_source(c % t.n_sources if srcs is None else srcs[c], ch=c)
        t.set_frequency_word(FWS[c % len(FWS)] + 977 * (c // len(FWS)), ch=c)


def rows(rng, fmt, n_src, n):
    """Stored rows with the format's specials on their first and last samples."""
    raw = FM.raw_noise(rng, fmt, n_src, n)
    sp = FM.specials(fmt)
    if fmt == "rs16":
        raw[:, -sp.size:] = sp[::-1]
    else:
        raw[:, -sp.size:, 0] = sp[::-1]
        raw[:, -sp.size:, 1] = sp
    return raw


def padded(raw, fmt, gap):
    out = np.full((raw.shape[0], raw.shape[1] + gap) + raw.shape[2:], RAIL[fmt], dtype=raw.dtype)
    out[:, :raw.shape[1]] = raw
    return out


def same(got, want, what):
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    for g, w, part in ((got[0], want[0], "I"), (got[1], want[1], "Q")):
        bad = np.argwhere(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, (what, part, len(bad), bad[0])


def call_device(hip, stream, bank, raw, fmt, nf, gap=None, int16_entry=False):
    """One update through device pointers with a padded row stride; returns (I, Q) of the blocks written."""
    n = raw.shape[1]
    gap = 3 * (16 // FM.BYTES[fmt]) if gap is None else gap
    nb = bank.out_blocks(nf)
    n_ch = bank.n_channels
    dIn = hip.upload(padded(raw, fmt, gap))
    dI, dQ = hip.malloc(n_ch * (nb + 1) * 256), hip.malloc(n_ch * (nb + 1) * 256)
    entry = bank.update_rate_device if int16_entry else bank.update_samples_device
    assert entry(dIn, dI, dQ, nf, nb + 1, in_stride_samples=n + gap, stream=stream) == nb
    hip.sync(stream)
    return (hip.download(dI, (n_ch, nb + 1, 128), np.int16)[:, :nb], hip.download(dQ, (n_ch, nb + 1, 128), np.int16)[:, :nb])


def stats_array(gpu, per_source):
    out = np.zeros(len(per_source), dtype=gpu.IQ_STATS_DTYPE)
    for s, st in enumerate(per_source):
        for k, v in zip(CR.STAT_NAMES, st):
            out[k][s] = v
    return out


def run_case(gpu, make, fmt, frames, corrections, seed, stats_from=0, gap=None, int16_entry=False, srcs=None):
    """frames[k] frames in call k with corrections[k][s] on source s (set before the call); the statistics go on before call
    stats_from.  Output against the yardstick bank call by call, then the statistics (read without and with clear)."""
    bank, yard = make(), make()
    tune(bank, srcs); tune(yard, srcs)
    n_src = bank.n_sources
    bank.set_input_format(fmt)
    yard.set_input_format("rs16" if fmt == "rs16" else "cs16")
    rng = np.random.default_rng(seed)
    hip = Hip()
    stream = hip.stream()
    per = 128 * bank.decimation
    want_stats = [(0,) * 7] * n_src
    launches = 0
    for k, nf in enumerate(frames):
        if k == stats_from:
            bank.enable_iq_stats()
        for s in range(n_src):
            bank.set_iq_correction(words=corrections[k][s], source=s)
        raw = rows(rng, fmt, n_src, nf * per)
        got = call_device(hip, stream, bank, raw, fmt, nf, gap, int16_entry)
        cond = np.stack([CR.condition_raw(raw[s], corrections[k][s], fmt) for s in range(n_src)])
        same(got, yard.update_samples(cond), (fmt, "call", k))
        assert bank.position() == yard.position() and bank.output_position() == yard.output_position()
        if k >= stats_from:
            want_stats = [CR.add_stats(want_stats[s], CR.stats(raw[s], fmt)) for s in range(n_src)]
        launches += 1
        assert bank.condition_launches() == launches and yard.condition_launches() == 0
    want = stats_array(gpu, want_stats)
    for clear in (False, True):
        st = bank.iq_stats(clear=clear)
        for name in CR.STAT_NAMES:
            assert st[name].tolist() == want[name].tolist(), (fmt, name, clear, st[name], want[name])
    assert not any(bank.iq_stats(clear=False)[name].any() for name in CR.STAT_NAMES)
    assert want["n"].all() and (fmt == "rs16" or want["sum_im2"].all()) and want["clipped"].all()
    hip.free_all()
    bank.close(); yard.close()


@pytest.mark.parametrize("fmt", ["cs16", "cu8", "cs8", "cf32", "rs16"])
def test_plain_bank_every_format(gpu, fmt):
    """D = 1, 2 sources, 4 channels, 257 taps: 4 blocks per call, two calls, the corrections changed between them (the 256 samples
    of history the second call's filter reads hold x' of the old ones).  One source at the identity, one at the range limits."""
    run_case(gpu, plain(gpu), fmt, [4, 4], [[CR.IDENTITY, LIMITS_A], [MILD_A, LIMITS_B]], seed=11 + len(fmt) + ord(fmt[1]))


def test_plain_bank_cs16_rows_that_start_on_a_sample(gpu):
    """CS16 through the int16 entry point with a row stride that is no multiple of 16 bytes: the pre-pass reads by dwords."""
    run_case(gpu, plain(gpu), "cs16", [4, 4], [[MILD_B, LIMITS_B], [CR.IDENTITY, MILD_A]], seed=5, gap=7, int16_entry=True)


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
def test_rate_bank(gpu, fmt):
    """Fs_in = 96 kHz, D = 2 (stage 2: 147 / 160): 3 frames x 2 calls."""
    run_case(gpu, rate(gpu), fmt, [3, 3], [[LIMITS_B, CR.IDENTITY], [MILD_B, LIMITS_A]], seed=96 + len(fmt))


@pytest.mark.parametrize("fmt", ["cs16", "cs8", "cf32", "rs16"])
def test_fastconv_single_transform(gpu, fmt):
    """R = 2 (N = 512): 2 frames x 2 calls; the window of the second call's first frame holds x' of the first call's corrections.
    RS16: the half-size transform, with only d_r acting."""
    run_case(gpu, fastconv(gpu, 2), fmt, [2, 2], [[CR.IDENTITY, LIMITS_A], [MILD_A, MILD_B]], seed=512 + len(fmt) + ord(fmt[1]))


def test_fastconv_four_step(gpu):
    """R = 32 (N = 8192, the four-step path, which reads the window differently): 1 source, 2 channels, 2 frames per call."""
    run_case(gpu, fastconv(gpu, 32, n_ch=2, n_src=1), "cs16", [2, 2], [[MILD_B], [LIMITS_A]], seed=8192)


def test_rows_longer_than_the_grid(gpu):
    """64 sources x 384 blocks of a D = 1 bank: 12,288 items per row against 32 workgroups x 256 lanes, so every workgroup
    strides, the first half of them once more than the others.  Three channels, on the first, a middle and the last source."""
    n_src = 64
    corr = [[(17 * s - 500, 300 - 11 * s, 100 * s - 3000, 65536 + 512 * s) for s in range(n_src)]]
    corr[0][5] = CR.IDENTITY
    run_case(gpu, plain(gpu, n_ch=3, n_src=n_src), "cs16", [384], corr, seed=64, srcs=[0, 31, 63])


def test_statistics_enabled_after_the_first_call_count_only_the_second(gpu):
    run_case(gpu, fastconv(gpu, 2), "cu8", [2, 2], [[MILD_A, MILD_B], [MILD_A, MILD_B]], seed=77, stats_from=1)


@pytest.mark.parametrize("kind,fmt", [("plain", "cf32"), ("fastconv", "cs16"), ("fastconv", "rs16"), ("rate", "cu8")])
def test_statistics_alone_leave_the_output_bit_identical(gpu, kind, fmt):
    """Statistics on, every correction at the identity: the pre-pass only reads (condition_launches() goes up) and the bank's
    kernels read the caller's rows, in the caller's format, as a bank without statistics does."""
    make = {"plain": plain(gpu), "fastconv": fastconv(gpu, 2), "rate": rate(gpu)}[kind]
    bank, yard = make(), make()
    rng = np.random.default_rng(len(kind) + len(fmt))
    hip = Hip()
    stream = hip.stream()
    want = [(0,) * 7] * 2
    for t in (bank, yard):
        tune(t); t.set_input_format(fmt)
    bank.enable_iq_stats()
    for k in range(2):
        raw = rows(rng, fmt, 2, 3 * 128 * bank.decimation)
        same(call_device(hip, stream, bank, raw, fmt, 3), yard.update_samples(raw), (kind, fmt, k))
        want = [CR.add_stats(want[s], CR.stats(raw[s], fmt)) for s in range(2)]
    assert bank.condition_launches() == 2 and yard.condition_launches() == 0
    st, w = bank.iq_stats(), stats_array(gpu, want)
    assert all(st[name].tolist() == w[name].tolist() for name in CR.STAT_NAMES), (st, w)
    bank.enable_iq_stats(False)                                # off again: no pre-pass
    raw = rows(rng, fmt, 2, 128 * bank.decimation)
    same(call_device(hip, stream, bank, raw, fmt, 1), yard.update_samples(raw), (kind, fmt, "off"))
    assert bank.condition_launches() == 2
    hip.free_all()
    bank.close(); yard.close()


def test_off_state_launches_nothing_and_the_identity_stops_the_pre_pass(gpu):
    for make in (plain(gpu), rate(gpu), fastconv(gpu, 2)):
        bank, yard = make(), make()
        tune(bank); tune(yard)
        rng = np.random.default_rng(3)
        per = 128 * bank.decimation
        raw = rows(rng, "cs16", 2, 2 * per)
        same(bank.update_samples(raw), yard.update_samples(raw), "never conditioned")
        assert bank.condition_launches() == 0
        bank.set_iq_correction(words=MILD_B, source=1)
        raw = rows(rng, "cs16", 2, 2 * per)
        cond = np.stack([raw[0], CR.condition_raw(raw[1], MILD_B, "cs16")])
        same(bank.update_samples(raw), yard.update_samples(cond), "one source corrected")
        assert bank.condition_launches() == 1
        bank.set_iq_correction(source=1)                       # back to the identity
        raw = rows(rng, "cs16", 2, 2 * per)
        same(bank.update_samples(raw), yard.update_samples(raw), "back to the identity")
        bank.reset(); yard.reset()                             # reset keeps the (identity) corrections
        same(bank.update_samples(raw), yard.update_samples(raw), "after reset")
        assert bank.condition_launches() == 1 and yard.condition_launches() == 0
        bank.close(); yard.close()


def test_reset_keeps_the_corrections_and_clears_the_statistics(gpu):
    bank, yard = fastconv(gpu, 2)(), fastconv(gpu, 2)()
    tune(bank); tune(yard)
    rng = np.random.default_rng(9)
    bank.set_iq_correction(words=MILD_A); bank.enable_iq_stats()
    raw = rows(rng, "cs16", 2, 512)
    bank.update_samples(raw); yard.update_samples(raw)
    assert bank.iq_stats(clear=False)["n"].tolist() == [512, 512]
    bank.reset(); yard.reset()
    assert not bank.iq_stats(clear=False)["n"].any() and bank.iq_correction(1) == MILD_A
    tune(bank); tune(yard)
    cond = np.stack([CR.condition_raw(raw[s], MILD_A, "cs16") for s in range(2)])
    same(bank.update_samples(raw), yard.update_samples(cond), "after reset")
    assert bank.iq_stats()["n"].tolist() == [512, 512]
    bank.close(); yard.close()


def test_track_iq_end_to_end(gpu):
    """The quality known answer as CS16 through a plain bank (512 blocks of D = 1) with the statistics on; track_iq sets the known
    words, clears the statistics, and the next call is the yardstick's on the restatement-conditioned rows.  Tracking again from
    the same source gives the same words: the statistics are taken of x."""
    make = plain(gpu, n_ch=2, n_src=1)
    bank, yard = make(), make()
    tune(bank); tune(yard)
    x = CR.known_answer_rows()[None]
    bank.enable_iq_stats()
    same(bank.update_samples(x), yard.update_samples(x), "first call, identity")
    st = bank.iq_stats(clear=False)
    assert tuple(int(st[name][0]) for name in CR.STAT_NAMES) == CR.stats(x[0], "cs16")
    assert bank.track_iq() == 1
    assert bank.iq_correction(0) == CR.KA_WORDS
    assert not bank.iq_stats(clear=False)["n"].any()
    cond = CR.condition(x, CR.KA_WORDS)
    same(bank.update_samples(x), yard.update_samples(cond), "second call, tracked")
    assert bank.track_iq(0) == 1 and bank.iq_correction(0) == CR.KA_WORDS
    same(bank.update_samples(x[:, :512]), yard.update_samples(cond[:, :512]), "third call")
    assert bank.condition_launches() == 3
    # a source whose estimate fails keeps its correction: a constant row has no variance
    flat = np.full((1, 512, 2), 100, np.int16)
    bank.clear_iq_stats()
    bank.update_samples(flat)
    assert bank.track_iq() == 0 and bank.iq_correction(0) == CR.KA_WORDS
    bank.close(); yard.close()
