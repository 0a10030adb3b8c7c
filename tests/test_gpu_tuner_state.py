"""Tuner state records on the GPU (include/asdr_tuner.h, "State records"; asdr_tuner_state.hip): a bank restored from its blob and
its channel records, or a channel moved between banks in lockstep, writes as its next output what the uninterrupted bank would have
written -- tolerance 0 everywhere.  Expected values: the uninterrupted numpy restatements (tests/tuner_ref.py, tuner_rate_ref.py) for
direct-form and rate banks; for fast-convolution banks an uninterrupted GPU bank given the same calls, which runs none of the new
code (test_gpu_tuner_full.py holds the loaded bank to float64; the monitors use no float atomics, so equality is exact there too)."""
import numpy as np
import pytest

import tuner_rate_ref as RR
import tuner_ref as R
from helpers import Hip

pytestmark = pytest.mark.gpu

FWS = [0, 1 << 31, 0xFFF00000, 0x01234567, 0x7FFFFFFF, 0x80000001, 0x0FEDCBA9]
REC = 2560


def random_iq(rng, n_src, n, amp=20000):
    return rng.integers(-amp, amp, size=(n_src, n, 2), endpoint=True).astype(np.int16)


def tune(objs, c, n_src, k=0):
    for o in objs:
        o.set_source((c + k) % n_src, ch=c); o.set_frequency_word(FWS[(c + 3 * k) % len(FWS)], ch=c)
        if (c + k) % 3 == 0:
            o.set_phase(0x9E3779B9 * (c + k + 1), ch=c)


def restore(gpu, bank, n_channels=None):
    new = gpu.TunerBank.from_bank_state(bank.export_bank_state(), n_channels or bank.n_channels)
    new.import_channels(bank.export_channels(), channels=list(range(bank.n_channels)))
    return new


def same(got, want, what=""):
    for g, w in zip(got, want):
        assert g.shape == w.shape, (what, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: first mismatch at %s of %s" % (what, bad[0], g.shape)


def same_state(bank, ref):
    st = bank.read_state()
    assert (st["src"] == ref.src).all() and (st["fw"] == ref.fw).all() and (st["pos_a"] == ref.pos_a).all() and (st["ph_a"] == ref.ph_a).all()
    assert bank.position() == ref.P


# ---- 1. direct form
@pytest.mark.parametrize("cut", [1, 2])
def test_direct_form_restored_bank_continues_bit_exactly(gpu, cut):
    n, n_src, D, nb = 24, 2, 7, 3
    rng = np.random.default_rng(100 + cut)
    a = gpu.TunerBank(n, n_src, D)
    h, g = a.get_filter()
    assert h.size == 85
    ref = R.TunerRef(n, n_src, D, h, g)
    for c in range(n):
        tune((a, ref), c, n_src)
    for k in range(cut):
        for c in range(k, n, 5):
            tune((a, ref), c, n_src, k + 1)          # retunes land between calls
        iq = random_iq(rng, n_src, nb * 128 * D)
        same(a.update_rate(iq), ref.update(iq), "before the cut")
    for c in range(2, n, 4):
        tune((a, ref), c, n_src, 7)                  # anchors AT the cut: the whole filter history of these channels is flushed
    b = restore(gpu, a)
    assert b.position() == a.position() == cut * nb * 128 * D
    same_state(b, ref)
    for k in range(3):
        iq = random_iq(rng, n_src, nb * 128 * D)
        want = ref.update(iq)
        same(b.update_rate(iq), want, "restored bank, call %d" % k)
        same(a.update_rate(iq), want, "exporting bank, call %d" % k)
        same_state(b, ref); same_state(a, ref)
        for c in range(k, n, 6):
            tune((a, b, ref), c, n_src, 9 + k)


# ---- 2. rate banks
def rate_bank(gpu, rng, fs, D, n=8, n_src=2):
    a = gpu.TunerBank(n, n_src, D, fs_in=fs)
    if D > 1:                                        # a short stage-1 filter keeps the numpy restatement quick
        hh = np.round(rng.standard_normal(61) * 400).astype(np.int16)
        a.set_filter(hh, 1)
    h, g = a.get_filter()
    h2, g2 = a.get_resampler()
    ref = RR.TunerRateRef(n, n_src, D, fs, h, g, h2, g2)
    for c in range(n):
        tune((a, ref), c, n_src)
    return a, ref


def rate_step(banks, ref, iq, what):
    nf = iq.shape[1] // (128 * ref.D)
    want = ref.update(iq)
    for b in banks:
        assert b.out_blocks(nf) == want[0].shape[1], what
        same(b.update_rate(iq), want, what)
        assert b.output_position() == ref.out_pos


@pytest.mark.parametrize("fs,D", [(48000, 1), (2400000, 50)])
@pytest.mark.parametrize("cut", [0, 1, 2])
def test_rate_bank_restored_at_either_carry_parity(gpu, fs, D, cut):
    """cut = 0: before the first stage-2 call (the carry does not exist yet); 1 and 2: both parities of the carry rows."""
    rng = np.random.default_rng(200 + 10 * cut + D)
    a, ref = rate_bank(gpu, rng, fs, D)
    for k in range(cut):
        rate_step([a], ref, random_iq(rng, 2, 2 * 128 * D), "before the cut")
        tune((a, ref), k, 2, k + 1)
    b = restore(gpu, a)
    for k in range(3):
        rate_step([b, a], ref, random_iq(rng, 2, 2 * 128 * D), "call %d after the cut" % k)
    same_state(b, ref)


def test_rate_bank_restored_in_the_stale_condition(gpu):
    """Pass-through calls, then a real stage 2, then the cut: the restored bank's first stage-2 call sees u = 0 before it too."""
    n, n_src, D = 8, 2, 4
    rng = np.random.default_rng(300)
    a = gpu.TunerBank(n, n_src, D)
    h, g = a.get_filter()
    ref = RR.TunerRateRef(n, n_src, D, 44100 * D, h, g)
    for c in range(n):
        tune((a, ref), c, n_src)
    for k in range(2):
        rate_step([a], ref, random_iq(rng, n_src, 2 * 128 * D), "pass-through call")
    h2 = np.array([3000, -9000, 20000, 11000, -4000], dtype=np.int16)
    for o in (a, ref):
        o.set_resampler(h2, 1)
    b = restore(gpu, a)
    for k in range(3):
        rate_step([b, a], ref, random_iq(rng, n_src, 2 * 128 * D), "call %d after the cut" % k)
    c = restore(gpu, a)                              # ... and once more with a live carry, into a bank whose own carry is fresh
    rate_step([c, b, a], ref, random_iq(rng, n_src, 2 * 128 * D), "second restore")


# ---- 3. fast convolution, against an uninterrupted GPU bank
def fc_bank(gpu, fs, R, n_src, n, fmt):
    t = gpu.TunerBank.fastconv(n, n_src, fs, R)
    t.set_input_format(fmt)
    t.set_palette_filter(3, gpu.design_channel_filter(fs / R, 300.0, 2700.0))      # a complex slot
    t.set_palette_filter(9, np.array([0.5, 0.25, -0.125], dtype=np.float32))
    for c in range(n):
        tune((t,), c, n_src)
        t.set_gain([1.0, -0.5, 2.25][c % 3], ch=c)
    t.set_channel_slot(3, ch=1); t.set_channel_slot(9, ch=n - 1)
    t.set_iq_correction(words=(37, -21, 1200, 66000), source=n_src - 1)
    t.enable_iq_stats(True)
    t.enable_spectrum(256, "hann", "sum"); t.enable_levels(True)
    return t


def fc_rows(rng, fmt, n_src, n):
    x = rng.integers(-20000, 20000, size=(n_src, n, 2), endpoint=True).astype(np.int16)
    return np.ascontiguousarray(x[..., 0]) if fmt == "rs16" else x


def fc_observe(t):
    return [t.iq_stats(clear=False).tobytes(), t.spectrum(clear=False)[0].tobytes(), t.spectrum_frames(), t.levels(clear=False)[0].tobytes(),
            t.levels_frames(), t.position(), t.output_position(), t.read_state().tobytes(), t.slots().tobytes(), t.gains().tobytes()]


@pytest.mark.parametrize("fs,R,n_src,n,fmt,cut", [(96000, 2, 2, 6, "cs16", 1), (96000, 2, 2, 6, "rs16", 2), (2400000, 32, 2, 6, "rs16", 1),
                                                  (2400000, 32, 2, 6, "cs16", 2), (61440000, 1024, 1, 2, "cs16", 1)])
def test_fastconv_restored_bank_equals_the_uninterrupted_one(gpu, fs, R, n_src, n, fmt, cut):
    rng = np.random.default_rng(400 + R + cut)
    H = 128 * R
    u, a = fc_bank(gpu, fs, R, n_src, n, fmt), fc_bank(gpu, fs, R, n_src, n, fmt)
    for k, nf in enumerate([1, 2][:cut]):
        x = fc_rows(rng, fmt, n_src, nf * H)
        same(a.update_samples(x), u.update_samples(x), "before the cut")
        tune((u, a), k, n_src, k + 1)
    b = restore(gpu, a)
    assert fc_observe(b) == fc_observe(u)
    for k, nf in enumerate([2, 1]):
        x = fc_rows(rng, fmt, n_src, nf * H)
        want = u.update_samples(x)
        same(b.update_samples(x), want, "restored bank, call %d" % k)
        same(a.update_samples(x), want, "exporting bank, call %d" % k)
        assert fc_observe(b) == fc_observe(u) and fc_observe(a) == fc_observe(u)
        tune((u, a, b), n - 1 - k, n_src, 5 + k)


# ---- 4. moving and cloning between banks in lockstep, device forms on the caller's stream
def test_channels_move_between_lockstep_banks_on_a_stream(gpu):
    fs, D, n_src = 48000, 1, 2
    rng = np.random.default_rng(500)
    hip = Hip()
    try:
        a = gpu.TunerBank(16, n_src, D, fs_in=fs)
        b = gpu.TunerBank(40, n_src, D, fs_in=fs)
        h, g = a.get_filter()
        h2, g2 = a.get_resampler()
        ra, rb = RR.TunerRateRef(16, n_src, D, fs, h, g, h2, g2), RR.TunerRateRef(40, n_src, D, fs, h, g, h2, g2)
        for c in range(16):
            tune((a, ra), c, n_src, 1)
        for c in range(40):
            tune((b, rb), c, n_src, 2)
        for k in range(2):
            iq = random_iq(rng, n_src, 2 * 128)
            rate_step([a], ra, iq, "bank A"); rate_step([b], rb, iq, "bank B")
        src, dst = [3, 9, 15], [39, 0, 17]
        stream = hip.stream()
        d_rec = hip.malloc(3 * REC)
        a.export_channels_device(d_rec, src, stream)
        b.import_channels_device(d_rec, dst, stream)             # no host synchronisation in between
        others = [c for c in range(40) if c not in dst]
        for k in range(2):
            iq = random_iq(rng, n_src, 2 * 128)
            wa, wb = ra.update(iq), rb.update(iq)
            got = b.update_rate(iq)
            same([got[0][dst], got[1][dst]], [wa[0][src], wa[1][src]], "moved rows, call %d" % k)
            same([got[0][others], got[1][others]], [wb[0][others], wb[1][others]], "other rows, call %d" % k)
            same(a.update_rate(iq), wa, "bank A goes on")
        one = a.export_channels([5])
        five = [2, 7, 11, 30, 31]
        b.import_channels(np.repeat(one, 5, axis=0), channels=five)
        iq = random_iq(rng, n_src, 2 * 128)
        wa = ra.update(iq)
        got = b.update_rate(iq)
        for c in five:
            same([got[0][c], got[1][c]], [wa[0][5], wa[1][5]], "clone in channel %d" % c)
        hip.sync(stream)
    finally:
        hip.free_all()


# ---- 5. grow
def test_a_bank_grows_and_the_new_channels_start_in_creation_state(gpu):
    n_src, D, nb = 2, 7, 2
    rng = np.random.default_rng(600)
    a = gpu.TunerBank(6, n_src, D)
    h, g = a.get_filter()
    ra, rb = R.TunerRef(6, n_src, D, h, g), R.TunerRef(10, n_src, D, h, g)     # rb: channels never touched stay in creation state
    src, dst = [0, 2, 4], [7, 1, 9]
    for c in range(6):
        tune((a, ra), c, n_src, 1)
    for s, d in zip(src, dst):
        rb.src[d], rb.fw[d], rb.pos_a[d], rb.ph_a[d] = ra.src[s], ra.fw[s], ra.pos_a[s], ra.ph_a[s]
    for k in range(2):
        iq = random_iq(rng, n_src, nb * 128 * D)
        same(a.update_rate(iq), ra.update(iq), "before")
        rb.update(iq)
    b = gpu.TunerBank.from_bank_state(a.export_bank_state(), 10)
    b.import_channels(a.export_channels(src), channels=dst)
    same_state(b, rb)
    for k in range(3):
        iq = random_iq(rng, n_src, nb * 128 * D)
        same(b.update_rate(iq), rb.update(iq), "grown bank, call %d" % k)
        tune((b, rb), 3 + k, n_src, 4)                          # a new channel is tuned like any other
    same_state(b, rb)


# ---- 6. canonical bytes
@pytest.mark.parametrize("kind", ["rate", "fastconv"])
def test_exports_do_not_depend_on_the_buffer_parities(gpu, kind):
    rng = np.random.default_rng(700)
    n, n_src = 5, 2
    if kind == "rate":
        mk, per = (lambda: gpu.TunerBank(n, n_src, 1, fs_in=48000)), 128
    else:
        mk, per = (lambda: gpu.TunerBank.fastconv(n, n_src, 96000, 2)), 256
    a, b = mk(), mk()
    for c in range(n):
        tune((a, b), c, n_src)
    iq = random_iq(rng, n_src, 4 * per)
    a.update_rate(iq)                                            # 1 x 4 frames: one flip of every double buffer
    for k in range(4):
        b.update_rate(iq[:, k * per:(k + 1) * per])              # 4 x 1 frames: four
    blob, rec = a.export_bank_state(), a.export_channels()
    assert blob.tobytes() == b.export_bank_state().tobytes() and rec.tobytes() == b.export_channels().tobytes()
    assert rec[:, 256:].any() and (gpu.tuner_channel_field(rec, "content") == 3).all()
    assert not rec[:, 104:256].any()
    c = restore(gpu, a)                                          # an export directly after an import returns the bytes that went in
    assert c.export_bank_state().tobytes() == blob.tobytes() and c.export_channels().tobytes() == rec.tobytes()
    c.update_rate(iq[:, :per])                                   # ... at the other parity too
    d = restore(gpu, c)
    assert d.export_bank_state().tobytes() == c.export_bank_state().tobytes() and d.export_channels().tobytes() == c.export_channels().tobytes()


# ---- 7. a rejected device import
def test_a_rejected_device_import_changes_nothing(gpu):
    fs, D, n_src, n = 48000, 1, 2, 8
    rng = np.random.default_rng(800)
    hip = Hip()
    try:
        a, ref = rate_bank(gpu, rng, fs, D, n, n_src)
        for k in range(2):
            rate_step([a], ref, random_iq(rng, n_src, 2 * 128), "before")
        rec = a.export_channels([4, 5, 6])
        gpu.tuner_channel_field(rec, "src")[:] = (gpu.tuner_channel_field(rec, "src") + 1) % n_src     # would change rows 0 and 1 ...
        gpu.tuner_channel_field(rec, "carry")[:] ^= 0x5A5A5A5A
        gpu.tuner_channel_field(rec, "position")[2] += 128 * D                                        # ... but the LAST record is refused
        d_rec = hip.upload(rec)
        stream = hip.stream()
        before = a.read_state().tobytes()
        with pytest.raises(gpu.AsdrError, match=r"record 2 \(channel 2\): taken at position"):
            a.import_channels_device(d_rec, [0, 1, 2], stream)
        assert a.read_state().tobytes() == before
        for k in range(2):
            rate_step([a], ref, random_iq(rng, n_src, 2 * 128), "after the refusal")
    finally:
        hip.free_all()


# ---- 8. list shapes
def cyc_bank(gpu, n, n_src=2):
    """A 48 kHz bank whose channel c is tuned like channel c % 7, and the 7-channel restatement."""
    a = gpu.TunerBank(n, n_src, 1, fs_in=48000)
    h, g = a.get_filter()
    h2, g2 = a.get_resampler()
    ref = RR.TunerRateRef(7, n_src, 1, 48000, h, g, h2, g2)
    for c in range(7):
        tune((ref,), c, n_src)
    for c in range(n):
        a.set_source(ref.src[c % 7], ch=c); a.set_frequency_word(int(ref.fw[c % 7]), ch=c); a.set_phase(int(ref.ph_a[c % 7]), ch=c)
    return a, ref


def cyc_same(bank, ref, iq, what):
    want = ref.update(iq)
    got = bank.update_rate(iq)
    idx = np.arange(bank.n_channels) % 7
    same(got, [want[0][idx], want[1][idx]], what)


def test_list_shapes_against_the_host_forms(gpu):
    rng = np.random.default_rng(900)
    hip = Hip()
    try:
        a, ref = cyc_bank(gpu, 300)
        for k in range(2):
            cyc_same(a, ref, random_iq(rng, 2, 2 * 128), "before")
        stream = hip.stream()
        d_rec = hip.malloc(300 * REC)
        b = gpu.TunerBank.from_bank_state(a.export_bank_state(), 300)
        at = 300
        for m in (1, 3, 4, 5, 257):
            chans = list(range(at - 1, at - 1 - m, -1))          # descending
            at -= m
            hip.fill(d_rec, 0xEE, 300 * REC)
            a.export_channels_device(d_rec, chans, stream)
            hip.sync(stream)
            got = hip.download(d_rec, (300, REC), np.uint8)
            assert got[:m].tobytes() == a.export_channels(chans).tobytes(), m
            assert (got[m:] == 0xEE).all(), m                    # nothing past the list's records is written
            b.import_channels_device(d_rec, chans, stream)
        assert at == 30
        b.import_channels(a.export_channels(list(range(30))), channels=list(range(30)))
        assert b.export_channels().tobytes() == a.export_channels().tobytes()
        for bank in (b, a):
            iq = random_iq(rng, 2, 2 * 128)
            if bank is b:
                a.update_rate(iq)
            else:
                b.update_rate(iq)
            cyc_same(bank, ref, iq, "restored through lists" if bank is b else "the exporting bank")
    finally:
        hip.free_all()


def test_a_whole_4099_channel_bank_as_a_range(gpu):
    rng = np.random.default_rng(901)
    hip = Hip()
    try:
        n = 4099
        a, ref = cyc_bank(gpu, n)
        cyc_same(a, ref, random_iq(rng, 2, 128), "before")
        stream = hip.stream()
        d_rec = hip.malloc(n * REC)
        a.export_channels_device(d_rec, None, stream)
        hip.sync(stream)
        assert hip.download(d_rec, (n, REC), np.uint8).tobytes() == a.export_channels().tobytes()
        b = gpu.TunerBank.from_bank_state(a.export_bank_state(), n)
        b.import_channels_device(d_rec, None, stream)
        cyc_same(b, ref, random_iq(rng, 2, 128), "restored from the range")
    finally:
        hip.free_all()
