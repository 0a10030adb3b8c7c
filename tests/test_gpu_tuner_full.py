"""A fully loaded fast-convolution bank on the GPU -- a stored input format, per-source corrections with statistics, a palette with
slots and gains, the spectrum and the level monitors, and a real stage 2, all on at once -- against the composed float64
restatement tests/tuner_full_ref.py, which chains the restatements of the single features in the order include/asdr_tuner.h states
them.  Every other GPU file holds one feature with the rest at the defaults; the combination is a code path of its own: with a
correction off the identity the pre-pass redirects stage 1 to a CS16 / RS16 scratch, and the call after the last correction has
gone back to the identity returns to the format's own kernels, so that the first frame of that call takes half its window from a
history row written by the other kernel family.  The streams below end on exactly that call.  Direct-form and rate banks with a
format and corrections are held to tuner_ref / tuner_rate_ref on condition(to_cs16(raw)) in one step, tolerance 0.

Every call goes through update_samples_device with a padded row stride and the gap filled with the format's rail value
(test_gpu_tuner_condition.call_device), and every row starts and ends on a rail-valued sample: a stride error shows in the output
and in `clipped`.

Tolerances: EPS[recipe] is min(8 x the largest |float32 model - float64 restatement| of stage 1 on the
recipe's own conditioned inputs, both clipped as compare_u clips, 0.1); EPS_A[recipe] the same factor on the amplitude-domain
difference of the complex64 spectrum model.  Both are measured on the CPU against the restatement, produced by
    python tests/test_gpu_tuner_full.py
and recomputed (R = 2) by tests/test_tuner_full_ref.py, which also shows that each recipe tells eight deliberately wrong
compositions apart by more than 10 x its bounds.  The levels go by EPS (the rule of test_gpu_tuner_monitor.py); the statistics,
positions, slots, gains and launch counts are exact; the outputs behind a real stage 2 go by Stage2Cap's own bounds."""
import collections
import os
import sys

import numpy as np
import pytest

import test_gpu_tuner_condition as TC
import test_gpu_tuner_fastconv as T
import test_gpu_tuner_monitor as TM
import test_gpu_tuner_palette as TP
import test_gpu_tuner_state as TS
import tuner_condition_ref as CR
import tuner_fastconv_ref as F
import tuner_formats_ref as FM
import tuner_full_ref as FR
import tuner_rate_ref as RR
import tuner_ref as TR
from helpers import Hip

pytestmark = pytest.mark.gpu

FMTS = ["cs16", "cu8", "cs8", "cf32", "rs16"]
RS = [2, 32]
SPEC = (256, "hann", "sum")
ENDS = {"cs16": (-32768, 32767), "rs16": (-32768, 32767), "cu8": (0, 255), "cs8": (-128, 127), "cf32": (-1.0, 1.0)}   # the rails
RESTORED = [("cu8", 2), ("rs16", 32), ("cf32", 32)]
S2_FMTS = ["cu8", "rs16"]
S2 = dict(fs=2400000, R=16, n_ch=6, n_src=2, frames=[1, 4, 2, 3])

# A stream is a bank's shape and format and a list of events: ("set", fn) -> fn(o) on the bank and on the LoadedBankRef alike;
# ("raw", rows, label) -> one update call on stored rows of the format.
Stream = collections.namedtuple("Stream", "key n_ch n_src fs R fmt events")


def stored(iq, fmt):
    """CS16 rows -> stored rows of the format whose conversion is as close as the format allows, the first sample of every row at
    (low rail, high rail) and the last at (high, low)."""
    raw = FM.from_cs16(iq, fmt)
    lo, hi = ENDS[fmt]
    if fmt == "rs16":
        raw[:, 0], raw[:, -1] = lo, hi
    else:
        raw[:, 0], raw[:, -1] = (lo, hi), (hi, lo)
    return np.ascontiguousarray(raw)


def monitors_and_corrections(o, fmt):
    """What every loaded bank adds to its base: the format, the spectrum, the levels, the statistics, source 1 at MILD_A."""
    o.set_input_format(fmt)
    o.enable_spectrum(*SPEC); o.enable_levels(); o.enable_iq_stats()
    o.set_iq_correction(words=TC.MILD_A, source=1)


def back_to_the_identity(o):
    o.set_iq_correction(words=CR.IDENTITY, source=0); o.set_iq_correction(words=CR.IDENTITY, source=1)


def loaded_stream(fmt, R):
    """test_gpu_tuner_palette.parity_case(R) -- 16 channels over 2 sources at coarse bins 0, +-1, N / 2 - 1 and -N / 2, every
    pairing of slots 1, 2, 3, 0 with gains 1, 0.25, 8, -1, tones at both ends of the gathers -- as stored rows of `fmt`, with
    monitors_and_corrections.  Calls of 1, 3 and 2 frames; the third call's rows are the first two frames of the second call's
    read backwards with I and Q exchanged (x -> j conj x reversed: the same noise level, every tone still on its frequency).
    Before call 2: a retune and a new phase, a slot reassignment, a gain change (the gain-8 channel 2 to -0.5), source 0 to
    MILD_B.  Before call 3: both sources back to the identity."""
    H, N, q = F.sizes(R)
    case = TP.parity_case(R)
    ev = list(case.events)
    configure, iq1, iq3 = ev[0][1], ev[1][1], ev[2][1]
    assert iq1.shape[1] == H and iq3.shape[1] == 3 * H
    iq2 = np.ascontiguousarray(iq3[:, :2 * H][:, ::-1, ::-1])

    def changes(o):
        o.set_frequency_word((5 * q + q // 3) & 0xFFFFFFFF, ch=9); o.set_phase(0xDEADBEEF, ch=1)
        o.set_channel_slot(3, ch=4); o.set_gain(-0.5, ch=2)
        o.set_iq_correction(words=TC.MILD_B, source=0)

    events = [("set", lambda o: (configure(o), monitors_and_corrections(o, fmt))), ("raw", stored(iq1, fmt), (fmt, R, "call 1")),
              ("set", changes), ("raw", stored(iq3, fmt), (fmt, R, "call 2")),
              ("set", back_to_the_identity), ("raw", stored(iq2, fmt), (fmt, R, "call 3"))]
    return Stream((fmt, R), case.n_ch, case.n_src, case.fs, R, fmt, events)


def stage2_stream(fmt, A):
    """test_gpu_tuner_palette.test_palette_behind_a_real_stage_2 (2.4 MS/s, R = 16, stage 2: 147 / 500; designed slots, mixed
    gains) as stored rows of `fmt` with monitors_and_corrections; calls of 1, 4, 2 and 3 frames (10 frames of u give two
    output blocks, which end inside call 3).  Before call 2 source 0 goes to MILD_B; before call 3 that test's changes, and both
    sources back to the identity: the frame that straddles the switch is one the outputs reach."""
    fs, R, n_ch, n_src = S2["fs"], S2["R"], S2["n_ch"], S2["n_src"]
    rng = np.random.default_rng(2401 + len(fmt))
    usb, am = A.design_channel_filter(fs / R, 300.0, 3000.0), A.design_channel_filter(fs / R, -5000.0, 5000.0)

    def configure(o):
        T.setup(o, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
        o.set_palette_filter(1, usb); o.set_palette_filter(2, am)
        for c, (s, a) in enumerate(zip([0, 1, 2, 1, 2, 0], [1.0, 2.0, 0.5, -1.0, 1.0, 2.0])):
            o.set_channel_slot(s, ch=c); o.set_gain(a, ch=c)
        monitors_and_corrections(o, fmt)

    def changes(o):
        o.set_channel_slot(2, ch=1); o.set_gain(-2.0, ch=0); o.set_frequency(-fs * 0.3, ch=3)
        back_to_the_identity(o)

    events = [("set", configure)]
    for k, nf in enumerate(S2["frames"]):
        if k in (1, 2):
            events.append(("set", changes if k == 2 else lambda o: o.set_iq_correction(words=TC.MILD_B, source=0)))
        iq = T.cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0)], fs, -5000, 5000)
        events.append(("raw", stored(iq, fmt), (fmt, "stage 2", "call %d" % (k + 1))))
    return Stream((fmt + "+s2", R), n_ch, n_src, fs, R, fmt, events)


def stream(key, A=None):
    return stage2_stream(key[0][:-3], A) if key[0].endswith("+s2") else loaded_stream(*key)


KEYS = [(f, R) for f in FMTS for R in RS] + [(f + "+s2", S2["R"]) for f in S2_FMTS]


def taps(A, s):
    """The bank's own default taps (channel filter; stage 2 where it is a real one), from a bank that needs no device."""
    bank = A.TunerBank.fastconv(s.n_ch, s.n_src, s.fs, s.R, device=A.NO_DEVICE)
    kw = dict(g=bank.get_channel_filter())
    if bank.ratio() != (1, 1):
        kw["h2"], kw["g2"] = bank.get_resampler()
    bank.close()
    return kw


def composed(s, kw, f32=False, cls=FR.LoadedBankRef):
    return cls(s.n_ch, s.n_src, s.fs, s.R, f32=f32, **kw)


def measure(key, A):
    """(largest |float32 model - restatement| of stage 1 on either part, both clipped as compare_u clips; peak |z|; largest amplitude
    difference of the complex64 spectrum model; peak amplitude) over the recipe's own calls."""
    s = stream(key, A)
    kw = taps(A, s)
    a, b = composed(s, kw), composed(s, kw, f32=True)
    worst = peak = 0.0
    for ev in s.events:
        if ev[0] == "set":
            ev[1](a); ev[1](b)
        else:
            z, w = a.update_samples(ev[1])[2], b.update_samples(ev[1])[2]
            worst = max(worst, float(np.abs(T.clip16(w.real) - T.clip16(z.real)).max()), float(np.abs(T.clip16(w.imag) - T.clip16(z.imag)).max()))
            peak = max(peak, float(np.abs(z).max()))
    return (worst, peak) + tuple(a.spectrum_model_error())


# EPS[recipe] = min(8 x measure(recipe)[0], 0.1) to three digits (int16 units).
EPS = {
    ("cs16", 2): 0.0619,   # measured 0.00773 at peak |z| 187654
    ("cs16", 32): 0.0213,   # measured 0.00266 at peak |z| 20315
    ("cu8", 2): 0.0707,   # measured 0.00884 at peak |z| 187511
    ("cu8", 32): 0.0245,   # measured 0.00306 at peak |z| 20406
    ("cs8", 2): 0.0713,   # measured 0.00891 at peak |z| 187835
    ("cs8", 32): 0.0204,   # measured 0.00255 at peak |z| 20255
    ("cf32", 2): 0.0619,   # measured 0.00773 at peak |z| 187654
    ("cf32", 32): 0.0213,   # measured 0.00266 at peak |z| 20315
    ("rs16", 2): 0.0587,   # measured 0.00734 at peak |z| 132841
    ("rs16", 32): 0.0219,   # measured 0.00274 at peak |z| 14109
    ("cu8+s2", 16): 0.0114,   # measured 0.00142 at peak |z| 10659
    ("rs16+s2", 16): 0.00477,   # measured 0.000597 at peak |z| 2767
}
# EPS_A[recipe] = 8 x measure(recipe)[2] to three digits (amplitude, int16 units).
EPS_A = {
    ("cs16", 2): 0.000163,   # measured 2.04e-05 at peak amplitude 1760
    ("cs16", 32): 0.00055,   # measured 6.87e-05 at peak amplitude 1795
    ("cu8", 2): 0.000702,   # measured 8.78e-05 at peak amplitude 1759
    ("cu8", 32): 0.000339,   # measured 4.24e-05 at peak amplitude 1795
    ("cs8", 2): 0.00033,   # measured 4.13e-05 at peak amplitude 1759
    ("cs8", 32): 0.000356,   # measured 4.45e-05 at peak amplitude 1794
    ("cf32", 2): 0.000163,   # measured 2.04e-05 at peak amplitude 1760
    ("cf32", 32): 0.00055,   # measured 6.87e-05 at peak amplitude 1795
    ("rs16", 2): 9.82e-05,   # measured 1.23e-05 at peak amplitude 458
    ("rs16", 32): 0.000117,   # measured 1.47e-05 at peak amplitude 475
    ("cu8+s2", 16): 0.000728,   # measured 9.1e-05 at peak amplitude 3600
    ("rs16+s2", 16): 0.000243,   # measured 3.03e-05 at peak amplitude 1773
}
assert max(EPS.values(), default=0.0) <= 0.1


# ---- the comparisons ---------------------------------------------------------------------------------------------------------
def check_stats(gpu, bank, L, clear):
    """The seven sums of every source, exactly: read without clear, and (clear) once more with it, after which both are empty."""
    want = TC.stats_array(gpu, L.iq_stats(clear=False))
    assert want["n"].all() and want["clipped"].all()
    for c in ((False, True) if clear else (False,)):
        st = bank.iq_stats(clear=c)
        for name in CR.STAT_NAMES:
            assert st[name].tolist() == want[name].tolist(), (name, c, st[name], want[name])
    if clear:
        L.clear_iq_stats()
        assert not any(bank.iq_stats(clear=False)[name].any() for name in CR.STAT_NAMES)


def check_observables(gpu, bank, L, key, what, launches, clear_stats=True):
    """Everything but the outputs, after a call: the spectrum, the levels, the statistics, positions, slots, gains, launches."""
    got, frames = bank.spectrum(clear=False)
    TM.check_spectrum(got, frames, L.spectrum(), EPS_A[key], SPEC, what)
    TM.check_levels(bank, L.mon, EPS[key], what)
    check_stats(gpu, bank, L, clear_stats)
    assert bank.position() == L.position() and bank.output_position() == L.output_position(), what
    assert list(bank.slots()) == list(L.slots()) and list(bank.gains()) == list(L.gains()), what
    assert bank.condition_launches() == launches, (what, bank.condition_launches(), launches)


def check_u(got, z, key, what):
    print(what, "max |got - z| = %.4f re, %.4f im (bound %.4f)" % (
        np.abs(got[0].reshape(got[0].shape[0], -1) - T.clip16(z.real)).max(),
        np.abs(got[1].reshape(got[1].shape[0], -1) - T.clip16(z.imag)).max(), 0.5 + EPS[key]))
    T.compare_u(got, z, EPS[key], what)


def pair(gpu, s):
    bank = gpu.TunerBank.fastconv(s.n_ch, s.n_src, s.fs, s.R)
    kw = dict(g=bank.get_channel_filter())
    if bank.ratio() != (1, 1):
        kw["h2"], kw["g2"] = bank.get_resampler()
    return bank, composed(s, kw)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("fmt", FMTS)
def test_loaded_bank_matches_the_composed_restatement(gpu, fmt, R):
    s = loaded_stream(fmt, R)
    bank, L = pair(gpu, s)
    assert bank.ratio() == (1, 1) and bank.fft_size() == 256 * R
    hip = Hip()
    st = hip.stream()
    calls = 0
    for ev in s.events:
        if ev[0] == "set":
            ev[1](bank); ev[1](L)
            continue
        nf = ev[1].shape[1] // L.H
        got = TC.call_device(hip, st, bank, ev[1], fmt, nf)
        z = L.update_samples(ev[1])[2]
        calls += 1
        check_u(got, z, s.key, ev[2])
        assert L.condition_launches() == calls                # the statistics are on throughout: a pre-pass launch in every call
        check_observables(gpu, bank, L, s.key, ev[2], calls)
    assert calls == 3 and bank.iq_correction(0) == bank.iq_correction(1) == CR.IDENTITY and bank.input_format() == fmt
    hip.free_all()
    bank.close()


@pytest.mark.parametrize("fmt", S2_FMTS)
def test_loaded_bank_behind_a_real_stage_2(gpu, fmt):
    s = stage2_stream(fmt, gpu)
    bank, L = pair(gpu, s)
    assert bank.ratio() == (147, 500) and not L.pass_through()
    cap = T.Stage2Cap(2401)
    hip = Hip()
    st = hip.stream()
    calls = 0
    for ev in s.events:
        if ev[0] == "set":
            ev[1](bank); ev[1](L)
            continue
        nf = ev[1].shape[1] // L.H
        assert bank.out_blocks(nf) == L.out_blocks(nf)
        I, Q = TC.call_device(hip, st, bank, ev[1], fmt, nf)
        wI, wQ = L.update_samples(ev[1], run=cap.update)
        calls += 1
        assert I.shape == wI.shape
        cap.check(I, wI, what=ev[2]); cap.check(Q, wQ, what=ev[2])
        check_observables(gpu, bank, L, s.key, ev[2], calls)
    assert calls == len(S2["frames"])
    cap.finish("the loaded bank behind stage 2, %s" % fmt)
    hip.free_all()
    bank.close()


@pytest.mark.parametrize("fmt,R", RESTORED)
def test_loaded_bank_restored_mid_stream(gpu, fmt, R):
    """The first test's stream; after call 2 a new bank is made of the blob and the channel records.  Call 3 -- both sources back
    at the identity, its first frame straddling the switch of kernel families -- runs on the exporting and on the restored bank:
    equal to each other bit for bit in every observable, and both held to the composed restatement, which was never interrupted."""
    s = loaded_stream(fmt, R)
    a, L = pair(gpu, s)
    hip = Hip()
    st = hip.stream()
    for ev in s.events[:4]:
        if ev[0] == "set":
            ev[1](a); ev[1](L)
        else:
            got = TC.call_device(hip, st, a, ev[1], fmt, ev[1].shape[1] // L.H)
            check_u(got, L.update_samples(ev[1])[2], s.key, ev[2])
    check_observables(gpu, a, L, s.key, "before the export", 2, clear_stats=False)
    b = TS.restore(gpu, a)
    assert TS.fc_observe(b) == TS.fc_observe(a)
    change, raw, what = s.events[4][1], s.events[5][1], s.events[5][2]
    for o in (a, b, L):
        change(o)
    nf = raw.shape[1] // L.H
    got_a = TC.call_device(hip, st, a, raw, fmt, nf)
    got_b = TC.call_device(hip, st, b, raw, fmt, nf)
    TS.same(got_b, got_a, "restored against exporting bank")
    assert TS.fc_observe(b) == TS.fc_observe(a)
    z = L.update_samples(raw)[2]
    check_u(got_a, z, s.key, (what, "exporting bank"))
    check_u(got_b, z, s.key, (what, "restored bank"))
    check_observables(gpu, a, L, s.key, (what, "exporting bank"), 3, clear_stats=False)
    check_observables(gpu, b, L, s.key, (what, "restored bank"), 1, clear_stats=True)     # launches count from a bank's creation
    hip.free_all()
    a.close(); b.close()


# ---- direct-form and rate banks ----------------------------------------------------------------------------------------------
INT_CASES = [("plain", "cu8"), ("plain", "cf32"), ("rate", "cs8"), ("rate", "rs16")]
INT_N_CH, INT_N_SRC, INT_FRAMES = 6, 2, [2, 3, 2]
INT_CORRECTIONS = [[CR.IDENTITY, TC.MILD_A], [TC.MILD_B, TC.LIMITS_A], [CR.IDENTITY, CR.IDENTITY]]


def int_pair(mod, kind, device=0):
    """plain: D = 7 at 44100 D with the default filter; rate: Fs_in = 96000, D = 2 (stage 2: 147 / 160) with a short stage-1 filter,
    which keeps the numpy restatement quick.  6 channels over 2 sources."""
    if kind == "plain":
        bank = mod.TunerBank(INT_N_CH, INT_N_SRC, 7, device=device)
        h, g = bank.get_filter()
        ref = TR.TunerRef(INT_N_CH, INT_N_SRC, 7, h, g)
    else:
        bank = mod.TunerBank(INT_N_CH, INT_N_SRC, 2, fs_in=96000, device=device)
        bank.set_filter(np.round(np.random.default_rng(61).standard_normal(61) * 400).astype(np.int16), 1)
        h, g = bank.get_filter()
        h2, g2 = bank.get_resampler()
        ref = RR.TunerRateRef(INT_N_CH, INT_N_SRC, 2, 96000, h, g, h2, g2)
    for o in (bank, ref):
        for c in range(INT_N_CH):
            o.set_source(c % INT_N_SRC, ch=c); o.set_frequency_word(TC.FWS[c % 4] + 977 * (c // 4), ch=c)
    return bank, ref


def int_rows(kind, fmt):
    """The three calls' stored rows: noise in +-20000 with the format's specials on the first and last samples of every row."""
    rng = np.random.default_rng(70 + len(kind) + sum(map(ord, fmt)))
    per = 128 * (7 if kind == "plain" else 2)
    return [TC.rows(rng, fmt, INT_N_SRC, nf * per) for nf in INT_FRAMES]


@pytest.mark.parametrize("kind,fmt", INT_CASES)
def test_direct_and_rate_banks_with_formats_and_corrections(gpu, kind, fmt):
    """Format x correction on the integer banks against tuner_ref / tuner_rate_ref in one step: three calls, the corrections
    changing between them (mild, then the range limits on one source, then both back at the identity, where the pre-pass stops
    writing and the filter's history still holds x' of the call before).  Tolerance 0; the statistics exact."""
    bank, ref = int_pair(gpu, kind)
    bank.set_input_format(fmt)
    bank.enable_iq_stats()
    hip = Hip()
    st = hip.stream()
    want_stats = [(0,) * 7] * INT_N_SRC
    written = 0
    for k, (raw, corr) in enumerate(zip(int_rows(kind, fmt), INT_CORRECTIONS)):
        for s_ in range(INT_N_SRC):
            bank.set_iq_correction(words=corr[s_], source=s_)
        got = TC.call_device(hip, st, bank, raw, fmt, INT_FRAMES[k])
        want = FR.integer_bank_update(ref, raw, fmt, corr)
        TC.same(got, want, (kind, fmt, "call", k + 1))
        written += got[0].shape[1]
        assert bank.position() == ref.P and bank.condition_launches() == k + 1
        if kind == "rate":
            assert bank.output_position() == ref.out_pos
        want_stats = [CR.add_stats(want_stats[s_], CR.stats(raw[s_], fmt)) for s_ in range(INT_N_SRC)]
        w = TC.stats_array(gpu, want_stats)
        for clear in ((False, True) if k == 2 else (False,)):
            got_st = bank.iq_stats(clear=clear)
            for name in CR.STAT_NAMES:
                assert got_st[name].tolist() == w[name].tolist(), (kind, fmt, k, name, clear, got_st[name], w[name])
    assert written >= 5 and w["n"].all() and w["clipped"].all()
    hip.free_all()
    bank.close()


if __name__ == "__main__":                                    # the EPS and EPS_A tables: measured on the CPU, pasted in above
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import audiosdr_amd
    audiosdr_amd.load_library()
    rows = [(key, measure(key, audiosdr_amd)) for key in KEYS]
    for key, m in rows:
        print('    ("%s", %d): %.3g,   # measured %.3g at peak |z| %.0f' % (key[0], key[1], min(8 * m[0], 0.1), m[0], m[1]), flush=True)
    for key, m in rows:
        print('    ("%s", %d): %.3g,   # measured %.3g at peak amplitude %.0f' % (key[0], key[1], 8 * m[2], m[2], m[3]), flush=True)
