"""The filter palette and the gains of a fast-convolution bank on the GPU (include/asdr_tuner.h, "Filter palette and gain";
asdr_tuner_palette.hip) against the float64 restatement tests/tuner_palette_ref.py: u within 0.5 + EPS of the unrounded value
(test_gpu_tuner_fastconv.compare_u), untouched channels and call splits bit for bit, the levels without the gain, CU8 rows, and a
real stage 2 behind it.  Small banks: at most 16 channels, 2 sources and 4 frames per call, at R = 2 (N = 512: the
one-workgroup transform) and R = 32 (N = 8,192: four-step).

EPS[recipe, R] follows the rule of test_gpu_tuner_fastconv.py: 8 x the largest |stage1_f32 - stage1| on the
recipe's own inputs, gains included, both clipped to the int16 range as compare_u clips, with a ceiling of 0.1.  Produced by
    python tests/test_gpu_tuner_palette.py
and recomputed by tests/test_tuner_palette_ref.py.  The absolute float32 error of y grows with |a_c| as y does, so the recipes
keep |a_c y| of a sample that is not clamped inside the int16 range (the parity recipe feeds its gain-8 channels an eighth of what
the older recipes feed); the gain-64 recipe sits on the rails, where the clamp is what is looked at."""
import numpy as np
import pytest

import test_gpu_tuner_fastconv as T
import tuner_fastconv_ref as F
import tuner_formats_ref as FM
import tuner_palette_ref as P
from test_gpu_tuner_fastconv import Stage2Cap

pytestmark = pytest.mark.gpu

RS = [2, 32]
_rng = np.random.default_rng(1290)
G_CASYM = ((_rng.uniform(-1.0, 1.0, 129) + 1j * _rng.uniform(-1.0, 1.0, 129)) / 16.0 * np.linspace(0.25, 1.75, 129)).astype(np.complex64)
G_J = np.array([1j], dtype=np.complex64)                      # G = j on all 256 bins
G_SHORT = T.G_SHORT                                           # real, two taps
GAINS = [1.0, 0.25, 8.0, -1.0]


def palette(o):
    """Slot 1: an asymmetric complex 129-tap filter; slot 2: the one tap j; slot 3: a short real filter."""
    o.set_palette_filter(1, G_CASYM); o.set_palette_filter(2, G_J); o.set_palette_filter(3, G_SHORT)


def parity_case(R, gains=True):
    """16 channels over 2 sources: coarse bins 0, +-1, N / 2 - 1 and -N / 2 (the gather wraps around N), every (slot, gain) pair of
    slots 1, 2, 3, 0 and gains 1, 0.25, 8, -1 once.  Noise of amplitude min(20000, 5000 sqrt R) / 4 and tones of 625 within half a
    bin of k0 + 127 and k0 - 128 for the first channels at k0 = N / 2 - 1 and -N / 2: both ends of their gathers carry signal.
    One frame, then three (both parities of b - 1).  gains = False leaves every gain at 1: the levels' recipe."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(6400 + R)
    k0s = [0, 1, -1, N // 2 - 1, -N // 2]
    n_ch, n_src = 16, 2
    fws, slots, gs = [], [], []
    for i in range(n_ch):
        k0 = k0s[i % 5]
        res = int(rng.integers(-q // 2, q // 2))
        if k0 == -N // 2:
            res = abs(res) % (q // 2)                         # below -N / 2 there is no bin: it would be N / 2 - 1
        fws.append((k0 * q + res) & 0xFFFFFFFF)
        slots.append([1, 2, 3, 0][i % 4])
        gs.append(GAINS[(i + i // 4) % 4])
    assert len(set(zip(slots, gs))) == 16 and [int(k) for k in F.coarse(fws, R)[0]] == [k0s[i % 5] for i in range(n_ch)]
    srcs = [c % n_src for c in range(n_ch)]
    amp = int(min(20000.0, 5000.0 * np.sqrt(R)) / 4)
    tones = []
    for c in (3, 4):                                          # k0 = N / 2 - 1 and -N / 2
        for m in (127, -128):
            k = (k0s[c] + m + N // 2) % N - N // 2
            tones.append((srcs[c], (k + float(rng.uniform(-0.5, 0.5))) * fs / N, 625.0))

    def configure(o):
        T.setup(o, srcs, fws)
        palette(o)
        for c in range(n_ch):
            o.set_channel_slot(slots[c], ch=c)
            if gains:
                o.set_gain(gs[c], ch=c)

    def events():
        yield ("set", configure)
        for k, nf in enumerate([1, 3]):
            yield ("iq", T.cs16(rng, n_src, nf * H, tones, fs, -amp, amp), (R, k))
    return T.Case(n_ch, n_src, fs, R, events())


def gain_case(R):
    """Full-scale sources: source 0 is (-32768, -32768) throughout (channels at fw = 0 with phase 0 and half a turn: y =
    -+32768 (1 + j)), source 1 alternates (32767, -32768), (-32768, 32767) (channels at Fs_in / 2).  One frame at gain 1 fills the
    windows; then channels 0 .. 3 go to gains 64, 64, -64, 64 (64 times full scale: both clamps), channels 4 and 5 to gain 0 and
    -0.0, one of them on the complex slot 1; channel 6 stays at gain 1.  Two frames, then two more."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    fws = [0, 0, 1 << 31, 1 << 31, 0, 1 << 31, 0]
    srcs = [0, 0, 1, 1, 0, 1, 0]

    def source(m0, n):
        m = m0 + np.arange(n)
        x = np.zeros((2, n, 2))
        x[0] = -32768
        x[1, :, 0] = np.where(m % 2 == 0, 32767, -32768)
        x[1, :, 1] = np.where(m % 2 == 0, -32768, 32767)
        return x.astype(np.int16)

    def gains(o):
        for c, a in enumerate([64.0, 64.0, -64.0, 64.0, 0.0, -0.0]):
            o.set_gain(a, ch=c)

    def events():
        yield ("set", lambda o: (T.setup(o, srcs, fws), o.set_phase(1 << 31, ch=1), o.set_phase(1 << 30, ch=3), palette(o),
                                 o.set_channel_slot(1, ch=5), o.set_channel_slot(3, ch=6)))
        yield ("iq", source(0, H), (R, "gain 1"))
        yield ("set", gains)
        yield ("iq", source(H, 2 * H), (R, "gain 64, 0"))
        yield ("iq", source(3 * H, 2 * H), (R, "again"))
    return T.Case(len(fws), 2, fs, R, events())


def timing_before(o):
    palette(o)
    o.set_channel_slot(1, ch=0); o.set_channel_slot(2, ch=1); o.set_gain(0.5, ch=2)


def timing_change(o):
    """A reassignment (channel 0), a redefinition (slot 2: channels 0 and 1 follow) and two gain changes."""
    o.set_channel_slot(2, ch=0); o.set_palette_filter(2, G_SHORT); o.set_gain(-3.0, ch=2); o.set_gain(2.0, ch=3)


def timing_case(R):
    """6 channels, 2 sources, noise of amplitude min(20000, 5000 sqrt R) / 4; two frames, timing_change, two frames."""
    fs = 44100 * R
    H = 128 * R
    rng = np.random.default_rng(7700 + R)
    fws = [int(v) for v in rng.integers(0, 2 ** 32, size=6, dtype=np.uint64)]
    amp = int(min(20000.0, 5000.0 * np.sqrt(R)) / 4)

    def events():
        yield ("set", lambda o: (T.setup(o, [c % 2 for c in range(6)], fws), timing_before(o)))
        yield ("iq", T.cs16(rng, 2, 2 * H, (), fs, -amp, amp), (R, "before"))
        yield ("set", timing_change)
        yield ("iq", T.cs16(rng, 2, 2 * H, (), fs, -amp, amp), (R, "after"))
    return T.Case(6, 2, fs, R, events())


CASES = {"parity": parity_case, "gain": gain_case, "timing": timing_case, "levels": lambda R: parity_case(R, gains=False)}


def measure(recipe, R):
    """(largest |stage1_f32 - stage1| on either part, both clipped as compare_u clips; peak |z|) over the recipe's own inputs."""
    case = CASES[recipe](R)
    a, b = (P.TunerPaletteRef(case.n_ch, case.n_src, case.fs, R) for _ in range(2))
    worst = peak = 0.0
    for ev in case.events:
        if ev[0] == "set":
            ev[1](a); ev[1](b)
        else:
            z = a.update(ev[1], keep_float=True)[2]
            w = b.update(ev[1], keep_float=True, f32=True)[2]
            worst = max(worst, float(np.abs(T.clip16(w.real) - T.clip16(z.real)).max()), float(np.abs(T.clip16(w.imag) - T.clip16(z.imag)).max()))
            peak = max(peak, float(np.abs(z).max()))
    return worst, peak


# EPS[recipe, R] = min(8 x measure(recipe, R)[0], 0.1) to three digits.
EPS = {
    ("parity", 2): 0.0312,   # measured 0.0039 at peak |z| 23944
    ("parity", 32): 0.02,   # measured 0.0025 at peak |z| 14971
    ("gain", 2): 0.0615,   # measured 0.00769 at peak |z| 2965821
    ("gain", 32): 0.0449,   # measured 0.00561 at peak |z| 2965821
    ("timing", 2): 0.00607,   # measured 0.000759 at peak |z| 5279
    ("timing", 32): 0.00586,   # measured 0.000733 at peak |z| 3321
    ("levels", 2): 0.00402,   # measured 0.000502 at peak |z| 3170
    ("levels", 32): 0.00423,   # measured 0.000529 at peak |z| 2983
}
assert max(EPS.values()) <= 0.1


def pair(gpu, case):
    bank = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, case.R)
    return bank, P.TunerPaletteRef(case.n_ch, case.n_src, case.fs, case.R, g=bank.get_channel_filter())


@pytest.mark.parametrize("R", RS)
def test_parity_with_three_slots_and_four_gains(gpu, R):
    case = parity_case(R)
    bank, ref = pair(gpu, case)
    outs = T.run_pass_through(bank, ref, case.events, EPS["parity", R])
    assert len(outs) == 2 and list(bank.slots()) == list(ref.slots()) and list(bank.gains()) == list(ref.gains())
    assert max(float(np.abs(z).max()) for _, _, z in outs) < 32000.0     # no sample leans on the clamp
    bank.close()


@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("R", RS)
def test_untouched_channels_are_bit_identical(gpu, R, levels):
    """Bank A is plain; bank B has channel 2 on a defined slot, which puts the palette's kernel in the channel step's place for all
    of its channels.  Every other channel of B is A's, bit for bit -- with levels on, its level accumulator too."""
    case = T.edge_case(R)
    iqs = [T.cs16(np.random.default_rng(90 + R), case.n_src, nf * 128 * R) for nf in (1, 3)]
    fws = T.edge_words(R)
    outs, levs = [], []
    for moved in (False, True):
        bank = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
        T.setup(bank, [c % case.n_src for c in range(case.n_ch)], fws)
        if levels:
            bank.enable_levels()
        if moved:
            bank.set_palette_filter(5, G_CASYM); bank.set_channel_slot(5, ch=2)
        outs.append([bank.update(iq) for iq in iqs])
        levs.append(bank.levels()[0] if levels else None)
        bank.close()
    others = [c for c in range(case.n_ch) if c != 2]
    for (I0, Q0), (I1, Q1) in zip(*outs):
        assert np.array_equal(I0[others], I1[others]) and np.array_equal(Q0[others], Q1[others])
        assert not np.array_equal(I0[2], I1[2])
    if levels:
        assert np.array_equal(levs[0][others], levs[1][others]) and levs[0][2] != levs[1][2] and (levs[1] > 0).all()


@pytest.mark.parametrize("R", RS)
def test_gain_zero_and_gain_64_on_full_scale_sources(gpu, R):
    case = gain_case(R)
    bank, ref = pair(gpu, case)
    outs = T.run_pass_through(bank, ref, case.events, EPS["gain", R])
    assert len(outs) == 3
    for I, Q, z in outs[1:]:
        assert not I[4:6].any() and not Q[4:6].any()                    # gain 0 and -0.0: all-zero rows, exactly
        assert I[6].any() and np.abs(z[:4]).min() > 60 * 32768.0
        assert I[:4].min() == Q[:4].min() == -32768 and I[:4].max() == Q[:4].max() == 32767   # both clamps
        assert (np.abs(I[:4].astype(np.int64)) >= 32767).all() and (np.abs(Q[:4].astype(np.int64)) >= 32767).all()
    bank.close()


@pytest.mark.parametrize("R", RS)
def test_changes_apply_from_the_next_call_and_not_before(gpu, R):
    """Bank P runs the case: two frames, the changes, two frames; both calls within the bound of the restatement.  Bank Q never
    gets the changes: its first call is P's bit for bit (nothing applied early).  Bank S has them from the start: its second call
    is P's bit for bit (everything applied from the first frame; overlap-save keeps no per-channel state), and one call of 4
    frames on a third such bank equals the two calls of 2."""
    case = timing_case(R)
    bank, ref = pair(gpu, case)
    evs = list(case.events)
    outs = T.run_pass_through(bank, ref, evs, EPS["timing", R])
    assert len(outs) == 2 and list(bank.slots()) == [2, 2, 0, 0, 0, 0] and list(bank.gains()) == [1.0, 1.0, -3.0, 2.0, 1.0, 1.0]
    bank.close()
    iq_a, iq_b = evs[1][1], evs[3][1]
    q = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
    evs[0][1](q)
    Ia, Qa = q.update(iq_a)
    assert np.array_equal(Ia, outs[0][0]) and np.array_equal(Qa, outs[0][1])
    q.close()
    s = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
    evs[0][1](s); timing_change(s)
    Ia, Qa = s.update(iq_a)
    Ib, Qb = s.update(iq_b)
    assert np.array_equal(Ib, outs[1][0]) and np.array_equal(Qb, outs[1][1])
    assert not np.array_equal(Ia, outs[0][0])
    s.close()
    w = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
    evs[0][1](w); timing_change(w)
    I4, Q4 = w.update(np.concatenate([iq_a, iq_b], axis=1))
    assert np.array_equal(I4, np.concatenate([Ia, Ib], axis=1)) and np.array_equal(Q4, np.concatenate([Qa, Qb], axis=1))
    w.close()


@pytest.mark.parametrize("R", RS)
def test_levels_under_a_palette_exclude_the_gain(gpu, R):
    """The parity recipe with levels on: the rms of every channel against the restatement's, which takes G_{f_c} and no gain, after
    each call.  The rule of test_gpu_tuner_monitor.py: within the EPS of the same inputs -- here the recipe with
    every gain at 1, which is what the level sees."""
    import test_gpu_tuner_monitor as TM
    case = parity_case(R)
    bank, ref = pair(gpu, case)
    mon = P.PaletteMonitorRef(ref, levels=True)
    bank.enable_levels()
    for ev in case.events:
        if ev[0] == "set":
            ev[1](bank); ev[1](ref)
        else:
            bank.update(ev[1]); mon.update(ev[1])
            TM.check_levels(bank, mon, EPS["levels", R], ("palette", ev[2]))
    plain = P.TunerPaletteRef(case.n_ch, case.n_src, case.fs, R, g=bank.get_channel_filter())
    assert not np.array_equal(ref.channel_G(), plain.channel_G()) and (ref.gains() != 1.0).any()
    bank.close()


@pytest.mark.parametrize("R", RS)
def test_a_tone_outside_a_narrow_slot_reads_60_db_lower(gpu, R):
    """Two channels on one frequency, channel 1 on a +-250 Hz slot; a tone 8 kHz up.  The first frame (the tone's onset) is
    cleared away; over the next three the narrow channel's level is at least 60 dB below the default filter's."""
    A = 20000.0
    fs, H = 44100 * R, 128 * R
    bank = gpu.TunerBank.fastconv(2, 1, fs, R)
    bank.set_frequency(10000.0)
    bank.set_palette_filter(1, gpu.design_channel_filter(fs / R, -250.0, 250.0))
    bank.set_channel_slot(1, ch=1)
    bank.enable_levels()
    m = np.arange(4 * H)
    x = A * np.exp(2j * np.pi * 18000.0 * m / fs)
    iq = np.stack([np.round(x.real), np.round(x.imag)], axis=-1).astype(np.int16)[None]
    bank.update(iq[:, :H])
    bank.clear_levels()
    bank.update(iq[:, H:])
    lv, frames = bank.levels()
    assert frames == 3
    wide, narrow = lv / (128.0 * frames)
    print("tone of %.0f: default filter reads %.1f rms, the +-250 Hz slot %.3f rms (%.1f dB lower)" % (
        A, np.sqrt(wide), np.sqrt(narrow), 10 * np.log10(wide / max(narrow, 1e-30))))
    assert abs(np.sqrt(wide) - A) < 0.01 * A and wide >= 1e6 * narrow
    bank.close()


@pytest.mark.parametrize("R", RS)
def test_cu8_rows_give_what_their_cs16_conversion_gives(gpu, R):
    case = parity_case(R)
    configure = next(case.events)[1]
    outs = []
    for fmt in ("cu8", "cs16"):
        bank = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
        configure(bank)
        bank.set_input_format(fmt)
        outs.append([])
        rng = np.random.default_rng(88 + R)
        for nf in (1, 3):
            raw = rng.integers(0, 255, size=(case.n_src, nf * 128 * R, 2), endpoint=True).astype(np.uint8)
            outs[-1].append(bank.update_samples(raw if fmt == "cu8" else FM.to_cs16(raw, "cu8")))
        bank.close()
    for (I0, Q0), (I1, Q1) in zip(*outs):
        assert I0.any() and np.array_equal(I0, I1) and np.array_equal(Q0, Q1)


def test_palette_behind_a_real_stage_2(gpu):
    """2.4 MS/s, R = 16 (Fs_mid = 150 kHz; stage 2: 147 / 500): designed slots (an upper sideband and +-5 kHz), mixed gains, a
    reassignment and a gain change between calls, under the stage-2 bounds of test_gpu_tuner_fastconv.py."""
    fs, R, n_ch, n_src = 2400000, 16, 6, 2
    rng = np.random.default_rng(2401)
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    h2, g2 = bank.get_resampler()
    ref = P.TunerPaletteRef(n_ch, n_src, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2)
    usb, am = gpu.design_channel_filter(fs / R, 300.0, 3000.0), gpu.design_channel_filter(fs / R, -5000.0, 5000.0)
    assert usb.dtype == np.complex64 and am.dtype == np.float32
    for o in (bank, ref):
        T.setup(o, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
        o.set_palette_filter(1, usb); o.set_palette_filter(2, am)
        for c, (s, a) in enumerate(zip([0, 1, 2, 1, 2, 0], [1.0, 2.0, 0.5, -1.0, 1.0, 2.0])):
            o.set_channel_slot(s, ch=c); o.set_gain(a, ch=c)
    cap = Stage2Cap(2401)
    for k, nf in enumerate([1, 4, 2, 3]):
        if k == 2:
            for o in (bank, ref):
                o.set_channel_slot(2, ch=1); o.set_gain(-2.0, ch=0); o.set_frequency(-fs * 0.3, ch=3)
        iq = T.cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0)], fs, -5000, 5000)
        n = bank.out_blocks(nf)
        assert n == ref.out_blocks(nf)
        I, Q = bank.update_rate(iq)
        wI, wQ = cap.update(ref, iq)
        assert I.shape == wI.shape == (n_ch, n, 128)
        cap.check(I, wI, what=k); cap.check(Q, wQ, what=k)
        assert bank.output_position() == ref.out_pos
    cap.finish("palette behind stage 2")
    bank.close()


if __name__ == "__main__":                                    # the EPS table: measured on the CPU, pasted in above
    for recipe in CASES:
        for R in RS:
            worst, peak = measure(recipe, R)
            print('    ("%s", %d): %.3g,   # measured %.3g at peak |z| %.0f' % (recipe, R, min(8 * worst, 0.1), worst, peak), flush=True)
