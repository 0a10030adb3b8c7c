"""The palette restatement (tests/tuner_palette_ref.py) and the filter designer (audiosdr_amd.design_channel_filter) on the CPU: a
slot holding filter 0's taps is filter 0, a complex one-sided slot passes one sideband and holds the other down, the gain and
reset semantics of the restatement, the designed filters' pass and stop bands at four Fs_mid, and the GPU suite's EPS table
recomputed from the float32 model."""
import numpy as np
import pytest

import test_gpu_tuner_palette as TP
import tuner_fastconv_ref as F
import tuner_palette_ref as P

DELTA = 0.0392
PASSBANDS = [(-250.0, 250.0), (300.0, 3000.0), (-3000.0, -300.0), (-5000.0, 5000.0), (400.0, 1000.0), (-11500.0, 11500.0)]


def response_db(g, hz, fs_mid):
    """20 log10 |G| of taps g (real or complex) at the frequencies hz."""
    g = np.asarray(g).astype(np.complex128)
    G = (g[None, :] * np.exp(-2j * np.pi * np.outer(np.asarray(hz) / fs_mid, np.arange(g.size)))).sum(axis=1)
    return 20 * np.log10(np.maximum(np.abs(G), 1e-30))


def test_a_slot_with_filter_0s_taps_at_gain_1_is_the_plain_restatement():
    R = 4
    fs = 44100 * R
    rng = np.random.default_rng(4)
    fws = TP.T.edge_words(R)
    n_ch = len(fws)
    plain = F.TunerFastconvRef(n_ch, 2, fs, R, g=TP.T.G_ASYM)
    pal = P.TunerPaletteRef(n_ch, 2, fs, R, g=TP.T.G_ASYM)
    for o in (plain, pal):
        TP.T.setup(o, [c % 2 for c in range(n_ch)], fws)
    pal.set_palette_filter(7, TP.T.G_ASYM)
    pal.set_channel_slot(7)
    assert list(pal.slots()) == [7] * n_ch and list(pal.gains()) == [1.0] * n_ch
    for nf in (1, 3):
        iq = TP.T.cs16(rng, 2, nf * 128 * R)
        a, b = plain.update(iq, keep_float=True), pal.update(iq, keep_float=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    iq = TP.T.cs16(rng, 2, 128 * R)
    assert np.array_equal(plain.stage1_f32(iq), pal.stage1_f32(iq))


def test_a_one_sided_slot_passes_one_sideband_and_rejects_the_other(A):
    """Fs_mid = 44.1 kHz: a 500 .. 3000 Hz slot on a tone at +1.5 kHz and on the same tone at -1.5 kHz, in the unrounded output.
    (The transition is 1.73 kHz + 86 Hz wide there: this slot's stop band starts at -1315 Hz, that of a 300 Hz one at -1515 Hz.)"""
    R, nf, amp = 2, 6, 10000.0
    fs = 44100 * R
    usb = A.design_channel_filter(44100.0, 500.0, 3000.0)
    assert usb.dtype == np.complex64 and usb.size == 129
    m = np.arange(nf * 128 * R)
    rms = {}
    for off in (1500.0, -1500.0):
        ref = P.TunerPaletteRef(2, 1, fs, R)
        ref.set_frequency(20000.0)
        ref.set_palette_filter(1, usb)
        ref.set_channel_slot(1, ch=1)
        z = ref.stage1((amp * np.exp(2j * np.pi * (20000.0 + off) * m / fs))[None])
        rms[off] = np.sqrt((np.abs(z[:, 256:]) ** 2).mean(axis=1))   # past the onset
    assert abs(rms[1500.0][1] - amp) <= 0.002 * amp and abs(rms[-1500.0][0] - amp) <= 0.002 * amp   # in the band; the default filter
    down = 20 * np.log10(rms[-1500.0][1] / amp)
    assert down <= -70.0, down


def test_gain_and_reset_of_the_restatement():
    R = 2
    fs = 44100 * R
    rng = np.random.default_rng(9)
    ref = P.TunerPaletteRef(3, 1, fs, R)
    ref.set_frequency_word(0x12345678)
    ref.set_palette_filter(1, TP.G_J)
    ref.set_channel_slot(1, ch=1); ref.set_gain(-2.5, ch=2)
    iq = TP.T.cs16(rng, 1, 2 * 128 * R, (), fs, -3000, 3000)
    z = ref.stage1(iq)
    ref2 = F.TunerFastconvRef(1, 1, fs, R)
    ref2.set_frequency_word(0x12345678)
    z0 = ref2.stage1(iq)[0]
    assert np.array_equal(z[0], z0) and np.abs(z[2] + 2.5 * z0).max() <= 1e-9 * np.abs(z0).max()
    ref2.set_channel_filter([1.0])
    ref2.reset(); ref2.set_frequency_word(0x12345678)
    assert np.abs(z[1] - 1j * ref2.stage1(iq)[0]).max() <= 1e-9 * np.abs(z0).max()      # G = j times the all-pass
    mon = P.PaletteMonitorRef(P.TunerPaletteRef(3, 1, fs, R), levels=True)
    mon.ref.set_frequency_word(0x12345678); mon.ref.set_gain(-2.5, ch=2)
    mon.update(iq)
    assert mon.level[2] == mon.level[0] > 0                                              # the level leaves the gain out
    ref.reset()
    assert not ref.slots().any() and list(ref.gains()) == [1.0] * 3 and ref.get_palette_filter(1).tobytes() == TP.G_J.tobytes()
    with pytest.raises(AssertionError):
        ref.set_channel_slot(9)
    with pytest.raises(AssertionError):
        ref.set_gain(40000.0)


@pytest.mark.parametrize("fs_mid", [44100.0, 150000.0, 156250.0, 176400.0])
def test_designed_filters_meet_their_bars(A, fs_mid):
    """Within +-0.01 dB over [lo, hi] and at least 77 dB down outside [lo - d, hi + d], d = 0.0392 Fs_mid + Fs_mid / 512 (the
    widened design measures within +-0.0024 dB and 77.9 dB on this list), for the float32 / complex64 taps as returned."""
    d = DELTA * fs_mid + fs_mid / 512.0
    grid = np.linspace(-fs_mid / 2, fs_mid / 2, 16385)
    for lo, hi in PASSBANDS:
        g = A.design_channel_filter(fs_mid, lo, hi)
        assert g.size == 129 and g.dtype == (np.float32 if lo == -hi else np.complex64)
        assert abs(response_db(g, [0.5 * (lo + hi)], fs_mid)[0]) <= 0.01
        pb = response_db(g, np.linspace(lo, hi, 501), fs_mid)
        assert np.abs(pb).max() <= 0.01, (fs_mid, lo, hi, float(np.abs(pb).max()))
        sb = response_db(g, grid[(grid < lo - d) | (grid > hi + d)], fs_mid)
        assert sb.max() <= -77.0, (fs_mid, lo, hi, float(sb.max()))
    g = A.design_channel_filter(fs_mid, -11500.0, 11500.0).astype(np.float64)      # the default filter, Fs_mid / 512 wider
    assert abs(g.sum() - 1.0) < 1e-6 and np.array_equal(g, g[::-1])
    for bad in ((100.0, 100.0), (200.0, 100.0), (-fs_mid, 0.0), (-0.49 * fs_mid, 0.49 * fs_mid)):
        with pytest.raises(A.AsdrError):
            A.design_channel_filter(fs_mid, *bad)


def test_eps_table_is_eight_times_the_float32_model():
    assert set(TP.EPS) == {(r, R) for r in TP.CASES for R in TP.RS} and max(TP.EPS.values()) <= 0.1
    for (recipe, R), eps in sorted(TP.EPS.items()):
        want = min(8 * TP.measure(recipe, R)[0], 0.1)
        assert abs(eps - want) <= 0.1 * want, (recipe, R, eps, want)
